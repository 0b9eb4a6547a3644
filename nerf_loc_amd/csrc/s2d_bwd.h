// The matcher MLP's way back, shared by the two training kernels that recompute it per pair (s2d_bwd.hip: every 3-D row against every 2-D column; fine_bwd.hip: a
// match's centre descriptor against its 49 window cells).  s2d_bwd_chain takes layer 1's accumulators of the wave's two 32-pair tiles (s2d.h's convention) and
// leaves g_a1 as the split B operand of W1^T: h1, its mask, layer 2 again, the mask of h2, the fp64 decision of both masks for the pairs with a pre-activation
// near zero, g_a2 = g_logit w3 [h2 > 0], the wave's share of gW3 / gb3, g_a1 = (W2^T g_a2) [h1 > 0], and the stores of the weight gradients' operands.  What a
// pair is, where its logit's gradient comes from and what happens to g_x = W1^T g_a1 stay in the kernel files.  Include after s2d.h.
#pragma once
#include "common.h"
#include "mfma.h"
#include "s2d.h"

namespace {

constexpr int S2D_W3P_LD = 132;            // floats of a wave's gW3 / gb3 partial row: [hh][64 accumulator slots], gb3, padding

__device__ __forceinline__ void bwd_store4(float* p, const nl_f32x16& v, int r4) { *(float4*)p = make_float4(v[4 * r4], v[4 * r4 + 1], v[4 * r4 + 2], v[4 * r4 + 3]); }

// accumulators (final values) -> the split B operands of the next product: k-step (b, s) = words 4 s .. 4 s + 3 of block b (accumulator registers 8 s .. 8 s + 7)
__device__ __forceinline__ void bwd_split(const nl_f32x16 (&acc)[2][4], unsigned (&hi)[2][4][8], unsigned (&lo)[2][4][8]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        nl_split_bf16_pair(acc[t][b][4 * r4 + 0], acc[t][b][4 * r4 + 1], hi[t][b][2 * r4], lo[t][b][2 * r4]);
        nl_split_bf16_pair(acc[t][b][4 * r4 + 2], acc[t][b][4 * r4 + 3], hi[t][b][2 * r4 + 1], lo[t][b][2 * r4 + 1]);
      }
}
// row block rb of a transposed product (K = 128 in accumulator order, nrb row blocks in the image) into o0 / o1 (tile 0 / 1)
template <bool X3>
__device__ __forceinline__ void bwd_mult(nl_f32x16& o0, nl_f32x16& o1, const unsigned (&hi)[2][4][8], const unsigned (&lo)[2][4][8], const uint4* whi, const uint4* wlo,
                                         int nrb, int rb, int lane) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const nl_i16x8 bh0 = nl_frag(hi[0][b][4 * s], hi[0][b][4 * s + 1], hi[0][b][4 * s + 2], hi[0][b][4 * s + 3]);
      const nl_i16x8 bh1 = nl_frag(hi[1][b][4 * s], hi[1][b][4 * s + 1], hi[1][b][4 * s + 2], hi[1][b][4 * s + 3]);
      const int f = ((b * 2 + s) * nrb + rb) * 64 + lane;
      const nl_i16x8 ah = nl_frag(whi[f]);
      if (X3) {
        const nl_i16x8 bl0 = nl_frag(lo[0][b][4 * s], lo[0][b][4 * s + 1], lo[0][b][4 * s + 2], lo[0][b][4 * s + 3]);
        const nl_i16x8 bl1 = nl_frag(lo[1][b][4 * s], lo[1][b][4 * s + 1], lo[1][b][4 * s + 2], lo[1][b][4 * s + 3]);
        const nl_i16x8 al = nl_frag(wlo[f]);
        o0 = nl_mfma<false>(al, bh0, o0); o1 = nl_mfma<false>(al, bh1, o1);
        o0 = nl_mfma<false>(ah, bl0, o0); o1 = nl_mfma<false>(ah, bl1, o1);
      }
      o0 = nl_mfma<false>(ah, bh0, o0); o1 = nl_mfma<false>(ah, bh1, o1);
    }
}
// one step of the halving exchange over the 32 lanes of a half-wave: lanes with bit O keep the upper NH values, the others the lower NH, plus the partner's
template <int NH, int O>
__device__ __forceinline__ void bwd_halve(float (&v)[64], int lane) {
  const bool up = (lane & O) != 0;
#pragma unroll
  for (int i = 0; i < NH; ++i) {
    const float send = up ? v[i] : v[i + NH], keep = up ? v[i + NH] : v[i];
    v[i] = keep + __shfl_xor(send, O);
  }
}

// index into a bias table of the image's `small` block (accumulator order: [hh][16 b + r]) of hidden unit u
__device__ __forceinline__ int bwd_small_index(int u) { const int w = u & 31; return 64 * ((w >> 2) & 1) + 16 * (u >> 5) + 4 * (w >> 3) + (w & 3); }
// the lane's 64 mask bits (bit 16 b + r) out of the two ballots over the hidden units 0..63 / 64..127
__device__ __forceinline__ unsigned long long bwd_mask_from_units(unsigned long long lo, unsigned long long hi, int hh) {
  unsigned long long mk = 0ull;
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = 32 * b + 8 * (r >> 2) + 4 * hh + (r & 3);
      mk |= (((b < 2 ? lo : hi) >> (u & 63)) & 1ull) << (16 * b + r);
    }
  return mk;
}
// The signs of both layers' pre-activations of ONE pair in fp64, by the whole wave: lane l evaluates hidden units l and l + 64 (w1t: W1^T [C][128], w2t: W2^T
// [128 k][128 j], fp32; small: the image's bias tables), h1 goes round by shuffles, the signs come back as ballots over units 0..63 / 64..127.  Its own function so
// that the rare path reads as one; the register pressure it puts on the kernels (spilled VGPRs; DESIGN.md section 5.32 has the A/B) is the same inlined or not.
__device__ __attribute__((noinline)) void bwd_fp64_signs(const float* pd0, const float* pd1, int C, const float* w1t, const float* w2t, const float* small, int lane,
                                                         unsigned long long& m1lo, unsigned long long& m1hi, unsigned long long& m2lo, unsigned long long& m2hi) {
  const int i0 = bwd_small_index(lane), i1 = bwd_small_index(lane + 64);
  double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
  for (int k = 0; k < C; ++k) {
    const double xv = (double)pd0[k] * (double)pd1[k];
    s0 += xv * (double)w1t[k * S2D_H + lane];
    s1 += xv * (double)w1t[k * S2D_H + 64 + lane];
  }
  s0 += (double)small[i0]; s1 += (double)small[i1];
  m1lo = __ballot(s0 > 0.0); m1hi = __ballot(s1 > 0.0);
  s0 = s0 > 0.0 ? s0 : 0.0; s1 = s1 > 0.0 ? s1 : 0.0;
  double t0 = 0.0, t1 = 0.0;
#pragma unroll 8
  for (int k = 0; k < 64; ++k) {
    const double hk = __shfl(s0, k);
    t0 += hk * (double)w2t[k * S2D_H + lane];
    t1 += hk * (double)w2t[k * S2D_H + 64 + lane];
  }
#pragma unroll 8
  for (int k = 0; k < 64; ++k) {
    const double hk = __shfl(s1, k);
    t0 += hk * (double)w2t[(64 + k) * S2D_H + lane];
    t1 += hk * (double)w2t[(64 + k) * S2D_H + 64 + lane];
  }
  t0 += (double)small[128 + i0]; t1 += (double)small[128 + i1];
  m2lo = __ballot(t0 > 0.0); m2hi = __ballot(t1 > 0.0);
}
// relative width of the band around zero inside which a pre-activation's sign is decided again in fp64 (of the lane's largest |pre-activation| of the layer):
// some forty times the typical error of the fp32 chains, so that the masks are those of the fp64 evaluation; 1.6e-6 of the units fall inside (one pair in 2400)
constexpr float S2D_BWD_BAND = 1e-6f;

// where a wave's tiles go: rows prow[t] of the row-major operand matrices of the weight gradients (h1, ga2, ga1: 128 columns) and the wave's partial row of
// gW3 / gb3 (S2D_W3P_LD floats); each may be null (that parameter is frozen)
struct S2dBwdStores { float* h1; float* ga2; float* ga1; float* w3row; };

// acc in: layer 1's accumulators of the two tiles (before the bias); hi / lo out: g_a1 split, the B operand of W1^T.  ok[t] / prow[t]: whether the lane's pair
// of tile t exists and its row in the operand matrices.  hidden: EXACT, the lane's private LDS column (s2d.h: s2d_f32_layer2).  gl_of(gl): the logit's gradient
// of the lane's two pairs (0 where !ok; both half-waves hold both).  pair_of(t, c, pd0, pd1): the two descriptors whose product is the pair in column c of tile t.
//
// EXACT (NL_PREC_F32, NL_PREC_BF16X3): layer 2 is recomputed with the exact fp32 body (v_mfma_f32_32x32x2_f32) and the gradient products are three-term
// split-bf16; otherwise (NL_PREC_BF16) both are one-term bf16.  The recomputation decides the ReLU masks, and a mask is not a smooth function of its input: a
// pre-activation within the recomputation's error of zero flips its unit's gradient between g and 0.  With the three-term bodies (5e-6 of the row's scale) about
// one unit in 10^5 flipped, a planted pair among them every other case, each worth 5e-3 of max |gradient|.  Exact fp32 still flipped one unit in 10^7 — as the fp32
// reference does against fp64 — which a random cotangent of the scores shows as 1e-3 in gW2, so the pairs that have a pre-activation inside a narrow band around zero
// get their masks from an fp64 evaluation of that pair by the whole wave (two hidden units per lane; fp32 transposes of the training image).
template <bool EXACT, class GL, class PAIR>
__device__ __forceinline__ void s2d_bwd_chain(nl_f32x16 (&acc)[2][4], const unsigned char* img, const unsigned char* timg, int C, const bool (&ok)[2],
                                              const size_t (&prow)[2], const S2dBwdStores& o, float* hidden, int lane, GL&& gl_of, PAIR&& pair_of,
                                              unsigned (&hi)[2][4][8], unsigned (&lo)[2][4][8]) {
  constexpr bool X3 = EXACT;
  const int hh = lane >> 5;
  const S2dLayout L = s2d_layout(C);
  const S2dTrainLayout T = s2d_train_layout(C);
  const float* small = (const float*)(img + L.small);
  const float* b1p = small + 64 * hh;
  // h1 = relu(a1 + b1): its sign bits (bit 16 b + r of the tile's word) and, for gW2, its values
  unsigned long long mask1[2] = {0ull, 0ull};
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 bb = *(const float4*)(b1p + 16 * b + 4 * r4);
      const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        float h[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          h[e] = fmaxf(acc[t][b][4 * r4 + e] + bv[e], 0.f);
          if (h[e] > 0.f) mask1[t] |= 1ull << (16 * b + 4 * r4 + e);
        }
        if (o.h1 && ok[t]) *(float4*)(o.h1 + prow[t] * S2D_H + 32 * b + 8 * r4 + 4 * hh) = make_float4(h[0], h[1], h[2], h[3]);
      }
    }
  bool amb[2] = {false, false};   // EXACT: a pre-activation of the pair lies inside the band
  if constexpr (EXACT) {
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float amax = 0.f, amin = 3.4e38f;
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = fabsf(acc[t][b][r] + b1p[16 * b + r]);
          amax = fmaxf(amax, v); amin = fminf(amin, v);
        }
      amb[t] = amin < S2D_BWD_BAND * amax;
    }
  }
  if constexpr (EXACT) s2d_f32_layer2(acc, b1p, hidden, (const float*)(img + L.f32w2), lane);
  else s2d_layer2<false>(acc, b1p, (const uint4*)(img + L.w2hi), (const uint4*)(img + L.w2lo), lane);

  // ---- sign bits of h2 (bit 16 b + r); EXACT: the pairs with a pre-activation inside the band get the masks of both layers from an fp64 evaluation by the whole wave
  unsigned long long mask2[2] = {0ull, 0ull};
  {
    const float* b2p = small + 128 + 64 * hh;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float amax = 0.f, amin = 3.4e38f;
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const float v = acc[t][b][r] + b2p[16 * b + r];
          if (v > 0.f) mask2[t] |= 1ull << (16 * b + r);
          amax = fmaxf(amax, fabsf(v)); amin = fminf(amin, fabsf(v));
        }
      if (EXACT) amb[t] = amb[t] || amin < S2D_BWD_BAND * amax;
    }
  }
  if constexpr (EXACT) {
    const float* w1t = (const float*)(timg + T.f32w1t);   // [C][128]
    const float* w2t = (const float*)(timg + T.f32w2t);   // [128 k][128 j]
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const unsigned long long bal = __ballot(amb[t] && ok[t]);
      unsigned pairs = (unsigned)(bal | (bal >> 32));   // wave-uniform: either half-wave of a pair may have flagged it
      while (pairs) {
        const int c = __builtin_ctz(pairs);
        pairs &= pairs - 1;
        unsigned long long m1lo, m1hi, m2lo, m2hi;
        const float* pd0; const float* pd1;
        pair_of(t, c, pd0, pd1);
        bwd_fp64_signs(pd0, pd1, C, w1t, w2t, small, lane, m1lo, m1hi, m2lo, m2hi);
        if ((lane & 31) == c) {
          mask1[t] = bwd_mask_from_units(m1lo, m1hi, hh);
          mask2[t] = bwd_mask_from_units(m2lo, m2hi, hh);
        }
      }
    }
  }

  // ---- the logit's gradient of the lane's two pairs (both half-waves hold both)
  float gl[2];
  gl_of(gl);
  // ---- g_a2 = g_logit w3 [h2 > 0] in place; the lane's share of gW3
  {
    const float* b2p = small + 128 + 64 * hh;
    const float* w3p = small + 256 + 64 * hh;
    float gw3[64];
#pragma unroll
    for (int b = 0; b < 4; ++b)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) {
        const float4 bb = *(const float4*)(b2p + 16 * b + 4 * r4), ww = *(const float4*)(w3p + 16 * b + 4 * r4);
        const float bv[4] = {bb.x, bb.y, bb.z, bb.w}, wv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int r = 4 * r4 + e;
          const float h0 = fmaxf(acc[0][b][r] + bv[e], 0.f), h1 = fmaxf(acc[1][b][r] + bv[e], 0.f);
          gw3[16 * b + r] = gl[0] * h0 + gl[1] * h1;
          acc[0][b][r] = ((mask2[0] >> (16 * b + r)) & 1ull) ? gl[0] * wv[e] : 0.f;
          acc[1][b][r] = ((mask2[1] >> (16 * b + r)) & 1ull) ? gl[1] * wv[e] : 0.f;
        }
#pragma unroll
        for (int t = 0; t < 2; ++t)
          if (o.ga2 && ok[t]) bwd_store4(o.ga2 + prow[t] * S2D_H + 32 * b + 8 * r4 + 4 * hh, acc[t][b], r4);
      }
    if (o.w3row) {
      bwd_halve<32, 16>(gw3, lane);
      bwd_halve<16, 8>(gw3, lane);
      bwd_halve<8, 4>(gw3, lane);
      bwd_halve<4, 2>(gw3, lane);
      bwd_halve<2, 1>(gw3, lane);   // the lane now holds slots 2 (lane & 31) and + 1 of its half-wave
      *(float2*)(o.w3row + 64 * hh + 2 * (lane & 31)) = make_float2(gw3[0], gw3[1]);
      float g = gl[0] + gl[1];
#pragma unroll
      for (int x = 16; x >= 1; x >>= 1) g += __shfl_xor(g, x);
      if (lane == 0) o.w3row[128] = g;
    }
  }
  // ---- g_a1 = (W2^T g_a2) [h1 > 0]
  bwd_split(acc, hi, lo);
  nl_acc_zero(acc);
  {
    const uint4* w2thi = (const uint4*)(timg + T.w2t_hi);
    const uint4* w2tlo = (const uint4*)(timg + T.w2t_lo);
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) bwd_mult<X3>(acc[0][rb], acc[1][rb], hi, lo, w2thi, w2tlo, 4, rb, lane);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (!((mask1[t] >> (16 * b + r)) & 1ull)) acc[t][b][r] = 0.f;
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
        if (o.ga1 && ok[t]) bwd_store4(o.ga1 + prow[t] * S2D_H + 32 * b + 8 * r4 + 4 * hh, acc[t][b], r4);
    }
  bwd_split(acc, hi, lo);
}

}  // namespace
