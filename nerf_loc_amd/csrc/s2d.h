// What the two users of the matcher MLP (C -> 128 -> ReLU -> 128 -> ReLU -> 1) share: s2d.hip (coarse: every 3-D row against every 2-D column) and fine.hip (fine: a
// match's centre descriptor against its 49 window cells).  ONE packed image (nl_s2d_pack_weights: s2d_layout), the accumulator convention (s2d_unit) and one copy
// of the layer bodies and of the last layer (s2d_logits) — nothing else: the 16-bit operand helpers (nl_frag, nl_split_pair, nl_mfma, nl_acc_zero) and the fragment
// maps of the image's planes are mfma.h's.  Everything here is __device__ __forceinline__ or constexpr; how the B operand of layer 1 is built, where the weights live
// (LDS or L2) and what happens to the 128 -> 1 output stay in the kernel files.  Include after common.h and mfma.h.
#pragma once
#include "common.h"
#include "mfma.h"

constexpr int S2D_H = 128;                 // hidden width (fixed, as the reference)
constexpr int S2D_SMALL_BYTES = 2048;      // b1p[2][64], b2p[2][64], w3p[2][64], b3
constexpr int S2D_W2_BYTES = 32 * 1024;    // one bf16 plane of W2: 32 fragments
constexpr int S2D_F32_LDS = 4 * 128 * 64 * 4;   // fp32 kernels: the hidden activations of 4 waves x 2 tiles, lane-private columns

struct S2dLayout {
  size_t w1hi, w2hi, w2lo, small, w1lo, f32w1, f32w2, h1hi, h1lo, h2hi, h2lo, total;   // h*: the bf16 planes' fragments again as split-FP16 (fine.hip)
  size_t lds_bytes;   // the prefix [0, lds_bytes) is what the coarse bf16 kernels keep in LDS
};
__host__ __device__ inline S2dLayout s2d_layout(int C) {
  S2dLayout l;
  const size_t w1 = (size_t)C * S2D_H * 2;   // one bf16 plane of W1
  l.w1hi = 0;
  l.w2hi = l.w1hi + w1;
  l.w2lo = l.w2hi + S2D_W2_BYTES;
  l.small = l.w2lo + S2D_W2_BYTES;
  l.lds_bytes = l.small + S2D_SMALL_BYTES;
  l.w1lo = l.lds_bytes;
  l.f32w1 = l.w1lo + w1;
  l.f32w2 = l.f32w1 + (size_t)C * S2D_H * 4;
  l.h1hi = l.f32w2 + (size_t)S2D_H * S2D_H * 4;
  l.h1lo = l.h1hi + w1;
  l.h2hi = l.h1lo + w1;
  l.h2lo = l.h2hi + S2D_W2_BYTES;
  l.total = l.h2lo + S2D_W2_BYTES;
  return l;
}
inline bool s2d_c_ok(int C) { return C >= 32 && C <= 256 && (C & 31) == 0; }

// hidden unit held by accumulator register r of 32-block b in half-wave hh (C/D layout of the 32x32 MFMAs: row = (r & 3) + 8 (r >> 2) + 4 hh)
__host__ __device__ inline int s2d_unit(int b, int r, int hh) { return 32 * b + 8 * (r >> 2) + 4 * hh + (r & 3); }

// ---- 16-bit path (split-bf16 or, F16, split-FP16: mfma.h).  acc[t][b]: column tile t (32 pairs), hidden 32-block b.
// k-step s of layer 1: the four row blocks of W1 against the two tiles' B operands (hi / lo words of 8 products per lane)
template <bool X3, bool F16 = false>
__device__ __forceinline__ void s2d_layer1_step(nl_f32x16 (&acc)[2][4], const uint4* w1hi, const uint4* w1lo, int s, int lane, const unsigned (&ph)[2][4],
                                                const unsigned (&pl)[2][4]) {
  nl_i16x8 bh[2], bl[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    bh[t] = nl_frag(ph[t][0], ph[t][1], ph[t][2], ph[t][3]);
    bl[t] = nl_frag(pl[t][0], pl[t][1], pl[t][2], pl[t][3]);
  }
#pragma unroll
  for (int rb = 0; rb < 4; ++rb) {
    const int f = ((s << 2) + rb) * 64 + lane;
    const nl_i16x8 ah = nl_frag(w1hi[f]);
    if (X3) {
      const nl_i16x8 al = nl_frag(w1lo[f]);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        acc[t][rb] = nl_mfma<F16>(al, bh[t], acc[t][rb]);
        acc[t][rb] = nl_mfma<F16>(ah, bl[t], acc[t][rb]);
      }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t) acc[t][rb] = nl_mfma<F16>(ah, bh[t], acc[t][rb]);
  }
}

// bias + ReLU + split of layer 1's accumulators, then layer 2 (K = 128) into the same accumulators: k-step (b, s) = accumulator registers 8 s .. 8 s + 7 of block b.
// b1p: the lane's half of the bias table (small + 64 hh)
template <bool X3, bool F16 = false>
__device__ __forceinline__ void s2d_layer2(nl_f32x16 (&acc)[2][4], const float* b1p, const uint4* w2hi, const uint4* w2lo, int lane) {
  unsigned hhi[2][4][8], hlo[2][4][8];
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 bb = *(const float4*)(b1p + 16 * b + 4 * r4);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        nl_split_pair<F16>(fmaxf(acc[t][b][4 * r4 + 0] + bb.x, 0.f), fmaxf(acc[t][b][4 * r4 + 1] + bb.y, 0.f), hhi[t][b][2 * r4], hlo[t][b][2 * r4]);
        nl_split_pair<F16>(fmaxf(acc[t][b][4 * r4 + 2] + bb.z, 0.f), fmaxf(acc[t][b][4 * r4 + 3] + bb.w, 0.f), hhi[t][b][2 * r4 + 1], hlo[t][b][2 * r4 + 1]);
      }
    }
  nl_acc_zero(acc);
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      nl_i16x8 bh[2], bl[2];
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        bh[t] = nl_frag(hhi[t][b][4 * s], hhi[t][b][4 * s + 1], hhi[t][b][4 * s + 2], hhi[t][b][4 * s + 3]);
        bl[t] = nl_frag(hlo[t][b][4 * s], hlo[t][b][4 * s + 1], hlo[t][b][4 * s + 2], hlo[t][b][4 * s + 3]);
      }
#pragma unroll
      for (int rb = 0; rb < 4; ++rb) {
        const int f = (((b * 2 + s) << 2) + rb) * 64 + lane;
        const nl_i16x8 ah = nl_frag(w2hi[f]);
        if (X3) {
          const nl_i16x8 al = nl_frag(w2lo[f]);
#pragma unroll
          for (int t = 0; t < 2; ++t) {
            acc[t][rb] = nl_mfma<F16>(al, bh[t], acc[t][rb]);
            acc[t][rb] = nl_mfma<F16>(ah, bl[t], acc[t][rb]);
          }
        }
#pragma unroll
        for (int t = 0; t < 2; ++t) acc[t][rb] = nl_mfma<F16>(ah, bh[t], acc[t][rb]);
      }
    }
}

// ---- exact fp32 path (v_mfma_f32_32x32x2_f32; half-wave hh supplies k slot hh of every step)
// channel group g of layer 1: step t multiplies channel 8 g + 4 hh + t; pa / pb: the lane's four products of tile 0 / 1
__device__ __forceinline__ void s2d_f32_layer1_group(nl_f32x16 (&acc)[2][4], const float* w1f, int g, int lane, const float (&pa)[4], const float (&pb)[4]) {
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      const float w = w1f[(((g * 4 + t) << 2) + rb) * 64 + lane];
      acc[0][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, pa[t], acc[0][rb], 0, 0, 0);
      acc[1][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, pb[t], acc[1][rb], 0, 0, 0);
    }
}
// bias + ReLU; the 128 values per lane are parked in a lane-private LDS column (hbuf: [2 tiles x 64 values][64 lanes] of this wave, + lane) so that layer 2 can be
// a rolled loop (fully unrolled, its 256 fragment loads are hoisted and the kernel spills).  Step t of block b takes accumulator register t (k = 16 b + t).
__device__ __forceinline__ void s2d_f32_layer2(nl_f32x16 (&acc)[2][4], const float* b1p, float* hbuf, const float* w2f, int lane) {
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 bb = *(const float4*)(b1p + 16 * b + 4 * r4);
      const float bv[4] = {bb.x, bb.y, bb.z, bb.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 2; ++t) hbuf[(t * 64 + 16 * b + 4 * r4 + e) * 64] = fmaxf(acc[t][b][4 * r4 + e] + bv[e], 0.f);
    }
  nl_acc_zero(acc);
#pragma unroll 2
  for (int k = 0; k < 64; ++k) {
    const float h0 = hbuf[k * 64], h1 = hbuf[(64 + k) * 64];
#pragma unroll
    for (int rb = 0; rb < 4; ++rb) {
      const float w = w2f[((k << 2) + rb) * 64 + lane];
      acc[0][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, h0, acc[0][rb], 0, 0, 0);
      acc[1][rb] = __builtin_amdgcn_mfma_f32_32x32x2f32(w, h1, acc[1][rb], 0, 0, 0);
    }
  }
}

// ---- last layer (both paths): bias + ReLU of layer 2's accumulators, the in-lane dot over the lane's 64 hidden units plus the other half-wave's 64 (a + b == b + a:
// both halves hold the same bits), + b3.  logit[t]: the pair in column lane & 31 of tile t.
__device__ __forceinline__ void s2d_logits(const nl_f32x16 (&acc)[2][4], const float* small, int hh, float (&logit)[2]) {
  const float* b2p = small + 128 + 64 * hh;
  const float* w3p = small + 256 + 64 * hh;
  float dot[2] = {0.f, 0.f};
#pragma unroll
  for (int b = 0; b < 4; ++b)
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const float4 bb = *(const float4*)(b2p + 16 * b + 4 * r4), ww = *(const float4*)(w3p + 16 * b + 4 * r4);
      const float bv[4] = {bb.x, bb.y, bb.z, bb.w}, wv[4] = {ww.x, ww.y, ww.z, ww.w};
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int t = 0; t < 2; ++t) dot[t] += fmaxf(acc[t][b][4 * r4 + e] + bv[e], 0.f) * wv[e];
    }
  const float b3 = small[384];
#pragma unroll
  for (int t = 0; t < 2; ++t) logit[t] = dot[t] + __shfl_xor(dot[t], 32) + b3;
}

// ---- training (s2d.hip: the loss of nl_s2d_forward_train; s2d_bwd.hip: its derivative).  The reference's sigmoid focal loss of one pair with unit anchor weight
// (sparse_to_dense.py:14-78: alpha 0.25, gamma 2) from the logit z and a float target y, before the mean over N * M:
//   L = (y a + (1 - y)(1 - a)) pt^2 bce,   pt = y (1 - p) + (1 - y) p,   bce = max(z, 0) - z y + log1p(exp(-|z|)),   dL/dz = aw (2 pt (1 - 2 y) p (1 - p) bce + pt^2 (p - y))
// p and 1 - p both come from e = exp(-|z|), so neither cancels in saturation (z large: p == 1.0f, 1 - p == e); dsig = p (1 - p) is also the score's derivative.
constexpr float S2D_FOCAL_ALPHA = 0.25f;
__device__ __forceinline__ void s2d_focal(float z, float y, float& loss, float& dz, float& dsig) {
  const float e = expf(-fabsf(z)), r = 1.f / (1.f + e);
  const float big = r, small = e * r;   // sigmoid(|z|), sigmoid(-|z|)
  const float p = z >= 0.f ? big : small, q = z >= 0.f ? small : big;
  const float aw = y * S2D_FOCAL_ALPHA + (1.f - y) * (1.f - S2D_FOCAL_ALPHA);
  const float pt = y * q + (1.f - y) * p;
  const float bce = fmaxf(z, 0.f) - z * y + log1pf(e);
  dsig = p * q;
  loss = aw * pt * pt * bce;
  dz = aw * (2.f * pt * (1.f - 2.f * y) * dsig * bce + pt * pt * (p - y));
}

// The training image (nl_s2d_pack_train_weights): the transposed weights as A fragments whose K order is the accumulator order (nl_frag16_src, acc_order), so that a
// gradient held in layer accumulators is the B operand of the transposed product without leaving the lane.  The fp32 transposes are the packer's source rows.
struct S2dTrainLayout { size_t w2t_hi, w2t_lo, w1t_hi, w1t_lo, f32w2t, f32w1t, total; };
__host__ __device__ inline S2dTrainLayout s2d_train_layout(int C) {
  S2dTrainLayout l;
  const size_t w1 = (size_t)C * S2D_H * 2;
  l.w2t_hi = 0;
  l.w2t_lo = l.w2t_hi + S2D_W2_BYTES;
  l.w1t_hi = l.w2t_lo + S2D_W2_BYTES;
  l.w1t_lo = l.w1t_hi + w1;
  l.f32w2t = l.w1t_lo + w1;
  l.f32w1t = l.f32w2t + (size_t)S2D_H * S2D_H * 4;
  l.total = l.f32w1t + (size_t)C * S2D_H * 4;
  return l;
}
