// Training step of the sparse-to-dense coarse matcher (s2d.hip is the forward: nl_s2d_forward_train keeps the N x M logits and the focal loss): the gradients of
//   loss = mean focal(logit, target),  score = sigmoid(logit),  logit[n, m] = W3 . relu( W2 . relu( W1 . (desc0[n] * desc1[m]) + b1 ) + b2 ) + b3
// with respect to both descriptor sets and the six parameters, from the saved logits alone: the hidden activations are recomputed, never kept.
//
// The rows n are walked in chunks of about S2D_BWD_PAIRS pairs (half of that for small problems); the buffers below hold one chunk and are reused by the next, so the workspace does not grow with N.
// Per chunk:
//   1. s2d_bwd_kernel, one wave per (32 columns m) x (two rows n), the tile shape and the layer bodies of the score kernel (s2d.h), weight fragments from L2:
//      layer 1 and 2 again (exact fp32 in the parity modes: see the kernel); g_logit = g_loss / (N M) focal'(logit) + g_score s (1 - s); g_a2 = g_logit w3 [h2 > 0] in the accumulators of layer 2, which are at once
//      the B operand of W2^T (the training image holds the transposed weights with their K in accumulator order): g_a1 = (W2^T g_a2) [h1 > 0], and the same again with
//      W1^T, one 32-channel block at a time: g_x = W1^T g_a1.  Stored per pair (row-major chunk matrices): x, h1, g_a2, g_a1 (the operands of the weight gradients;
//      skipped when the parameter pointers are null) and g_x.  gW3 / gb3: the lane's sums over its two pairs, added across the 32 lanes of a half-wave by a halving
//      exchange (62 adds for 64 values), one partial row per wave.
//   2. gW2 += g_a2^T h1, gb2, gW1 += g_a1^T x, gb1: the split-K kernel of wgrad.hip on the chunk's rows (partials added in a fixed order, += over the chunks).
//   3. g_desc0[n] = sum_m g_x[n, m] * desc1[m] (256-column segments, four interleaved sub-sums each, then the segments in order), g_desc1[m] += sum_n g_x[n, m] * desc0[n]
//      (one thread per (m, 4 channels), rows in order), gW3 / gb3 += the waves' partials in order.
// Every sum has a fixed order that depends on the shape alone and no float atomic touches a result: two calls give the same bits.
// Gradient products are split-bf16 (three terms under NL_PREC_F32 and NL_PREC_BF16X3, one under NL_PREC_BF16) as in wgrad.hip: a gradient's scale is arbitrary.
// The recomputation of the activations is exact fp32 in both parity modes (the ReLU masks hang on it) and one-term bf16 under NL_PREC_BF16.
#include <algorithm>
#include "common.h"
#include "mfma.h"
#include "s2d.h"
#include "s2d_bwd.h"
#include "host.h"
#include "s2d_bwd_host.h"

namespace {

// pairs of one chunk (rounded to an even number of rows, at least two): 64 pairs per wave, so 65 536 pairs are one workgroup on each of 256 CUs; problems below
// 2^20 pairs take half of that, which keeps the workspace under half the product tensor down to a quarter of a million pairs
constexpr int64_t S2D_BWD_PAIRS = 65536, S2D_BWD_PAIRS_SMALL = 32768, S2D_BWD_SMALL_BELOW = 1 << 20;

struct BwdArgs {
  const unsigned char* img; const unsigned char* timg;
  const float* desc0; const float* desc1;
  const float* logits; const float* target; const float* g_loss; const float* g_score;
  float *x, *h1, *ga2, *ga1, *gx;   // the chunk's matrices, row (n - r0) * M + m; x, h1, ga2, ga1 may be null
  float* w3part;                    // [items][S2D_W3P_LD] or null
  int N, M, C, r0, r1;              // the chunk's rows [r0, r1)
  float inv_total;
};

// EXACT (NL_PREC_F32, NL_PREC_BF16X3): layers 1 and 2 are recomputed with the exact fp32 bodies (v_mfma_f32_32x32x2_f32) and the gradient products are three-term
// split-bf16; otherwise (NL_PREC_BF16) both are one-term bf16.  Why, and the fp64 decision of the masks near zero: s2d_bwd.h (s2d_bwd_chain), which the fine
// matcher's backward shares.
template <bool EXACT>
__global__ __launch_bounds__(256) void s2d_bwd_kernel(const BwdArgs a) {
  constexpr bool X3 = EXACT;
  extern __shared__ __attribute__((aligned(16))) float s2d_bwd_hidden[];   // EXACT: S2D_F32_LDS bytes, lane-private columns (s2d.h: s2d_f32_layer2)
  const int tid = threadIdx.x, lane = tid & 63, hh = lane >> 5;
  const int C = a.C, M = a.M, nrb1 = C >> 5;
  const int MT = (M + 31) >> 5, RP = (a.r1 - a.r0 + 1) >> 1;
  const int item = blockIdx.x * 4 + (tid >> 6);
  if (item >= MT * RP) return;   // wave-uniform; the kernel has no barrier
  const int rp = item / MT, mt = item - rp * MT;
  const S2dLayout L = s2d_layout(C);
  const S2dTrainLayout T = s2d_train_layout(C);
  const uint4* w1hi = (const uint4*)(a.img + L.w1hi);
  const uint4* w1lo = (const uint4*)(a.img + L.w1lo);

  const int m = mt * 32 + (lane & 31), n0 = a.r0 + 2 * rp;
  const bool has1 = n0 + 1 < a.r1;
  const bool ok[2] = {m < M, m < M && has1};
  const size_t prow[2] = {(size_t)(n0 - a.r0) * M + m, (size_t)(n0 + 1 - a.r0) * M + m};
  nl_f32x16 acc[2][4];
  nl_acc_zero(acc);
  // ---- layer 1 again (s2d.hip's walks); the products are also the X operand of gW1
  if constexpr (EXACT) {
    const float* w1f = (const float*)(a.img + L.f32w1);
    const float* d1p = a.desc1 + (size_t)min(m, M - 1) * C + 4 * hh;
    const float* d0a = a.desc0 + (size_t)n0 * C + 4 * hh;
    const float* d0b = a.desc0 + (size_t)(has1 ? n0 + 1 : n0) * C + 4 * hh;
    for (int g = 0; g < (C >> 3); ++g) {
      const float4 x = *(const float4*)(d1p + 8 * g), ya = *(const float4*)(d0a + 8 * g), yb = *(const float4*)(d0b + 8 * g);
      const float pa[4] = {x.x * ya.x, x.y * ya.y, x.z * ya.z, x.w * ya.w};
      const float pb[4] = {x.x * yb.x, x.y * yb.y, x.z * yb.z, x.w * yb.w};
      if (a.x) {
        if (ok[0]) *(float4*)(a.x + prow[0] * C + 8 * g + 4 * hh) = make_float4(pa[0], pa[1], pa[2], pa[3]);
        if (ok[1]) *(float4*)(a.x + prow[1] * C + 8 * g + 4 * hh) = make_float4(pb[0], pb[1], pb[2], pb[3]);
      }
      s2d_f32_layer1_group(acc, w1f, g, lane, pa, pb);
    }
  } else {
    const float* d1p = a.desc1 + (size_t)min(m, M - 1) * C + 8 * hh;
    const float* d0a = a.desc0 + (size_t)n0 * C + 8 * hh;
    const float* d0b = a.desc0 + (size_t)(has1 ? n0 + 1 : n0) * C + 8 * hh;
    for (int s = 0; s < (C >> 4); ++s) {
      const float4 x0 = *(const float4*)(d1p + 16 * s), x1 = *(const float4*)(d1p + 16 * s + 4);
      const float4 ya0 = *(const float4*)(d0a + 16 * s), ya1 = *(const float4*)(d0a + 16 * s + 4);
      const float4 yb0 = *(const float4*)(d0b + 16 * s), yb1 = *(const float4*)(d0b + 16 * s + 4);
      const float4 pa0 = make_float4(x0.x * ya0.x, x0.y * ya0.y, x0.z * ya0.z, x0.w * ya0.w), pa1 = make_float4(x1.x * ya1.x, x1.y * ya1.y, x1.z * ya1.z, x1.w * ya1.w);
      const float4 pb0 = make_float4(x0.x * yb0.x, x0.y * yb0.y, x0.z * yb0.z, x0.w * yb0.w), pb1 = make_float4(x1.x * yb1.x, x1.y * yb1.y, x1.z * yb1.z, x1.w * yb1.w);
      if (a.x) {
        if (ok[0]) { float* p = a.x + prow[0] * C + 16 * s + 8 * hh; *(float4*)p = pa0; *(float4*)(p + 4) = pa1; }
        if (ok[1]) { float* p = a.x + prow[1] * C + 16 * s + 8 * hh; *(float4*)p = pb0; *(float4*)(p + 4) = pb1; }
      }
      unsigned ph[2][4], pl[2][4];
      nl_split_bf16_pair(pa0.x, pa0.y, ph[0][0], pl[0][0]);
      nl_split_bf16_pair(pa0.z, pa0.w, ph[0][1], pl[0][1]);
      nl_split_bf16_pair(pa1.x, pa1.y, ph[0][2], pl[0][2]);
      nl_split_bf16_pair(pa1.z, pa1.w, ph[0][3], pl[0][3]);
      nl_split_bf16_pair(pb0.x, pb0.y, ph[1][0], pl[1][0]);
      nl_split_bf16_pair(pb0.z, pb0.w, ph[1][1], pl[1][1]);
      nl_split_bf16_pair(pb1.x, pb1.y, ph[1][2], pl[1][2]);
      nl_split_bf16_pair(pb1.z, pb1.w, ph[1][3], pl[1][3]);
      s2d_layer1_step<X3>(acc, w1hi, w1lo, s, lane, ph, pl);
    }
  }
  // ---- the way back to g_a1 (s2d_bwd.h); the logit's gradient of the lane's two pairs comes from the focal loss and the scores' cotangent
  unsigned hi[2][4][8], lo[2][4][8];
  const S2dBwdStores stores = {a.h1, a.ga2, a.ga1, a.w3part ? a.w3part + (size_t)item * S2D_W3P_LD : nullptr};
  s2d_bwd_chain<EXACT>(
      acc, a.img, a.timg, C, ok, prow, stores, s2d_bwd_hidden + (tid >> 6) * (128 * 64) + lane, lane,
      [&](float (&gl)[2]) {
        const float gloss = a.g_loss ? a.g_loss[0] * a.inv_total : 0.f;
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          gl[t] = 0.f;
          if (ok[t]) {
            const size_t i = (size_t)(n0 + t) * M + m;
            float l, dz, ds;
            s2d_focal(a.logits[i], a.target ? a.target[i] : 0.f, l, dz, ds);
            if (a.target) gl[t] = gloss * dz;
            if (a.g_score) gl[t] += a.g_score[i] * ds;
          }
        }
      },
      [&](int t, int c, const float*& pd0, const float*& pd1) {
        pd0 = a.desc0 + (size_t)(n0 + t) * C;
        pd1 = a.desc1 + (size_t)(mt * 32 + c) * C;
      },
      hi, lo);
  // ---- g_x = W1^T g_a1, 32 channels at a time
  {
    const uint4* w1thi = (const uint4*)(a.timg + T.w1t_hi);
    const uint4* w1tlo = (const uint4*)(a.timg + T.w1t_lo);
    for (int rb = 0; rb < nrb1; ++rb) {
      nl_f32x16 o[2];
      nl_acc_zero(o);
      bwd_mult<X3>(o[0], o[1], hi, lo, w1thi, w1tlo, nrb1, rb, lane);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
          if (ok[t]) bwd_store4(a.gx + prow[t] * C + 32 * rb + 8 * r4 + 4 * hh, o[t], r4);
    }
  }
}

// ------------------------------------------------------------------------------------------ reductions of a chunk
// g_desc0: partial sums of row `blockIdx.x` over the 256-column segment blockIdx.y; thread (c4, sub) adds columns sub, sub + 4, .. of the segment
__global__ __launch_bounds__(256) void s2d_gd0_part_kernel(const float* gx, const float* desc1, int M, int C, int nseg, float* part) {
  __shared__ float4 red[4][64];
  const int c4 = threadIdx.x & 63, sub = threadIdx.x >> 6, row = blockIdx.x, seg = blockIdx.y;
  float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
  if (4 * c4 < C) {
    const int m_end = min(M, seg * 256 + 256);
    for (int m = seg * 256 + sub; m < m_end; m += 4) {
      const float4 g = *(const float4*)(gx + ((size_t)row * M + m) * C + 4 * c4), d = *(const float4*)(desc1 + (size_t)m * C + 4 * c4);
      s.x += g.x * d.x; s.y += g.y * d.y; s.z += g.z * d.z; s.w += g.w * d.w;
    }
  }
  red[sub][c4] = s;
  __syncthreads();
  if (sub == 0 && 4 * c4 < C) {
    const float4 p = red[0][c4], q = red[1][c4], u = red[2][c4], v = red[3][c4];
    *(float4*)(part + ((size_t)row * nseg + seg) * C + 4 * c4) = make_float4((p.x + q.x) + (u.x + v.x), (p.y + q.y) + (u.y + v.y), (p.z + q.z) + (u.z + v.z), (p.w + q.w) + (u.w + v.w));
  }
}
__global__ __launch_bounds__(256) void s2d_gd0_final_kernel(const float* part, int rows, int C, int nseg, float* g_desc0) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * C) return;
  const int row = e / C, c = e - row * C;
  float s = 0.f;
  for (int g = 0; g < nseg; ++g) s += part[((size_t)row * nseg + g) * C + c];
  g_desc0[e] = s;
}
// g_desc1[m] += sum over the chunk's rows, in order
__global__ __launch_bounds__(256) void s2d_gd1_kernel(const float* gx, const float* desc0, int rows, int M, int C, float* g_desc1) {
  const int c4n = C >> 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)M * c4n) return;
  const int m = (int)(e / c4n), c4 = (int)(e - (long long)m * c4n);
  float4 s = *(float4*)(g_desc1 + (size_t)m * C + 4 * c4);
  for (int r = 0; r < rows; ++r) {
    const float4 g = *(const float4*)(gx + ((size_t)r * M + m) * C + 4 * c4), d = *(const float4*)(desc0 + (size_t)r * C + 4 * c4);
    s.x += g.x * d.x; s.y += g.y * d.y; s.z += g.z * d.z; s.w += g.w * d.w;
  }
  *(float4*)(g_desc1 + (size_t)m * C + 4 * c4) = s;
}
// gW3[unit] += the waves' partials, block j = one output (128: gb3): 256 interleaved in-thread sums, then a tree in a fixed order
__global__ __launch_bounds__(256) void s2d_w3_reduce_kernel(const float* part, int items, float* gw3, float* gb3) {
  __shared__ float red[256];
  const int j = blockIdx.x, tid = threadIdx.x;
  float s = 0.f;
  for (int i = tid; i < items; i += 256) s += part[(size_t)i * S2D_W3P_LD + j];
  red[tid] = s;
  __syncthreads();
#pragma unroll
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid != 0) return;
  if (j == 128) { if (gb3) gb3[0] += red[0]; }
  else if (gw3) { const int q = j & 63; gw3[s2d_unit(q >> 4, q & 15, j >> 6)] += red[0]; }
}
__global__ __launch_bounds__(256) void s2d_transpose_kernel(const float* w, int rows, int cols, float* wt) {   // wt[c][r] = w[r][c]
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * cols) return;
  const int c = e / rows, r = e - c * rows;
  wt[e] = w[(size_t)r * cols + c];
}

bool bwd_shape_ok(int64_t N, int64_t M) { return N >= 1 && M >= 1 && M <= (1 << 20) && N <= (1 << 30) && N * M < (1ll << 31); }
int64_t bwd_chunk_rows(int64_t N, int64_t M) {
  const int64_t pairs = N * M < S2D_BWD_SMALL_BELOW ? S2D_BWD_PAIRS_SMALL : S2D_BWD_PAIRS;
  const int64_t r = std::max<int64_t>(2, (pairs / M) & ~(int64_t)1);
  return std::min<int64_t>(r, (N + 1) & ~(int64_t)1);
}
// the shared operand block (s2d_bwd_host.h) for one chunk, then the chunk's g_x and the segment sums of g_desc0
struct BwdWs : S2dMlpBwdWs { size_t gx, gd0part; int64_t rows; int nseg; using S2dMlpBwdWs::S2dMlpBwdWs; };
BwdWs bwd_ws(int64_t N, int64_t M, int C) {
  const int64_t rows = bwd_chunk_rows(N, M);
  const size_t P = (size_t)rows * (size_t)M;
  BwdWs w(P, (size_t)nl_cdiv(M, 32) * (size_t)(rows / 2), C);
  w.rows = rows;
  w.nseg = (int)nl_cdiv(M, 256);
  w.gx = w.take(P * C * 4);
  w.gd0part = w.take((size_t)w.rows * w.nseg * C * 4);
  return w;
}

}  // namespace

int nl_launch_s2d_w3_reduce(const float* part, int items, float* gw3, float* gb3, hipStream_t st) {
  hipLaunchKernelGGL(s2d_w3_reduce_kernel, dim3(129), dim3(256), 0, st, part, items, gw3, gb3);
  NL_LAUNCH_CHECK();
  return NL_OK;
}
int nl_launch_transpose(const float* w, int rows, int cols, float* wt, hipStream_t st) {
  hipLaunchKernelGGL(s2d_transpose_kernel, dim3((unsigned)nl_cdiv((int64_t)rows * cols, 256)), dim3(256), 0, st, w, rows, cols, wt);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

extern "C" {

size_t nl_s2d_train_weights_bytes(int C) { return s2d_c_ok(C) ? s2d_train_layout(C).total : 0; }

int nl_s2d_pack_train_weights(int C, const float* w1, const float* w2, void* packed, size_t packed_bytes, void* stream) {
  if (!s2d_c_ok(C)) return C > 0 ? NL_ERR_UNSUPPORTED : NL_ERR_BAD_ARG;
  if (!w1 || !w2 || !packed) return NL_ERR_BAD_ARG;
  if (((uintptr_t)packed & 15) != 0 || (((uintptr_t)w1 | (uintptr_t)w2) & 3) != 0) return NL_ERR_BAD_ARG;
  const S2dTrainLayout T = s2d_train_layout(C);
  if (packed_bytes < T.total) return NL_ERR_WORKSPACE;
  unsigned char* img = (unsigned char*)packed;
  hipStream_t st = (hipStream_t)stream;
  float* w2t = (float*)(img + T.f32w2t);
  float* w1t = (float*)(img + T.f32w1t);
  if (const int e = nl_launch_transpose(w2, S2D_H, S2D_H, w2t, st)) return e;
  if (const int e = nl_launch_transpose(w1, S2D_H, C, w1t, st)) return e;
  auto u16 = [&](size_t off) { return (unsigned short*)(img + off); };
  if (const int e = nl_launch_frag_pack(w2t, S2D_H, S2D_H, u16(T.w2t_hi), u16(T.w2t_lo), nullptr, nullptr, nullptr, true, st)) return e;
  if (const int e = nl_launch_frag_pack(w1t, C, S2D_H, u16(T.w1t_hi), u16(T.w1t_lo), nullptr, nullptr, nullptr, true, st)) return e;
  return NL_OK;
}

size_t nl_s2d_backward_train_workspace_bytes(int64_t N, int64_t M, int C) {
  if (!s2d_c_ok(C) || !bwd_shape_ok(N, M)) return 0;
  return bwd_ws(N, M, C).total;
}

int nl_s2d_backward_train(const void* packed, const void* train_packed, int C, int precision, const float* desc0, int64_t N, const float* desc1, int64_t M,
                          const float* logits, const float* target, const float* g_loss, const float* g_score, float* g_desc0, float* g_desc1, float* g_w1,
                          float* g_b1, float* g_w2, float* g_b2, float* g_w3, float* g_b3, void* workspace, size_t workspace_bytes, void* stream) {
  if (N < 1 || M < 1 || C < 1) return NL_ERR_BAD_ARG;
  if (!s2d_c_ok(C) || !bwd_shape_ok(N, M)) return NL_ERR_UNSUPPORTED;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (!packed || !train_packed || !desc0 || !desc1 || !logits || !g_desc0 || !g_desc1) return NL_ERR_BAD_ARG;
  if ((target != nullptr) != (g_loss != nullptr)) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)packed | (uintptr_t)train_packed | (uintptr_t)desc0 | (uintptr_t)desc1 | (uintptr_t)g_desc0 | (uintptr_t)g_desc1) & 15) != 0) return NL_ERR_BAD_ARG;
  const S2dMlpGrads g{g_w1, g_b1, g_w2, g_b2, g_w3, g_b3};
  if ((((uintptr_t)logits | (uintptr_t)target | (uintptr_t)g_loss | (uintptr_t)g_score | g.addr_bits()) & 3) != 0) return NL_ERR_BAD_ARG;
  const BwdWs w = bwd_ws(N, M, C);
  if (!workspace || workspace_bytes < w.total || ((uintptr_t)workspace & 15) != 0) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;

  NL_CHECK_HIP(hipMemsetAsync(g_desc1, 0, (size_t)M * C * 4, st));
  if (const int e = s2d_mlp_grads_zero(g, C, st)) return e;

  BwdArgs a;
  a.img = (const unsigned char*)packed; a.timg = (const unsigned char*)train_packed;
  a.desc0 = desc0; a.desc1 = desc1;
  a.logits = logits; a.target = target; a.g_loss = g_loss; a.g_score = g_score;
  w.operands(ws, g, a.x, a.ga1, a.h1, a.ga2);
  a.gx = (float*)(ws + w.gx);
  a.w3part = g.want3() ? (float*)(ws + w.w3part) : nullptr;
  a.N = (int)N; a.M = (int)M; a.C = C;
  a.inv_total = (float)(1.0 / ((double)N * (double)M));
  float* wg = (float*)(ws + w.wg);
  float* dummy = (float*)(ws + w.dummy);
  float* gd0part = (float*)(ws + w.gd0part);
  const int MT = (int)nl_cdiv(M, 32);
  static std::atomic<unsigned long long> lds_set{0};

  for (int64_t r0 = 0; r0 < N; r0 += w.rows) {
    const int64_t r1 = std::min(N, r0 + w.rows);
    const int rows = (int)(r1 - r0);
    const int64_t P = (int64_t)rows * M;
    a.r0 = (int)r0; a.r1 = (int)r1;
    const int items = MT * ((rows + 1) / 2);
    const dim3 grid((unsigned)nl_cdiv(items, 4));
    if (const int e = s2d_mlp_bwd_launch(s2d_bwd_kernel<true>, s2d_bwd_kernel<false>, grid, a, precision, lds_set, st)) return e;
    if (const int e = s2d_mlp_wgrad(a.x, a.ga1, a.h1, a.ga2, C, P, g, dummy, wg, w.wg_floats, st)) return e;
    if (g.want3()) {
      hipLaunchKernelGGL(s2d_w3_reduce_kernel, dim3(129), dim3(256), 0, st, a.w3part, items, g_w3, g_b3);
      NL_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(s2d_gd0_part_kernel, dim3(rows, w.nseg), dim3(256), 0, st, a.gx, desc1, (int)M, C, w.nseg, gd0part);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(s2d_gd0_final_kernel, dim3((unsigned)nl_cdiv((int64_t)rows * C, 256)), dim3(256), 0, st, gd0part, rows, C, w.nseg, g_desc0 + (size_t)r0 * C);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(s2d_gd1_kernel, dim3((unsigned)nl_cdiv(M * (C >> 2), 256)), dim3(256), 0, st, a.gx, desc0 + (size_t)r0 * C, rows, (int)M, C, g_desc1);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

}  // extern "C"
