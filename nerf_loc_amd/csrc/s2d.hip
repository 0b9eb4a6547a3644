// Sparse-to-dense coarse matcher (reference: models/matching/sparse_to_dense.py:80-151): for N sparse 3-D descriptors and M dense 2-D descriptors, both C wide,
//   score[n, m] = sigmoid( W3 . relu( W2 . relu( W1 . (desc0[n] * desc1[m]) + b1 ) + b2 ) + b3 )          (C -> 128 -> 128 -> 1)
// then the mutual-nearest selection on those scores.  Nothing of size N x M x anything but the N x M scores is written.
//
// Score kernel (transposed form, as tgemm.hip: D[hidden unit][pair] = W . X): a wave owns 32 columns m and TWO rows n (two 32-pair column tiles that share every
// weight fragment and every desc1 load); the product rows x = desc0[n] * desc1[m] are built in registers per 16-wide k-step and split to bf16 hi / lo; layer 1's
// accumulators (4 x 32 hidden units x 32 pairs per tile) become layer 2's B operand without leaving the lane: layer 2's K order inside every 32-block is the
// accumulator order (k-step s of block b takes accumulator registers 8 s .. 8 s + 7), the weights are packed to match.  The last 128 -> 1 layer is an in-lane dot
// over the lane's 64 hidden units plus the other half-wave's 64.
// Weights: one packed image (nl_s2d_pack_weights; s2d.h: s2d_layout) of A fragments in lane order (mfma.h's fragment maps: 16 B per lane, 1 KiB per fragment).  The hi planes of W1 and W2, the lo plane of W2
// and the bias / W3 tables are copied to LDS once per workgroup (112 KiB at C = 192, 128 KiB at C = 256) by a persistent grid; the lo plane of W1 (48 .. 64 KiB) does
// not fit next to them and is read from L2, where every workgroup reads the same bytes.  NL_PREC_F32 reads a second, fp32 fragment image (v_mfma_f32_32x32x2_f32) from L2.
// The value of a pair depends on its two descriptor rows, the weights and the mode only: each output column of an MFMA is an independent dot product in a fixed
// order, the cross-half sum of the last layer is commutative, and no float atomic touches a value.
// Selection: the score kernel reduces rowmax[N] / colmax[M] with unsigned atomic max on the float bits (scores are >= 0); pass 2, one wave per row, finds the FIRST j
// with s > thr, s == rowmax[i], s == colmax[j] — the reference's rule on the scores themselves, ties included.
#include <algorithm>
#include "common.h"
#include "mfma.h"
#include "s2d.h"
#include "host.h"

namespace {

constexpr int S2D_NROWS = 32;              // rows n of one work item (4 waves x 2 rows x 4 iterations)

// ------------------------------------------------------------------------------------------ packing
// The image's matrices are packed by pack.hip's nl_launch_frag_pack (W2's 16-bit planes in accumulator order); what is left is the 2-KB table of the last
// layers: b1p / b2p / w3p [hh][16 b + r] in accumulator order, then b3 and zero padding
__global__ __launch_bounds__(256) void s2d_pack_small_kernel(const float* b1, const float* b2, const float* w3, const float* b3, float* small) {
  const int e = blockIdx.x * 256 + threadIdx.x;   // < S2D_SMALL_BYTES / 4: the launch is two blocks
  float v = 0.f;
  if (e < 384) {
    const int which = e >> 7, q = e & 127, hh = q >> 6, b = (q >> 4) & 3, r = q & 15;
    const float* src = which == 0 ? b1 : (which == 1 ? b2 : w3);
    v = src[s2d_unit(b, r, hh)];
  } else if (e == 384) {
    v = b3[0];
  }
  small[e] = v;
}

// ------------------------------------------------------------------------------------------ scores
struct S2dArgs {
  const unsigned char* img;
  const float* desc0; const float* desc1;
  float* scores;
  float* logits;   // (N,M) or null: the training forward keeps them for the loss and the backward pass (s2d_bwd.hip)
  unsigned* rowmax; unsigned* colmax;
  int N, M, C;
};

// bias + ReLU + last layer + sigmoid + stores + maxima, shared by the two score kernels.  acc[t][b]: tile t (row n0 + t), hidden 32-block b.
__device__ __forceinline__ void s2d_finish(const S2dArgs& a, const float* small, const nl_f32x16 (&acc)[2][4], int lane, int n0, bool has1, int m, unsigned& colmax) {
  const int hh = lane >> 5;
  float logit[2];
  s2d_logits(acc, small, hh, logit);
  const float sc[2] = {nl_sigmoid(logit[0]), nl_sigmoid(logit[1])};
  const bool mok = m < a.M;
  const bool ok0 = mok, ok1 = mok && has1;
  const unsigned u0 = ok0 ? __float_as_uint(sc[0]) : 0u, u1 = ok1 ? __float_as_uint(sc[1]) : 0u;
  colmax = max(colmax, max(u0, u1));
  // half-wave hh stores tile hh: 32 consecutive floats of row n0 + hh
  const bool okm = hh ? ok1 : ok0;
  const float mine = hh ? sc[1] : sc[0];
  const int nm = n0 + hh;
  if (okm) a.scores[(size_t)nm * a.M + m] = mine;
  if (a.logits && okm) a.logits[(size_t)nm * a.M + m] = hh ? logit[1] : logit[0];
  unsigned rm = okm ? __float_as_uint(mine) : 0u;   // scores are >= 0: the order of the bits is the order of the values
#pragma unroll
  for (int o = 16; o >= 1; o >>= 1) rm = max(rm, (unsigned)__shfl_xor((int)rm, o));
  if ((lane & 31) == 0 && (hh == 0 || has1)) atomicMax(a.rowmax + nm, rm);
}

template <bool X3>
__global__ __launch_bounds__(256) void s2d_bf16_kernel(const S2dArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char s2d_lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
  const int C = a.C, nk1 = C >> 4;
  const S2dLayout L = s2d_layout(C);
  {
    const uint4* src = (const uint4*)a.img;
    uint4* dst = (uint4*)s2d_lds;
    const int n16 = (int)(L.lds_bytes >> 4);
    for (int i = tid; i < n16; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  const uint4* w1hi = (const uint4*)(s2d_lds + L.w1hi);
  const uint4* w2hi = (const uint4*)(s2d_lds + L.w2hi);
  const uint4* w2lo = (const uint4*)(s2d_lds + L.w2lo);
  const float* small = (const float*)(s2d_lds + L.small);
  const uint4* w1lo = (const uint4*)(a.img + L.w1lo);
  const float* b1p = small + 64 * hh;

  const int MT = (a.M + 31) >> 5, NB = (a.N + S2D_NROWS - 1) / S2D_NROWS;
  const long long items = (long long)MT * NB;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int mt = (int)(item / NB), nb = (int)(item - (long long)mt * NB);
    const int m = mt * 32 + (lane & 31);
    const float* d1p = a.desc1 + (size_t)min(m, a.M - 1) * C + 8 * hh;
    unsigned colmax = 0u;
    for (int it = 0; it < S2D_NROWS / 8; ++it) {
      const int n0 = nb * S2D_NROWS + it * 8 + wave * 2;
      if (n0 >= a.N) break;   // wave-uniform; no barrier inside the item loop
      const bool has1 = n0 + 1 < a.N;
      const float* d0a = a.desc0 + (size_t)n0 * C + 8 * hh;
      const float* d0b = a.desc0 + (size_t)(has1 ? n0 + 1 : n0) * C + 8 * hh;

      nl_f32x16 acc[2][4];
      nl_acc_zero(acc);

      // ---- layer 1: K = C, the B operand built per k-step from desc1 (shared by both tiles) and the two desc0 rows
      for (int s = 0; s < nk1; ++s) {
        const float4 x0 = *(const float4*)(d1p + 16 * s), x1 = *(const float4*)(d1p + 16 * s + 4);
        const float4 ya0 = *(const float4*)(d0a + 16 * s), ya1 = *(const float4*)(d0a + 16 * s + 4);
        const float4 yb0 = *(const float4*)(d0b + 16 * s), yb1 = *(const float4*)(d0b + 16 * s + 4);
        unsigned ph[2][4], pl[2][4];
        nl_split_bf16_pair(x0.x * ya0.x, x0.y * ya0.y, ph[0][0], pl[0][0]);
        nl_split_bf16_pair(x0.z * ya0.z, x0.w * ya0.w, ph[0][1], pl[0][1]);
        nl_split_bf16_pair(x1.x * ya1.x, x1.y * ya1.y, ph[0][2], pl[0][2]);
        nl_split_bf16_pair(x1.z * ya1.z, x1.w * ya1.w, ph[0][3], pl[0][3]);
        nl_split_bf16_pair(x0.x * yb0.x, x0.y * yb0.y, ph[1][0], pl[1][0]);
        nl_split_bf16_pair(x0.z * yb0.z, x0.w * yb0.w, ph[1][1], pl[1][1]);
        nl_split_bf16_pair(x1.x * yb1.x, x1.y * yb1.y, ph[1][2], pl[1][2]);
        nl_split_bf16_pair(x1.z * yb1.z, x1.w * yb1.w, ph[1][3], pl[1][3]);
        s2d_layer1_step<X3>(acc, w1hi, w1lo, s, lane, ph, pl);
      }
      s2d_layer2<X3>(acc, b1p, w2hi, w2lo, lane);

      s2d_finish(a, small, acc, lane, n0, has1, m, colmax);
    }
    if (hh == 0 && m < a.M && colmax != 0u) atomicMax(a.colmax + m, colmax);
  }
}

// NL_PREC_F32: the same walk with v_mfma_f32_32x32x2_f32; half-wave hh supplies k slot hh of every step.  Layer 1 takes 8 channels per group (a float4 of desc1 per
// half-wave: step t of group g multiplies channel 8 g + 4 hh + t), layer 2's step t of block b takes accumulator register t.  Weight fragments come from L2 / L1.
__global__ __launch_bounds__(256) void s2d_f32_kernel(const S2dArgs a) {
  __shared__ __attribute__((aligned(16))) float small[S2D_SMALL_BYTES / 4];
  extern __shared__ __attribute__((aligned(16))) float hidden[];   // S2D_F32_LDS bytes
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
  const int C = a.C, ng = C >> 3;
  const S2dLayout L = s2d_layout(C);
  for (int i = tid; i < S2D_SMALL_BYTES / 4; i += 256) small[i] = ((const float*)(a.img + L.small))[i];
  __syncthreads();
  const float* w1f = (const float*)(a.img + L.f32w1);
  const float* w2f = (const float*)(a.img + L.f32w2);
  const float* b1p = small + 64 * hh;
  float* hbuf = hidden + wave * (128 * 64) + lane;   // [2 tiles x 64 values][64 lanes] per wave: only this lane reads what it wrote

  const int MT = (a.M + 31) >> 5, NB = (a.N + S2D_NROWS - 1) / S2D_NROWS;
  const long long items = (long long)MT * NB;
  for (long long item = blockIdx.x; item < items; item += gridDim.x) {
    const int mt = (int)(item / NB), nb = (int)(item - (long long)mt * NB);
    const int m = mt * 32 + (lane & 31);
    const float* d1p = a.desc1 + (size_t)min(m, a.M - 1) * C + 4 * hh;
    unsigned colmax = 0u;
    for (int it = 0; it < S2D_NROWS / 8; ++it) {
      const int n0 = nb * S2D_NROWS + it * 8 + wave * 2;
      if (n0 >= a.N) break;
      const bool has1 = n0 + 1 < a.N;
      const float* d0a = a.desc0 + (size_t)n0 * C + 4 * hh;
      const float* d0b = a.desc0 + (size_t)(has1 ? n0 + 1 : n0) * C + 4 * hh;

      nl_f32x16 acc[2][4];
      nl_acc_zero(acc);

      for (int g = 0; g < ng; ++g) {
        const float4 x = *(const float4*)(d1p + 8 * g), ya = *(const float4*)(d0a + 8 * g), yb = *(const float4*)(d0b + 8 * g);
        const float pa[4] = {x.x * ya.x, x.y * ya.y, x.z * ya.z, x.w * ya.w};
        const float pb[4] = {x.x * yb.x, x.y * yb.y, x.z * yb.z, x.w * yb.w};
        s2d_f32_layer1_group(acc, w1f, g, lane, pa, pb);
      }
      s2d_f32_layer2(acc, b1p, hbuf, w2f, lane);

      s2d_finish(a, small, acc, lane, n0, has1, m, colmax);
    }
    if (hh == 0 && m < a.M && colmax != 0u) atomicMax(a.colmax + m, colmax);
  }
}

// ------------------------------------------------------------------------------------------ selection
// one wave per row: the first column j with s > thr, s == rowmax[i], s == colmax[j] (sparse_to_dense.py:136-142 on the kernel's own scores)
__global__ __launch_bounds__(256) void s2d_select_kernel(const float* scores, const unsigned* rowmax, const unsigned* colmax, int N, int M, float thr,
                                                         int32_t* match_j, float* match_score) {
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  const unsigned rm = rowmax[n];
  int found = -1;
  if (__uint_as_float(rm) > thr) {
    const float* row = scores + (size_t)n * M;
    for (int j0 = 0; j0 < M; j0 += 64) {
      const int j = j0 + lane;
      bool hit = false;
      if (j < M) {
        const unsigned s = __float_as_uint(row[j]);
        hit = s == rm && s == colmax[j];
      }
      const unsigned long long bal = __ballot(hit);
      if (bal) { found = j0 + __builtin_ctzll(bal); break; }
    }
  }
  if (lane == 0) {
    match_j[n] = found;
    match_score[n] = found >= 0 ? __uint_as_float(rm) : 0.f;
  }
}


// ------------------------------------------------------------------------------------------ loss (training forward)
// mean sigmoid focal loss over N * M logits in a fixed order: block b adds elements b * 256 + tid + k * nblk * 256 in-thread, then a tree over the block; a second, single
// block adds the nblk partials the same way.  nblk depends on N * M only, so the order does not depend on the device.
constexpr int S2D_LOSS_MAX_BLOCKS = 1024;
__device__ __forceinline__ float s2d_block_sum(float v, float* red) {
  const int tid = threadIdx.x;
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o >= 1; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  return red[0];
}
__global__ __launch_bounds__(256) void s2d_loss_part_kernel(const float* logits, const float* target, long long total, float* part) {
  __shared__ float red[256];
  float s = 0.f;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    float l, dz, ds;
    s2d_focal(logits[i], target[i], l, dz, ds);
    s += l;
  }
  const float v = s2d_block_sum(s, red);
  if (threadIdx.x == 0) part[blockIdx.x] = v;
}
__global__ __launch_bounds__(256) void s2d_loss_final_kernel(const float* part, int nblk, float inv_total, float* loss) {
  __shared__ float red[256];
  float s = 0.f;
  for (int i = threadIdx.x; i < nblk; i += 256) s += part[i];
  const float v = s2d_block_sum(s, red);
  if (threadIdx.x == 0) loss[0] = v * inv_total;
}

struct S2dWs { size_t rowmax, colmax, scores, total; };
S2dWs s2d_ws(int64_t N, int64_t M, bool want_scores) {
  S2dWs w;
  w.rowmax = 0;
  w.colmax = nl_align_up((size_t)N * 4, 256);
  w.scores = w.colmax + nl_align_up((size_t)M * 4, 256);
  w.total = w.scores + (want_scores ? 0 : nl_align_up((size_t)N * (size_t)M * 4, 256));
  return w;
}
bool s2d_shape_ok(int64_t N, int64_t M) { return N >= 1 && M >= 1 && N <= (1 << 30) && M <= (1 << 30); }

}  // namespace

// nl_s2d_match, and with logits_out the first half of nl_s2d_forward_train: the same kernels, scores and selection
static int s2d_run(const void* packed, int C, int precision, const float* desc0, int64_t N, const float* desc1, int64_t M, float thr, float* scores_out,
                   float* logits_out, int32_t* match_j, float* match_score, void* workspace, size_t workspace_bytes, void* stream) {
  if (N < 1 || M < 1 || C < 1) return NL_ERR_BAD_ARG;
  if (!s2d_c_ok(C) || !s2d_shape_ok(N, M)) return NL_ERR_UNSUPPORTED;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (!packed || !desc0 || !desc1 || !match_j || !match_score) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)packed | (uintptr_t)desc0 | (uintptr_t)desc1) & 15) != 0) return NL_ERR_BAD_ARG;   // read as 16-byte pieces
  if ((((uintptr_t)scores_out | (uintptr_t)logits_out | (uintptr_t)match_j | (uintptr_t)match_score) & 3) != 0) return NL_ERR_BAD_ARG;
  const S2dWs w = s2d_ws(N, M, scores_out != nullptr);
  if (!workspace || workspace_bytes < w.total || ((uintptr_t)workspace & 15) != 0) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  S2dArgs a;
  a.img = (const unsigned char*)packed;
  a.desc0 = desc0; a.desc1 = desc1;
  a.scores = scores_out ? scores_out : (float*)(ws + w.scores);
  a.logits = logits_out;
  a.rowmax = (unsigned*)(ws + w.rowmax);
  a.colmax = (unsigned*)(ws + w.colmax);
  a.N = (int)N; a.M = (int)M; a.C = C;
  const int cus = nl_persistent_cus();
  if (cus < 0) return cus;
  NL_CHECK_HIP(hipMemsetAsync(ws, 0, w.scores, st));
  const int64_t items = nl_cdiv(M, 32) * nl_cdiv(N, S2D_NROWS);
  const unsigned grid = (unsigned)(items < cus ? items : cus);
  // dynamic LDS beyond 64 KB: each kernel's limit is raised once per device to what the largest supported C needs; a launch asks for its own size
  static std::atomic<unsigned long long> f32_set{0}, x3_set{0}, bf_set{0};
  if (precision == NL_PREC_F32) {
    if (const int e = nl_allow_dynamic_lds((const void*)s2d_f32_kernel, S2D_F32_LDS, f32_set)) return e;
    hipLaunchKernelGGL(s2d_f32_kernel, dim3(grid), dim3(256), S2D_F32_LDS, st, a);
  } else {
    const size_t lds = s2d_layout(C).lds_bytes, lds_max = s2d_layout(256).lds_bytes;
    if (precision == NL_PREC_BF16X3) {
      if (const int e = nl_allow_dynamic_lds((const void*)s2d_bf16_kernel<true>, lds_max, x3_set)) return e;
      hipLaunchKernelGGL(s2d_bf16_kernel<true>, dim3(grid), dim3(256), lds, st, a);
    } else {
      if (const int e = nl_allow_dynamic_lds((const void*)s2d_bf16_kernel<false>, lds_max, bf_set)) return e;
      hipLaunchKernelGGL(s2d_bf16_kernel<false>, dim3(grid), dim3(256), lds, st, a);
    }
  }
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(s2d_select_kernel, dim3((unsigned)nl_cdiv(N, 4)), dim3(256), 0, st, a.scores, a.rowmax, a.colmax, (int)N, (int)M, thr, match_j, match_score);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

extern "C" {

size_t nl_s2d_packed_weights_bytes(int C) { return s2d_c_ok(C) ? s2d_layout(C).total : 0; }

int nl_s2d_pack_weights(int C, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, void* packed,
                        size_t packed_bytes, void* stream) {
  if (!s2d_c_ok(C)) return C > 0 ? NL_ERR_UNSUPPORTED : NL_ERR_BAD_ARG;
  if (!w1 || !b1 || !w2 || !b2 || !w3 || !b3 || !packed) return NL_ERR_BAD_ARG;
  if (((uintptr_t)packed & 15) != 0) return NL_ERR_BAD_ARG;
  if (packed_bytes < s2d_layout(C).total) return NL_ERR_WORKSPACE;
  const S2dLayout L = s2d_layout(C);
  unsigned char* img = (unsigned char*)packed;
  hipStream_t st = (hipStream_t)stream;
  auto u16 = [&](size_t off) { return (unsigned short*)(img + off); };
  if (const int e = nl_launch_frag_pack(w1, S2D_H, C, u16(L.w1hi), u16(L.w1lo), u16(L.h1hi), u16(L.h1lo), (float*)(img + L.f32w1), false, st)) return e;
  if (const int e = nl_launch_frag_pack(w2, S2D_H, S2D_H, u16(L.w2hi), u16(L.w2lo), u16(L.h2hi), u16(L.h2lo), (float*)(img + L.f32w2), true, st)) return e;
  hipLaunchKernelGGL(s2d_pack_small_kernel, dim3(S2D_SMALL_BYTES / 4 / 256), dim3(256), 0, st, b1, b2, w3, b3, (float*)(img + L.small));
  NL_LAUNCH_CHECK();
  return NL_OK;
}

size_t nl_s2d_min_workspace_bytes(int64_t N, int64_t M, int C, int want_scores) {
  if (!s2d_c_ok(C) || !s2d_shape_ok(N, M)) return 0;
  return s2d_ws(N, M, want_scores != 0).total;
}

int nl_s2d_match(const void* packed, int C, int precision, const float* desc0, int64_t N, const float* desc1, int64_t M, float thr, float* scores_out,
                 int32_t* match_j, float* match_score, void* workspace, size_t workspace_bytes, void* stream) {
  return s2d_run(packed, C, precision, desc0, N, desc1, M, thr, scores_out, nullptr, match_j, match_score, workspace, workspace_bytes, stream);
}

size_t nl_s2d_forward_train_workspace_bytes(int64_t N, int64_t M, int C) {
  if (!s2d_c_ok(C) || !s2d_shape_ok(N, M)) return 0;
  return s2d_ws(N, M, true).total + S2D_LOSS_MAX_BLOCKS * sizeof(float);
}

int nl_s2d_forward_train(const void* packed, int C, int precision, const float* desc0, int64_t N, const float* desc1, int64_t M, float thr, const float* target,
                         float* scores_out, float* logits_out, float* loss_out, int32_t* match_j, float* match_score, void* workspace, size_t workspace_bytes,
                         void* stream) {
  if (N < 1 || M < 1 || C < 1) return NL_ERR_BAD_ARG;
  if (!s2d_c_ok(C) || !s2d_shape_ok(N, M)) return NL_ERR_UNSUPPORTED;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (!packed || !desc0 || !desc1 || !match_j || !match_score || !scores_out || !logits_out || (target != nullptr) != (loss_out != nullptr)) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)target | (uintptr_t)loss_out) & 3) != 0) return NL_ERR_BAD_ARG;
  const size_t match_bytes = s2d_ws(N, M, true).total;
  if (!workspace || workspace_bytes < match_bytes + S2D_LOSS_MAX_BLOCKS * sizeof(float) || ((uintptr_t)workspace & 15) != 0) return NL_ERR_WORKSPACE;
  if (const int e = s2d_run(packed, C, precision, desc0, N, desc1, M, thr, scores_out, logits_out, match_j, match_score, workspace, match_bytes, stream)) return e;
  if (target) {
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)((unsigned char*)workspace + match_bytes);
    const long long total = (long long)N * M;
    const int nblk = (int)std::min<int64_t>(S2D_LOSS_MAX_BLOCKS, nl_cdiv(total, 1024));
    hipLaunchKernelGGL(s2d_loss_part_kernel, dim3(nblk), dim3(256), 0, st, logits_out, target, total, part);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(s2d_loss_final_kernel, dim3(1), dim3(256), 0, st, part, nblk, (float)(1.0 / (double)total), loss_out);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

}  // extern "C"
