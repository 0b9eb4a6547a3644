// What the SelfCrossTransformer forward (sct.hip) and its training step (sct_bwd.hip) share: the layout of the packed image and of the module's parameters, the
// argument blocks of the three forward kernels, the operand helpers of the MFMA products (sct_load8, sct_split8, sct_mfma, sct_gemm),
// the row chain — one kernel for inference, the training forward and the training forward with dropout — and the host-side limits, argument checks and launch
// helpers.  Include after common.h and mfma.h.
#pragma once
#include <type_traits>
#include "common.h"
#include "mfma.h"
#include "host.h"
#include "sct_drop.h"

namespace {

constexpr int SCT_HEADS = 8, SCT_LAYERS = 4, SCT_TENSORS = 52;
constexpr int SCT_PAD = 4;   // floats between LDS rows
constexpr float SCT_EPS = 1e-5f;
enum { SCT_F32 = 0, SCT_X3 = 1, SCT_BF = 2 };   // = NL_PREC_F32 / NL_PREC_BF16X3 / NL_PREC_BF16

// ------------------------------------------------------------------------------------------ the module's parameters
// state-dict order: two encoder layers of 12 tensors (in_proj w/b, out_proj w/b, linear1 w/b, linear2 w/b, norm1 w/b, norm2 w/b), two decoder layers of 14
// (.., norm1 w/b [constructed, never applied], norm2 w/b, norm3 w/b).  Layers 0..3 in forward order; k: a tensor's index inside its layer.
constexpr int sct_param_first(int l) { return l < 2 ? 12 * l : 14 * l - 4; }   // 0, 12, 24, 38
constexpr int sct_param_count(int l) { return l < 2 ? 12 : 14; }
constexpr int sct_param_norm(int l) { return l < 2 ? 8 : 10; }   // first of the four LayerNorm tensors the layer applies
inline bool sct_param_applied(int l, int k) { return k < 8 || k >= sct_param_norm(l); }
inline size_t sct_param_floats(int k, int C, int F) {
  const size_t n[8] = {(size_t)3 * C * C, (size_t)3 * C, (size_t)C * C, (size_t)C, (size_t)F * C, (size_t)F, (size_t)C * F, (size_t)C};
  return k < 8 ? n[k] : (size_t)C;
}
inline float sct_scale(int C) { return (float)(1.0 / sqrt((double)(C / SCT_HEADS))); }   // of the logits: 1 / sqrt(head dimension)

// ------------------------------------------------------------------------------------------ packed image
// per layer: in_proj_weight (3C x C), out_proj.weight (C x C), linear1.weight (F x C), linear2.weight (C x F), each as four planes — fp16 hi, fp16 lo, bf16 and fp32,
// in mfma.h's fragment maps (nl_frag16_src / nl_frag32_src; written by pack.hip's nl_launch_frag_pack) — then the vectors: in_proj_bias (3C), out_proj.bias (C), linear1.bias (F), linear2.bias (C), first norm weight / bias, second norm weight / bias (C each).
struct SctW { const uint4* hi; const uint4* lo; const uint4* bf; const float* f32; int nrb; };
struct SctMatOff { size_t hi, lo, bf, f32; };
struct SctLayerOff { SctMatOff m[4]; size_t vec; };
struct SctLayout { SctLayerOff l[SCT_LAYERS]; size_t total; };

inline SctLayout sct_layout(int C, int F) {
  SctLayout L;
  size_t o = 0;
  for (int i = 0; i < SCT_LAYERS; ++i) {
    const size_t n[4] = {(size_t)3 * C * C, (size_t)C * C, (size_t)F * C, (size_t)C * F};
    for (int k = 0; k < 4; ++k) {
      L.l[i].m[k].hi = o; o += n[k] * 2;
      L.l[i].m[k].lo = o; o += n[k] * 2;
      L.l[i].m[k].bf = o; o += n[k] * 2;
      L.l[i].m[k].f32 = o; o += n[k] * 4;
    }
    L.l[i].vec = o; o += (size_t)(9 * C + F) * 4;
  }
  L.total = o;
  return L;
}
inline SctW sct_mat(const unsigned char* img, const SctMatOff& m, int N) {
  return SctW{(const uint4*)(img + m.hi), (const uint4*)(img + m.lo), (const uint4*)(img + m.bf), (const float*)(img + m.f32), N >> 5};
}

// ------------------------------------------------------------------------------------------ operand helpers
__device__ __forceinline__ void sct_load8(const float* p, float (&v)[8]) {
  const float4 a = *(const float4*)p, b = *(const float4*)(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w; v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
// 8 values -> the 16-bit fragment(s) of the mode: split-FP16 hi / lo (SCT_X3) or bf16 (SCT_BF; lo unused)
template <int MODE>
__device__ __forceinline__ void sct_split8(const float (&v)[8], nl_i16x8& hi, nl_i16x8& lo) {
  unsigned h[4], l[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if constexpr (MODE == SCT_X3) nl_split_pair<true>(v[2 * t], v[2 * t + 1], h[t], l[t]);
    else h[t] = nl_bf16_pair(v[2 * t], v[2 * t + 1]);
  }
  hi = nl_frag(h[0], h[1], h[2], h[3]);
  lo = nl_frag(l[0], l[1], l[2], l[3]);
}
// acc += a . b: three terms, small ones first (SCT_X3), or the one bf16 product
template <int MODE>
__device__ __forceinline__ nl_f32x16 sct_mfma(const nl_i16x8 ah, const nl_i16x8 al, const nl_i16x8 bh, const nl_i16x8 bl, nl_f32x16 acc) {
  if constexpr (MODE == SCT_X3) {
    acc = nl_mfma<true>(al, bh, acc);
    acc = nl_mfma<true>(ah, bl, acc);
  }
  return nl_mfma<MODE == SCT_X3>(ah, bh, acc);
}

// acc[i] += X[32 rows][K] . W[rows 32 rb .. 32 rb + 31][K]^T for the wave's output blocks rb = rbs + 4 i < rbe.  xrow: the lane's row (lane & 31) of the LDS tile.
// Accumulator register r of half-wave hh is row nl_acc_row(r, hh); the lane's column is output 32 rb + (lane & 31).
template <int MODE, int NB>
__device__ __forceinline__ void sct_gemm(nl_f32x16 (&acc)[NB], const float* xrow, int K, const SctW& w, int rbs, int rbe, int lane) {
  const int hh = lane >> 5;
  if constexpr (MODE == SCT_F32) {
    for (int g = 0; g < (K >> 3); ++g) {
      const float4 v = *(const float4*)(xrow + 8 * g + 4 * hh);
      const float x[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
      for (int t = 0; t < 4; ++t)
#pragma unroll
        for (int i = 0; i < NB; ++i) {
          const int rb = rbs + 4 * i;
          if (rb < rbe) acc[i] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[t], w.f32[((size_t)(g * 4 + t) * w.nrb + rb) * 64 + lane], acc[i], 0, 0, 0);
        }
    }
  } else {
    const uint4* whi = MODE == SCT_X3 ? w.hi : w.bf;
    for (int s = 0; s < (K >> 4); ++s) {
      float v[8];
      sct_load8(xrow + 16 * s + 8 * hh, v);
      nl_i16x8 ah, al;
      sct_split8<MODE>(v, ah, al);
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const int rb = rbs + 4 * i;
        if (rb < rbe) {
          const size_t f = ((size_t)s * w.nrb + rb) * 64 + lane;
          const nl_i16x8 bh = nl_frag(whi[f]);
          nl_i16x8 bl = bh;
          if constexpr (MODE == SCT_X3) bl = nl_frag(w.lo[f]);
          acc[i] = sct_mfma<MODE>(ah, al, bh, bl, acc[i]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ argument blocks of the forward kernels
struct SctProjArgs {
  const float* x; const float* pos;
  float* out[3];        // q, k, v rows ([rows][C]); only the parts inside [rb_lo, rb_hi) are written
  SctW w; const float* bias;
  long long rows;
  int C, rb_lo, rb_hi;  // output blocks of in_proj_weight: [0, C/32) = q, [C/32, 2C/32) = k, [2C/32, 3C/32) = v
};

struct SctAttnArgs {
  const float* q; const float* k; const float* v; float* out;   // [B][Nq | Nk][C]
  long long Nq, Nk, items;   // items = B * 8 * ceil(Nq / 32)
  int nqt, nkt;              // 32-row query / key tiles
  int lg, tps;               // a workgroup's four waves are (4 >> lg) items x (1 << lg) key ranges of tps tiles each
  float scale;
};

struct SctChainArgs {
  const float* attn; const float* x; float* out;   // out may be x: a workgroup reads its 32 rows of x before it writes them
  SctW wo, w1, w2;
  const float* vec;   // the layer's vectors (layout above)
  long long rows;
  int C, F;
};
inline SctChainArgs sct_chain_args(const unsigned char* img, const SctLayerOff& lo, int C, int F, const float* attn, const float* x, float* out, long long rows) {
  return SctChainArgs{attn, x, out, sct_mat(img, lo.m[1], C), sct_mat(img, lo.m[2], F), sct_mat(img, lo.m[3], C), (const float*)(img + lo.vec), rows, C, F};
}
// what the training forward keeps of the chain ([rows][C] each, rstd [rows][2]): the rows after the first LayerNorm, both LayerNorms' normalised rows and 1 / std,
// and a second copy of the output (null: none) for the layers whose output the in-place forward overwrites
struct SctKeepRows { float *y1, *xa, *xb, *rstd, *out; };
// ... as they reach the kernel: five pointer arguments at the head of its trailing pack (SctNone: the pack has none).  Not the struct: as ONE argument the compiler
// fetches the five in the kernel's prologue and hoists the first LayerNorm's column tests — other device code than the kernel that was measured.
__device__ __forceinline__ SctNone sct_keep_rows() { return SctNone{}; }
template <class... D>
__device__ __forceinline__ SctKeepRows sct_keep_rows(float* y1, float* xa, float* xb, float* rstd, float* out, const D&...) { return SctKeepRows{y1, xa, xb, rstd, out}; }

// ------------------------------------------------------------------------------------------ post-attention row chain
// LayerNorm of the wave's 8 rows of the LDS tile.  which 0, the first (dst null without KEEP): in place; 1, the second: to the output rows dst.  KEEP: the
// normalised rows go to xn, 1 / std to rs[row][which], and the result also to dst (the first) / dst2 (the second) where given.
// The chain kernels' device code follows small things here; three lines (marked) keep what each of the two functions this one replaced had, so that all nine
// kernels stay byte for byte the ones that were measured (tools/kernel_identity.py).  Move one only together with a new measurement.
template <bool KEEP>
__device__ __forceinline__ void sct_layernorm(float* y, int ld, int C, const float* g, const float* bta, int lane, int wave, int which, float* dst, long long row0,
                                              long long rows, float* xn = nullptr, float* rs = nullptr, float* dst2 = nullptr) {
  const int nci = C >> 6;
  for (int rr = 0; rr < 8; ++rr) {
    const int row = 8 * wave + rr;
    bool live = KEEP && row0 + row < rows;   // the row exists.  (marked) KEEP tests it here, before the reductions ...
    float v[4] = {0.f, 0.f, 0.f, 0.f}, s = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nci) { v[i] = y[row * ld + lane + 64 * i]; s += v[i]; }
    const float mean = wave_sum(s) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nci) { v[i] -= mean; sq += v[i] * v[i]; }
    const float rstd = 1.f / sqrtf(wave_sum(sq) / (float)C + SCT_EPS);
    if constexpr (!KEEP) live = row0 + row < rows;   // (marked) ... inference here, behind them: either test at the other place reschedules the second norm
    if constexpr (KEEP)
      if (live && lane == 0) rs[(size_t)(row0 + row) * 2 + which] = rstd;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nci) {
        const int c = lane + 64 * i;
        const float n = v[i] * rstd;
        const float r = n * g[c] + bta[c];
        // (marked) inference tells the first norm by its null dst, a run-time value in the second: told by the compile-time `which`, the second norm loses this
        // branch, the compiler unrolls its row loop and the fp32 kernel grows from 19.9 to 28.4 KB
        if (KEEP ? which == 0 : !dst) {
          y[row * ld + c] = r;
        } else if constexpr (!KEEP) {
          if (live) dst[(size_t)(row0 + row) * C + c] = r;
        }
        if constexpr (KEEP)
          if (live) {
            const size_t e = (size_t)(row0 + row) * C + c;
            xn[e] = n;
            if (dst) dst[e] = r;
            if (dst2) dst2[e] = r;
          }
      }
  }
}

// out_proj, + residual, LayerNorm, linear1, ReLU, linear2, + residual, LayerNorm for a workgroup's 32 rows (sct.hip's header).  EXTRA: nothing (inference), the five
// pointers of SctKeepRows (the training forward: the same expressions in the same order, and the kept rows' stores), or those and an SctDrop: sct_drop.h's sites 1 (out_proj's
// output before the residual), 2 (the ReLU'd hidden rows) and 3 (linear2's output before the residual) on the accumulator registers, which run along the rows — four
// generator calls per 32 x 32 output block and lane.  The kept state has the same layout with and without dropout; no mask is stored.
template <int MODE, class... EXTRA>
__global__ __launch_bounds__(256) void sct_chain_kernel(const SctChainArgs a, const EXTRA... extra) {
  constexpr bool KEEP = sizeof...(EXTRA) >= 5, DROP = sizeof...(EXTRA) == 1 + 5 * KEEP;
  [[maybe_unused]] const auto k = sct_keep_rows(extra...);
  [[maybe_unused]] const auto d = sct_arg<SctDrop>(extra...);
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);
  extern __shared__ __attribute__((aligned(16))) float sct_smem[];
  const int C = a.C, F = a.F, ldc = C + SCT_PAD, ldf = F + SCT_PAD, c4n = C >> 2, nc = C >> 5, nf = F >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long row0 = (long long)blockIdx.x * 32;
  float* y = sct_smem;               // [32][ldc]: the running rows
  float* hb = sct_smem + 32 * ldc;   // [32][ldc] attention output, then [32][ldf] hidden rows
  const float* bo = a.vec + 3 * C;
  const float* b1 = a.vec + 4 * C;
  const float* b2 = b1 + F;
  const float* lnp = b2 + C;   // weight A, bias A, weight B, bias B

  for (int i = threadIdx.x; i < 32 * c4n; i += 256) {
    const int r = i / c4n, c = 4 * (i - r * c4n);
    const long long row = row0 + r < a.rows ? row0 + r : a.rows - 1;
    *(float4*)(hb + r * ldc + c) = *(const float4*)(a.attn + (size_t)row * C + c);
  }
  __syncthreads();
  {   // out_proj + bias + residual
    nl_f32x16 acc[2];
    nl_acc_zero(acc);
    sct_gemm<MODE, 2>(acc, hb + col * ldc, C, a.wo, wave, nc, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rb = wave + 4 * i;
      if (rb >= nc) break;
      const int n = 32 * rb + col;
      const float bv = bo[n];
      unsigned kb = 0;
      if constexpr (DROP) kb = sct_drop_bits_major(d, 1, 0, (unsigned)row0, hh, (unsigned)n);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = nl_acc_row(r, hh);
        const long long grow = row0 + row < a.rows ? row0 + row : a.rows - 1;
        if constexpr (DROP) y[row * ldc + n] = a.x[(size_t)grow * C + n] + sct_drop_apply(d, kb, r, acc[i][r] + bv);
        else y[row * ldc + n] = a.x[(size_t)grow * C + n] + (acc[i][r] + bv);
      }
    }
  }
  __syncthreads();
  if constexpr (KEEP) sct_layernorm<true>(y, ldc, C, lnp, lnp + C, lane, wave, 0, k.y1, row0, a.rows, k.xa, k.rstd);
  else sct_layernorm<false>(y, ldc, C, lnp, lnp + C, lane, wave, 0, nullptr, 0, 0);
  __syncthreads();
  {   // linear1 + bias + ReLU -> hidden rows (the attention tile is dead)
    nl_f32x16 acc[4];
    nl_acc_zero(acc);
    sct_gemm<MODE, 4>(acc, y + col * ldc, C, a.w1, wave, nf, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rb = wave + 4 * i;
      if (rb >= nf) break;
      const int n = 32 * rb + col;
      const float bv = b1[n];
      unsigned kb = 0;
      if constexpr (DROP) kb = sct_drop_bits_major(d, 2, 0, (unsigned)row0, hh, (unsigned)n);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        if constexpr (DROP) hb[nl_acc_row(r, hh) * ldf + n] = sct_drop_apply(d, kb, r, fmaxf(acc[i][r] + bv, 0.f));
        else hb[nl_acc_row(r, hh) * ldf + n] = fmaxf(acc[i][r] + bv, 0.f);
      }
    }
  }
  __syncthreads();
  {   // linear2 + bias + residual
    nl_f32x16 acc[2];
    nl_acc_zero(acc);
    sct_gemm<MODE, 2>(acc, hb + col * ldf, F, a.w2, wave, nc, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rb = wave + 4 * i;
      if (rb >= nc) break;
      const int n = 32 * rb + col;
      const float bv = b2[n];
      unsigned kb = 0;
      if constexpr (DROP) kb = sct_drop_bits_major(d, 3, 0, (unsigned)row0, hh, (unsigned)n);
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = nl_acc_row(r, hh);
        if constexpr (DROP) y[row * ldc + n] = y[row * ldc + n] + sct_drop_apply(d, kb, r, acc[i][r] + bv);
        else y[row * ldc + n] = y[row * ldc + n] + (acc[i][r] + bv);
      }
    }
  }
  __syncthreads();
  if constexpr (KEEP) sct_layernorm<true>(y, ldc, C, lnp + 2 * C, lnp + 3 * C, lane, wave, 1, a.out, row0, a.rows, k.xb, k.rstd, k.out);
  else sct_layernorm<false>(y, ldc, C, lnp + 2 * C, lnp + 3 * C, lane, wave, 1, a.out, row0, a.rows);
}

// the training forward's instantiations of the chain: the five SctKeepRows pointers [+ SctDrop]
template <int MODE, class... D>
constexpr auto sct_chain_keep = sct_chain_kernel<MODE, float*, float*, float*, float*, float*, D...>;

// ------------------------------------------------------------------------------------------ host side: limits and checks
inline bool sct_cfg_ok(int C, int nhead, int F) {
  return nhead == SCT_HEADS && (C == 64 || C == 128 || C == 192 || C == 256) && F >= 32 && F <= 512 && (F & 31) == 0;
}
constexpr int64_t SCT_MAX_ROWS = (int64_t)1 << 24;   // B * max(N0, N1): keeps every grid and the attention's work-item count far inside 32 bits
// a call's counts: the batch may be empty, the two lengths not; none of them, nor the rows of the batch (`longest` each), may pass SCT_MAX_ROWS
inline bool sct_counts_ok(int64_t B, int64_t N0, int64_t N1) { return B >= 0 && N0 >= 1 && N1 >= 1; }
inline bool sct_counts_fit(int64_t B, int64_t N0, int64_t N1, int64_t longest) {
  return B <= SCT_MAX_ROWS && N0 <= SCT_MAX_ROWS && N1 <= SCT_MAX_ROWS && B * longest <= SCT_MAX_ROWS;
}
// everything about a call's shape, configuration and precision that can be refused, in the order the errors win; NL_OK + *empty for B == 0
inline int sct_shape_status(int C, int nhead, int F, int precision, int64_t B, int64_t N0, int64_t N1, bool* empty) {
  *empty = false;
  if (!sct_counts_ok(B, N0, N1)) return NL_ERR_BAD_ARG;
  if (!sct_cfg_ok(C, nhead, F)) return NL_ERR_UNSUPPORTED;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (!sct_counts_fit(B, N0, N1, N0 > N1 ? N0 : N1)) return NL_ERR_UNSUPPORTED;
  *empty = B == 0;
  return NL_OK;
}
inline size_t sct_ws_part(int64_t B, int64_t N0, int64_t N1, int C) { return nl_align_up((size_t)B * (size_t)(N0 > N1 ? N0 : N1) * C * 4, 256); }
inline size_t sct_proj_lds(int C) { return (size_t)2 * 32 * (C + SCT_PAD) * 4; }
inline size_t sct_chain_lds(int C, int F) { return (size_t)32 * ((C + SCT_PAD) + (C > F ? C : F) + SCT_PAD) * 4; }

// ... and the pointers, without touching their targets
inline int sct_check(const void* packed, int C, int nhead, int F, int precision, int64_t B, int64_t N0, int64_t N1, const void* const* ptrs, int nptr, const void* ws,
                     size_t ws_bytes, bool* empty) {
  if (const int s = sct_shape_status(C, nhead, F, precision, B, N0, N1, empty)) return s;
  if (*empty) return NL_OK;
  if (!packed || ((uintptr_t)packed & 15) != 0) return NL_ERR_BAD_ARG;
  for (int i = 0; i < nptr; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & 15) != 0) return NL_ERR_BAD_ARG;   // rows are read and written as 16-byte pieces
  if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < 4 * sct_ws_part(B, N0, N1, C)) return NL_ERR_WORKSPACE;
  return NL_OK;
}

// ------------------------------------------------------------------------------------------ host side: launches
// f(std::integral_constant<int, DH>) for the head dimension of C
template <class Fn>
auto sct_by_head(int C, Fn f) {
  switch (C) {
    case 64: return f(std::integral_constant<int, 8>{});
    case 128: return f(std::integral_constant<int, 16>{});
    case 192: return f(std::integral_constant<int, 24>{});
    default: return f(std::integral_constant<int, 32>{});
  }
}
// Launches KERNEL(args...) or — d given — DROPPING(args..., *d), the kernel's instantiation with the trailing SctDrop, on `blocks` workgroups of 256.  lds_max: the
// dynamic LDS of the largest configuration where that may exceed 64 KB (0: it cannot; the two flags then stay unused); the instantiation that is launched is allowed it
// first.  The flags belong to the instantiation of THIS function, <KERNEL, DROPPING, A...>: one pair per kernel pair as long as every call site of a pair passes the
// same argument types (a second list of types would get a second pair and set the attribute once more — harmless).
template <auto KERNEL, auto DROPPING, class... A>
int sct_launch(int64_t blocks, size_t lds, size_t lds_max, hipStream_t st, const SctDrop* d, const A&... args) {
  static std::atomic<unsigned long long> plain_set{0}, drop_set{0};
  if (lds_max)
    if (const int e = nl_allow_dynamic_lds(d ? (const void*)DROPPING : (const void*)KERNEL, lds_max, d ? drop_set : plain_set)) return e;
  if (d) hipLaunchKernelGGL(DROPPING, dim3((unsigned)blocks), dim3(256), lds, st, args..., *d);
  else hipLaunchKernelGGL(KERNEL, dim3((unsigned)blocks), dim3(256), lds, st, args...);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // namespace
