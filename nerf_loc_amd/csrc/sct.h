// What the SelfCrossTransformer forward (sct.hip) and its training step (sct_bwd.hip) share: the layout of the packed image, the argument blocks of the three
// forward kernels, the operand helpers of the MFMA products (sct_load8, sct_split8, sct_mfma, sct_gemm), the LayerNorm helper of the row chain, and the host-side
// limits and argument checks.  Include after common.h and mfma.h.
#pragma once
#include "common.h"
#include "mfma.h"
#include "host.h"

namespace {

constexpr int SCT_HEADS = 8, SCT_LAYERS = 4, SCT_TENSORS = 52;
constexpr int SCT_PAD = 4;   // floats between LDS rows
constexpr float SCT_EPS = 1e-5f;
enum { SCT_F32 = 0, SCT_X3 = 1, SCT_BF = 2 };   // = NL_PREC_F32 / NL_PREC_BF16X3 / NL_PREC_BF16

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

// LayerNorm of the wave's 8 rows of the LDS tile: in place, or (dst) to the output rows
__device__ __forceinline__ void sct_layernorm(float* y, int ld, int C, const float* g, const float* bta, int lane, int wave, float* dst, long long row0, long long rows) {
  const int nci = C >> 6;
  for (int rr = 0; rr < 8; ++rr) {
    const int row = 8 * wave + rr;
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
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nci) {
        const int c = lane + 64 * i;
        const float r = v[i] * rstd * g[c] + bta[c];
        if (!dst) y[row * ld + c] = r;
        else if (row0 + row < rows) dst[(size_t)(row0 + row) * C + c] = r;
      }
  }
}

// ------------------------------------------------------------------------------------------ host side: limits and checks
bool sct_cfg_ok(int C, int nhead, int F) {
  return nhead == SCT_HEADS && (C == 64 || C == 128 || C == 192 || C == 256) && F >= 32 && F <= 512 && (F & 31) == 0;
}
constexpr int64_t SCT_MAX_ROWS = (int64_t)1 << 24;   // B * max(N0, N1): keeps every grid and the attention's work-item count far inside 32 bits
size_t sct_ws_part(int64_t B, int64_t N0, int64_t N1, int C) { return nl_align_up((size_t)B * (size_t)(N0 > N1 ? N0 : N1) * C * 4, 256); }
size_t sct_proj_lds(int C) { return (size_t)2 * 32 * (C + SCT_PAD) * 4; }
size_t sct_chain_lds(int C, int F) { return (size_t)32 * ((C + SCT_PAD) + (C > F ? C : F) + SCT_PAD) * 4; }

// everything that can be refused without touching a pointer's target; NL_OK + *empty for B == 0
int sct_check(const void* packed, int C, int nhead, int F, int precision, int64_t B, int64_t N0, int64_t N1, const void* const* ptrs, int nptr, const void* ws,
              size_t ws_bytes, bool* empty) {
  *empty = false;
  if (B < 0 || N0 < 1 || N1 < 1) return NL_ERR_BAD_ARG;
  if (!sct_cfg_ok(C, nhead, F)) return NL_ERR_UNSUPPORTED;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (N0 > SCT_MAX_ROWS || N1 > SCT_MAX_ROWS || B > SCT_MAX_ROWS || B * (N0 > N1 ? N0 : N1) > SCT_MAX_ROWS) return NL_ERR_UNSUPPORTED;
  if (B == 0) { *empty = true; return NL_OK; }
  if (!packed || ((uintptr_t)packed & 15) != 0) return NL_ERR_BAD_ARG;
  for (int i = 0; i < nptr; ++i)
    if (!ptrs[i] || ((uintptr_t)ptrs[i] & 15) != 0) return NL_ERR_BAD_ARG;   // rows are read and written as 16-byte pieces
  if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < 4 * sct_ws_part(B, N0, N1, C)) return NL_ERR_WORKSPACE;
  return NL_OK;
}

}  // namespace
