// Training step of SelfCrossTransformer (sct.hip is the inference forward): nl_sct_forward_train keeps O(rows x C) of state per layer, nl_sct_backward returns the
// gradients of the four inputs and of the 48 tensors the module applies.  No Nq x Nk value reaches memory in either direction: the probabilities are rebuilt tile by
// tile from the kept row maximum and sum (the two parts of the log-sum-exp).  The *_dropout entry points are the same step with the reference's four dropout sites
// per layer inside the kernels: the kernels' instantiations with a trailing SctDrop argument (sct_drop.h).
//
// Forward (per layer): the INFERENCE projection and attention kernels write q, k, v and the attention output straight into the state (launch.h:
//   nl_launch_sct_qkv_attn), sct_stats_kernel adds the (maximum, sum) of every (row, head), and the row chain is sct_chain_kernel (sct.h) with the SctKeepRows
//   pointers, i.e. with four more stores: the rows after the first LayerNorm, both LayerNorms' normalised rows and 1 / std, and the outputs of layers 0..2 that the
//   in-place forward overwrites.  The library is built without floating-point contraction, so the same expressions give the same bits: out0 / out1 equal
//   nl_sct_forward's (tests/test_gpu_sct_train.py).
// Backward (layers 3, 2, 1, 0; rows flattened over the batch):
//   sct_chain_bwd_kernel  32 rows per workgroup in LDS: hidden rows again from the kept y1 with sct_chain_kernel's own product (same fragments, same order: the
//     ReLU mask is the one the forward applied), second LayerNorm backward, g . W2, mask, g . W1, + the residual's gradient, first LayerNorm backward, g . Wo.
//     It writes g_attn, the gradient rows the weight gradients read (g_z2, g_y1, g_z1), adds g_z1 to g_x, and stages the hidden rows and their gradients for
//     linear1 / linear2 in two (chunk x F) buffers, chunk = 32 768 rows at most — the only F-wide values in memory.
//   sct_dd_kernel         D[row, head] = sum_c dO . O.
//   sct_attn_bwd_kernel   <KV = false>: a wave owns (batch item, head, 32 queries) and walks the key tiles: S^T = K . Q^T and dP^T = V . dO^T put a query in a lane's
//     column (as the forward), P = exp(S - max) / sum, dS = P (dP - D), and dS is already the B operand of dQ^T += K^T . dS^T.  <KV = true>: the same code with the
//     sides exchanged — a wave owns 32 keys and walks the query tiles, S = Q . K^T puts a key in a lane's column, dV^T += dO^T . P and dK^T += Q^T . dS.  Rows of
//     the walked side beyond its length get P = dS = 0 exactly (loads clamped); columns beyond the owned side are not stored.  One wave walks a whole sequence, so
//     there is nothing to add across waves: each output element has one writer and one order.  Head dimensions 8 / 16 / 24 are padded as in the forward.
//     With one key dS is an exact zero (the softmax is constant), as autograd's: the position encodings of a (1, 1) call get exact zeros.
//   sct_proj_bwd_kernel   g_xq = dQ . Wq, g_mem_k = dK . Wk, g_mem_v = dV . Wv on 32-row tiles, added to g_x / g_pos_x and g_mem / g_pos_mem.
//   wgrad.hip             in_proj (three blocks), out_proj, linear1, linear2 and their biases; the LayerNorm weight / bias are two-stage column sums.
// The transposed weights come from a second image (nl_sct_pack_weights_train; pack.hip's fragment packer), in sct.h's plane layout so that sct_gemm reads them.
// Products run in the call's mode (sct.h).  In NL_PREC_BF16X3 the gradient operands are split-FP16 like everything else here: values below 6e-5 in magnitude lose
// their low term, i.e. gradients are exact to 2^-22 relative to values around one and coarser far below.
// Dropout: the masks are recomputed from (seed, p, layer, site, element) wherever they are needed — nothing per element is kept and the state and workspace sizes are
// the same; the kept attention output is the dropped one, so D = sum dO . O holds unchanged.  A zero threshold (p == 0) launches the kernels without the argument.
// Accumulation across layers (g_x, g_pos, g_mem) is by kernels of one stream that each own their elements: a fixed order, no atomics; two calls give the same bits.
#include <algorithm>
#include "common.h"
#include "mfma.h"
#include "host.h"
#include "sct.h"

namespace {

constexpr int64_t SCT_BWD_CHUNK = 32768;   // rows per launch of the chain backward: bounds the two rows x F staging buffers of linear1 / linear2
constexpr int SCT_LN_ROWS = 128;           // rows per partial sum of the LayerNorm parameter gradients

// ------------------------------------------------------------------------------------------ training image
// per layer Wq^T, Wk^T, Wv^T, out_proj.weight^T (C x C), linear1.weight^T (C x F), linear2.weight^T (F x C), each in the four planes of the inference image
// (SctMatOff), then one staging area for the plain transposes
struct SctTrainLayout { SctMatOff m[SCT_LAYERS][6]; size_t stage, total; };
inline SctTrainLayout sct_train_layout(int C, int F) {
  SctTrainLayout L;
  size_t o = 0;
  for (int i = 0; i < SCT_LAYERS; ++i) {
    const size_t n[6] = {(size_t)C * C, (size_t)C * C, (size_t)C * C, (size_t)C * C, (size_t)C * F, (size_t)F * C};
    for (int k = 0; k < 6; ++k) {
      L.m[i][k].hi = o; o += n[k] * 2;
      L.m[i][k].lo = o; o += n[k] * 2;
      L.m[i][k].bf = o; o += n[k] * 2;
      L.m[i][k].f32 = o; o += n[k] * 4;
    }
  }
  L.stage = o; o += (size_t)std::max(C, F) * C * 4;
  L.total = nl_align_up(o, 256);
  return L;
}

// ------------------------------------------------------------------------------------------ kept state of one layer
struct SctKeep { float *q, *k, *v, *attn, *ml, *y1, *xa, *xb, *rstd, *out; };
// the next `floats` floats of a carved buffer, at base + o (base may be null: sizes only); o moves behind them, to the next multiple of 256 bytes
float* sct_take(unsigned char* base, size_t& o, size_t floats) {
  float* p = base ? (float*)(base + o) : nullptr;
  o += nl_align_up(floats * 4, 256);
  return p;
}
// carves the layer's buffers at base + o; returns the offset behind them
size_t sct_keep_carve(unsigned char* base, size_t o, int64_t rq, int64_t rk, int C, SctKeep& k, bool no_out = false) {
  const size_t q = (size_t)rq * C, m = (size_t)rk * C;
  k.q = sct_take(base, o, q); k.k = sct_take(base, o, m); k.v = sct_take(base, o, m); k.attn = sct_take(base, o, q);
  k.ml = sct_take(base, o, (size_t)rq * 16); k.y1 = sct_take(base, o, q); k.xa = sct_take(base, o, q); k.xb = sct_take(base, o, q);
  k.rstd = sct_take(base, o, (size_t)rq * 2); k.out = no_out ? nullptr : sct_take(base, o, q);
  return o;
}
size_t sct_state_carve(unsigned char* base, int64_t B, int64_t N0, int64_t N1, int C, SctKeep (&k)[SCT_LAYERS]) {
  size_t o = 0;
  for (int l = 0; l < SCT_LAYERS; ++l) {
    const int64_t nq = (l == 0 || l == 2) ? N0 : N1, nk = (l == 0 || l == 3) ? N0 : N1;
    o = sct_keep_carve(base, o, B * nq, B * nk, C, k[l], l == 3);
  }
  return o;
}

// ------------------------------------------------------------------------------------------ attention tiles
template <int MODE, int DH>
struct SctHd {
  static constexpr int KS = DH <= 16 ? 1 : 2;   // 16-wide k steps of the (zero-padded) head dimension
  static constexpr int HD = DH / 2;             // fp32: half-wave hh multiplies dimensions hh * HD .. hh * HD + HD - 1
  nl_i16x8 h[KS], l[KS];
  float f[HD];
};
// the lane's row of a head (p: its first channel) times `scale` as an operand of the 32 x 32 products, A or B alike: fp32 the half-wave's DH / 2 dimensions,
// else the 8-wide groups 16 s + 8 hh, zeros where the group is padding
template <int MODE, int DH>
__device__ __forceinline__ void sct_head_row(const float* p, int hh, float scale, SctHd<MODE, DH>& o) {
  if constexpr (MODE == SCT_F32) {
#pragma unroll
    for (int t = 0; t < SctHd<MODE, DH>::HD; t += 4) {
      const float4 v = *(const float4*)(p + hh * SctHd<MODE, DH>::HD + t);
      o.f[t] = v.x * scale; o.f[t + 1] = v.y * scale; o.f[t + 2] = v.z * scale; o.f[t + 3] = v.w * scale;
    }
  } else {
#pragma unroll
    for (int s = 0; s < SctHd<MODE, DH>::KS; ++s) {
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (16 * s + 8 * hh < DH) sct_load8(p + 16 * s + 8 * hh, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] *= scale;
      sct_split8<MODE>(v, o.h[s], o.l[s]);
    }
  }
}
// T[i][j] = sum_d a_i[d] b_j[d]: the lane holds column j = lane & 31, register r is row nl_acc_row(r, hh)
template <int MODE, int DH>
__device__ __forceinline__ nl_f32x16 sct_head_prod(const SctHd<MODE, DH>& a, const SctHd<MODE, DH>& b) {
  nl_f32x16 t;
#pragma unroll
  for (int r = 0; r < 16; ++r) t[r] = 0.f;
  if constexpr (MODE == SCT_F32) {
#pragma unroll
    for (int d = 0; d < SctHd<MODE, DH>::HD; ++d) t = __builtin_amdgcn_mfma_f32_32x32x2f32(a.f[d], b.f[d], t, 0, 0, 0);
  } else {
#pragma unroll
    for (int s = 0; s < SctHd<MODE, DH>::KS; ++s) t = sct_mfma<MODE>(a.h[s], a.l[s], b.h[s], b.l[s], t);
  }
  return t;
}
// X[row0 + nl_acc_row(r, hh)][the lane's channel] for the 16 registers (base: the channel of row 0); rows past n repeat the last one — their weight is an exact zero
__device__ __forceinline__ void sct_gather16(const float* base, long long row0, long long n, int hh, int C, float (&g)[16]) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long long row = row0 + nl_acc_row(r, hh);
    g[r] = base[(size_t)(row < n ? row : n - 1) * C];
  }
}
// acc[channel][column] += sum over the tile's 32 rows of g[row][channel] * w[row][column]: w is a score tile's accumulator registers, which are already the B
// operand (k slot (hh, j) of step s = register 8 s + j), g the A operand gathered in that order
template <int MODE>
__device__ __forceinline__ nl_f32x16 sct_tile_acc(const float (&g)[16], const float (&w)[16], nl_f32x16 acc) {
  if constexpr (MODE == SCT_F32) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(g[r], w[r], acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      float a[8], b[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) { a[j] = g[8 * s + j]; b[j] = w[8 * s + j]; }
      nl_i16x8 ah, al, bh, bl;
      sct_split8<MODE>(a, ah, al);
      sct_split8<MODE>(b, bh, bl);
      acc = sct_mfma<MODE>(ah, al, bh, bl, acc);
    }
  }
  return acc;
}

// ---- (maximum, sum) of every (row, head): ml[row][head][2]
struct SctStatsArgs { const float* q; const float* k; float* ml; long long Nq, Nk, items; int nqt; float scale; };

template <int MODE, int DH>
__global__ __launch_bounds__(256) void sct_stats_kernel(const SctStatsArgs a) {
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);
  constexpr int C = 8 * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= a.items) return;   // wave-uniform; no barrier
  const long long bh = item / a.nqt, b = bh >> 3, q0 = (item - bh * a.nqt) * 32;
  const int h = (int)(bh & 7);
  const long long qrow = q0 + col < a.Nq ? q0 + col : a.Nq - 1;
  SctHd<MODE, DH> qo;
  sct_head_row<MODE, DH>(a.q + ((size_t)b * a.Nq + qrow) * C + h * DH, hh, a.scale, qo);
  const float* kbase = a.k + (size_t)b * a.Nk * C + h * DH;
  float m = -INFINITY, l = 0.f;
  for (long long k0 = 0; k0 < a.Nk; k0 += 32) {
    const long long krow = k0 + col < a.Nk ? k0 + col : a.Nk - 1;
    SctHd<MODE, DH> ko;
    sct_head_row<MODE, DH>(kbase + (size_t)krow * C, hh, 1.f, ko);
    nl_f32x16 st = sct_head_prod<MODE, DH>(ko, qo);   // S^T[key][query]
    if (k0 + 32 > a.Nk) {
#pragma unroll
      for (int r = 0; r < 16; ++r)
        if (k0 + nl_acc_row(r, hh) >= a.Nk) st[r] = -INFINITY;
    }
    float mx = st[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mnew = fmaxf(m, mx);   // finite: key k0 exists
    float ps = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) ps += __expf(st[r] - mnew);
    ps += __shfl_xor(ps, 32);
    l = l * __expf(m - mnew) + ps;
    m = mnew;
  }
  if (hh == 0 && q0 + col < a.Nq) {
    float* o = a.ml + (((size_t)b * a.Nq + q0 + col) * 8 + h) * 2;
    o[0] = m; o[1] = l;
  }
}

// ---- D[row][head] = sum_c dO . O
__global__ __launch_bounds__(256) void sct_dd_kernel(const float* dO, const float* O, long long rows, int DH, float* dd) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= rows * 8) return;
  const float* a = dO + (size_t)e * DH;   // element (row, head) starts at row * C + head * DH = e * DH
  const float* b = O + (size_t)e * DH;
  float s = 0.f;
  for (int c = 0; c < DH; c += 4) {
    const float4 x = *(const float4*)(a + c), y = *(const float4*)(b + c);
    s += x.x * y.x; s += x.y * y.y; s += x.z * y.z; s += x.w * y.w;
  }
  dd[e] = s;
}

// ---- the two passes
struct SctAttnBwdArgs {
  const float *q, *k, *v, *dO, *ml, *dd;
  float *dq, *dk, *dv;
  long long Nq, Nk, items;
  int nto;   // 32-row tiles of the owned side
  float scale;
};

// DROP (sct_drop.h site 0): P is the undropped softmax rebuilt from (m, l); dP_eff = keep ? dP / (1 - p) : 0, dS = P (dP_eff - D), and dV accumulates
// keep ? P / (1 - p) : 0.  dQ pass: the registers run along the keys (four generator calls per tile and lane); dK / dV pass: along the queries (eight).
template <int MODE, int DH, bool KV, class... DROPARG>
__global__ __launch_bounds__(256) void sct_attn_bwd_kernel(const SctAttnBwdArgs a, const DROPARG... drop) {
  constexpr bool DROP = sizeof...(DROPARG) != 0;
  [[maybe_unused]] const auto d = sct_arg<SctDrop>(drop...);
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);
  constexpr int C = 8 * DH;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= a.items) return;   // wave-uniform; no barrier
  const long long bh = item / a.nto, b = bh >> 3, o0 = (item - bh * a.nto) * 32;
  const int h = (int)(bh & 7);
  const long long No = KV ? a.Nk : a.Nq, Nl = KV ? a.Nq : a.Nk;   // owned side (a lane's column), walked side (a tile's rows)
  const long long orow = o0 + col < No ? o0 + col : No - 1;
  const float* qb = a.q + (size_t)b * a.Nq * C + h * DH;
  const float* kb = a.k + (size_t)b * a.Nk * C + h * DH;
  const float* vb = a.v + (size_t)b * a.Nk * C + h * DH;
  const float* gb = a.dO + (size_t)b * a.Nq * C + h * DH;
  const int ch = col < DH ? col : DH - 1;   // channel rows >= DH of the transposed outputs repeat the last one and are not stored
  const size_t sbase = (size_t)b * a.Nq * 8 + h;   // (row, head) statistics of the batch item: + 8 * query

  // the owned side's two B operands: (q * scale, dO) or (k, v)
  SctHd<MODE, DH> b1, b2;
  sct_head_row<MODE, DH>((KV ? kb : qb) + (size_t)orow * C, hh, KV ? 1.f : a.scale, b1);
  sct_head_row<MODE, DH>((KV ? vb : gb) + (size_t)orow * C, hh, 1.f, b2);
  float om = 0.f, orinv = 0.f, odd = 0.f;
  if constexpr (!KV) {
    om = a.ml[(sbase + 8 * orow) * 2];
    orinv = 1.f / a.ml[(sbase + 8 * orow) * 2 + 1];
    odd = a.dd[sbase + 8 * orow];
  }
  nl_f32x16 acc1, acc2;   // dQ^T, or dK^T and dV^T: [channel][owned row]
#pragma unroll
  for (int r = 0; r < 16; ++r) { acc1[r] = 0.f; acc2[r] = 0.f; }

  for (long long l0 = 0; l0 < Nl; l0 += 32) {
    const long long lrow = l0 + col < Nl ? l0 + col : Nl - 1;
    SctHd<MODE, DH> a1, a2;   // the walked side's two A operands: (k, v) or (q * scale, dO)
    sct_head_row<MODE, DH>((KV ? qb : kb) + (size_t)lrow * C, hh, KV ? a.scale : 1.f, a1);
    sct_head_row<MODE, DH>((KV ? gb : vb) + (size_t)lrow * C, hh, 1.f, a2);
    const nl_f32x16 s = sct_head_prod<MODE, DH>(a1, b1);    // S^T[key][query] / S[query][key]
    const nl_f32x16 dp = sct_head_prod<MODE, DH>(a2, b2);   // dP in the same orientation
    float p[16], ds[16];
    unsigned keepb = 0;
    if constexpr (DROP) {
      if constexpr (KV) keepb = sct_drop_bits_minor(d, 0, (unsigned)(b * 8 + h), (unsigned)(o0 + col), (unsigned)l0, hh);
      else keepb = sct_drop_bits_major(d, 0, (unsigned)(b * 8 + h), (unsigned)l0, hh, (unsigned)(o0 + col));
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = l0 + nl_acc_row(r, hh);
      float m = om, ri = orinv, dd = odd;
      if constexpr (KV) {
        const size_t e = sbase + 8 * (row < Nl ? row : Nl - 1);
        m = a.ml[e * 2]; ri = 1.f / a.ml[e * 2 + 1]; dd = a.dd[e];
      }
      p[r] = row < Nl ? __expf(s[r] - m) * ri : 0.f;
      float dpe = dp[r];
      if constexpr (DROP) dpe = sct_drop_apply(d, keepb, r, dpe);
      ds[r] = a.Nk == 1 ? 0.f : p[r] * (dpe - dd);   // one key: the softmax is the constant 1, its derivative an exact zero (dP - D would leave rounding noise)
      if constexpr (DROP && KV) p[r] = sct_drop_apply(d, keepb, r, p[r]);   // dV's operand
    }
    float g[16];
    sct_gather16((KV ? qb : kb) + ch, l0, Nl, hh, C, g);
    acc1 = sct_tile_acc<MODE>(g, ds, acc1);
    if constexpr (KV) {
      sct_gather16(gb + ch, l0, Nl, hh, C, g);
      acc2 = sct_tile_acc<MODE>(g, p, acc2);
    }
  }
  if (o0 + col < No) {
    float* o1 = (KV ? a.dk : a.dq) + ((size_t)b * No + o0 + col) * C + h * DH;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = nl_acc_row(r, hh);
      if (c < DH) {
        o1[c] = acc1[r] * a.scale;
        if constexpr (KV) a.dv[((size_t)b * No + o0 + col) * C + h * DH + c] = acc2[r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ row chain backward
struct SctChainBwdArgs {
  const float *g_out, *xb, *xa, *rstd, *y1;
  SctW w1, w2t, w1t, wot;
  const float* vec;   // the layer's vectors of the inference image
  float *gz2, *gy1, *gz1, *gattn;   // gradient rows ([rows][C]); gy1 may be null
  float* gx;           // += g_z1 (the residual's part of g_x), or null
  float *hst, *gst;    // [row - row_begin][F]: hidden rows and their pre-activation gradients of this launch's rows, or null
  long long row_begin, row_end;
  int C, F;
};

// LayerNorm backward of the wave's 8 rows: g_in = rstd (t - mean(t) - xn mean(t xn)), t = g gamma.  g comes from gsrc (global rows) or from the LDS tile, the result
// goes to the LDS tile and to dst (and is added to add, if given).
// With a trailing SctDrop the LayerNorm's input was x + dropout(z) (sct_drop.h `site`): the residual takes the gradient as it is — added to `add`, or stored to `raw`
// — and z takes it masked and scaled: that goes to the LDS tile (the next product's operand) and to dst (the rows the weight gradient reads).  The lane's columns
// run along `minor` and its 8 rows along `major`: two generator calls per 64 columns, kept as one bit per (row, column).
template <class... DROPARG>
__device__ __forceinline__ void sct_layernorm_bwd(float* tile, int ld, int C, const float* gsrc, const float* xn, const float* rstd, int which, const float* gamma,
                                                  int lane, int wave, long long row0, long long row_end, float* dst, float* add, float* raw, int site,
                                                  const DROPARG&... drop) {
  constexpr bool DROP = sizeof...(DROPARG) != 0;
  [[maybe_unused]] const auto d = sct_arg<SctDrop>(drop...);
  const int nci = C >> 6;
  [[maybe_unused]] unsigned kb = 0;
  if constexpr (DROP) {
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (i < nci) {
          const uint4 w = sct_drop_words(d, site, 0, (unsigned)((row0 + 8 * wave + 4 * g) >> 2), (unsigned)(lane + 64 * i) >> 1);
          const unsigned h = lane & 1;
          kb |= (unsigned)sct_drop_keep(d, w.x, h) << (16 * g + i) | (unsigned)sct_drop_keep(d, w.y, h) << (16 * g + 4 + i) |
                (unsigned)sct_drop_keep(d, w.z, h) << (16 * g + 8 + i) | (unsigned)sct_drop_keep(d, w.w, h) << (16 * g + 12 + i);
        }
  }
  for (int rr = 0; rr < 8; ++rr) {
    const int row = 8 * wave + rr;
    const bool live = row0 + row < row_end;
    const size_t grow = (size_t)(live ? row0 + row : row_end - 1);
    float t[4] = {0.f, 0.f, 0.f, 0.f}, x[4] = {0.f, 0.f, 0.f, 0.f}, s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nci) {
        const int c = lane + 64 * i;
        const float g = gsrc ? gsrc[grow * C + c] : tile[row * ld + c];
        x[i] = xn[grow * C + c];
        t[i] = g * gamma[c];
        s1 += t[i];
        s2 += t[i] * x[i];
      }
    const float m1 = wave_sum(s1) / (float)C, m2 = wave_sum(s2) / (float)C;
    const float rs = rstd[grow * 2 + which];
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (i < nci) {
        const int c = lane + 64 * i;
        const float r = rs * ((t[i] - m1) - x[i] * m2);
        float rm = r;
        if constexpr (DROP) rm = sct_drop_apply(d, kb, 4 * rr + i, r);
        tile[row * ld + c] = rm;
        if (live) {
          dst[grow * C + c] = rm;
          if (add) add[grow * C + c] += r;
          if (raw) raw[grow * C + c] = r;
        }
      }
  }
}

// DROP: g_z2 and g_z1 reach the residuals undropped and linear2 / out_proj masked and scaled (sites 3 and 1) — so do the rows gz2 / gz1 that wgrad.hip reads and
// the operands of g . W2 and g . Wo.  The hidden rows are rebuilt DROPPED (site 2; that is what linear2 multiplied, and what hst stages): a dropped value is positive
// exactly where the element was kept and the forward's own pre-activation was positive, so one test gives g_pre = both masks, times the scale.  The undropped g_z2
// waits in the gy1 rows (never null here) between the second LayerNorm's backward and the sum that overwrites them with g_y1.
template <int MODE, class... DROPARG>
__global__ __launch_bounds__(256) void sct_chain_bwd_kernel(const SctChainBwdArgs a, const DROPARG... drop) {
  constexpr bool DROP = sizeof...(DROPARG) != 0;
  [[maybe_unused]] const auto d = sct_arg<SctDrop>(drop...);
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);
  extern __shared__ __attribute__((aligned(16))) float sct_smem[];
  const int C = a.C, F = a.F, ldc = C + SCT_PAD, ldf = F + SCT_PAD, c4n = C >> 2, nc = C >> 5, nf = F >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long row0 = a.row_begin + (long long)blockIdx.x * 32;
  float* ga = sct_smem;               // [32][ldc]: y1, then the running gradient rows
  float* hb = sct_smem + 32 * ldc;    // [32][ldf]: hidden rows, then their gradients
  const float* b1 = a.vec + 4 * C;
  const float* lnp = b1 + F + C;      // weight A, bias A, weight B, bias B

  for (int i = threadIdx.x; i < 32 * c4n; i += 256) {
    const int r = i / c4n, c = 4 * (i - r * c4n);
    const long long row = row0 + r < a.row_end ? row0 + r : a.row_end - 1;
    *(float4*)(ga + r * ldc + c) = *(const float4*)(a.y1 + (size_t)row * C + c);
  }
  __syncthreads();
  {   // the hidden rows again: sct_chain_kernel's linear1 + bias + ReLU on the same rows
    nl_f32x16 acc[4];
    nl_acc_zero(acc);
    sct_gemm<MODE, 4>(acc, ga + col * ldc, C, a.w1, wave, nf, lane);
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
        const int row = nl_acc_row(r, hh);
        float hv = fmaxf(acc[i][r] + bv, 0.f);
        if constexpr (DROP) hv = sct_drop_apply(d, kb, r, hv);
        hb[row * ldf + n] = hv;
        if (a.hst && row0 + row < a.row_end) a.hst[(size_t)(row0 + row - a.row_begin) * F + n] = hv;
      }
    }
  }
  __syncthreads();
  // second LayerNorm backward: g_z2 (the gradient of linear2's output and of the residual beside it)
  sct_layernorm_bwd(ga, ldc, C, a.g_out, a.xb, a.rstd, 1, lnp + 2 * C, lane, wave, row0, a.row_end, a.gz2, nullptr, DROP ? a.gy1 : nullptr, 3, drop...);
  __syncthreads();
  {   // g_h = g_z2 . W2, masked: each hidden value is replaced by its pre-activation's gradient (the same lane reads and writes it)
    nl_f32x16 acc[4];
    nl_acc_zero(acc);
    sct_gemm<MODE, 4>(acc, ga + col * ldc, C, a.w2t, wave, nf, lane);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int rb = wave + 4 * i;
      if (rb >= nf) break;
      const int n = 32 * rb + col;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = nl_acc_row(r, hh);
        float gv = hb[row * ldf + n] > 0.f ? acc[i][r] : 0.f;
        if constexpr (DROP) gv *= d.scale;
        hb[row * ldf + n] = gv;
        if (a.gst && row0 + row < a.row_end) a.gst[(size_t)(row0 + row - a.row_begin) * F + n] = gv;
      }
    }
  }
  __syncthreads();
  {   // g_y1 = g_z2 + g_pre . W1
    nl_f32x16 acc[2];
    nl_acc_zero(acc);
    sct_gemm<MODE, 2>(acc, hb + col * ldf, F, a.w1t, wave, nc, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rb = wave + 4 * i;
      if (rb >= nc) break;
      const int n = 32 * rb + col;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int row = nl_acc_row(r, hh);
        float gz = ga[row * ldc + n];
        if constexpr (DROP) gz = a.gy1[(size_t)(row0 + row < a.row_end ? row0 + row : a.row_end - 1) * C + n];
        const float gv = gz + acc[i][r];
        ga[row * ldc + n] = gv;
        if (a.gy1 && row0 + row < a.row_end) a.gy1[(size_t)(row0 + row) * C + n] = gv;
      }
    }
  }
  __syncthreads();
  // first LayerNorm backward: g_z1 (the gradient of out_proj's output and of the residual x)
  sct_layernorm_bwd(ga, ldc, C, nullptr, a.xa, a.rstd, 0, lnp, lane, wave, row0, a.row_end, a.gz1, a.gx, nullptr, 1, drop...);
  __syncthreads();
  {   // g_attn = g_z1 . Wo
    nl_f32x16 acc[2];
    nl_acc_zero(acc);
    sct_gemm<MODE, 2>(acc, ga + col * ldc, C, a.wot, wave, nc, lane);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      const int rb = wave + 4 * i;
      if (rb >= nc) break;
      const int n = 32 * rb + col;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const long long row = row0 + nl_acc_row(r, hh);
        if (row < a.row_end) a.gattn[(size_t)row * C + n] = acc[i][r];
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ projection backward
// sum = a0 . W0 (+ a1 . W1) on 32-row tiles (W: transposed blocks of in_proj_weight): out_sum += sum, out_first += a0 . W0; either output may be null
struct SctProjBwdArgs { const float* a[2]; SctW w[2]; int na; float* out_sum; float* out_first; long long rows; int C; };

template <int MODE>
__global__ __launch_bounds__(256) void sct_proj_bwd_kernel(const SctProjBwdArgs a) {
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);
  extern __shared__ __attribute__((aligned(16))) float sct_smem[];
  const int C = a.C, ld = C + SCT_PAD, c4n = C >> 2, nc = C >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long row0 = (long long)blockIdx.x * 32;
  for (int t = 0; t < a.na; ++t)
    for (int i = threadIdx.x; i < 32 * c4n; i += 256) {
      const int r = i / c4n, c = 4 * (i - r * c4n);
      const long long row = row0 + r < a.rows ? row0 + r : a.rows - 1;
      *(float4*)(sct_smem + (t * 32 + r) * ld + c) = *(const float4*)(a.a[t] + (size_t)row * C + c);
    }
  __syncthreads();
  nl_f32x16 acc[2][2];
  nl_acc_zero(acc);
  sct_gemm<MODE, 2>(acc[0], sct_smem + col * ld, C, a.w[0], wave, nc, lane);
  if (a.na > 1) sct_gemm<MODE, 2>(acc[1], sct_smem + (32 + col) * ld, C, a.w[1], wave, nc, lane);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int rb = wave + 4 * i;
    if (rb >= nc) break;
    const int n = 32 * rb + col;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = row0 + nl_acc_row(r, hh);
      if (row >= a.rows) continue;
      const size_t e = (size_t)row * C + n;
      if (a.out_first) a.out_first[e] += acc[0][i][r];
      if (a.out_sum) a.out_sum[e] += acc[0][i][r] + acc[1][i][r];
    }
  }
}

// ------------------------------------------------------------------------------------------ LayerNorm parameter gradients, element-wise sums
// part[blk][0][c] = sum over the block's SCT_LN_ROWS rows of g xn, part[blk][1][c] = of g.  A workgroup owns 64 columns: wave w sums the rows r % 4 == w
// (each a coalesced 256-byte piece) and the four sums meet in LDS as (0 + 1) + (2 + 3) — a fixed order.  grid (row blocks, C / 64)
__global__ __launch_bounds__(256) void sct_ln_part_kernel(const float* g, const float* xn, long long rows, int C, float* part) {
  __shared__ float red[2][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.y * 64 + lane;
  const long long r0 = (long long)blockIdx.x * SCT_LN_ROWS, r1 = r0 + SCT_LN_ROWS < rows ? r0 + SCT_LN_ROWS : rows;
  float sw = 0.f, sb = 0.f;
  for (long long r = r0 + w; r < r1; r += 4) {
    const float gv = g[(size_t)r * C + c];
    sw += gv * xn[(size_t)r * C + c];
    sb += gv;
  }
  red[0][w][lane] = sw;
  red[1][w][lane] = sb;
  __syncthreads();
  if (w == 0) {
    part[((size_t)blockIdx.x * 2) * C + c] = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
    part[((size_t)blockIdx.x * 2 + 1) * C + c] = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
  }
}
// the partial sums added the same way: wave w takes the blocks b % 4 == w in ascending order.  grid (C / 64)
__global__ __launch_bounds__(256) void sct_ln_sum_kernel(const float* part, int nblk, int C, float* gw, float* gb) {
  __shared__ float red[2][4][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, c = blockIdx.x * 64 + lane;
  float sw = 0.f, sb = 0.f;
  for (int b = w; b < nblk; b += 4) {
    sw += part[((size_t)b * 2) * C + c];
    sb += part[((size_t)b * 2 + 1) * C + c];
  }
  red[0][w][lane] = sw;
  red[1][w][lane] = sb;
  __syncthreads();
  if (w == 0) {
    if (gw) gw[c] = (red[0][0][lane] + red[0][1][lane]) + (red[0][2][lane] + red[0][3][lane]);
    if (gb) gb[c] = (red[1][0][lane] + red[1][1][lane]) + (red[1][2][lane] + red[1][3][lane]);
  }
}
__global__ __launch_bounds__(256) void sct_add_kernel(const float* x, const float* y, float* o, size_t n4) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n4) return;
  const float4 a = ((const float4*)x)[e], b = ((const float4*)y)[e];
  ((float4*)o)[e] = make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// ------------------------------------------------------------------------------------------ host side
int sct_wg_splits(int64_t rows) { return (int)std::min<int64_t>(256, std::max<int64_t>(1, nl_cdiv(rows, 256))); }

// workspace of the backward: the gradients at the three inner layer outputs and one layer's temporaries (sized by the longer side); x + pos and mem + pos of the
// in_proj weight gradient reuse g_z2 and g_y1, which are dead by then.  layer: nl_sct_layer_backward runs its own forward — room for that layer's output and state
struct SctBwdWs {
  float *G[3], *gz2, *gy1, *gz1, *gattn, *dd, *dq, *dk, *dv, *xp, *mp, *hst, *gst, *wg, *lnp, *dummy, *lout;
  size_t wg_floats, keep_off, total;
  int64_t chunk;
};
SctBwdWs sct_bwd_ws(unsigned char* base, int64_t B, int64_t N0, int64_t N1, int C, int F, bool layer) {
  SctBwdWs w;
  size_t o = 0;
  const int64_t r0 = B * N0, r1 = B * N1, rm = std::max(r0, r1);
  const size_t rc = (size_t)rm * C;
  w.G[0] = sct_take(base, o, (size_t)r0 * C); w.G[1] = sct_take(base, o, (size_t)r1 * C); w.G[2] = sct_take(base, o, (size_t)r0 * C);
  w.gz2 = sct_take(base, o, rc); w.gy1 = sct_take(base, o, rc); w.gz1 = sct_take(base, o, rc); w.gattn = sct_take(base, o, rc);
  w.dd = sct_take(base, o, (size_t)rm * 8);
  w.dq = sct_take(base, o, rc); w.dk = sct_take(base, o, rc); w.dv = sct_take(base, o, rc); w.xp = w.gz2; w.mp = w.gy1;
  w.chunk = std::min<int64_t>(rm, SCT_BWD_CHUNK);
  w.hst = sct_take(base, o, (size_t)w.chunk * F); w.gst = sct_take(base, o, (size_t)w.chunk * F);
  const size_t mn = (size_t)C * std::max(C, F);
  w.wg_floats = (size_t)sct_wg_splits(rm) * (mn + std::max(C, F));
  w.wg = sct_take(base, o, w.wg_floats);
  w.lnp = sct_take(base, o, (size_t)nl_cdiv(rm, SCT_LN_ROWS) * 2 * C);
  w.dummy = sct_take(base, o, mn);
  w.lout = nullptr;
  w.keep_off = o;
  if (layer) {
    w.lout = sct_take(base, o, (size_t)r0 * C);
    w.keep_off = o;
    SctKeep k;
    o = sct_keep_carve(nullptr, o, r0, r1, C, k, true);
  }
  w.total = o;
  return w;
}

struct SctLayerFwd {
  const unsigned char* img; int C, F, layer, precision;
  const float *x, *xpos, *mem, *mpos; int64_t Nq, Nk, B;
  float* out; SctKeep keep; bool keep_out;
  float p; unsigned long long seed;   // dropout (sct_drop.h); p == 0: the kernels without it
};

template <int MODE>
int sct_layer_forward_train(const SctLayerFwd& r, hipStream_t st) {
  const int C = r.C, F = r.F;
  const SctLayout L = sct_layout(C, F);
  const long long rowsq = r.B * r.Nq;
  if (const int e = nl_launch_sct_qkv_attn(r.img, C, F, r.layer, r.precision, r.x, r.xpos, r.Nq, r.mem, r.mpos, r.Nk, r.B, r.keep.q, r.keep.k, r.keep.v, r.keep.attn,
                                           r.p, r.seed, st))
    return e;
  const SctDrop d = sct_drop_make(r.p, r.seed, r.layer);
  SctStatsArgs s;
  s.q = r.keep.q; s.k = r.keep.k; s.ml = r.keep.ml; s.Nq = r.Nq; s.Nk = r.Nk; s.nqt = (int)nl_cdiv(r.Nq, 32); s.items = r.B * SCT_HEADS * s.nqt;
  s.scale = sct_scale(C);
  sct_by_head(C, [&](auto dh) { hipLaunchKernelGGL((sct_stats_kernel<MODE, decltype(dh)::value>), dim3((unsigned)nl_cdiv(s.items, 4)), dim3(256), 0, st, s); });
  NL_LAUNCH_CHECK();
  return sct_launch<sct_chain_keep<MODE>, sct_chain_keep<MODE, SctDrop>>(
      nl_cdiv(rowsq, 32), sct_chain_lds(C, F), sct_chain_lds(256, 512), st, d.thr ? &d : nullptr,
      sct_chain_args(r.img, L.l[r.layer], C, F, r.keep.attn, r.x, r.out, rowsq),
      r.keep.y1, r.keep.xa, r.keep.xb, r.keep.rstd, r.keep_out ? r.keep.out : nullptr);
}

struct SctLayerBwd {
  const unsigned char *img, *timg; int C, F, layer;
  const float *x, *xpos, *mem, *mpos; int64_t Nq, Nk, B;
  SctKeep keep; const float* g_out;
  float *g_x, *g_xpos, *g_mem, *g_mpos;   // += targets; any may be null
  float* const* gp;                       // the layer's 12 / 14 parameter gradients in state-dict order; entries may be null
  float p; unsigned long long seed;       // the forward's dropout (sct_drop.h)
};

template <int MODE>
int sct_layer_backward(const SctLayerBwd& r, const SctBwdWs& w, hipStream_t st) {
  const int C = r.C, F = r.F, l = r.layer;
  const bool cross = l >= 2;
  const SctLayout L = sct_layout(C, F);
  const SctTrainLayout T = sct_train_layout(C, F);
  const SctLayerOff& lo = L.l[l];
  const int64_t rq = r.B * r.Nq, rk = r.B * r.Nk;
  float* const* gp = r.gp;
  const int ln = sct_param_norm(l);
  const bool want_in = gp[0] || gp[1], want_o = gp[2] || gp[3], want_1 = gp[4] || gp[5], want_2 = gp[6] || gp[7];
  const bool want_lna = gp[ln] || gp[ln + 1], want_lnb = gp[ln + 2] || gp[ln + 3];
  const bool in_x = r.g_x || r.g_xpos, in_m = r.g_mem || r.g_mpos;
  if (!(want_in || want_o || want_1 || want_2 || want_lna || want_lnb || in_x || in_m)) return NL_OK;

  static std::atomic<unsigned long long> proj_set{0};
  if (const int e = nl_allow_dynamic_lds((const void*)sct_proj_bwd_kernel<MODE>, sct_proj_lds(256), proj_set)) return e;
  const SctDrop d = sct_drop_make(r.p, r.seed, l);
  const SctDrop* dp = d.thr ? &d : nullptr;

  // ---- row chain, in row chunks with the two F-wide weight gradients behind each
  SctChainBwdArgs c;
  c.g_out = r.g_out; c.xb = r.keep.xb; c.xa = r.keep.xa; c.rstd = r.keep.rstd; c.y1 = r.keep.y1;
  c.w1 = sct_mat(r.img, lo.m[2], F);
  c.w2t = sct_mat(r.timg, T.m[l][5], F); c.w1t = sct_mat(r.timg, T.m[l][4], C); c.wot = sct_mat(r.timg, T.m[l][3], C);
  c.vec = (const float*)(r.img + lo.vec);
  c.gz2 = w.gz2; c.gy1 = want_lna || dp ? w.gy1 : nullptr; c.gz1 = w.gz1; c.gattn = w.gattn;   // dropping: the undropped g_z2 waits in the gy1 rows
  c.gx = r.g_x;
  c.hst = want_2 ? w.hst : nullptr; c.gst = want_1 ? w.gst : nullptr;
  c.C = C; c.F = F;
  for (int64_t b0 = 0; b0 < rq; b0 += w.chunk) {
    const int64_t n = std::min<int64_t>(w.chunk, rq - b0);
    c.row_begin = b0; c.row_end = b0 + n;
    if (const int e = sct_launch<sct_chain_bwd_kernel<MODE>, sct_chain_bwd_kernel<MODE, SctDrop>>(nl_cdiv(n, 32), sct_chain_lds(C, F), sct_chain_lds(256, 512), st, dp, c))
      return e;
    if (want_1)
      if (const int e = nl_launch_wgrad(w.gst, F, F, r.keep.y1 + (size_t)b0 * C, C, C, n, 0, 0, gp[4] ? gp[4] : w.dummy, C, 1, 0, gp[5], w.wg, w.wg_floats, st)) return e;
    if (want_2)
      if (const int e = nl_launch_wgrad(w.gz2 + (size_t)b0 * C, C, C, w.hst, F, F, n, 0, 0, gp[6] ? gp[6] : w.dummy, F, 1, 0, gp[7], w.wg, w.wg_floats, st)) return e;
  }
  const int nblk = (int)nl_cdiv(rq, SCT_LN_ROWS);
  if (want_lnb) {
    hipLaunchKernelGGL(sct_ln_part_kernel, dim3(nblk, C >> 6), dim3(256), 0, st, r.g_out, (const float*)r.keep.xb, (long long)rq, C, w.lnp);
    hipLaunchKernelGGL(sct_ln_sum_kernel, dim3(C >> 6), dim3(256), 0, st, (const float*)w.lnp, nblk, C, gp[ln + 2], gp[ln + 3]);
  }
  if (want_lna) {
    hipLaunchKernelGGL(sct_ln_part_kernel, dim3(nblk, C >> 6), dim3(256), 0, st, (const float*)w.gy1, (const float*)r.keep.xa, (long long)rq, C, w.lnp);
    hipLaunchKernelGGL(sct_ln_sum_kernel, dim3(C >> 6), dim3(256), 0, st, (const float*)w.lnp, nblk, C, gp[ln], gp[ln + 1]);
  }
  NL_LAUNCH_CHECK();
  if (want_o)
    if (const int e = nl_launch_wgrad(w.gz1, C, C, r.keep.attn, C, C, rq, 0, 0, gp[2] ? gp[2] : w.dummy, C, 1, 0, gp[3], w.wg, w.wg_floats, st)) return e;
  if (!(want_in || in_x || in_m)) return NL_OK;

  // ---- attention
  hipLaunchKernelGGL(sct_dd_kernel, dim3((unsigned)nl_cdiv(rq * 8, 256)), dim3(256), 0, st, (const float*)w.gattn, (const float*)r.keep.attn, (long long)rq, C / SCT_HEADS,
                     w.dd);
  NL_LAUNCH_CHECK();
  SctAttnBwdArgs t;
  t.q = r.keep.q; t.k = r.keep.k; t.v = r.keep.v; t.dO = w.gattn; t.ml = r.keep.ml; t.dd = w.dd;
  t.dq = w.dq; t.dk = w.dk; t.dv = w.dv;
  t.Nq = r.Nq; t.Nk = r.Nk;
  t.scale = sct_scale(C);
  const bool self_tgt = !cross && in_x;   // a self layer's memory side is its own x
  const bool need_q = want_in || in_x, need_kv = want_in || in_m || self_tgt;
  auto pass = [&](auto kv, int64_t n_owned) {   // kv: std::bool_constant — the dK / dV pass, or the dQ pass
    t.nto = (int)nl_cdiv(n_owned, 32); t.items = r.B * SCT_HEADS * t.nto;
    return sct_by_head(C, [&](auto dh) {
      constexpr int DH = decltype(dh)::value;
      constexpr bool KV = decltype(kv)::value;
      return sct_launch<sct_attn_bwd_kernel<MODE, DH, KV>, sct_attn_bwd_kernel<MODE, DH, KV, SctDrop>>(nl_cdiv(t.items, 4), 0, 0, st, dp, t);
    });
  };
  if (need_q)
    if (const int e = pass(std::false_type{}, r.Nq)) return e;
  if (need_kv)
    if (const int e = pass(std::true_type{}, r.Nk)) return e;

  // ---- in_proj: weight and bias from (x + pos, mem + pos, mem)
  if (want_in) {
    hipLaunchKernelGGL(sct_add_kernel, dim3((unsigned)nl_cdiv(rq * (C >> 2), 256)), dim3(256), 0, st, r.x, r.xpos, w.xp, (size_t)rq * (C >> 2));
    const float* mp = w.xp;
    if (cross) {
      hipLaunchKernelGGL(sct_add_kernel, dim3((unsigned)nl_cdiv(rk * (C >> 2), 256)), dim3(256), 0, st, r.mem, r.mpos, w.mp, (size_t)rk * (C >> 2));
      mp = w.mp;
    }
    NL_LAUNCH_CHECK();
    const float* dy[3] = {w.dq, w.dk, w.dv};
    const float* xs[3] = {w.xp, mp, r.mem};
    const int64_t rows[3] = {rq, rk, rk};
    for (int i = 0; i < 3; ++i)
      if (const int e = nl_launch_wgrad(dy[i], C, C, xs[i], C, C, rows[i], 0, 0, gp[0] ? gp[0] + (size_t)i * C * C : w.dummy, C, 1, 0, gp[1] ? gp[1] + i * C : nullptr,
                                        w.wg, w.wg_floats, st))
        return e;
  }
  // ---- towards the inputs
  SctProjBwdArgs p;
  p.C = C;
  if (in_x) {
    p.a[0] = w.dq; p.a[1] = w.dq; p.w[0] = sct_mat(r.timg, T.m[l][0], C); p.w[1] = p.w[0]; p.na = 1;
    p.out_sum = r.g_x; p.out_first = r.g_xpos; p.rows = rq;
    hipLaunchKernelGGL(sct_proj_bwd_kernel<MODE>, dim3((unsigned)nl_cdiv(rq, 32)), dim3(256), sct_proj_lds(C), st, p);
  }
  if (cross ? in_m : in_x) {
    p.a[0] = w.dk; p.a[1] = w.dv; p.w[0] = sct_mat(r.timg, T.m[l][1], C); p.w[1] = sct_mat(r.timg, T.m[l][2], C); p.na = 2;
    p.out_sum = cross ? r.g_mem : r.g_x; p.out_first = cross ? r.g_mpos : r.g_xpos; p.rows = rk;
    hipLaunchKernelGGL(sct_proj_bwd_kernel<MODE>, dim3((unsigned)nl_cdiv(rk, 32)), dim3(256), sct_proj_lds(C), st, p);
  }
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int sct_fwd_train(const SctLayerFwd& r, hipStream_t st) {
  if (r.precision == NL_PREC_F32) return sct_layer_forward_train<SCT_F32>(r, st);
  if (r.precision == NL_PREC_BF16X3) return sct_layer_forward_train<SCT_X3>(r, st);
  return sct_layer_forward_train<SCT_BF>(r, st);
}
int sct_bwd(const SctLayerBwd& r, int precision, const SctBwdWs& w, hipStream_t st) {
  if (precision == NL_PREC_F32) return sct_layer_backward<SCT_F32>(r, w, st);
  if (precision == NL_PREC_BF16X3) return sct_layer_backward<SCT_X3>(r, w, st);
  return sct_layer_backward<SCT_BF>(r, w, st);
}

// the size queries' answer to a shape a call would refuse: 0
bool sct_shape_ok(int64_t B, int64_t N0, int64_t N1, int C, int F) {
  bool empty;
  return sct_shape_status(C, SCT_HEADS, F, NL_PREC_F32, B, N0, N1, &empty) == NL_OK;
}
bool sct_all16(const void* const* p, int n, bool required) {
  for (int i = 0; i < n; ++i)
    if ((required && !p[i]) || ((uintptr_t)p[i] & 15) != 0) return false;
  return true;
}
// What the two backward entry points check alike before anything is dereferenced: both images, the rows a call needs (req) and may leave out (opt), and the grads
// array, which may be null and else holds n_want pointers, each null or aligned
int sct_bwd_args_status(const void* packed, const void* train_packed, const void* const* req, int nreq, const void* const* opt, int nopt, float* const* grads,
                        int n_grads, int n_want) {
  if (!packed || !train_packed || (((uintptr_t)packed | (uintptr_t)train_packed) & 15) != 0) return NL_ERR_BAD_ARG;
  if (!sct_all16(req, nreq, true) || !sct_all16(opt, nopt, false)) return NL_ERR_BAD_ARG;
  if (grads && (n_grads != n_want || !sct_all16((const void* const*)grads, n_want, false))) return NL_ERR_BAD_ARG;
  return NL_OK;
}
// ... and clear alike.  gp[i]: the requested gradient of tensor i of layers [l0, l1), counted from the first of them — null where it is not asked for and for a
// decoder layer's norm1, which is never applied; any[l]: layer l has one.  Those and the four input-gradient targets (tgt[0], tgt[1]: b0 bytes; tgt[2], tgt[3]:
// b1 bytes) are zeroed.
int sct_bwd_zero(float* const* grads, int l0, int l1, int C, int F, float** gp, bool* any, float* const (&tgt)[4], size_t b0, size_t b1, hipStream_t st) {
  for (int l = l0; l < l1; ++l) {
    any[l] = false;
    for (int k = 0; k < sct_param_count(l); ++k) {
      const int i = sct_param_first(l) - sct_param_first(l0) + k;
      gp[i] = grads && sct_param_applied(l, k) ? grads[i] : nullptr;
      if (gp[i]) {
        any[l] = true;
        NL_CHECK_HIP(hipMemsetAsync(gp[i], 0, sct_param_floats(k, C, F) * 4, st));
      }
    }
  }
  for (int i = 0; i < 4; ++i)
    if (tgt[i]) NL_CHECK_HIP(hipMemsetAsync(tgt[i], 0, i < 2 ? b0 : b1, st));
  return NL_OK;
}

// ---- the keep mask of one site, one byte per element, by the kernels' own function (nl_sct_dropout_mask).  site 0: out[(b * 8 + h) * Nq + q][k], n = Nk;
// sites 1 - 3: out[b * Nq + q][column], n = the width
__global__ __launch_bounds__(256) void sct_drop_mask_kernel(const SctDrop d, int site, long long Nq, long long n, long long total, unsigned char* out) {
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= total) return;
  const long long row = e / n, c = e - row * n;
  bool keep;
  if (site == 0) {
    const long long g = row / Nq;
    keep = sct_drop_keep_at(d, 0, (unsigned)g, (unsigned)c, (unsigned)(row - g * Nq));
  } else {
    keep = sct_drop_keep_at(d, site, 0, (unsigned)row, (unsigned)c);
  }
  out[e] = keep ? 1 : 0;
}

int sct_forward_train_impl(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1,
                           const float* pos1, int64_t N1, int64_t B, float* out0, float* out1, void* state, size_t state_bytes, void* ws, size_t ws_bytes, float p,
                           unsigned long long seed, void* stream) {
  const void* ptrs[6] = {v0, pos0, v1, pos1, out0, out1};
  bool empty;
  if (const int s = sct_check(packed, C, nhead, F, precision, B, N0, N1, ptrs, 6, ws, ws_bytes, &empty)) return s;
  if (empty) return NL_OK;
  if (out0 == out1) return NL_ERR_BAD_ARG;
  if (!state || ((uintptr_t)state & 255) != 0 || state_bytes < nl_sct_train_state_bytes(B, N0, N1, C, F)) return NL_ERR_WORKSPACE;
  if (!sct_drop_p_ok(p)) return NL_ERR_BAD_ARG;
  const unsigned char* img = (const unsigned char*)packed;
  hipStream_t st = (hipStream_t)stream;
  SctKeep k[SCT_LAYERS];
  sct_state_carve((unsigned char*)state, B, N0, N1, C, k);
  const SctLayerFwd r[SCT_LAYERS] = {{img, C, F, 0, precision, v0, pos0, v0, pos0, N0, N0, B, out0, k[0], true, p, seed},
                                     {img, C, F, 1, precision, v1, pos1, v1, pos1, N1, N1, B, out1, k[1], true, p, seed},
                                     {img, C, F, 2, precision, out0, pos0, out1, pos1, N0, N1, B, out0, k[2], true, p, seed},
                                     {img, C, F, 3, precision, out1, pos1, out0, pos0, N1, N0, B, out1, k[3], false, p, seed}};
  for (int l = 0; l < SCT_LAYERS; ++l)
    if (const int s = sct_fwd_train(r[l], st)) return s;
  return NL_OK;
}

}  // namespace

extern "C" {

size_t nl_sct_train_packed_bytes(int C, int nhead, int F) { return sct_cfg_ok(C, nhead, F) ? sct_train_layout(C, F).total : 0; }

int nl_sct_pack_weights_train(int C, int nhead, int F, const float* const* tensors, int n_tensors, void* packed, size_t packed_bytes, void* stream) {
  if (!sct_cfg_ok(C, nhead, F)) return NL_ERR_UNSUPPORTED;
  if (!tensors || n_tensors != SCT_TENSORS || !packed || ((uintptr_t)packed & 15) != 0) return NL_ERR_BAD_ARG;
  for (int i = 0; i < SCT_TENSORS; ++i)
    if (!tensors[i]) return NL_ERR_BAD_ARG;
  if (packed_bytes < nl_sct_train_packed_bytes(C, nhead, F)) return NL_ERR_WORKSPACE;
  const SctTrainLayout L = sct_train_layout(C, F);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* img = (unsigned char*)packed;
  float* stage = (float*)(img + L.stage);
  for (int l = 0; l < SCT_LAYERS; ++l) {
    const float* const* t = tensors + sct_param_first(l);
    // source (rows x cols, torch layout) of the six transposes: the three blocks of in_proj_weight, out_proj, linear1, linear2
    const float* src[6] = {t[0], t[0] + (size_t)C * C, t[0] + (size_t)2 * C * C, t[2], t[4], t[6]};
    const int rows[6] = {C, C, C, C, F, C}, cols[6] = {C, C, C, C, C, F};
    for (int k = 0; k < 6; ++k) {
      const SctMatOff& m = L.m[l][k];
      if (const int e = nl_launch_transpose(src[k], rows[k], cols[k], stage, st)) return e;   // (cols x rows): N = cols, K = rows
      if (const int e = nl_launch_frag_pack(stage, cols[k], rows[k], (unsigned short*)(img + m.bf), nullptr, (unsigned short*)(img + m.hi),
                                            (unsigned short*)(img + m.lo), (float*)(img + m.f32), false, st))
        return e;
    }
  }
  return NL_OK;
}

size_t nl_sct_train_state_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F) {
  if (!sct_shape_ok(B, N0, N1, C, F)) return 0;
  SctKeep k[SCT_LAYERS];
  return sct_state_carve(nullptr, B ? B : 1, N0, N1, C, k);
}

int nl_sct_forward_train(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1,
                         const float* pos1, int64_t N1, int64_t B, float* out0, float* out1, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                         void* stream) {
  return sct_forward_train_impl(packed, C, nhead, F, precision, v0, pos0, N0, v1, pos1, N1, B, out0, out1, state, state_bytes, ws, ws_bytes, 0.f, 0, stream);
}
int nl_sct_forward_train_dropout(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1,
                                 const float* pos1, int64_t N1, int64_t B, float* out0, float* out1, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                                 float p, uint64_t seed, void* stream) {
  return sct_forward_train_impl(packed, C, nhead, F, precision, v0, pos0, N0, v1, pos1, N1, B, out0, out1, state, state_bytes, ws, ws_bytes, p, seed, stream);
}

size_t nl_sct_backward_workspace_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F) {
  if (!sct_shape_ok(B, N0, N1, C, F)) return 0;
  return sct_bwd_ws(nullptr, B ? B : 1, N0, N1, C, F, false).total;
}

size_t nl_sct_layer_backward_workspace_bytes(int64_t B, int64_t Nq, int64_t Nk, int C, int F) {
  if (!sct_shape_ok(B, Nq, Nk, C, F)) return 0;
  return sct_bwd_ws(nullptr, B ? B : 1, Nq, Nk, C, F, true).total;
}

static int sct_backward_impl(const void* packed, const void* train_packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0,
                             const float* v1, const float* pos1, int64_t N1, int64_t B, const void* state, size_t state_bytes, const float* g_out0,
                             const float* g_out1, float* g_v0, float* g_pos0, float* g_v1, float* g_pos1, float* const* grads, int n_grads, void* ws, size_t ws_bytes,
                             float p, unsigned long long seed, void* stream) {
  bool empty;
  if (const int s = sct_shape_status(C, nhead, F, precision, B, N0, N1, &empty)) return s;
  if (empty) return NL_OK;
  const void* in[4] = {v0, pos0, v1, pos1};
  const void* opt[6] = {g_out0, g_out1, g_v0, g_pos0, g_v1, g_pos1};
  if (const int s = sct_bwd_args_status(packed, train_packed, in, 4, opt, 6, grads, n_grads, SCT_TENSORS)) return s;
  if (!state || ((uintptr_t)state & 255) != 0 || state_bytes < nl_sct_train_state_bytes(B, N0, N1, C, F)) return NL_ERR_WORKSPACE;
  if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < nl_sct_backward_workspace_bytes(B, N0, N1, C, F)) return NL_ERR_WORKSPACE;
  if (!sct_drop_p_ok(p)) return NL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const unsigned char* img = (const unsigned char*)packed;
  const unsigned char* timg = (const unsigned char*)train_packed;
  SctKeep k[SCT_LAYERS];
  sct_state_carve((unsigned char*)state, B, N0, N1, C, k);
  const SctBwdWs w = sct_bwd_ws((unsigned char*)ws, B, N0, N1, C, F, false);
  const size_t b0 = (size_t)B * N0 * C * 4, b1 = (size_t)B * N1 * C * 4;

  float* gp[SCT_TENSORS];
  bool anyp[SCT_LAYERS];
  if (const int s = sct_bwd_zero(grads, 0, SCT_LAYERS, C, F, gp, anyp, {g_v0, g_pos0, g_v1, g_pos1}, b0, b1, st)) return s;
  if (!g_out0 && !g_out1) return NL_OK;   // zero cotangents: every gradient is zero

  // which layers anything asked for depends on; a layer's gradient towards a side nobody needs is not formed
  const bool need0 = anyp[0] || g_v0 || g_pos0, need1 = anyp[1] || g_v1 || g_pos1;
  const bool need2 = anyp[2] || need0 || need1 || g_pos0 || g_pos1;
  const bool run3 = g_out1 != nullptr;
  if (need0) NL_CHECK_HIP(hipMemsetAsync(w.G[0], 0, b0, st));
  if (need1) NL_CHECK_HIP(hipMemsetAsync(w.G[1], 0, b1, st));
  if (need2) {
    if (g_out0) NL_CHECK_HIP(hipMemcpyAsync(w.G[2], g_out0, b0, hipMemcpyDeviceToDevice, st));
    else NL_CHECK_HIP(hipMemsetAsync(w.G[2], 0, b0, st));
  }
  if (run3) {
    const SctLayerBwd r{img, timg, C, F, 3, k[1].out, pos1, k[2].out, pos0, N1, N0, B, k[3], g_out1, need1 ? w.G[1] : nullptr, g_pos1, need2 ? w.G[2] : nullptr, g_pos0,
                        gp + sct_param_first(3), p, seed};
    if (const int s = sct_bwd(r, precision, w, st)) return s;
  }
  if (need2) {
    const SctLayerBwd r{img, timg, C, F, 2, k[0].out, pos0, k[1].out, pos1, N0, N1, B, k[2], w.G[2], need0 ? w.G[0] : nullptr, g_pos0, need1 ? w.G[1] : nullptr, g_pos1,
                        gp + sct_param_first(2), p, seed};
    if (const int s = sct_bwd(r, precision, w, st)) return s;
  }
  if (need1) {
    const SctLayerBwd r{img, timg, C, F, 1, v1, pos1, v1, pos1, N1, N1, B, k[1], w.G[1], g_v1, g_pos1, nullptr, nullptr, gp + sct_param_first(1), p, seed};
    if (const int s = sct_bwd(r, precision, w, st)) return s;
  }
  if (need0) {
    const SctLayerBwd r{img, timg, C, F, 0, v0, pos0, v0, pos0, N0, N0, B, k[0], w.G[0], g_v0, g_pos0, nullptr, nullptr, gp, p, seed};
    if (const int s = sct_bwd(r, precision, w, st)) return s;
  }
  return NL_OK;
}

int nl_sct_backward(const void* packed, const void* train_packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0,
                    const float* v1, const float* pos1, int64_t N1, int64_t B, const void* state, size_t state_bytes, const float* g_out0, const float* g_out1,
                    float* g_v0, float* g_pos0, float* g_v1, float* g_pos1, float* const* grads, int n_grads, void* ws, size_t ws_bytes, void* stream) {
  return sct_backward_impl(packed, train_packed, C, nhead, F, precision, v0, pos0, N0, v1, pos1, N1, B, state, state_bytes, g_out0, g_out1, g_v0, g_pos0, g_v1, g_pos1,
                           grads, n_grads, ws, ws_bytes, 0.f, 0, stream);
}
int nl_sct_backward_dropout(const void* packed, const void* train_packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0,
                            const float* v1, const float* pos1, int64_t N1, int64_t B, const void* state, size_t state_bytes, const float* g_out0,
                            const float* g_out1, float* g_v0, float* g_pos0, float* g_v1, float* g_pos1, float* const* grads, int n_grads, void* ws, size_t ws_bytes,
                            float p, uint64_t seed, void* stream) {
  return sct_backward_impl(packed, train_packed, C, nhead, F, precision, v0, pos0, N0, v1, pos1, N1, B, state, state_bytes, g_out0, g_out1, g_v0, g_pos0, g_v1, g_pos1,
                           grads, n_grads, ws, ws_bytes, p, seed, stream);
}

static int sct_layer_backward_impl(const void* packed, const void* train_packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos,
                                   int64_t Nq, const float* mem, const float* mem_pos, int64_t Nk, int64_t B, const float* g_out, float* g_x, float* g_x_pos,
                                   float* g_mem, float* g_mem_pos, float* const* grads, int n_grads, void* ws, size_t ws_bytes, float p, unsigned long long seed,
                                   void* stream) {
  if (layer < 0 || layer >= SCT_LAYERS) return NL_ERR_BAD_ARG;
  const bool cross = layer >= 2;
  if (!cross) {   // self layers: the memory side is the target side, and its gradient is part of g_x / g_x_pos
    if ((mem && mem != x) || (mem_pos && mem_pos != x_pos) || Nk != Nq || g_mem || g_mem_pos) return NL_ERR_BAD_ARG;
    mem = x; mem_pos = x_pos;
  }
  bool empty;
  if (const int s = sct_shape_status(C, nhead, F, precision, B, Nq, Nk, &empty)) return s;
  if (empty) return NL_OK;
  const void* in[5] = {x, x_pos, mem, mem_pos, g_out};
  const void* opt[4] = {g_x, g_x_pos, g_mem, g_mem_pos};
  if (const int s = sct_bwd_args_status(packed, train_packed, in, 5, opt, 4, grads, n_grads, sct_param_count(layer))) return s;
  if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < nl_sct_layer_backward_workspace_bytes(B, Nq, Nk, C, F)) return NL_ERR_WORKSPACE;
  if (!sct_drop_p_ok(p)) return NL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const SctBwdWs w = sct_bwd_ws((unsigned char*)ws, B, Nq, Nk, C, F, true);
  SctKeep k;
  sct_keep_carve((unsigned char*)ws, w.keep_off, B * Nq, B * Nk, C, k, true);
  const unsigned char* img = (const unsigned char*)packed;
  const SctLayerFwd f{img, C, F, layer, precision, x, x_pos, mem, mem_pos, Nq, Nk, B, w.lout, k, false, p, seed};
  if (const int s = sct_fwd_train(f, st)) return s;
  float* gp[14];
  bool anyp[SCT_LAYERS];
  if (const int s = sct_bwd_zero(grads, layer, layer + 1, C, F, gp, anyp, {g_x, g_x_pos, g_mem, g_mem_pos}, (size_t)B * Nq * C * 4, (size_t)B * Nk * C * 4, st)) return s;
  const SctLayerBwd r{img, (const unsigned char*)train_packed, C, F, layer, x, x_pos, mem, mem_pos, Nq, Nk, B, k, g_out, g_x, g_x_pos, g_mem, g_mem_pos, gp, p, seed};
  return sct_bwd(r, precision, w, st);
}

int nl_sct_layer_backward(const void* packed, const void* train_packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos,
                          int64_t Nq, const float* mem, const float* mem_pos, int64_t Nk, int64_t B, const float* g_out, float* g_x, float* g_x_pos, float* g_mem,
                          float* g_mem_pos, float* const* grads, int n_grads, void* ws, size_t ws_bytes, void* stream) {
  return sct_layer_backward_impl(packed, train_packed, C, nhead, F, layer, precision, x, x_pos, Nq, mem, mem_pos, Nk, B, g_out, g_x, g_x_pos, g_mem, g_mem_pos, grads,
                                 n_grads, ws, ws_bytes, 0.f, 0, stream);
}
int nl_sct_layer_backward_dropout(const void* packed, const void* train_packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos,
                                  int64_t Nq, const float* mem, const float* mem_pos, int64_t Nk, int64_t B, const float* g_out, float* g_x, float* g_x_pos,
                                  float* g_mem, float* g_mem_pos, float* const* grads, int n_grads, void* ws, size_t ws_bytes, float p, uint64_t seed, void* stream) {
  return sct_layer_backward_impl(packed, train_packed, C, nhead, F, layer, precision, x, x_pos, Nq, mem, mem_pos, Nk, B, g_out, g_x, g_x_pos, g_mem, g_mem_pos, grads,
                                 n_grads, ws, ws_bytes, p, seed, stream);
}

int nl_sct_dropout_mask(uint64_t seed, float p, int layer, int site, int64_t B, int64_t Nq, int64_t n, uint8_t* out, void* stream) {
  if (layer < 0 || layer >= SCT_LAYERS || site < 0 || site > 3 || !sct_counts_ok(B, Nq, n) || !sct_drop_p_ok(p)) return NL_ERR_BAD_ARG;
  if (!sct_counts_fit(B, Nq, n, Nq)) return NL_ERR_UNSUPPORTED;
  const long long rows = (site == 0 ? 8 : 1) * B * Nq;
  if ((double)rows * (double)n > 2147483647.0 * 256.0) return NL_ERR_UNSUPPORTED;   // one thread per element, a 32-bit grid
  if (B == 0) return NL_OK;
  if (!out) return NL_ERR_BAD_ARG;
  const SctDrop d = sct_drop_make(p, seed, layer);
  const long long total = rows * n;
  hipLaunchKernelGGL(sct_drop_mask_kernel, dim3((unsigned)nl_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, d, site, (long long)Nq, (long long)n, total, out);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // extern "C"
