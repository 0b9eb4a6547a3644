// SelfCrossTransformer (reference: models/COTR/transformer.py:17-64, 171-250): four post-norm layers (self v0, self v1, cross v0 <- v1, cross v1 <- new v0), each
// three kernels on rows flattened over the batch ([B * N][C] fp32, batch first).  The kernels serve three uses.  Inference (eval mode) is this file's entry points.
// The training forward (sct_bwd.hip) launches the same projections and attention from here, into rows it keeps (nl_launch_sct_qkv_attn), and the row chain itself,
// with the stores of what the backward needs.  The training forward with dropout takes the attention's and the chain's instantiations with a trailing SctDrop
// argument (sct_drop.h); a kernel without that argument is the kernel as it was.
//
// sct_proj_kernel   q / k / v = (x [+ pos]) . W^T + b.  A workgroup owns 32 rows: x and x + pos are formed once while the tile is loaded into LDS (no x + pos tensor),
//   the four waves share the 32-column output blocks of in_proj_weight; [q; k] blocks multiply the x + pos tile, v blocks the x tile.  Cross layers launch it twice
//   (q from the target side, k and v once from the memory side).
// sct_attn_kernel   flash-style attention: a wave owns (batch item, head, 32-query tile, key range).  S^T = K . Q^T on the 32x32 MFMAs puts a query in a lane's
//   COLUMN, so a row's running maximum and sum are in-lane reductions over the 16 accumulator registers plus one exchange between the half-waves, and the probabilities
//   are already the B operand of O^T = V^T . P^T (k slot (hh, j) of step s = accumulator register 8 s + j; the V fragment is gathered in that key order).  Keys beyond Nk
//   get -inf before the maximum; their loads are clamped to the last key.  The next key tile's K / V values are fetched before the current tile's arithmetic.  A long
//   key sequence is cut into 2 or 4 ranges (>= 4 / >= 16 tiles) held by neighbouring waves of the workgroup, whose (maximum, sum, accumulator) meet in 18 KB of LDS and
//   are added in range order by the first of them: with one range per item the 4800 x 4800 layer is 1200 waves for 1024 SIMDs, each waiting on its own loads.
//   No Nq x Nk value ever reaches memory.  The head dimension (8 / 16 / 24 / 32) is padded with zero k slots to 16 / 32; fp32 mode needs no padding (k step 2).
//   The same kernel serves every Nq, also Nq == 1 (the fine shape: B x 8 waves with one live column each, four (batch item, head) pairs to a workgroup): a row's bits
//   must not depend on how many rows or batch items the call holds (tests/test_gpu_sct.py), which rules out a second kernel chosen by Nq or B; the number of key
//   ranges depends on Nk alone.
// sct_chain_kernel  (sct.h) out_proj, + residual, LayerNorm, linear1, ReLU, linear2, + residual, LayerNorm for 32 rows that stay in LDS from the attention output to the
//   layer output; the F-wide hidden rows live in LDS only.  The four waves split the output blocks of each product, so every weight fragment is read by exactly ONE wave
//   of the workgroup, straight from L2 in 1-KB coalesced pieces (fragment order): a copy through LDS would add a barrier pair per chunk and no reuse.
//   Measured: the kernel takes ~90 us per launch whatever the row count — it waits on these loads, which are not requested ahead of use; not yet changed.
//
// Precision: NL_PREC_F32 = v_mfma_f32_32x32x2_f32 on fp32 operands; NL_PREC_BF16X3 = three-term split-FP16 (mfma.h: hi = f16(v), lo = f16(v - hi)) for every product —
//   the logits feed a softmax (as in fine.hip) and one format keeps one code path; NL_PREC_BF16 = one bf16 product.  LayerNorm, softmax and residuals are fp32 everywhere.
// Every output row depends on its own row, the memory side, the weights and the mode only: fixed reduction orders, no atomics.
#include "common.h"
#include "mfma.h"
#include "host.h"
#include "sct.h"

namespace {

// ------------------------------------------------------------------------------------------ q / k / v projections
template <int MODE, int NB>
__device__ __forceinline__ void sct_proj_pass(const SctProjArgs& a, const float* tile, int lo, int hi, long long row0, int lane, int wave) {
  if (lo + wave >= hi) return;   // wave-uniform
  const int C = a.C, nc = C >> 5, hh = lane >> 5, col = lane & 31;
  nl_f32x16 acc[NB];
  nl_acc_zero(acc);
  sct_gemm<MODE, NB>(acc, tile + col * (C + SCT_PAD), C, a.w, lo + wave, hi, lane);
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    const int rb = lo + wave + 4 * i;
    if (rb >= hi) break;
    const int part = rb / nc, n = 32 * (rb - part * nc) + col;
    const float bv = a.bias[32 * rb + col];
    float* o = a.out[part];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long row = row0 + nl_acc_row(r, hh);
      if (row < a.rows) o[(size_t)row * C + n] = acc[i][r] + bv;
    }
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void sct_proj_kernel(const SctProjArgs a) {
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);   // MODE.FP16_OVFL: conversions to f16 saturate at 65504 (as fine.hip)
  extern __shared__ __attribute__((aligned(16))) float sct_smem[];
  const int C = a.C, ld = C + SCT_PAD, c4n = C >> 2, nc = C >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long row0 = (long long)blockIdx.x * 32;
  float* xp = sct_smem;             // x + pos
  float* xs = sct_smem + 32 * ld;   // x
  const bool need_p = a.rb_lo < 2 * nc, need_x = a.rb_hi > 2 * nc;   // the q-only launch of a cross layer has no v block: it neither stages nor reads the x tile
  for (int i = threadIdx.x; i < 32 * c4n; i += 256) {
    const int r = i / c4n, c = 4 * (i - r * c4n);
    const long long row = row0 + r < a.rows ? row0 + r : a.rows - 1;   // rows past the end repeat the last one and are not stored
    const float4 v = *(const float4*)(a.x + (size_t)row * C + c);
    if (need_x) *(float4*)(xs + r * ld + c) = v;
    if (need_p) {
      const float4 p = *(const float4*)(a.pos + (size_t)row * C + c);
      *(float4*)(xp + r * ld + c) = make_float4(v.x + p.x, v.y + p.y, v.z + p.z, v.w + p.w);
    }
  }
  __syncthreads();
  sct_proj_pass<MODE, 4>(a, xp, a.rb_lo, a.rb_hi < 2 * nc ? a.rb_hi : 2 * nc, row0, lane, wave);
  sct_proj_pass<MODE, 2>(a, xs, a.rb_lo > 2 * nc ? a.rb_lo : 2 * nc, a.rb_hi, row0, lane, wave);
}

// ------------------------------------------------------------------------------------------ attention
// A wave's operands of one key tile as they come from memory: K row (k0 + column) of the head — fp32: the half-wave's DH / 2 dimensions, else the 8-wide groups
// 16 s + 8 hh (zeros where the group is padding) — and V[key of accumulator register r][the lane's channel].  Keys past Nk repeat the last one.
template <int MODE, int DH>
__device__ __forceinline__ void sct_attn_load(const float* kbase, const float* vbase, long long k0, long long Nk, int hh, int col,
                                              float (&kr)[MODE == SCT_F32 ? DH / 2 : (DH <= 16 ? 8 : 16)], float (&vr)[16]) {
  constexpr int C = 8 * DH;
  const long long krow = k0 + col < Nk ? k0 + col : Nk - 1;
  const float* kp = kbase + (size_t)krow * C;
  if constexpr (MODE == SCT_F32) {
#pragma unroll
    for (int t = 0; t < DH / 2; t += 4) {
      const float4 v = *(const float4*)(kp + hh * (DH / 2) + t);
      kr[t] = v.x; kr[t + 1] = v.y; kr[t + 2] = v.z; kr[t + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int s = 0; s < (DH <= 16 ? 1 : 2); ++s) {
      float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (16 * s + 8 * hh < DH) sct_load8(kp + 16 * s + 8 * hh, v);
#pragma unroll
      for (int j = 0; j < 8; ++j) kr[8 * s + j] = v[j];
    }
  }
  if (k0 + 32 <= Nk) {   // wave-uniform: a full tile needs no clamp, and its 16 rows sit at constant offsets
    const float* vp = vbase + (size_t)(k0 + 4 * hh) * C;
#pragma unroll
    for (int r = 0; r < 16; ++r) vr[r] = vp[((r & 3) + 8 * (r >> 2)) * C];
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const long long key = k0 + nl_acc_row(r, hh);
      vr[r] = vbase[(size_t)(key < Nk ? key : Nk - 1) * C];   // the probability is 0 there
    }
  }
}

// DROP (the training forward with dropout in effect, sct_drop.h site 0): the maximum and the sum stay those of the undropped softmax; only the operand of
// V^T . P^T is keep ? P / (1 - p) : 0.  The registers run along the keys: four generator calls per tile and lane, between the softmax and the second product.
template <int MODE, int DH, class... DROPARG>
__global__ __launch_bounds__(256) void sct_attn_kernel(const SctAttnArgs a, const DROPARG... drop) {
  constexpr bool DROP = sizeof...(DROPARG) != 0;
  [[maybe_unused]] const auto d = sct_arg<SctDrop>(drop...);
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);
  __shared__ float part[4][18][64];   // per wave: running maximum, sum, and the 16 accumulator registers, lane-major
  constexpr int C = 8 * DH;
  constexpr int KS = DH <= 16 ? 1 : 2;   // 16-wide k steps of the (zero-padded) head dimension
  constexpr int HD = DH / 2;             // fp32: half-wave hh multiplies dimensions hh * HD .. hh * HD + HD - 1
  constexpr int KF = MODE == SCT_F32 ? HD : 8 * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long item = (long long)blockIdx.x * (4 >> a.lg) + (wave >> a.lg), Nq = a.Nq, Nk = a.Nk;
  const int sp = wave & ((1 << a.lg) - 1);
  const bool valid = item < a.items;   // wave-uniform

  float m = -INFINITY, l = 0.f;
  nl_f32x16 o;
#pragma unroll
  for (int r = 0; r < 16; ++r) o[r] = 0.f;
  long long b = 0, q0 = 0;
  int h = 0;

  if (valid) {
    const long long bh = item / a.nqt;
    h = (int)(bh & 7); b = bh >> 3; q0 = (item - bh * a.nqt) * 32;
    const long long qrow = q0 + col < Nq ? q0 + col : Nq - 1;
    const float* qp = a.q + ((size_t)b * Nq + qrow) * C + h * DH;
    const float* kbase = a.k + (size_t)b * Nk * C + h * DH;
    const float* vbase = a.v + (size_t)b * Nk * C + h * DH + (col < DH ? col : DH - 1);   // channel rows >= DH of O^T repeat the last one and are not stored

    nl_i16x8 qh[KS], ql[KS];
    float qf[HD];
    if constexpr (MODE == SCT_F32) {
#pragma unroll
      for (int t = 0; t < HD; t += 4) {
        const float4 v = *(const float4*)(qp + hh * HD + t);
        qf[t] = v.x * a.scale; qf[t + 1] = v.y * a.scale; qf[t + 2] = v.z * a.scale; qf[t + 3] = v.w * a.scale;
      }
    } else {
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (16 * s + 8 * hh < DH) sct_load8(qp + 16 * s + 8 * hh, v);
#pragma unroll
        for (int j = 0; j < 8; ++j) v[j] *= a.scale;
        sct_split8<MODE>(v, qh[s], ql[s]);
      }
    }

    const int t0 = sp * a.tps, t1 = t0 + a.tps < a.nkt ? t0 + a.tps : a.nkt;
    float kr[KF], vr[16];
    if (t0 < t1) sct_attn_load<MODE, DH>(kbase, vbase, (long long)t0 * 32, Nk, hh, col, kr, vr);
    for (int t = t0; t < t1; ++t) {
      const long long k0 = (long long)t * 32;
      // the next tile's operands are fetched before this tile's arithmetic
      float kn[KF], vn[16];
      if (t + 1 < t1) {   // wave-uniform
        sct_attn_load<MODE, DH>(kbase, vbase, k0 + 32, Nk, hh, col, kn, vn);
      } else {
#pragma unroll
        for (int j = 0; j < KF; ++j) kn[j] = kr[j];
#pragma unroll
        for (int r = 0; r < 16; ++r) vn[r] = vr[r];
      }
      // ---- S^T[key][query] of this tile
      nl_f32x16 st;
#pragma unroll
      for (int r = 0; r < 16; ++r) st[r] = 0.f;
      if constexpr (MODE == SCT_F32) {
#pragma unroll
        for (int t2 = 0; t2 < HD; ++t2) st = __builtin_amdgcn_mfma_f32_32x32x2f32(kr[t2], qf[t2], st, 0, 0, 0);
      } else {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          float v[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) v[j] = kr[8 * s + j];
          nl_i16x8 kh, kl;
          sct_split8<MODE>(v, kh, kl);
          st = sct_mfma<MODE>(kh, kl, qh[s], ql[s], st);
        }
      }
      // ---- online softmax of the lane's query: keys past Nk leave the maximum and the sum
      if (k0 + 32 > Nk) {
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (k0 + nl_acc_row(r, hh) >= Nk) st[r] = -INFINITY;
      }
      float mx = st[0];
#pragma unroll
      for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
      mx = fmaxf(mx, __shfl_xor(mx, 32));
      const float mnew = fmaxf(m, mx);   // finite: key k0 is valid
      const float alpha = __expf(m - mnew);
      float p[16], ps = 0.f;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        p[r] = __expf(st[r] - mnew);
        ps += p[r];
      }
      ps += __shfl_xor(ps, 32);
      l = l * alpha + ps;
      m = mnew;
#pragma unroll
      for (int r = 0; r < 16; ++r) o[r] *= alpha;
      if constexpr (DROP) {
        const unsigned keep = sct_drop_bits_major(d, 0, (unsigned)(b * 8 + h), (unsigned)k0, hh, (unsigned)(q0 + col));
#pragma unroll
        for (int r = 0; r < 16; ++r) p[r] = sct_drop_apply(d, keep, r, p[r]);
      }
      // ---- O^T[channel][query] += V^T . P^T; k slot (hh, j) of step s is accumulator register 8 s + j, i.e. key k0 + nl_acc_row(8 s + j, hh)
      if constexpr (MODE == SCT_F32) {
#pragma unroll
        for (int r = 0; r < 16; ++r) o = __builtin_amdgcn_mfma_f32_32x32x2f32(vr[r], p[r], o, 0, 0, 0);
      } else {
#pragma unroll
        for (int s = 0; s < 2; ++s) {
          float v[8], pv[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) { v[j] = vr[8 * s + j]; pv[j] = p[8 * s + j]; }
          nl_i16x8 vh, vl, ph, pl;
          sct_split8<MODE>(v, vh, vl);
          sct_split8<MODE>(pv, ph, pl);
          o = sct_mfma<MODE>(vh, vl, ph, pl, o);
        }
      }
#pragma unroll
      for (int j = 0; j < KF; ++j) kr[j] = kn[j];
#pragma unroll
      for (int r = 0; r < 16; ++r) vr[r] = vn[r];
    }
  }

  // ---- the key ranges of an item meet in LDS; its first wave adds them in range order (one range: the factor is exp(0) = 1, the sum the wave's own)
  part[wave][0][lane] = m;
  part[wave][1][lane] = l;
#pragma unroll
  for (int r = 0; r < 16; ++r) part[wave][2 + r][lane] = o[r];
  __syncthreads();
  if (valid && sp == 0 && q0 + col < Nq) {
    const int ns = 1 << a.lg;
    float mt = m;
    for (int s = 1; s < ns; ++s) mt = fmaxf(mt, part[wave + s][0][lane]);
    float lt = 0.f, ot[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) ot[r] = 0.f;
    for (int s = 0; s < ns; ++s) {
      const float f = __expf(part[wave + s][0][lane] - mt);   // an empty range: exp(-inf) = 0 times its zeros
      lt += part[wave + s][1][lane] * f;
#pragma unroll
      for (int r = 0; r < 16; ++r) ot[r] += part[wave + s][2 + r][lane] * f;
    }
    float* op = a.out + ((size_t)b * Nq + q0 + col) * C + h * DH;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = nl_acc_row(r, hh);
      if (c < DH) op[c] = ot[r] / lt;
    }
  }
}

// ------------------------------------------------------------------------------------------ host side
struct SctRun {
  const unsigned char* img; int C, F, layer;
  const float* x; const float* xpos; int64_t Nq;
  const float* mem; const float* mpos; int64_t Nk;
  int64_t B; float* out; unsigned char* ws; size_t part;
  float* const* keep = nullptr;   // the training forward (sct_bwd.hip): q, k, v and the attention output go to these caller-owned rows and the row chain is left to it
  const SctDrop* drop = nullptr;  // ... with dropout in effect (thr > 0): the dropping attention kernel
};

template <int MODE>
int sct_run_layer(const SctRun& r, hipStream_t st) {
  const int C = r.C, F = r.F, nc = C >> 5;
  const SctLayout L = sct_layout(C, F);
  const SctLayerOff& lo = L.l[r.layer];
  const float* vec = (const float*)(r.img + lo.vec);
  float* qb = r.keep ? r.keep[0] : (float*)r.ws;
  float* kb = r.keep ? r.keep[1] : (float*)(r.ws + r.part);
  float* vb = r.keep ? r.keep[2] : (float*)(r.ws + 2 * r.part);
  float* ab = r.keep ? r.keep[3] : (float*)(r.ws + 3 * r.part);
  const long long rowsq = r.B * r.Nq, rowsk = r.B * r.Nk;
  const bool cross = r.layer >= 2;

  // the two kernels' dynamic LDS exceeds 64 KB at the larger configurations (per mode: one pair of flags per instantiation of this function)
  static std::atomic<unsigned long long> proj_set{0}, chain_set{0};
  if (const int e = nl_allow_dynamic_lds((const void*)sct_proj_kernel<MODE>, sct_proj_lds(256), proj_set)) return e;
  if (const int e = nl_allow_dynamic_lds((const void*)sct_chain_kernel<MODE>, sct_chain_lds(256, 512), chain_set)) return e;
  SctProjArgs p;
  p.x = r.x; p.pos = r.xpos;
  p.out[0] = qb; p.out[1] = kb; p.out[2] = vb;
  p.w = sct_mat(r.img, lo.m[0], 3 * C); p.bias = vec;
  p.rows = rowsq; p.C = C; p.rb_lo = 0; p.rb_hi = cross ? nc : 3 * nc;
  hipLaunchKernelGGL(sct_proj_kernel<MODE>, dim3((unsigned)nl_cdiv(rowsq, 32)), dim3(256), sct_proj_lds(C), st, p);
  if (cross) {   // k and v of the memory side, once
    p.x = r.mem; p.pos = r.mpos; p.rows = rowsk; p.rb_lo = nc; p.rb_hi = 3 * nc;
    hipLaunchKernelGGL(sct_proj_kernel<MODE>, dim3((unsigned)nl_cdiv(rowsk, 32)), dim3(256), sct_proj_lds(C), st, p);
  }

  SctAttnArgs t;
  t.q = qb; t.k = kb; t.v = vb; t.out = ab;
  t.Nq = r.Nq; t.Nk = r.Nk; t.nqt = (int)nl_cdiv(r.Nq, 32); t.nkt = (int)nl_cdiv(r.Nk, 32); t.items = r.B * SCT_HEADS * t.nqt;
  t.lg = t.nkt >= 16 ? 2 : t.nkt >= 4 ? 1 : 0;   // long key sequences are cut into 2 or 4 ranges: enough waves per SIMD to hide the loads; a function of Nk alone
  t.tps = (int)nl_cdiv(t.nkt, 1 << t.lg);
  t.scale = sct_scale(C);
  const int e = sct_by_head(C, [&](auto dh) {
    constexpr int DH = decltype(dh)::value;
    return sct_launch<sct_attn_kernel<MODE, DH>, sct_attn_kernel<MODE, DH, SctDrop>>(nl_cdiv(t.items, 4 >> t.lg), 0, 0, st, r.drop, t);
  });
  if (e || r.keep) return e;
  hipLaunchKernelGGL(sct_chain_kernel<MODE>, dim3((unsigned)nl_cdiv(rowsq, 32)), dim3(256), sct_chain_lds(C, F), st, sct_chain_args(r.img, lo, C, F, ab, r.x, r.out, rowsq));
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int sct_run(const SctRun& r, int precision, hipStream_t st) {
  if (precision == NL_PREC_F32) return sct_run_layer<SCT_F32>(r, st);
  if (precision == NL_PREC_BF16X3) return sct_run_layer<SCT_X3>(r, st);
  return sct_run_layer<SCT_BF>(r, st);
}

}  // namespace

int nl_launch_sct_qkv_attn(const void* img, int C, int F, int layer, int precision, const float* x, const float* xpos, int64_t Nq, const float* mem, const float* mpos,
                           int64_t Nk, int64_t B, float* q, float* k, float* v, float* attn, float drop_p, unsigned long long drop_seed, hipStream_t st) {
  float* const keep[4] = {q, k, v, attn};
  const SctDrop d = sct_drop_make(drop_p, drop_seed, layer);
  const SctRun r{(const unsigned char*)img, C, F, layer, x, xpos, Nq, mem, mpos, Nk, B, nullptr, nullptr, 0, keep, d.thr ? &d : nullptr};
  return sct_run(r, precision, st);
}

extern "C" {

size_t nl_sct_packed_bytes(int C, int nhead, int F) { return sct_cfg_ok(C, nhead, F) ? nl_align_up(sct_layout(C, F).total, 256) : 0; }

int nl_sct_pack_weights(int C, int nhead, int F, const float* const* tensors, int n_tensors, void* packed, size_t packed_bytes, void* stream) {
  if (!sct_cfg_ok(C, nhead, F)) return NL_ERR_UNSUPPORTED;
  if (!tensors || n_tensors != SCT_TENSORS || !packed || ((uintptr_t)packed & 15) != 0) return NL_ERR_BAD_ARG;
  for (int i = 0; i < SCT_TENSORS; ++i)
    if (!tensors[i]) return NL_ERR_BAD_ARG;
  if (packed_bytes < nl_sct_packed_bytes(C, nhead, F)) return NL_ERR_WORKSPACE;
  const SctLayout L = sct_layout(C, F);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* img = (unsigned char*)packed;
  for (int l = 0; l < SCT_LAYERS; ++l) {
    const float* const* t = tensors + sct_param_first(l);
    const int ln = sct_param_norm(l);
    const int N[4] = {3 * C, C, F, C}, K[4] = {C, C, C, F};
    for (int k = 0; k < 4; ++k) {
      const SctMatOff& m = L.l[l].m[k];
      if (const int e = nl_launch_frag_pack(t[2 * k], N[k], K[k], (unsigned short*)(img + m.bf), nullptr, (unsigned short*)(img + m.hi), (unsigned short*)(img + m.lo),
                                            (float*)(img + m.f32), false, st))
        return e;
    }
    float* vec = (float*)(img + L.l[l].vec);
    const float* src[8] = {t[1], t[3], t[5], t[7], t[ln], t[ln + 1], t[ln + 2], t[ln + 3]};
    const int cnt[8] = {3 * C, C, F, C, C, C, C, C};
    for (int k = 0; k < 8; ++k) {
      NL_CHECK_HIP(hipMemcpyAsync(vec, src[k], (size_t)cnt[k] * 4, hipMemcpyDeviceToDevice, st));
      vec += cnt[k];
    }
  }
  NL_LAUNCH_CHECK();
  return NL_OK;
}

size_t nl_sct_workspace_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F) {
  (void)F;   // the hidden rows never leave LDS
  if (!sct_counts_ok(B, N0, N1) || C < 1 || !sct_counts_fit(B, N0, N1, N0 > N1 ? N0 : N1)) return 0;
  return 4 * sct_ws_part(B ? B : 1, N0, N1, C);
}

int nl_sct_layer(const void* packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos, int64_t Nq, const float* mem,
                 const float* mem_pos, int64_t Nk, int64_t B, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (layer < 0 || layer >= SCT_LAYERS) return NL_ERR_BAD_ARG;
  if (layer < 2) {   // self layers: the memory side is the target side
    if ((mem && mem != x) || (mem_pos && mem_pos != x_pos) || Nk != Nq) return NL_ERR_BAD_ARG;
    mem = x; mem_pos = x_pos;
  }
  const void* ptrs[5] = {x, x_pos, mem, mem_pos, out};
  bool empty;
  if (const int s = sct_check(packed, C, nhead, F, precision, B, Nq, Nk, ptrs, 5, ws, ws_bytes, &empty)) return s;
  if (empty) return NL_OK;
  const SctRun r{(const unsigned char*)packed, C, F, layer, x, x_pos, Nq, mem, mem_pos, Nk, B, out, (unsigned char*)ws, sct_ws_part(B, Nq, Nk, C)};
  return sct_run(r, precision, (hipStream_t)stream);
}

int nl_sct_forward(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1, const float* pos1,
                   int64_t N1, int64_t B, float* out0, float* out1, void* ws, size_t ws_bytes, void* stream) {
  const void* ptrs[6] = {v0, pos0, v1, pos1, out0, out1};
  bool empty;
  if (const int s = sct_check(packed, C, nhead, F, precision, B, N0, N1, ptrs, 6, ws, ws_bytes, &empty)) return s;
  if (empty) return NL_OK;
  if (out0 == out1) return NL_ERR_BAD_ARG;
  const unsigned char* img = (const unsigned char*)packed;
  unsigned char* w = (unsigned char*)ws;
  const size_t part = sct_ws_part(B, N0, N1, C);
  hipStream_t st = (hipStream_t)stream;
  // out0 / out1 carry the self layers' results; the cross layers then work in place (transformer.py:57-61: layer 3 reads the OUTPUT of layer 2)
  const SctRun r[SCT_LAYERS] = {{img, C, F, 0, v0, pos0, N0, v0, pos0, N0, B, out0, w, part},
                                {img, C, F, 1, v1, pos1, N1, v1, pos1, N1, B, out1, w, part},
                                {img, C, F, 2, out0, pos0, N0, out1, pos1, N1, B, out0, w, part},
                                {img, C, F, 3, out1, pos1, N1, out0, pos0, N0, B, out1, w, part}};
  for (int l = 0; l < SCT_LAYERS; ++l)
    if (const int s = sct_run(r[l], precision, st)) return s;
  return NL_OK;
}

}  // extern "C"
