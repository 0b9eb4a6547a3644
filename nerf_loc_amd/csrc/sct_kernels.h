// The SelfCrossTransformer's inference kernels and their host driver, shared by sct.hip (libnerfloc_render.so: nl_sct_*) and counted.hip (libnerfloc_counted.so:
// nlk_sct_*), as pnp_kernels.h and cnn_kernels.h are shared: the projection and attention kernels, SctRun, sct_run_layer and sct_run.  sct.hip's header describes
// the kernels.  The attention kernel's trailing pack holds an SctDrop (the training forward with dropout), an SctCount (the counted form: the number of keys lies
// in device memory) or nothing: the kernel as it was.  Only counted.hip instantiates the counted form (sct_run<true>).
#pragma once
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
//
// COUNTED (a trailing SctCount): only keys 0 .. n - 1 exist, n = clamp(*cnt.n, 0, a.Nk) read once per wave; a.Nk is the CAPACITY — the batch stride of k / v and what
// the host sized the grid for.  Nk, nkt, lg and tps are derived from n by the host's own rule (sct_run_layer), so the key ranges, and with them every bit of a row,
// are those of the exact-size call on n keys.  lg(n) <= lg(capacity): with the device's lg a workgroup holds at least as many items as the host assumed, the
// block-to-item map covers every item, and surplus waves find item >= items.  Everything derived from n is wave-uniform (readfirstlane).  Keys at and beyond n are
// never loaded (the clamp below); n == 0 loads nothing and writes zeros.
struct SctCount { const int* n; };

template <int MODE, int DH, class... EXTRA>
__global__ __launch_bounds__(256) void sct_attn_kernel(const SctAttnArgs a, const EXTRA... extra) {
  constexpr bool DROP = (std::is_same_v<EXTRA, SctDrop> || ...), COUNTED = (std::is_same_v<EXTRA, SctCount> || ...);
  [[maybe_unused]] const auto d = sct_arg<SctDrop>(extra...);
  [[maybe_unused]] const auto cnt = sct_arg<SctCount>(extra...);
  if constexpr (MODE == SCT_X3) __builtin_amdgcn_s_setreg(1473, 1);
  __shared__ float part[4][18][64];   // per wave: running maximum, sum, and the 16 accumulator registers, lane-major
  constexpr int C = 8 * DH;
  constexpr int KS = DH <= 16 ? 1 : 2;   // 16-wide k steps of the (zero-padded) head dimension
  constexpr int HD = DH / 2;             // fp32: half-wave hh multiplies dimensions hh * HD .. hh * HD + HD - 1
  constexpr int KF = MODE == SCT_F32 ? HD : 8 * KS;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  long long Nk = a.Nk;
  int nkt = a.nkt, lg = a.lg, tps = a.tps;
  if constexpr (COUNTED) {
    const int raw = __builtin_amdgcn_readfirstlane(*cnt.n);   // a scalar load: the address is a kernel argument
    const int n = raw < 0 ? 0 : raw < (int)a.Nk ? raw : (int)a.Nk;
    Nk = n;
    nkt = (n + 31) >> 5;
    lg = nkt >= 16 ? 2 : nkt >= 4 ? 1 : 0;
    tps = (nkt + (1 << lg) - 1) >> lg;
  }
  const long long item = (long long)blockIdx.x * (4 >> lg) + (wave >> lg), Nq = a.Nq;
  const int sp = wave & ((1 << lg) - 1);
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
    const float* kbase = a.k + (size_t)b * a.Nk * C + h * DH;
    const float* vbase = a.v + (size_t)b * a.Nk * C + h * DH + (col < DH ? col : DH - 1);   // channel rows >= DH of O^T repeat the last one and are not stored

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

    const int t0 = sp * tps, t1 = t0 + tps < nkt ? t0 + tps : nkt;
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
    const int ns = 1 << lg;
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
      if constexpr (COUNTED) {
        if (c < DH) op[c] = Nk > 0 ? ot[r] / lt : 0.f;   // no key at all: every range is empty, mt = -inf and the factors are NaN
      } else {
        if (c < DH) op[c] = ot[r] / lt;
      }
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
  const int* nk_dev = nullptr;    // sct_run<true> alone: the key count in device memory (Nk is then the capacity); null: all Nk keys, the plain kernel
};

// COUNTED: the unit may launch the counted attention kernel (r.nk_dev).  sct.hip instantiates <.., false> only, so libnerfloc_render.so holds no counted kernel.
template <int MODE, bool COUNTED>
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
  const int e = sct_by_head(C, [&](auto dh) -> int {
    constexpr int DH = decltype(dh)::value;
    if constexpr (COUNTED) {
      if (r.nk_dev) {   // the grid is the capacity's: never smaller than the count's
        hipLaunchKernelGGL((sct_attn_kernel<MODE, DH, SctCount>), dim3((unsigned)nl_cdiv(t.items, 4 >> t.lg)), dim3(256), 0, st, t, SctCount{r.nk_dev});
        NL_LAUNCH_CHECK();
        return (int)NL_OK;
      }
    }
    return sct_launch<sct_attn_kernel<MODE, DH>, sct_attn_kernel<MODE, DH, SctDrop>>(nl_cdiv(t.items, 4 >> t.lg), 0, 0, st, r.drop, t);
  });
  if (e || r.keep) return e;
  hipLaunchKernelGGL(sct_chain_kernel<MODE>, dim3((unsigned)nl_cdiv(rowsq, 32)), dim3(256), sct_chain_lds(C, F), st, sct_chain_args(r.img, lo, C, F, ab, r.x, r.out, rowsq));
  NL_LAUNCH_CHECK();
  return NL_OK;
}

template <bool COUNTED = false>
int sct_run(const SctRun& r, int precision, hipStream_t st) {
  if (precision == NL_PREC_F32) return sct_run_layer<SCT_F32, COUNTED>(r, st);
  if (precision == NL_PREC_BF16X3) return sct_run_layer<SCT_X3, COUNTED>(r, st);
  return sct_run_layer<SCT_BF, COUNTED>(r, st);
}

}  // namespace
