// Device helpers shared by the units that use MFMA, LDS-DMA or split precision (gfx950 only): ONE definition of what the kernel files used to copy —
// vector types, pair conversions, the 16-bit operand helpers of the 32x32x16 MFMAs (nl_frag, nl_split_pair, nl_mfma, nl_acc_zero) and the two fragment maps of a
// packed weight matrix (nl_frag16_src, nl_frag32_src: what pack.hip's frag_pack_kernel writes and what s2d.h, fine.hip and sct.hip read).
// Include after common.h.  Everything here is __device__ __forceinline__ or inline (no emitted symbol) and carries the nl_ prefix; kernels, argument structs and
// per-kernel geometry stay in their files.
#pragma once
#include <utility>
#include "common.h"

// ------------------------------------------------------------------ vector types (MFMA operands / accumulators, raw dword groups)
typedef __bf16 nl_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 nl_bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 nl_f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 nl_f16x2 __attribute__((ext_vector_type(2)));
typedef short nl_i16x8 __attribute__((ext_vector_type(8)));   // 8 bf16 / fp16 as raw 16-bit lanes (gemm.hip, s2d.h, fine.hip, sct.hip)
typedef unsigned short nl_u16x2 __attribute__((ext_vector_type(2)));
typedef int nl_i32x8 __attribute__((ext_vector_type(8)));
typedef float nl_f32x4 __attribute__((ext_vector_type(4)));
typedef float nl_f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned int nl_u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int nl_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int nl_u32x6 __attribute__((ext_vector_type(6)));
typedef unsigned int nl_u32x16 __attribute__((ext_vector_type(16)));

// ------------------------------------------------------------------ compile-time loop, waits, LDS-DMA
template <int... Is, class F>
__device__ __forceinline__ void nl_static_for_impl(std::integer_sequence<int, Is...>, F&& f) {
  (f(std::integral_constant<int, Is>{}), ...);
}
template <int N, class F>
__device__ __forceinline__ void nl_static_for(F&& f) {   // every index is a constant expression; N <= 0: no iteration
  nl_static_for_impl(std::make_integer_sequence<int, (N > 0 ? N : 0)>{}, static_cast<F&&>(f));
}
template <int N>
__device__ __forceinline__ void nl_wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"i"(N) : "memory");
}
// LDS-DMA of 16 B per lane; the immediate offset OFF is added to BOTH addresses, so four consecutive 1-KB pieces share one
// scalar base and one M0 value
template <int OFF = 0>
__device__ __forceinline__ void nl_glds16(const void* g, void* l) {
  __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                   (__attribute__((address_space(3))) void*)l, 16, OFF, 0);
}

// ------------------------------------------------------------------ pair conversions as single asm statements
__device__ __forceinline__ unsigned nl_cvt_pk_bf16(float a, float b) {   // low half = bf16(a), high half = bf16(b), round to nearest even
  unsigned r;
  asm("v_cvt_pk_bf16_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// lo word of a pair: bf16(v - float(hi))
__device__ __forceinline__ unsigned nl_lo2(float v0, float v1, unsigned hi) {
  unsigned lo; float t0, t1;
  asm("v_lshlrev_b32 %1, 16, %5\n\tv_and_b32 %2, 0xffff0000, %5\n\tv_sub_f32 %1, %3, %1\n\tv_sub_f32 %2, %4, %2\n\tv_cvt_pk_bf16_f32 %0, %1, %2"
      : "=&v"(lo), "=&v"(t0), "=&v"(t1) : "v"(v0), "v"(v1), "v"(hi));
  return lo;
}
// f16 pair of two values + the running maximum of their magnitudes
__device__ __forceinline__ unsigned nl_hi2_f16_amax(float v0, float v1, float& m) {
  unsigned hi;
  asm("v_max3_f32 %1, |%2|, |%3|, %1\n\tv_cvt_pk_f16_f32 %0, %2, %3" : "=&v"(hi), "+v"(m) : "v"(v0), "v"(v1));
  return hi;
}
// residuals of a pair as floats: v - float(f16 hi half) (exact)
__device__ __forceinline__ void nl_lo2_f32(float v0, float v1, unsigned hi, float& l0, float& l1) {
  asm("v_fma_mix_f32 %0, %4, -1.0, %2 op_sel_hi:[1,0,0]\n\tv_fma_mix_f32 %1, %4, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
      : "=&v"(l0), "=&v"(l1) : "v"(v0), "v"(v1), "v"(hi));
}
// The two fp6 packing conversions as asm statements with EARLY-CLOBBER results: hipcc 7.2 lets the builtins' 6-register result overlap the scale operand (seen:
// v_cvt_scalef32_2xpk16_fp6_f32 v[206:211], v[122:137], v[138:153], v206), and the multi-pass instruction then reads a scale it has already overwritten — one slab of
// one layer came out with garbage residuals (found with tools/mx6_debug.py: only K slab 2 of base_mlp.4 was off).  The only definitions in the library
// (tests/test_build_invariants.py keeps the builtins out and the "=&v" in).
__device__ __forceinline__ nl_u32x6 nl_cvt_pk32_fp6_f16(nl_u32x16 h, float sc) {
  nl_u32x6 r;
  asm("v_cvt_scalef32_pk32_fp6_f16 %0, %1, %2" : "=&v"(r) : "v"(h), "v"(sc));
  return r;
}
__device__ __forceinline__ nl_u32x6 nl_cvt_2xpk16_fp6_f32(nl_f32x16 a, nl_f32x16 b, float sc) {
  nl_u32x6 r;
  asm("v_cvt_scalef32_2xpk16_fp6_f32 %0, %1, %2, %3" : "=&v"(r) : "v"(a), "v"(b), "v"(sc));
  return r;
}

// ------------------------------------------------------------------ split-bf16 of 8 values -> two B / A fragments: TWO forms, the same values through different instructions
// per element (hipcc: a conversion per element for the subtraction and a second, packed one for the store; 32 vector instructions with X3) ...
template <bool X3 = true>
__device__ __forceinline__ void nl_split8_elem(const float (&v)[8], nl_bf16x8& hi, nl_bf16x8& lo) {
#pragma unroll
  for (int t = 0; t < 8; ++t) {
    __bf16 h = (__bf16)v[t];
    hi[t] = h;
    if (X3) lo[t] = (__bf16)(v[t] - (float)h);
  }
}
// ... and on pairs (nl_split_bf16_pair: 20).  A caller keeps the form it was tuned and tested with.
template <bool X3>
__device__ __forceinline__ void nl_split8(const float (&v)[8], nl_bf16x8& hi, nl_bf16x8& lo) {
  unsigned h[4], l[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    if (X3) nl_split_bf16_pair(v[2 * t], v[2 * t + 1], h[t], l[t]);
    else h[t] = nl_bf16_pair(v[2 * t], v[2 * t + 1]);
  }
  hi = __builtin_bit_cast(nl_bf16x8, nl_u32x4{h[0], h[1], h[2], h[3]});
  if (X3) lo = __builtin_bit_cast(nl_bf16x8, nl_u32x4{l[0], l[1], l[2], l[3]});
}

// ------------------------------------------------------------------ 32x32x16 MFMA on 16-bit lanes: bf16, or the same storage holding fp16 bit patterns (split-FP16)
template <bool F16>
__device__ __forceinline__ nl_f32x16 nl_mfma(const nl_bf16x8& a, const nl_bf16x8& b, const nl_f32x16& c) {
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(nl_f16x8, a), __builtin_bit_cast(nl_f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
template <bool F16>
__device__ __forceinline__ nl_f32x16 nl_mfma(const nl_i16x8 a, const nl_i16x8 b, const nl_f32x16 c) {   // the same on raw 16-bit lanes
  if constexpr (F16) return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(nl_f16x8, a), __builtin_bit_cast(nl_f16x8, b), c, 0, 0, 0);
  else return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
}
// accumulator register r of half-wave hh -> row of the 32x32 tile (C/D layout of the 32x32 MFMAs)
__device__ __forceinline__ int nl_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }
template <int NB>
__device__ __forceinline__ void nl_acc_zero(nl_f32x16 (&acc)[NB]) {
#pragma unroll
  for (int i = 0; i < NB; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[i][r] = 0.f;
}
template <int A, int B>
__device__ __forceinline__ void nl_acc_zero(nl_f32x16 (&acc)[A][B]) {
#pragma unroll
  for (int t = 0; t < A; ++t) nl_acc_zero(acc[t]);
}

// A 16-bit operand from raw dwords.  The operands are split-bf16 (hi = bf16(v), lo = bf16(v - hi): 2^-17 per product, any magnitude) or, F16, split-FP16
// (hi = f16(v), lo = f16(v - hi): 2^-22 per product while |v| < 65504; the parity mode of the units whose logits feed a softmax, which multiplies a logit's error
// by the logit's size).  Same storage, same fragment order.
__device__ __forceinline__ nl_i16x8 nl_frag(const uint4 v) { return __builtin_bit_cast(nl_i16x8, v); }
__device__ __forceinline__ nl_i16x8 nl_frag(unsigned a, unsigned b, unsigned c, unsigned d) { return __builtin_bit_cast(nl_i16x8, nl_u32x4{a, b, c, d}); }
template <bool F16>
__device__ __forceinline__ void nl_split_pair(float a, float b, unsigned& hi, unsigned& lo) {
  if constexpr (F16) {
    const nl_f32x2 v = {a, b};
    const nl_f16x2 h = __builtin_convertvector(v, nl_f16x2);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, __builtin_convertvector(v - __builtin_convertvector(h, nl_f32x2), nl_f16x2));
  } else {
    nl_split_bf16_pair(a, b, hi, lo);
  }
}

// ------------------------------------------------------------------ fragment maps of a packed N x K weight matrix (row-major source, nrb = N / 32 row blocks)
// The source offset of element i of a plane; a plane is N * K elements, 64 lanes per fragment, so that a wave reads a fragment as one coalesced piece.
// 16-bit planes: fragment (s, rb), lane, slot j <-> W[32 rb + (lane & 31)][16 s + 8 (lane >> 5) + j], 8 slots (16 B) per lane.  acc_order: the 8 columns a lane
// holds of k-step s are the hidden units of accumulator registers 8 (s & 1) + j of 32-block s >> 1 — 16 s + 8 (j >> 2) + 4 (lane >> 5) + (j & 3) — for a layer whose
// B operand is the previous layer's accumulators (s2d.h: layer 2).
__host__ __device__ inline size_t nl_frag16_src(int i, int nrb, int K, bool acc_order) {
  const int j = i & 7, lane = (i >> 3) & 63, f = i >> 9, rb = f % nrb, s = f / nrb, hh = lane >> 5;
  return (size_t)(32 * rb + (lane & 31)) * K + 16 * s + (acc_order ? 8 * (j >> 2) + 4 * hh + (j & 3) : 8 * hh + j);
}
// fp32 plane (v_mfma_f32_32x32x2_f32: half-wave hh supplies k slot hh): fragment (g, t, rb), lane <-> W[32 rb + (lane & 31)][8 g + 4 (lane >> 5) + t], t < 4.
// Read with g = 4 b + (t' >> 2), t = t' & 3 this is already the accumulator order: column 32 b + 8 (t' >> 2) + 4 hh + (t' & 3) = register t' of 32-block b.
__host__ __device__ inline size_t nl_frag32_src(int i, int nrb, int K) {
  const int lane = i & 63, f = i >> 6, rb = f % nrb, q = f / nrb;   // q = 4 g + t
  return (size_t)(32 * rb + (lane & 31)) * K + 8 * (q >> 2) + 4 * (lane >> 5) + (q & 3);
}
// one value into the 16-bit planes that exist: bf16 hi / lo (round to nearest even, lo = bf16(v - float(hi))) and fp16 hi / lo (lo = f16(v - float(hi))).
// All four conversions are computed; only the store of a null plane is skipped.
__device__ __forceinline__ void nl_store_split(float v, size_t i, unsigned short* bf_hi, unsigned short* bf_lo, unsigned short* f16_hi, unsigned short* f16_lo) {
  const unsigned short h = nl_f2bf(v);
  if (bf_hi) bf_hi[i] = h;
  if (bf_lo) bf_lo[i] = nl_f2bf(v - __uint_as_float((unsigned)h << 16));
  const _Float16 g = (_Float16)v;
  if (f16_hi) f16_hi[i] = __builtin_bit_cast(unsigned short, g);
  if (f16_lo) f16_lo[i] = __builtin_bit_cast(unsigned short, (_Float16)(v - (float)g));
}

// ------------------------------------------------------------------ e2m3 (fp6) encoder of the weight-packing kernels
__device__ __forceinline__ unsigned nl_e2m3(float a) {   // a >= 0, already divided by the block scale; round to nearest even, saturating at 7.5
  if (!(a < 7.5f)) return 31u;
  if (a < 1.f) return (unsigned)rintf(a * 8.f);   // subnormals 0 .. 0.875; 8 = the smallest normal (encodings are contiguous)
  const int e = a < 2.f ? 0 : a < 4.f ? 1 : 2;
  unsigned m = (unsigned)rintf(ldexpf(a, 3 - e));   // 8 .. 16
  unsigned c = ((unsigned)(e + 1) << 3) + (m - 8u);    // m == 16 carries into the exponent
  return c > 31u ? 31u : c;
}
