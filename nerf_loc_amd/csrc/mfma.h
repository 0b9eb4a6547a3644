// Device helpers shared by the units that use MFMA, LDS-DMA or split precision (gfx950 only): ONE definition of what the kernel files used to copy.
// Include after common.h.  Everything here is __device__ __forceinline__ (no emitted symbol) and carries the nl_ prefix; kernels, argument structs and
// per-kernel geometry stay in their files.
#pragma once
#include <utility>
#include "common.h"

// ------------------------------------------------------------------ vector types (MFMA operands / accumulators, raw dword groups)
typedef __bf16 nl_bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 nl_bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 nl_f16x8 __attribute__((ext_vector_type(8)));
typedef short nl_i16x8 __attribute__((ext_vector_type(8)));   // 8 bf16 as raw 16-bit lanes (gemm.hip, s2d.hip)
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
// accumulator register r of half-wave hh -> row of the 32x32 tile (C/D layout of the 32x32 MFMAs)
__device__ __forceinline__ int nl_acc_row(int r, int hh) { return (r & 3) + 8 * (r >> 2) + 4 * hh; }

// ------------------------------------------------------------------ e2m3 (fp6) encoder of the weight-packing kernels
__device__ __forceinline__ unsigned nl_e2m3(float a) {   // a >= 0, already divided by the block scale; round to nearest even, saturating at 7.5
  if (!(a < 7.5f)) return 31u;
  if (a < 1.f) return (unsigned)rintf(a * 8.f);   // subnormals 0 .. 0.875; 8 = the smallest normal (encodings are contiguous)
  const int e = a < 2.f ? 0 : a < 4.f ? 1 : 2;
  unsigned m = (unsigned)rintf(ldexpf(a, 3 - e));   // 8 .. 16
  unsigned c = ((unsigned)(e + 1) << 3) + (m - 8u);    // m == 16 carries into the exponent
  return c > 31u ? 31u : c;
}
