// Host tail of the matcher MLP's backward, shared by the two entry points whose kernels run s2d_bwd.h's chain: nl_s2d_backward_train (s2d_bwd.hip) and
// nl_fine_match_backward (fine_bwd.hip).  The parameter gradients of one call, their zero fill, the carve of the operand block the kernel stores and wgrad.hip
// multiplies, the launch of the kernel's exact / bf16 instantiation, and the two weight-gradient products.  Host code only; include after s2d_bwd.h and host.h.
#pragma once
#include <algorithm>
#include "s2d_bwd.h"
#include "host.h"

namespace {

// where a call adds the gradients of mlps.{0,2,4}; each may be null (that parameter is frozen)
struct S2dMlpGrads {
  float *w1, *b1, *w2, *b2, *w3, *b3;
  bool want1() const { return w1 || b1; }
  bool want2() const { return w2 || b2; }
  bool want3() const { return w3 || b3; }
  uintptr_t addr_bits() const { return (uintptr_t)w1 | (uintptr_t)b1 | (uintptr_t)w2 | (uintptr_t)b2 | (uintptr_t)w3 | (uintptr_t)b3; }   // for the alignment checks
};

inline int s2d_mlp_grads_zero(const S2dMlpGrads& g, int C, hipStream_t st) {
  if (g.w1) NL_CHECK_HIP(hipMemsetAsync(g.w1, 0, (size_t)S2D_H * C * 4, st));
  if (g.b1) NL_CHECK_HIP(hipMemsetAsync(g.b1, 0, S2D_H * 4, st));
  if (g.w2) NL_CHECK_HIP(hipMemsetAsync(g.w2, 0, (size_t)S2D_H * S2D_H * 4, st));
  if (g.b2) NL_CHECK_HIP(hipMemsetAsync(g.b2, 0, S2D_H * 4, st));
  if (g.w3) NL_CHECK_HIP(hipMemsetAsync(g.w3, 0, S2D_H * 4, st));
  if (g.b3) NL_CHECK_HIP(hipMemsetAsync(g.b3, 0, 4, st));
  return NL_OK;
}

// Byte offsets of the operand block for P operand rows and `items` partial rows of gW3 / gb3: the row-major matrices x (P, C), h1, ga2, ga1 (P, 128), the
// waves' partial rows, the split-K scratch of the larger of the two products and a sink for a product whose weight is frozen while its bias is not.  Every
// piece is aligned up to 256 bytes, so `total` does not depend on the order of the pieces; an entry point with buffers of its own goes on with take().
struct S2dMlpBwdWs {
  size_t x, h1, ga2, ga1, w3part, wg, dummy, total = 0; size_t wg_floats;
  size_t take(size_t bytes) { const size_t at = total; total += nl_align_up(bytes, 256); return at; }
  S2dMlpBwdWs(size_t P, size_t items, int C) {
    x = take(P * C * 4);
    h1 = take(P * S2D_H * 4);
    ga2 = take(P * S2D_H * 4);
    ga1 = take(P * S2D_H * 4);
    w3part = take(items * S2D_W3P_LD * 4);
    wg_floats = std::max(nl_wgrad_scratch_floats((int64_t)P, S2D_H, C), nl_wgrad_scratch_floats((int64_t)P, S2D_H, S2D_H));
    wg = take(wg_floats * 4);
    dummy = take((size_t)S2D_H * 256 * 4);
  }
  // the kernel's operand stores: null where both parameters of the product they feed are frozen
  void operands(unsigned char* ws, const S2dMlpGrads& g, float*& px, float*& pga1, float*& ph1, float*& pga2) const {
    px = g.want1() ? (float*)(ws + x) : nullptr;
    pga1 = g.want1() ? (float*)(ws + ga1) : nullptr;
    ph1 = g.want2() ? (float*)(ws + h1) : nullptr;
    pga2 = g.want2() ? (float*)(ws + ga2) : nullptr;
  }
};

// the kernel of one entry point: its bf16 instantiation, or the exact one with its dynamic LDS (beyond the 64 KB a kernel gets unasked: `lds_set`, one static
// per entry point)
template <class Args>
inline int s2d_mlp_bwd_launch(void (*exact)(const Args), void (*bf16)(const Args), dim3 grid, const Args& a, int precision, std::atomic<unsigned long long>& lds_set,
                              hipStream_t st) {
  if (precision == NL_PREC_BF16) {
    hipLaunchKernelGGL(bf16, grid, dim3(256), 0, st, a);
  } else {
    if (const int e = nl_allow_dynamic_lds((const void*)exact, S2D_F32_LDS, lds_set)) return e;
    hipLaunchKernelGGL(exact, grid, dim3(256), S2D_F32_LDS, st, a);
  }
  NL_LAUNCH_CHECK();
  return NL_OK;
}

// gW2 += ga2^T h1, gb2, gW1 += ga1^T x, gb1 over P operand rows (wgrad.hip's split-K kernel; operands as S2dMlpBwdWs::operands left them)
inline int s2d_mlp_wgrad(const float* x, const float* ga1, const float* h1, const float* ga2, int C, int64_t P, const S2dMlpGrads& g, float* dummy, float* wg,
                         size_t wg_floats, hipStream_t st) {
  if (g.want2())
    if (const int e = nl_launch_wgrad(ga2, S2D_H, S2D_H, h1, S2D_H, S2D_H, P, 0, 0, g.w2 ? g.w2 : dummy, S2D_H, 1, 0, g.b2, wg, wg_floats, st)) return e;
  if (g.want1())
    if (const int e = nl_launch_wgrad(ga1, S2D_H, S2D_H, x, C, C, P, 0, 0, g.w1 ? g.w1 : dummy, C, 1, 0, g.b1, wg, wg_floats, st)) return e;
  return NL_OK;
}

}  // namespace
