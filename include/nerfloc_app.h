/* libnerfloc_app.so: appearance adaptation (HIP, gfx950 only) — the channel statistics of a feature map, the adaptation MLP and the per-channel affine rewrite
 * (FiLM) of the support maps, with the FiLM's gradients.
 *
 * A third library next to libnerfloc_render.so and libnerfloc_head.so.  Symbol prefix nla_; status codes are the NL_* codes of nerfloc_render.h (NL_OK = 0,
 * negative = error); the Python binding is nerf_loc_amd/_app_lib.py; tests/appearance_ref.py restates every contract below in numpy (fp64).
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises, copies or uses a float atomic; every
 * pointer is DEVICE memory unless it says HOST; two calls with the same arguments give the same bits; each call is a linear chain of launches and can be captured
 * in a HIP graph.  All arithmetic is fp32 and there are no precision modes: these kernels are bound by memory bandwidth.  The library is built with
 * -ffp-contract=off: a product followed by a sum is two roundings wherever this header writes them as two operations.
 * NL_ERR_BAD_ARG: a null / negative / misaligned argument or an unknown flag; NL_ERR_UNSUPPORTED: a size above a stated limit; NL_ERR_WORKSPACE: a missing, short
 * or not 256-byte aligned workspace; NL_ERR_HIP: a launch failed.  All of these are decided on the host before anything is launched or dereferenced.
 */
#ifndef NERFLOC_APP_H
#define NERFLOC_APP_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_render.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLA_ABI_VERSION 1
int nla_abi_version(void);

/* ---- nla_channel_stats: mean and unbiased standard deviation per (image, channel)      (AppearanceEmbedding: torch.std_mean over each channel's plane)
 * x: B images of C channels and HW pixels, fp32, contiguous in one of two layouts:
 *   NLA_LAYOUT_NCHW  x[b][c][p]      NLA_LAYOUT_NHWC  x[b][p][c]   (torch's channels_last)
 * out (B, 2 C) fp32:  out[b][c] = mean over p,  out[b][C + c] = sqrt(sum_p (x - mean)^2 / (HW - 1)).
 * 2 <= HW <= 2^30, 1 <= C <= 1024, B >= 0 (B == 0: NL_OK, nothing launched), at most 2^31 - 1 plane segments in all (see below: NL_ERR_UNSUPPORTED above that).
 * x needs 4-byte alignment only; 16-byte loads are used where x is 16-byte aligned and the contiguous run (HW for NCHW, C for NHWC) is a multiple of 4.
 * How: every plane is cut into segments of NLA_STATS_SEG_NCHW consecutive pixels (NCHW) or NLA_STATS_SEG_NHWC pixels (NHWC); the cut depends on HW and the layout
 * alone, never on B or C, so an image's row does not depend on the other images of the call.  One workgroup per segment takes the segment's mean from the sum of
 * its values and then the sum of squared deviations FROM THAT MEAN (no E[x^2] - E[x]^2 anywhere); the values are summed per thread in ascending order, the
 * threads in a fixed tree.  A second kernel, one wave per (b, c), merges the segments' (count, mean, M2) with Chan's update
 *   d = mean_B - mean_A;  mean = mean_A + d n_B / n;  M2 = M2_A + M2_B + d^2 n_A n_B / n
 * lane l first merging segments l, l + 64, ... in ascending order, then the lanes pairwise l <- l + 32, 16, 8, 4, 2, 1.
 * Workspace: nla_channel_stats_workspace_bytes(B, C, HW, layout) bytes (0: an argument outside the limits, or B == 0), 256-byte aligned. */
#define NLA_LAYOUT_NCHW 0
#define NLA_LAYOUT_NHWC 1
#define NLA_STATS_SEG_NCHW 4096
#define NLA_STATS_SEG_NHWC 256
size_t nla_channel_stats_workspace_bytes(int64_t B, int C, int64_t HW, int layout);
int nla_channel_stats(const float* x, int64_t B, int C, int64_t HW, int layout, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- nla_adapt_code: the adaptation MLP E -> 64 -> 64 -> 2 C of V embedding differences               (AppearanceAdaptLayer.mlp)
 * emb (V, E), target (E), code (V, 2 C), all fp32.  weights: a HOST array of six DEVICE pointers in state-dict order, the tensors read as they lie (row-major
 * (out, in) weights, no packed image):  mlp.0.weight (64, E), mlp.0.bias (64), mlp.2.weight (64, 64), mlp.2.bias (64), mlp.4.weight (2 C, 64), mlp.4.bias (2 C).
 *   d = target - emb[v];  h1 = LeakyReLU_0.01(W0 d + b0);  h2 = LeakyReLU_0.01(W2 h1 + b2);  code[v] = W4 h2 + b4
 * Each dot product of length K: four threads q = 0 .. 3 sum the products k = q, q + 4, ... in ascending order (product and sum are two operations), the four
 * partial sums are added as (s0 + s1) + (s2 + s3), and the bias is added last.
 * E a multiple of 4, 4 .. 512; 1 <= C <= 1024; V >= 0 (V == 0: NL_OK, nothing launched); V <= 2^20.  One launch, one workgroup per view. */
#define NLA_ADAPT_HIDDEN 64
int nla_adapt_code(const float* emb, const float* target, const void* const* weights, int64_t V, int E, int C, float* code, void* stream);

/* ---- nla_film: y[v][p][c] = code[v][c] * x[v][p][c] + code[v][C + c]                                   (the rest of AppearanceAdaptLayer.forward)
 * x, y (V, HW, C) fp32 contiguous, code (V, 2 C).  ONE multiply and ONE add per value, so the result equals torch's `a * x + b` in fp32 bit for bit.
 * flags: NLA_FILM_CLIP01 clamps y to [0, 1] afterwards (the rgb layer; a NaN stays a NaN); any other bit is NL_ERR_BAD_ARG.
 * y == x (in place) is allowed; any other overlap is not.  1 <= C <= 1024, HW >= 1, V >= 0 (V == 0: NL_OK), V HW C < 2^40; indices are 64-bit.
 * 16-byte accesses where C % 4 == 0 and x, y and code are 16-byte aligned; otherwise a scalar path (4-byte alignment). */
#define NLA_FILM_CLIP01 1u
int nla_film(const float* x, const float* code, int64_t V, int64_t HW, int C, unsigned flags, float* y, void* stream);

/* ---- nla_film_backward: the cotangents of nla_film
 * x, g_y (V, HW, C), code (V, 2 C); with m = 1 without NLA_FILM_CLIP01 and m = (0 <= y <= 1) on the recomputed y = code[v][c] x + code[v][C + c] with it
 * (both ends inclusive, as the backward of torch.clip):
 *   g_x[v][p][c] = m code[v][c] g_y[v][p][c]            g_code[v][c] = sum_p m g_y x            g_code[v][C + c] = sum_p m g_y
 * g_x (V, HW, C) and g_code (V, 2 C) may each be NULL (not wanted); g_x == g_y (in place) is allowed.  Limits and alignment rules as nla_film.
 * One pass reads x and g_y and writes g_x.  A workgroup owns nla_film_backward_block_pixels(C) consecutive pixels of one view: each thread sums its pixels in
 * ascending order, the threads of a channel are added in ascending order, and the workgroup's 2 C sums go to the workspace; a second kernel adds the
 * workgroups' partial sums of each (v, channel) in ascending pixel order.  The workspace is needed only where g_code is wanted.
 * Workspace: nla_film_backward_workspace_bytes(V, HW, C) bytes (0: an argument outside the limits, or V == 0), 256-byte aligned. */
int64_t nla_film_backward_block_pixels(int C);
size_t nla_film_backward_workspace_bytes(int64_t V, int64_t HW, int C);
int nla_film_backward(const float* x, const float* code, const float* g_y, int64_t V, int64_t HW, int C, unsigned flags, float* g_x, float* g_code, void* ws,
                      size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
