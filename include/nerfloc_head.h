/* libnerfloc_head.so: the device-side glue of the localisation head (HIP, gfx950 only).
 *
 * A second library next to libnerfloc_render.so: the entry points that keep the NUMBER OF MATCHES on the device from the coarse selection to the pose, and the two
 * position encodings of the head.  Symbol prefix nlh_; status codes are the NL_* codes of nerfloc_render.h (NL_OK = 0, negative = error); the Python binding is
 * nerf_loc_amd/_head_lib.py; tests/head_ref.py restates every contract below in numpy.
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises, copies or uses a float atomic; every
 * pointer is DEVICE memory unless it says HOST; two calls with the same arguments give the same bits; each call is a linear chain of launches and can be captured
 * in a HIP graph.  NL_ERR_BAD_ARG: a null / negative / misaligned argument; NL_ERR_UNSUPPORTED: a size above a stated limit; NL_ERR_WORKSPACE: a missing, short or
 * not 256-byte aligned workspace; NL_ERR_HIP: a launch failed.
 */
#ifndef NERFLOC_HEAD_H
#define NERFLOC_HEAD_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_render.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLH_ABI_VERSION 1
int nlh_abi_version(void);

/* ---- nlh_select_matches: fixed-capacity, ordered match lists with a device-side count
 * Input: match_j (N int32) as nl_s2d_match writes it: the partner of 3-D point i, -1 = unmatched.  An entry outside [0, Mc) counts as unmatched, whatever its
 * value; nothing is read through it.  kps3d (N, 3) fp32, kps2d (Mc, 2) fp32; rows_a, rows_b: two optional row tables (N, C) fp32, NULL = not wanted (then its
 * output is not touched and may be NULL).  1 <= N <= 2^20, 1 <= cap <= 2^24, 0 <= Mc < 2^31; with a table: C a multiple of 4, 4 .. 512, tables and their
 * outputs 16-byte aligned.
 * Output:
 *   info (4 int32):  total = the number of matched i;  count = min(total, cap);  overflow = total > cap ? 1 : 0;  stored as {count, total, overflow, 0}
 *   row k < count:   i = the k-th smallest matched i (the order torch.nonzero gives), j = match_j[i]:
 *                    i_ids[k] = i, j_ids[k] = j, b_ids[k] = 0 (int64);  mkps3d[k] = kps3d[i];  mkps2d_c[k] = kps2d[j];  out_a[k] = rows_a[i];  out_b[k] = rows_b[i]
 *   row count <= k < cap:  ids 0, every float output exactly 0.0 (so whatever consumes the padded rows reads defined, finite values)
 * All outputs hold cap rows: i_ids, j_ids, b_ids (cap) int64; mkps3d (cap, 3), mkps2d_c (cap, 2), out_a, out_b (cap, C) fp32.
 * The order comes from a prefix scan (ballot and popcount inside a wave, the waves and chunks added in ascending order), not from atomics.
 * Workspace: nlh_select_workspace_bytes(N) bytes (0: N outside the limits), 256-byte aligned. */
size_t nlh_select_workspace_bytes(int64_t N);
int nlh_select_matches(const int32_t* match_j, int64_t N, int64_t cap, int64_t Mc, int C, const float* kps3d, const float* kps2d, const float* rows_a, const float* rows_b,
                       int64_t* i_ids, int64_t* j_ids, int64_t* b_ids, float* mkps3d, float* mkps2d_c, float* out_a, float* out_b, int32_t* info, void* ws,
                       size_t ws_bytes, void* stream);

/* ---- nlh_pos_sine_grid: the 2-D sine position encoding of an (H, W) map, out (H, W, C) fp32, C a multiple of 4 (D = C / 4 frequencies)
 * (PositionEmbeddingSine(C / 2, normalize=True, sine_type='lin_sine'): the values depend on H and W alone.)  All in fp32, in this order of operations:
 *   ex(w) = ((w + 1) - 0.5) / (W + 1e-6),  ey(h) = ((h + 1) - 0.5) / (H + 1e-6)          (w, h from 0)
 *   a(f, e) = float(f * pi) * e,  f = 1 .. D                                              (f * pi rounded from double to fp32, then ONE fp32 product)
 *   out[h][w][2 (f - 1)]     = sin a(f, ex(w))      out[h][w][2 (f - 1) + 1]         = sin a(f, ey(h))
 *   out[h][w][C / 2 + 2 (f - 1)] = cos a(f, ex(w))  out[h][w][C / 2 + 2 (f - 1) + 1] = cos a(f, ey(h))
 * i.e. all sines, then all cosines; x before y inside a frequency.  sin / cos are full-range fp32 functions (within a few ulp).
 * Limits: H, W <= 32768, C <= 4096, H W C <= 2^31. */
int nlh_pos_sine_grid(int H, int W, int C, float* out, void* stream);

/* ---- nlh_embed_points: the NeRF embedder without the input, log-sampled frequencies 2^0 .. 2^(L - 1)   (get_embedder(L, 0, include_input=False))
 * x (N, D) fp32, out (N, 2 D L) fp32:  out[n][(2 l) D + d] = sin(x[n][d] 2^l),  out[n][(2 l + 1) D + d] = cos(x[n][d] 2^l),  l = 0 .. L - 1.
 * The product is exact in fp32 (a power of two); with L = 32 the arguments reach 2^31 |x|, so sin / cos are FULL-RANGE functions (exact argument reduction), never
 * the hardware's fast sine.  Limits: 1 <= L <= 32, 1 <= D <= 64, 0 <= N <= 2^24 (N == 0: NL_OK, nothing launched). */
int nlh_embed_points(const float* x, int64_t N, int D, int L, float* out, void* stream);

/* ---- nlh_pnp_ransac_counted: nl_pnp_ransac with the match counts in device memory
 * Arguments as nl_pnp_ransac (nerfloc_render.h) plus counts_dev (B int32, DEVICE).  offsets (B + 1 int32, HOST) now give each problem's CAPACITY and its place in
 * pts2d / pts3d / mask: problem b owns the rows offsets[b] .. offsets[b + 1] and uses the first M_b = min(capacity_b, max(counts_dev[b], 0)) of them.
 * For a problem with M_b matches the contract is the one of nl_pnp_ransac with M read on the device: the same Philox samples as a function of (seed, b, h, M_b), the
 * same P3P, integer scores and arg-max, the same NL_PNP_LO_ROUNDS x NL_PNP_GN_ITERS Gauss-Newton: poses, info, counts and the first M_b mask bytes equal, bit for
 * bit, those of nl_pnp_ransac called with that problem cut to its first M_b matches (at the same problem index b).  Mask bytes at and beyond M_b are 0.
 * M_b < 4 is a failure, not an error: the identity, success 0, num_inliers 0.  The host checks of offsets, intrinsics (HOST, B x 4 doubles: fx, fy, cx, cy), thr
 * (HOST, B doubles), H (a multiple of 64, 64 .. 65536), min_inliers (>= 4) are nl_pnp_ransac's; counts_dev must not be NULL.
 * Workspace: nlh_pnp_workspace_bytes(offsets[B], B, H) = nl_pnp_workspace_bytes of the same arguments. */
size_t nlh_pnp_workspace_bytes(int64_t cap_total, int64_t B, int H);
int nlh_pnp_ransac_counted(const float* pts2d, const float* pts3d, const int32_t* offsets, const int32_t* counts_dev, const double* intrinsics, const double* thr,
                           int64_t B, int H, uint64_t seed, int min_inliers, double* poses, uint8_t* mask, int32_t* info, int32_t* counts, void* ws, size_t ws_bytes,
                           void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
