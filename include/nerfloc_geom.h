/* libnerfloc_geom.so: keypoint geometry (HIP, gfx950 only) — which SfM points the support views see, the 3D-2D pairs of a pose with their coarse-cell indices,
 * the dense loss target those pairs encode, and the coarse cell grid.  It replaces the eager glue that NerfPoseEstimator.forward / estimate run around the head
 * (select_3d_keypoints, build_3d_2d_pairs, conf_matrix_gt, pts2d_grid).
 *
 * A fourth library next to libnerfloc_render.so, libnerfloc_head.so and libnerfloc_app.so.  Symbol prefix nlg_; status codes are the NL_* codes of
 * nerfloc_render.h (NL_OK = 0, negative = error); the Python binding is nerf_loc_amd/_geom_lib.py; tests/geom_ref.py restates every contract below in numpy (fp64).
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises, copies or uses a float atomic (there
 * is no atomic at all); every pointer is DEVICE memory unless it says HOST; two calls with the same arguments give the same bits; each call is a linear chain of
 * launches and can be captured in a HIP graph.  No kernel waits for another workgroup: order comes from three launches (counts per chunk, a scan, an emit pass).
 * NL_ERR_BAD_ARG: a null / non-positive / misaligned argument or an unknown flag; NL_ERR_UNSUPPORTED: a size above a stated limit; NL_ERR_WORKSPACE: a missing,
 * short or not 256-byte aligned workspace; NL_ERR_HIP: a launch failed.  All of these are decided on the host before anything is launched or dereferenced.
 *
 * ARITHMETIC.  Inputs are loaded as they lie (fp32 points, K and depths; fp32 or fp64 poses) and widened; from there to every decision all arithmetic is fp64,
 * each written operation one rounding (the library is built with -ffp-contract=off), sums taken left to right.
 *   pose   a row-major 4 x 4 camera-to-world matrix of which ONLY the top three rows are read:  A = pose[0:3][0:3],  c = pose[0:3][3]   (the affine part)
 *   w2c    R = adj(A) / det(A)  (each of the nine cofactors of the 3 x 3 adjugate divided by det = A00 C00 + A01 C01 + A02 C02, C the cofactors of row 0),
 *          t = -(R c)           — the inverse of a general affine map, not the transpose: a pose that is not exactly rigid is inverted as torch's .inverse() does
 *   P      the combined 3 x 4 matrix  P[r][0:3] = sum_k K[r][k] R[k][0:3],  P[r][3] = sum_k K[r][k] t[k]   with the full 3 x 3 K (row-major fp32, device memory)
 *   x      x[r] = P[r][0] p0 + P[r][1] p1 + P[r][2] p2 + P[r][3];   z = x[2],  u = x[0] / z,  v = x[1] / z
 *   valid  (u >= 0) & (v >= 0) & (u < W) & (v < H) & (z > 0)    — a NaN compares false
 * Each workgroup forms the V matrices P once, in LDS.
 * flags, one word for every call that takes it:  NLG_POSE_F64: `pose(s)` hold doubles (default NLG_POSE_F32: floats);  NLG_DEPTH_POINTS: see nlg_build_pairs.
 * Any other bit is NL_ERR_BAD_ARG.
 *
 * `info` (4 int32): { count = min(total, cap), total, overflow = total > cap, used_fallback (nlg_build_pairs; 0 for nlg_select_visible) }.
 */
#ifndef NERFLOC_GEOM_H
#define NERFLOC_GEOM_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_render.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLG_ABI_VERSION 1
int nlg_abi_version(void);

#define NLG_POSE_F32 0u
#define NLG_POSE_F64 1u
#define NLG_DEPTH_MAP 0u
#define NLG_DEPTH_POINTS 2u
#define NLG_MAX_POINTS 1048576
#define NLG_MAX_VIEWS 64
#define NLG_MAX_IMAGE 32768
#define NLG_CHUNK 256
#define NLG_MIN_POSITIVES 4

/* ---- nlg_select_visible: the points that at least one of V views sees                                      (NerfPoseEstimator.select_3d_keypoints)
 * pts (N, 3) fp32; poses (V, 4, 4) row-major c2w, fp32 or fp64 by flags; K (3, 3) fp32, shared by the views; H, W the image size in pixels.
 * mask (N) uint8:  mask[i] = OR over the views of valid (0 or 1).
 * idx (cap) int64: the i with mask[i] = 1 in ascending order, the first `cap` of them; idx[k] = 0 for count <= k < cap.
 * info (4) int32 as above.
 * 1 <= N <= NLG_MAX_POINTS, 1 <= V <= NLG_MAX_VIEWS, 1 <= H, W <= NLG_MAX_IMAGE, 1 <= cap <= 2^24.  pts, K, poses: 4-byte (fp64 poses: 8-byte) alignment, idx 8-byte.
 * Three launches: one workgroup per chunk of NLG_CHUNK points writes mask and the chunk's count (ballot + popcount per wave); one workgroup scans the counts and
 * writes info; one thread per max(N, cap) emits idx[rank] or the zero behind the count.
 * Workspace: nlg_select_visible_workspace_bytes(N) bytes (0: N outside the limits), 256-byte aligned. */
size_t nlg_select_visible_workspace_bytes(int64_t N);
int nlg_select_visible(const float* pts, int64_t N, const void* poses, int V, const float* K, int H, int W, unsigned flags, int64_t cap, uint8_t* mask,
                       int64_t* idx, int32_t* info, void* ws, size_t ws_bytes, void* stream);

/* ---- nlg_build_pairs: projections, the positive set and its (point, cell) pairs for one pose                 (NerfPoseEstimator.build_3d_2d_pairs)
 * pts (N, 3) fp32; pose (4, 4) as above; K; H, W; stride >= 1 with H % stride == 0 and W % stride == 0 (NL_ERR_BAD_ARG otherwise); Wc = W / stride.
 * depth: without NLG_DEPTH_POINTS a map (H, W) fp32, read at [trunc(v)][trunc(u)] for VALID points only (so the read is always inside the map); with it an
 *   array (N) fp32, one depth per point, read for valid points only (the caller fills it, e.g. from the renderer).
 * thr: a double.   depth_ok = |depth - z| < thr  (fp64; NaN: false),   pos = valid & depth_ok.
 * The positive set is `pos` if at least NLG_MIN_POSITIVES rows are pos, otherwise `valid` (info[3] = used_fallback = 1): decided on the device from the scanned totals.
 * proj (N, 2) fp32 = (u / stride, v / stride) rounded once from fp64, for EVERY point (for a point that is not valid it is whatever the formulas give);
 * z (N) fp32;  valid (N) uint8;  pos (N) uint8 — valid & depth_ok, BEFORE the fallback;
 * gt_j (N) int32 = trunc(u / stride) + trunc(v / stride) Wc for the rows of the positive set (0 <= gt_j < (H / stride) Wc, since they are valid), -1 otherwise;
 * pairs (2, cap) int64: pairs[0][k] = i, pairs[1][k] = gt_j[i] of the positive set in ascending i, the first `cap`; both rows 0 for count <= k < cap;
 * info (4) int32: count, total (of the positive set), overflow, used_fallback.
 * Limits as nlg_select_visible.  Three launches of the same shape: project / count both sets per chunk; scan both, decide, write info; emit.
 * Workspace: nlg_build_pairs_workspace_bytes(N) bytes (0: N outside the limits), 256-byte aligned. */
size_t nlg_build_pairs_workspace_bytes(int64_t N);
int nlg_build_pairs(const float* pts, int64_t N, const void* pose, const float* K, int H, int W, int stride, double thr, const float* depth, unsigned flags,
                    int64_t cap, float* proj, float* z, uint8_t* valid, uint8_t* pos, int32_t* gt_j, int64_t* pairs, int32_t* info, void* ws, size_t ws_bytes,
                    void* stream);

/* ---- nlg_conf_target: rows [row_begin, row_end) of the dense (N, M) matching target                          (conf_matrix_gt: zeros + index-put)
 * gt_j (N) int32.  out: the address of element (0, 0) of a row-major (N, M) matrix of dtype fp32 (NLG_TARGET_F32) or int64 (NLG_TARGET_I64);
 *   out[n][m] = (gt_j[n] == m) ? 1 : 0   for row_begin <= n < row_end — a gt_j outside [0, M) leaves its row zero.
 * ONLY the rows of the range are written or need to exist: a caller may hold a slice of a matrix too large to allocate.  0 <= row_begin <= row_end <= N
 * (an empty range: NL_OK, nothing launched).  1 <= N <= 2^24, 1 <= M <= 2^24; all element indices are 64-bit.
 * Every value is written exactly once: 16-byte stores over the 16-byte aligned part of the range (out itself must be 16-byte aligned for that; otherwise, and for
 * the at most three values before and after the aligned part, scalar stores).  out needs the alignment of its element type.  One launch. */
#define NLG_TARGET_F32 0
#define NLG_TARGET_I64 1
int nlg_conf_target(const int32_t* gt_j, int64_t N, int64_t M, int dtype, int64_t row_begin, int64_t row_end, void* out, void* stream);

/* ---- nlg_cell_grid: the coordinates of the coarse cells                                                      (pts2d_grid, and its `* stride_coarse / stride_fine`)
 * out (Hc Wc, 2) fp32:  out[y Wc + x] = ((float)x * scale, (float)y * scale), one fp32 product each.  1 <= Hc, Wc <= NLG_MAX_IMAGE; out 8-byte aligned
 * (16-byte stores of two cells where it is 16-byte aligned).  One launch. */
int nlg_cell_grid(int Hc, int Wc, float scale, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
