/* libnerfloc_counted.so: the coarse matching stage with the NUMBER OF 3-D POINTS in device memory (HIP, gfx950 only).
 *
 * A ninth library, next to libnerfloc_render.so, whose SelfCrossTransformer kernels it shares (csrc/sct_kernels.h) and whose packed weight image it reads
 * (nl_sct_pack_weights, nerfloc_render.h).  It exists for the second stage of cascade localisation (nerf_loc_amd/cascade.py): the 3-D side is a fixed-capacity
 * table of which only the first n rows exist, and n — the count keypoints.select_3d_keypoints_padded leaves on the device — is never read back.  Symbol prefix
 * nlk_; status codes are the NL_* codes of nerfloc_render.h; the Python binding is nerf_loc_amd/_counted_lib.py; tests/counted_ref.py restates the selection in
 * numpy.
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises or uses a float atomic; no kernel waits
 * on another workgroup; every pointer is DEVICE memory; two calls with the same arguments give the same bits; each call is a linear chain of kernel launches
 * and can be captured in a HIP graph.  NL_ERR_BAD_ARG: a null or misaligned argument, a count below 1 where one is required; NL_ERR_UNSUPPORTED: a
 * configuration, precision or size outside the limits; NL_ERR_WORKSPACE: a missing, short or misaligned workspace; NL_ERR_HIP: a launch failed.  All of these are
 * decided on the host before anything is launched or dereferenced.  A count is never an error: it is clamped on the device.
 *
 * The count.  n = min(capacity, max(*count, 0)), read from device memory by every kernel that needs it.  NULL for the pointer means n = capacity, and the call is
 * then, launch for launch, its counterpart in libnerfloc_render.so.  Rows at and beyond n of a counted table must hold FINITE values; they are projected and
 * passed through the row chain like any row (skipping them is a later optimisation), but no output row that the contracts below call valid depends on them.
 */
#ifndef NERFLOC_COUNTED_H
#define NERFLOC_COUNTED_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_render.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLK_ABI_VERSION 1
int nlk_abi_version(void);

/* ---- nlk_sct_forward_counted: nl_sct_forward with the length of sequence 0 in device memory
 * Arguments, limits, alignment, packed image (nl_sct_pack_weights) and workspace as nl_sct_forward; nlk_sct_workspace_bytes = nl_sct_workspace_bytes.  N0 is the
 * CAPACITY of sequence 0: v0, pos0 and out0 are (B, N0, C) and the batch stride is N0 whatever the count.  n0_dev (one int32) is shared by the B items.
 * Only rows 0 .. n - 1 of sequence 0 exist AS KEYS: layer 0 (self-attention of v0) and layer 3 (v1 attends to the new v0) see n keys; layers 1 and 2 have
 * sequence 1 on their key side and are unchanged.  All N0 rows of out0 are computed (a row is a query in layers 0 and 2 whether it exists or not).
 * Contract: out0[b][i] for i < n and every row of out1 equal, bit for bit, nl_sct_forward called with sequence 0 cut to its first n rows.  The attention kernel
 * derives the key-tile count, the number of key ranges (1, 2 or 4 at < 4, < 16, >= 16 tiles of 32 keys) and the tiles per range from n by the host's own rule,
 * so the order of every sum is the exact-size call's.  Keys at and beyond n are not loaded.  n == 0: the attention output of layers 0 and 3 is exactly zero
 * (the rows then carry the out_proj bias through the chain); every output is finite.  Rows i >= n of out0 are finite and mean nothing.
 * n0_dev == NULL: the bits of nl_sct_forward. */
size_t nlk_sct_workspace_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F);
int nlk_sct_forward_counted(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const int32_t* n0_dev,
                            const float* v1, const float* pos1, int64_t N1, int64_t B, float* out0, float* out1, void* ws, size_t ws_bytes, void* stream);

/* ---- nlk_sct_layer_counted: one layer with the count on its key side (the stage entry, the counterpart of nl_sct_layer)
 * Arguments as nl_sct_layer plus nk_dev (one int32): of the Nk rows of the memory side (mem, mem_pos; Nk is the capacity and the batch stride) only the first n
 * are keys.  layer 0 / 1 (self): mem is x (or NULL) and Nk == Nq; all Nq rows are queries and are written.  layer 2 / 3 (cross): mem (B, Nk, C).
 * Contract: every output row equals, bit for bit, nl_sct_layer with the memory side cut to its first n rows (for a self layer: rows i < n of the call on n
 * rows).  Workspace: nlk_sct_workspace_bytes(B, Nq, Nk, C, F).  nk_dev == NULL: the bits of nl_sct_layer. */
int nlk_sct_layer_counted(const void* packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos, int64_t Nq, const float* mem,
                          const float* mem_pos, int64_t Nk, const int32_t* nk_dev, int64_t B, float* out, void* ws, size_t ws_bytes, void* stream);

/* ---- nlk_s2d_select_counted: the mutual-nearest selection of S2DMatching on a score matrix in memory, over the first n rows
 * scores (N, M) fp32, row-major, every value >= +0 and not NaN (sigmoid outputs: their order is the order of their bit patterns); n_dev (one int32); thr the
 * score threshold.  1 <= N, M <= 2^30 and ceil(N / 64) ceil(M / 64) <= 2^24 (one workgroup per 64 x 64 tile in a one-dimensional grid).
 *   rowmax[i] = max over j of scores[i][j] for i < n;   colmax[j] = max over i < n of scores[i][j]          (integer max on the float bits: order-free, exact)
 *   match_j[i] = the FIRST j with scores[i][j] > thr, scores[i][j] == rowmax[i] and scores[i][j] == colmax[j], -1 if there is none  (i < n)
 *   match_score[i] = rowmax[i] if match_j[i] >= 0 else 0
 *   match_j[i] = -1 and match_score[i] = 0 for n <= i < N
 * which is sparse_to_dense.py:136-142 on rows 0 .. n - 1, ties included, and what nl_s2d_match's selection gives on those rows alone.  Rows at and beyond n are
 * not read.  Workspace: nlk_s2d_select_workspace_bytes(N, M) bytes (0: outside the limits), 256-byte aligned; the call clears it with a kernel of its own
 * (not a memset node: DESIGN 5.45).
 * n_dev == NULL: n = N. */
size_t nlk_s2d_select_workspace_bytes(int64_t N, int64_t M);
int nlk_s2d_select_counted(const float* scores, int64_t N, int64_t M, const int32_t* n_dev, float thr, int32_t* match_j, float* match_score, void* ws,
                           size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
