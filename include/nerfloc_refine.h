/* libnerfloc_refine.so: on-device pose refinement (HIP, gfx950 only) — everything PoseOptimizer (pose_optimizer.py:39-199) runs AROUND the renderer's
 * forward / backward pair: the se(3) maps and their gradient, the rays of a pose, the bilinear target, the masked MSE and its cotangent, the reduction of the ray
 * cotangents to the pose, and Adam on the six pose parameters.  The render pair itself is nl_render_rays_forward_keep / nl_render_rays_backward_kept of
 * libnerfloc_render.so, called by the host between nlr_pose_rays / nlr_loss / nlr_step on buffers they share; this library holds no render code.
 *
 * A seventh library.  Symbol prefix nlr_; status codes are the NL_* codes of nerfloc_render.h (NL_OK = 0, negative = error); the Python binding is
 * nerf_loc_amd/_refine_lib.py; tests/refine_ref.py restates every contract below in numpy (fp64).
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises, copies or uses an atomic; every pointer
 * is DEVICE memory; two calls with the same arguments give the same bits; the bits of one pose do not depend on the other poses of the call; each call is a linear
 * chain of launches (one launch, in fact) and can be captured in a HIP graph; no kernel waits for another workgroup.  B = 0, Rp = 0 or N = 0: NL_OK, nothing is
 * launched or dereferenced.  NL_ERR_BAD_ARG: a null / negative / misaligned argument or an unknown flag; NL_ERR_UNSUPPORTED: a size above a stated limit;
 * NL_ERR_HIP: a launch failed.  All decided on the host before anything is launched.
 *
 * ARITHMETIC.  fp32 inputs (K, uv, renderer outputs, cotangents, maps) are loaded as they lie and widened; from there everything is fp64, each written operation
 * one rounding (the library is built with -ffp-contract=off); fp32 outputs are rounded once on the store.  sin / cos / acos / sqrt / pow are the device library's.
 *
 * THE se(3) MAPS (the convention of the reference's utils/transform/se3.py, which returns the TRANSPOSE of PyTorch3D's matrix: a column-vector camera-to-world pose).
 *   p = [u | w]  (log-translation, log-rotation);  EPS = 1e-4;  n = w0 w0 + w1 w1 + w2 w2;  th = sqrt(max(n, EPS))  — the SQUARED angle is clamped;
 *   K = hat(w) = [[0, -w2, w1], [w2, 0, -w0], [-w1, w0, 0]],  K2 = K K  (the matrix product, as written);
 *   exp:  f1 = (1 / th) sin th,  f2 = (1 / th)(1 / th)(1 - cos th),  a = (1 - cos th) / th^2,  b = (th - sin th) / th^3;
 *         T[0:3][0:3] = I - f1 K + f2 K2   (= (I + f1 K + f2 K2)^T),   T[0:3][3] = (I + a K + b K2) u,   T[3] = (0, 0, 0, 1)
 *   exp backward: for a cotangent G (4 x 4, only its top three rows matter) the gradient of sum(G * T) with respect to p, differentiating the formulas above as
 *         written; the derivative of th with respect to n is 1 / (2 th) where n >= EPS and ZERO below the clamp (torch.clamp's rule).
 *   log:  R = T[0:3][0:3]^T;  c = ((R00 + R11 + R22) - 1) / 2;  bound = 1 - 1e-4;  phi = acos(c) for -bound < c < bound, otherwise the tangent line of acos at the
 *         bound that c passed: (c - x0)(-1 / sqrt(1 - x0 x0)) + acos(x0), x0 = -bound for c <= -bound, x0 = bound for c >= bound;
 *         s = sin phi;  fac = phi / (2 s) where |s| > 0.5 EPS, else 0.5 + phi phi / 12;
 *         w = fac (R21 - R12, R02 - R20, R10 - R01);  then th, K, K2, a, b from w as above,  V = I + a K + b K2,  u = V^-1 T[0:3][3]  (adjugate / determinant).
 *         The bottom row of T is not read and not checked.
 *
 * THE STATE BLOCK: B records of NLR_STATE_DOUBLES 8-byte words, one per pose, 8-byte aligned:
 *   [0:6) params  [6:12) m  [12:18) v  [18:24) grad (the last step's gradient of the loss with respect to params)  [24] loss_init  [25] loss_last
 *   [26:42) pose0, the pose given to nlr_init (row-major 4 x 4; an fp32 pose widened, which is exact)   [42] t, the step counter (int64)   [43] the NaN latch (int64, 0 / 1)
 */
#ifndef NERFLOC_REFINE_H
#define NERFLOC_REFINE_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_render.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLR_ABI_VERSION 1
int nlr_abi_version(void);

#define NLR_POSE_F32 0u
#define NLR_POSE_F64 1u
#define NLR_LAYOUT_NCHW 0
#define NLR_LAYOUT_NHWC 1
#define NLR_MAX_POSES 16
#define NLR_MAX_RAYS 1048576
#define NLR_MAX_CHANNELS 1024
#define NLR_MAX_IMAGE 32768
#define NLR_STATE_DOUBLES 44

/* ---- the three maps on their own: p (N, 6) fp64, T (N, 4, 4) fp64 row-major, G (N, 4, 4) fp64, g_p (N, 6) fp64.  0 <= N <= 2^20.  One thread per matrix. */
int nlr_se3_exp(const double* p, int64_t N, double* T, void* stream);
int nlr_se3_exp_backward(const double* p, const double* G, int64_t N, double* g_p, void* stream);
int nlr_se3_log(const double* T, int64_t N, double* p, void* stream);

/* ---- nlr_state_bytes / nlr_init
 * nlr_state_bytes(B) = B NLR_STATE_DOUBLES 8 for 1 <= B <= NLR_MAX_POSES, otherwise 0.
 * nlr_init: poses (B, 4, 4) row-major, fp32 (NLR_POSE_F32) or fp64 (NLR_POSE_F64) by pose_flags.  params = log(pose); m, v, grad, loss_init, loss_last, t and the
 * latch are zero; pose0 = the pose as given. */
size_t nlr_state_bytes(int B);
int nlr_init(const void* poses, unsigned pose_flags, int B, void* state, void* stream);

/* ---- nlr_pose_rays: the rays of every pose through the same Rp pixels                     (se3_exp_map + points_2d_to_rays, pose_optimizer.py:134-136)
 * K (3, 3) fp32: fx = K[0], cx = K[2], fy = K[4], cy = K[5].  uv (Rp, 2) fp32 = (x, y), truncated towards zero as nl_get_rays does.
 * T_b = exp(params_b);  pose32_out (B, 4, 4) fp32 = T_b (optional: may be NULL).  For ray r = b Rp + i:
 *   cam = ((x - cx) / fx, (y - cy) / fy, 1);  v_k = cam0 T[k][0] + cam1 T[k][1] + cam2 T[k][2];  len = sqrt(v0 v0 + v1 v1 + v2 v2);
 *   rays_d[r] = v / len;   rays_o[r] = centres[r] = T[0:3][3]      — all three (B Rp, 3) fp32.
 * One workgroup per 256 pixels; its first B threads form the B matrices once, in LDS; every thread then serves its pixel for all B poses.
 * 0 <= B <= NLR_MAX_POSES, 0 <= Rp <= NLR_MAX_RAYS. */
int nlr_pose_rays(const void* state, const float* K, const float* uv, int B, int Rp, float* pose32_out, float* rays_o, float* rays_d, float* centres, void* stream);

/* ---- nlr_sample_target: the values F.interpolate(map, size=(H, W), mode='bilinear', align_corners=False) has at Rp pixels, without forming the resized map
 * map: C channels of h x w, NLR_LAYOUT_NCHW (C, h, w) or NLR_LAYOUT_NHWC (h, w, C), fp32, read as it lies.  uv (Rp, 2) fp32, truncated towards zero, then clamped to
 * [0, W - 1] x [0, H - 1] (so that no read leaves the map).  Per axis: src = (x + 0.5)(w / W) - 0.5, negative -> 0;  i0 = min(trunc(src), w - 1);  i1 = min(i0 + 1, w - 1);
 * l1 = src - i0, l0 = 1 - l1.   out[i][c] = ly0 (lx0 m[y0][x0] + lx1 m[y0][x1]) + ly1 (lx0 m[y1][x0] + lx1 m[y1][x1]),   out (Rp, C) fp32.
 * 1 <= C <= NLR_MAX_CHANNELS, 1 <= h, w, H, W <= NLR_MAX_IMAGE.  One thread per value. */
int nlr_sample_target(const float* map, int layout, int C, int h, int w, int H, int W, const float* uv, int Rp, float* out, void* stream);

/* ---- nlr_loss: the masked squared error per ray and the cotangent of the mean                                               (pose_optimizer.py:149-156)
 * out (B Rp, C) fp32, mask (B Rp) uint8 (0 / 1), target (Rp, C) fp32: ray r is held against target[r mod Rp].   e = (out - target) mask   (a NaN stays a NaN)
 * row_loss[r] = sum_c e e  (fp64; one wave per ray, each lane sums its channels in ascending order, the 64 lane sums are added by a fixed butterfly);
 * g_out[r][c] = 2 mask e / (Rp C)  rounded to fp32: the cotangent of torch.mean over one pose's (Rp, C) block.  g_out may alias nothing it reads.
 * 16-byte loads and stores where C % 4 == 0 and out, target and g_out are 16-byte aligned.  1 <= C <= NLR_MAX_CHANNELS. */
int nlr_loss(const float* out, const uint8_t* mask, const float* target, int B, int Rp, int C, float* g_out, double* row_loss, void* stream);

/* ---- nlr_step: loss, latch, the pose gradient and one Adam step; one workgroup per pose                                    (pose_optimizer.py:150-168)
 * C is the channel count that nlr_loss summed over.  A pose whose latch is set is left untouched.  Otherwise, in this order:
 *  1. loss = (row_loss[b Rp] + ... + row_loss[b Rp + Rp - 1], left to right) / (Rp C);  2. if t == 0: loss_init = loss;  loss_last = loss;
 *  3. if loss is NaN: latch = 1 and the step ends here (params, moments and t keep their values from now on);
 *  4. with T = exp(params), cam and v as in nlr_pose_rays, and g_o, g_d, g_c the rows of g_rays_o, g_rays_d, g_centres (B Rp, 3) fp32:
 *       g_v = (g_d - dhat (dhat . g_d)) / len, dhat = v / len;   G[k][j] = sum_i g_v[k] cam[j];   G[k][3] = sum_i (g_o[k] + g_c[k]);
 *     the sums run over the pose's rays: thread q adds rays q, q + 256, ... in ascending order, the 256 partial sums are added in ascending q;
 *  5. grad = exp backward(params, G);
 *  6. torch.optim.Adam without weight decay: t += 1;  m += (grad - m)(1 - beta1);  v = v beta2 + (1 - beta2) grad grad;
 *     params += -(lr / (1 - beta1^t)) (m / (sqrt(v) / sqrt(1 - beta2^t) + eps)).
 * Nothing on the host changes from step to step: the counter lives in the state.
 * Cost: the fixed order is paid for with serial work — one thread adds the pose's Rp row losses, and each of twelve threads adds 256 partial sums.  At the few hundred
 * to few thousand rays of a refinement that is microseconds; towards NLR_MAX_RAYS the Rp serial additions (about a millisecond per 10^5 rays) would dominate the
 * step.  The limit is the other calls'; a caller with that many rays per pose should not expect this call to scale with them. */
int nlr_step(void* state, const double* row_loss, const float* g_rays_o, const float* g_rays_d, const float* g_centres, const float* K, const float* uv, int B, int Rp,
             int C, double lr, double beta1, double beta2, double eps, void* stream);

/* ---- nlr_finish: the refined poses under the reference's discard rule                                                       (pose_optimizer.py:157-176)
 * accepted = !(latch || loss_last > loss_init).  T_c2w64 (B, 4, 4) fp64 / T_c2w32 (B, 4, 4) fp32 (either may be NULL) = exp(params) where accepted, else pose0 —
 * the pose given to nlr_init, bit for bit.   info (B, 4) fp64 = (loss_init, loss_last, accepted, latch). */
int nlr_finish(const void* state, int B, double* T_c2w64, float* T_c2w32, double* info, void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
