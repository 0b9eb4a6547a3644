/* libnerfloc_cnn_train.so: the per-frame visibility encoder DepthFusionNet for training (HIP, gfx950 only) — a forward that keeps what its backward needs, and
 * that backward: the gradients of all 72 parameters from the cotangent of the 32-channel map.
 *
 * An eighth library, next to libnerfloc_cnn.so (include/nerfloc_cnn.h), whose kernels, weight table and arithmetic it shares (csrc/cnn_kernels.h): read that
 * header first; the names of maps and weights below are its names.  Symbol prefix nlct_; status codes are the NL_* codes of nerfloc_render.h; the Python
 * binding is nerf_loc_amd/_cnn_train_lib.py; tests/dfnet_train_ref.py restates the stage arithmetic below in numpy (fp64).
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises or uses a float atomic; no kernel
 * waits on another workgroup; every pointer is DEVICE memory unless it says HOST; two calls with the same arguments give the same bits; each call is a linear
 * chain of launches and can be captured in a HIP graph.  All arithmetic is fp32: the convolutions and their two gradients run on v_mfma_f32_32x32x2_f32 (exact
 * fp32 products, one rounding per product-and-add), everything else on the vector unit.  The library is built with -ffp-contract=off.
 * NL_ERR_BAD_ARG: a null or misaligned argument, or a wrong count; NL_ERR_UNSUPPORTED: a size outside the stated limits; NL_ERR_WORKSPACE: a missing, short or
 * not 256-byte aligned workspace, state or packed image; NL_ERR_HIP: a launch failed.  All of these are decided on the host before anything is launched or
 * dereferenced: a refused call writes nothing.
 * Limits of the dfnet calls, as nlc_dfnet_forward: H and W multiples of 16, each >= 32; 1 <= V <= 64; V H W <= 2^26.  Outside them the size queries answer 0.
 */
#ifndef NERFLOC_CNN_TRAIN_H
#define NERFLOC_CNN_TRAIN_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_cnn.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLCT_ABI_VERSION 1
int nlct_abi_version(void);

/* ---- the weights
 * ptrs: a HOST array of n = 72 DEVICE pointers, the tensors and the order of nlc_dfnet_weight_name.  The image (nlct_dfnet_packed_bytes() bytes, 256-byte
 * aligned) holds, first, the inference image of nlc_dfnet_pack_weights bit for bit (written by the same kernel), and behind it, for each of the 19 convolutions
 * that hand a gradient to their input (every 3 x 3 and every downsample 1 x 1; not conv1, not the head), the weights as [(ky ks + kx) Cout + out][in]: the
 * operand of the data gradient.  n != 72 or a null entry: NL_ERR_BAD_ARG; a short or misaligned image: NL_ERR_WORKSPACE. */
size_t nlct_dfnet_packed_bytes(void);
int nlct_dfnet_pack_weights(const void* const* ptrs, int n, void* packed, size_t packed_bytes, void* stream);

/* ---- nlct_dfnet_forward_train: (V, 12, H, W) -> (V, 32, H/4, W/4), keeping the state
 * The arithmetic of nlc_dfnet_forward in the same order, by the same kernels: `out` is bit-equal to it.  Nothing the backward needs is overwritten: where the
 * inference plan reuses a block's buffers and rewrites a plane in place as act(IN(x)), this plan gives every map its own buffer and writes act(IN(x)) next to
 * the raw sums.  NLCT_FORWARD_LAUNCHES launches.
 * The state, fp32, every buffer padded to a multiple of 64 values; n0 = (H/2 - 1)(W/2 - 1), n1 = (H/4)(W/4), n2 = n1 / 4, n3 = n1 / 16, C1 = 32, C2 = 64, C3 = 128:
 *   conv1: the raw sums and ReLU(IN) (V 32 n0 each), its norm (V 32 4)
 *   layer L = 1, 2, 3: nine maps of V CL nL — block 0's a raw, a = ReLU(IN(a raw)), b raw, the raw downsample, the block's output; block 1's a raw, a, b raw, the
 *              block's output (= x1, x2, x3) — and five norms of V CL 4
 *   decoder: up(x3) (V 128 n2); u3 raw, u3, i3 raw, i3 (V 64 n2 each); up(i3) (V 64 n1); u2 raw, u2, i2 raw, i2 (V 32 n1 each); four norms (V 64 4 twice, V 32 4 twice)
 * A norm is (mean, gamma / sqrt(var + eps), beta, 1 / sqrt(var + eps)) per (view, channel).
 * nlct_dfnet_state_bytes(V, H, W) = 4 x the sum of those padded sizes, rounded up to 256; `state` must be 256-byte aligned and state_bytes at least that. */
#define NLCT_FORWARD_LAUNCHES 49
size_t nlct_dfnet_state_bytes(int V, int H, int W);
int nlct_dfnet_forward_train(const void* packed, const float* cnn_in, int V, int H, int W, float* out, void* state, size_t state_bytes, void* stream);

/* ---- nlct_dfnet_backward: the 72 parameter gradients of sum(out * g_out)
 * packed, cnn_in, V, H, W, state: what the forward call had and left.  g_out (V, 32, H/4, W/4).  grads: a HOST array of 72 DEVICE pointers in the order of
 * nlc_dfnet_weight_name, each to a dense fp32 tensor of the parameter's own shape ((out, in, kh, kw) for a convolution); NULL = not wanted: a convolution
 * weight that is not wanted costs no weight-gradient launch.  The call WRITES the gradients, it does not add.  There is no gradient for cnn_in.
 * With every gradient wanted the chain is NLCT_BACKWARD_LAUNCHES launches, two fewer for every convolution weight and one fewer for every head bias that is not.
 *
 * The arithmetic.  ReLU' = (kept output > 0), the forward's own mask; ELU' = y > 0 ? 1 : y + 1 on the kept output y.
 * InstanceNorm, per (view, channel) plane of n values, g_z the cotangent of IN's output:  xhat = (x - mean) rstd,  s1 = sum g_z,  s2 = sum g_z xhat,
 *   g_x = (gamma rstd) (g_z - s1 / n - xhat (s2 / n)); both sums by the forward's scheme (thread t of 256 adds t, t + 256, ..., then the fixed tree);
 *   g_beta = sum over the views of s1, g_gamma = of s2, in ascending view order.
 * The four conv biases in front of an InstanceNorm (upconv3, iconv3, upconv2, iconv2) get exact zeros: their gradient is identically zero.
 * BasicBlock tail y = ReLU(IN(b) + i): g_y (y > 0) is the cotangent of both IN(b) and i.
 * A map read by several consumers receives the sum of their cotangents in this order: the decoder's skip convolution (iconv2 for x1, iconv3 for x2), then
 * the next layer's conv1, then its downsample; block 0's output: block 1's conv1, then block 1's identity; conv1's map: layer1.0.conv1, then its downsample.
 * Bilinear x 2: each source pixel sums g[oy][ox] (wy wx) over the destination pixels that read it, oy then ox ascending, wy = (y0 == sy ? 1 - ly : 0) +
 *   (y1 == sy ? ly : 0) with the forward's y0, y1, ly, likewise wx.
 * Convolution weight gradient: g_w[o][k] = sum over (v, p) of g_y[v][o][p] patch[v][p][k], patch the forward's reflecting, concatenating gather.  The pixels
 *   of a view are cut into `chunks` ranges of CH pixels (chunks = min(ceil(npix / 512), max(1, 256 / V)), CH = ceil(npix / chunks) rounded up to 32); one
 *   workgroup sums one (view, range) on the MFMA, pixels ascending from 0, into a partial; a second launch adds the partials, view-major ascending.
 * Convolution data gradient: on the PADDED input domain (hin + 2 pad) x (win + 2 pad), gp[ci][py][px] = sum over k = (ky ks + kx) Cout + o ascending of
 *   g_y[o][(py - ky) / s][(px - kx) / s] w[o][ci][ky][kx], a term being zero unless both quotients are exact and inside the output plane; then the fold:
 *   g_x[iy][ix] = the sum, rows then columns ascending, of gp over the padded rows {0 if iy == 1; iy + 1; hin + 1 if iy == hin - 2} and the like columns
 *   (pad 1; with pad 0 gp is g_x).  One thread writes each value.
 * Head: one thread per pixel recomputes d, f and the hidden depth-skip values with the forward's arithmetic and forms the cotangents of f, d, the ReLU'd
 *   hidden values and ELU(IN(iconv2)), each sum in ascending index order by fused multiply-add from 0; the four weight gradients are 1 x 1 (2 x 2 for
 *   depth_skip.0) weight gradients by the scheme above, the four bias gradients per-(view, channel) tree sums added in ascending view order.
 * Workspace: nlct_dfnet_backward_workspace_bytes(V, H, W) bytes, 256-byte aligned. */
#define NLCT_BACKWARD_LAUNCHES 116
size_t nlct_dfnet_backward_workspace_bytes(int V, int H, int W);
int nlct_dfnet_backward(const void* packed, const float* cnn_in, int V, int H, int W, const void* state, const float* g_out, void* const* grads, void* ws,
                        size_t ws_bytes, void* stream);

/* ---- the stages, one call each (what the tests reach the index arithmetic through)
 * nlct_conv_backward: one convolution of the net's kinds.  Input cat[x0 (V, C0, hin, win), x1 (V, C1, hin, win)] (C1 == 0: x1 is not read), weights w
 * (cout, C0 + C1, ks, ks) as in a state dict, ks in {1, 3, 8} with reflect pad 0, 1, 2, stride 1 or 2; g_y (V, cout, ho, wo), ho = (hin + 2 pad - ks) /
 * stride + 1.  Outputs, each optional (NULL): g_x0, g_x1 (the shapes of x0, x1), g_w (the shape of w).  The data gradients need ks in {1, 3}, cout and
 * C0 + C1 multiples of 32; the weight gradient needs x0 (and x1).  Limits: 1 <= V <= 64, C0 + C1 <= 512, cout <= 512, hin, win in 2 .. 8192 and > pad,
 * every tensor below 2^31 values.  nlct_conv_backward_workspace_bytes answers 0 outside them.
 * nlct_instnorm_backward: x raw (V, C, n), nrm (V, C, 4) as the state keeps it, y the kept act(IN(x)) (or the block's output for a tail; not read with
 * act == 0), act 0 none / 1 ReLU / 2 ELU, g_y the cotangent of y -> g_x (V, C, n; may be g_y itself), g_gamma (C), g_beta (C), each optional.
 * ws: at least 8 V C bytes, 256-byte aligned.  Limits: 1 <= V <= 64, 1 <= C <= 4096, 1 <= n < 2^31 / (V C).
 * nlct_up2_backward: g_y (planes, 2 h, 2 w) -> g_x (planes, h, w); h, w >= 2, planes >= 1, 4 planes h w < 2^31. */
size_t nlct_conv_backward_workspace_bytes(int V, int C0, int C1, int cout, int hin, int win, int ks, int stride);
int nlct_conv_backward(const float* x0, int C0, const float* x1, int C1, const float* w, const float* g_y, int V, int cout, int hin, int win, int ks, int stride,
                       float* g_x0, float* g_x1, float* g_w, void* ws, size_t ws_bytes, void* stream);
int nlct_instnorm_backward(const float* x, const float* nrm, const float* y, int act, const float* g_y, int V, int C, int n, float* g_x, float* g_gamma,
                           float* g_beta, void* ws, size_t ws_bytes, void* stream);
int nlct_up2_backward(const float* g_y, int planes, int h, int w, float* g_x, void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
