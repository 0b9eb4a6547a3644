/* libnerfloc_cnn.so: the per-frame visibility encoder DepthFusionNet (HIP, gfx950 only) — the 12-channel cross-view input of nl_cross_view_features to the
 * 32-channel map at 1/4 resolution that nl_frame_create takes as vis_featmaps.
 *
 * A fifth library next to libnerfloc_render.so, _head, _app and _geom.  Symbol prefix nlc_; status codes are the NL_* codes of nerfloc_render.h (NL_OK = 0,
 * negative = error); the Python binding is nerf_loc_amd/_cnn_lib.py; tests/dfnet_ref.py restates the arithmetic below in numpy (fp64).
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises or uses a float atomic; no kernel
 * waits on another workgroup; every pointer is DEVICE memory unless it says HOST; two calls with the same arguments give the same bits; each call is a linear
 * chain of launches and can be captured in a HIP graph.  All arithmetic is fp32: the convolutions run on v_mfma_f32_32x32x2_f32 (exact fp32 products, one
 * rounding per product-and-add, k ascending), everything else on the vector unit.  The library is built with -ffp-contract=off.
 * NL_ERR_BAD_ARG: a null or misaligned argument, or a wrong count; NL_ERR_UNSUPPORTED: a size outside the stated limits; NL_ERR_WORKSPACE: a missing, short or
 * not 256-byte aligned workspace (or packed image); NL_ERR_HIP: a launch failed.  All of these are decided on the host before anything is launched or
 * dereferenced: a refused call writes nothing.
 */
#ifndef NERFLOC_CNN_H
#define NERFLOC_CNN_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_render.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLC_ABI_VERSION 1
int nlc_abi_version(void);

/* ---- the weights
 * NLC_DFNET_NUM_WEIGHTS tensors, named as DepthFusionNet's state dict names them (below `multiview_aggregator.depth_fusion.`) and in the state dict's order:
 *   fuse_net.conv1.weight, fuse_net.bn1.{weight,bias},
 *   fuse_net.layer{1,2,3}.0.{conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias, downsample.0.weight, downsample.1.weight, downsample.1.bias},
 *   fuse_net.layer{1,2,3}.1.{conv1.weight, bn1.weight, bn1.bias, conv2.weight, bn2.weight, bn2.bias}          (layer by layer: L.0.* then L.1.*),
 *   fuse_net.{upconv3.conv, iconv3, upconv2.conv, iconv2}.{conv.weight, conv.bias, bn.weight, bn.bias},
 *   fuse_net.out_conv.{weight,bias}, depth_skip.0.{weight,bias}, depth_skip.2.{weight,bias}, conv_out.{weight,bias}.
 * nlc_dfnet_weight_name(i): the i-th name (a static string; NULL outside 0 .. 71).  Host-only: needs no device.
 * nlc_dfnet_pack_weights: ptrs is a HOST array of n = 72 DEVICE pointers to the fp32 tensors as they lie in the state dict (dense, (out, in, kh, kw) for a
 * convolution); the packed image (nlc_dfnet_packed_bytes() bytes, 256-byte aligned) holds every convolution transposed to [k][out] — the 3 x 3 ones with
 * k = (ky 3 + kx) Cin + in, the others with k = (in kh + ky) kw + kx — and everything else as it is.  n != 72 or a null entry: NL_ERR_BAD_ARG; a short or misaligned image: NL_ERR_WORKSPACE.
 * The four conv biases in front of an InstanceNorm (upconv3, iconv3, upconv2, iconv2) are copied but never read: InstanceNorm removes a per-channel constant. */
#define NLC_DFNET_NUM_WEIGHTS 72
int nlc_dfnet_num_weights(void);
const char* nlc_dfnet_weight_name(int i);
size_t nlc_dfnet_packed_bytes(void);
int nlc_dfnet_pack_weights(const void* const* ptrs, int n, void* packed, size_t packed_bytes, void* stream);

/* ---- nlc_dfnet_forward: (V, 12, H, W) -> (V, 32, H/4, W/4)
 * cnn_in (V, 12, H, W) fp32 NCHW: what nl_cross_view_features writes.  out (V, 32, H/4, W/4) fp32 NCHW: what nl_frame_create takes as vis_featmaps.
 * taps: NULL, or three optional NCHW outputs (a NULL member = not wanted): x1 (V, 32, H/4, W/4), x2 (V, 64, H/8, W/8), x3 (V, 128, H/16, W/16), the outputs of
 * layer1, layer2, layer3.  `out` has the same bits whether taps are taken or not.
 * Limits: H and W multiples of 16, each >= 32 (NLC_DFNET_MIN_SIDE); 1 <= V <= NLC_DFNET_MAX_VIEWS; V H W <= 2^26.  Anything else is NL_ERR_UNSUPPORTED and
 * nlc_dfnet_workspace_bytes answers 0.  (These are the sizes on which the decoder's maps meet the depth skip's map without padding.)
 * A view's bits do not depend on the other views of the call: every workgroup works on one view, and no sum's order depends on V.
 *
 * The arithmetic.  reflect(i, n) = -i for i < 0, 2 (n - 1) - i for i >= n.  conv(k, s, p) is a k x k convolution of stride s over the input padded by p with
 * reflect; its sums run in ascending k, one fused multiply-add per term from 0, with k = (ky 3 + kx) Cin + in for the 3 x 3 convolutions
 * (tap-major: the channels of cat[a, b] are a's, then b's) and k = (in k + ky) k + kx for the others.  IN is InstanceNorm per (view, channel)
 * over the plane's n values:  mean = (sum x) / n,  var = (sum (x - mean)^2) / n  (biased; the deviations are taken from the finished mean, there is no
 * E[x^2] - E[x]^2),  IN(x) = (x - mean) * (gamma / sqrt(var + 1e-5)) + beta.  Both sums: thread t of 256 adds values t, t + 256, ... in ascending order, the
 * 256 sums are added in a fixed tree (stride 128, 64, ..., 1).
 *   c0 = ReLU(IN(conv(8, 2, 2)(cnn_in)))                                            12 -> 32, (H/2 - 1) x (W/2 - 1), no bias
 *   BasicBlock(x; s): a = ReLU(IN(conv(3, s, 1)(x))); b = IN(conv(3, 1, 1)(a)); i = x if s == 1 else IN(conv(1, 2, 0)(x)); ReLU(b + i)
 *   x1 = layer1(c0), x2 = layer2(x1), x3 = layer3(x2): layerL(x) = BasicBlock(BasicBlock(x; 2); 1) with 32, 64, 128 channels
 *   up(x): bilinear x 2 with align_corners: source coordinate sy = oy * ((h - 1) / (2 h - 1)) (the ratio rounded to fp32 first), y0 = floor(sy), y1 = min(y0 + 1,
 *          h - 1), ly = sy - y0, likewise in x;  up = (1 - ly) ((1 - lx) x[y0][x0] + lx x[y0][x1]) + ly ((1 - lx) x[y1][x0] + lx x[y1][x1])
 *   u3 = ELU(IN(conv(3, 1, 1)(up(x3))))   128 -> 64          i3 = ELU(IN(conv(3, 1, 1)(cat[u3, x2])))   128 -> 64
 *   u2 = ELU(IN(conv(3, 1, 1)(up(i3))))    64 -> 32          i2 = ELU(IN(conv(3, 1, 1)(cat[u2, x1])))    64 -> 32         (their conv biases cancel in IN: skipped)
 *   f = out_conv(i2) (1 x 1, bias);  d = conv(2, 2, 0)(ReLU(conv(2, 2, 0)(cnn_in[:, 3]) + bias)) + bias  (1 -> 8 -> 16);  out = conv_out(cat[d, f]) (1 x 1, bias)
 * ELU(x) = x > 0 ? x : expm1f(x).  In f, d and out the bias is added after the sum.
 * The convolutions write raw sums; one launch per InstanceNorm, one workgroup per plane, takes (mean, gamma / sqrt(var + eps), beta) and, where every reader
 * of the map wants ReLU(IN(x)) or ELU(IN(x)), rewrites the plane in place; a BasicBlock's ReLU(IN(b) + i) is one more launch, out_conv + depth_skip + conv_out
 * the last.  The two bilinear x 2 are a launch each; the concatenations happen in the consuming convolution's loads.  NLC_DFNET_LAUNCHES launches in all.
 * Workspace: nlc_dfnet_workspace_bytes(V, H, W) bytes, 256-byte aligned. */
#define NLC_DFNET_MIN_SIDE 32
#define NLC_DFNET_MAX_VIEWS 64
#define NLC_DFNET_MAX_PIXELS 67108864
#define NLC_DFNET_LAUNCHES 49
typedef struct {
  float* x1;
  float* x2;
  float* x3;
} nlc_dfnet_taps;
size_t nlc_dfnet_workspace_bytes(int V, int H, int W);
int nlc_dfnet_forward(const void* packed, const float* cnn_in, int V, int H, int W, float* out, const nlc_dfnet_taps* taps, void* ws, size_t ws_bytes,
                      void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
