/* libnerfloc_backbone.so: the 2-D backbone (HIP, gfx950 only) — ResNet-50 up to layer2 with frozen BatchNorm, plus the two-level feature pyramid (FPN) with
 * InstanceNorm: (V, 3, H, W) images in [0, 1] to the raw conv1 map and the two FPN maps that the matchers, the appearance layers and the frame setup consume.
 *
 * A sixth library next to libnerfloc_render.so, _head, _app, _geom and _cnn.  Symbol prefix nlb_; status codes are the NL_* codes of nerfloc_render.h (NL_OK = 0,
 * negative = error); the Python binding is nerf_loc_amd/_backbone_lib.py; tests/backbone_ref.py restates the arithmetic below in numpy (fp64).
 *
 * Common to all calls: asynchronous on `stream` (a hipStream_t, NULL = the default stream); no call allocates, synchronises or uses a float atomic; no kernel
 * waits on another workgroup; every pointer is DEVICE memory unless it says HOST; indices are 64-bit; two calls with the same arguments give the same bits; each
 * call is a linear chain of launches and can be captured in a HIP graph.  With NLB_PRECISION_FP32 all arithmetic is fp32: the convolutions run on
 * v_mfma_f32_32x32x2_f32 (exact fp32 products, one rounding per product-and-add, k ascending), everything else on the vector unit; NLB_PRECISION_BF16X3 changes
 * the products of the 1 x 1 and 3 x 3 convolutions only (below).  The library is built with -ffp-contract=off.
 * NL_ERR_BAD_ARG: a null or misaligned argument, a wrong count, an unknown precision or layout; NL_ERR_UNSUPPORTED: a size or fpn_dim outside the stated limits;
 * NL_ERR_WORKSPACE: a missing, short or not 256-byte aligned workspace (or packed image); NL_ERR_HIP: a launch failed.
 * All of these are decided on the host before anything is launched or dereferenced: a refused call writes nothing.
 */
#ifndef NERFLOC_BACKBONE_H
#define NERFLOC_BACKBONE_H

#include <stddef.h>
#include <stdint.h>
#include "nerfloc_render.h"

/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#pragma GCC visibility push(default)
#ifdef __cplusplus
extern "C" {
#endif

#define NLB_ABI_VERSION 1
int nlb_abi_version(void);

/* fpn_dim: 64, 128, 192 or 256.  Any other value: the size queries answer 0 and the calls NL_ERR_UNSUPPORTED. */
#define NLB_PRECISION_FP32 0
#define NLB_PRECISION_BF16X3 1   /* three-term split-bf16 operands in the 1 x 1 and 3 x 3 convolutions */
#define NLB_LAYOUT_NCHW 0
#define NLB_LAYOUT_CHANNELS_LAST 1

/* ---- the weights
 * NLB_BACKBONE_NUM_WEIGHTS tensors, named as the state dict of Backbone(return_layers=['conv1', 'layer1', 'layer2'], use_fpn=True) names them, in its order:
 *   body.conv1.weight, body.bn1.{weight, bias, running_mean, running_var},
 *   body.layer1.0.{conv1.weight, bn1.*, conv2.weight, bn2.*, conv3.weight, bn3.*, downsample.0.weight, downsample.1.*},  body.layer1.{1,2}.{conv1 .. bn3.*},
 *   body.layer2.0.{conv1 .. downsample.1.*},  body.layer2.{1,2,3}.{conv1 .. bn3.*}        (bn*.* = weight, bias, running_mean, running_var),
 *   fpn.inner_blocks.{0,1}.0.weight, fpn.layer_blocks.{0,1}.0.weight.
 * The names do not depend on fpn_dim; only the shapes of the last four do.  nlb_backbone_weight_name(i): the i-th name (a static string; NULL outside 0 .. 123).
 * Host-only: needs no device.
 * nlb_backbone_pack_weights: ptrs is a HOST array of n = 124 DEVICE pointers to the fp32 tensors as they lie in the state dict (dense, (out, in, kh, kw) for a
 * convolution).  The packed image (nlb_backbone_packed_bytes(fpn_dim) bytes, 256-byte aligned) holds every convolution transposed to [k][out] — the 3 x 3 ones
 * with k = (ky 3 + kx) Cin + in, the 1 x 1 ones with k = in, conv1 with k = (in 7 + ky) 7 + kx and 13 rows of zeros after its 147 — and every frozen BatchNorm
 * folded to per-channel (scale, bias) as the module computes them:  scale = weight * (1 / sqrt(running_var + 1e-5)),  bias = bias - running_mean * scale.
 * Every 1 x 1 and 3 x 3 convolution lies there a second time, pre-split for NLB_PRECISION_BF16X3: w = hi + lo with hi = bf16(w), lo = bf16(w - hi) (round to
 * nearest even), each as [k / 8][out][8] 16-bit values, the order a lane of v_mfma_f32_32x32x16_bf16 reads them in.  One image serves both precisions.
 * n != 124 or a null entry: NL_ERR_BAD_ARG; a short or misaligned image: NL_ERR_WORKSPACE. */
#define NLB_BACKBONE_NUM_WEIGHTS 124
int nlb_backbone_num_weights(int fpn_dim);
const char* nlb_backbone_weight_name(int i);
size_t nlb_backbone_packed_bytes(int fpn_dim);
int nlb_backbone_pack_weights(const void* const* ptrs, int n, int fpn_dim, void* packed, size_t packed_bytes, void* stream);

/* ---- nlb_backbone_forward: (V, 3, H, W) -> conv1 (V, 64, h1, w1), layer1 (V, fpn_dim, h2, w2), layer2 (V, fpn_dim, h3, w3)
 * imgs (V, 3, H, W) fp32 NCHW in [0, 1].  h1 = (H - 1) / 2 + 1, h2 = (h1 - 1) / 2 + 1, h3 = (h2 - 1) / 2 + 1 in integers, likewise in w.
 * conv1_out (V, 64, h1, w1) fp32 NCHW: the raw sums of conv1, before bn1.  p_layer1 (V, fpn_dim, h2, w2) and p_layer2 (V, fpn_dim, h3, w3): the FPN outputs, as
 * dense NCHW (layout = NLB_LAYOUT_NCHW) or as dense (V, h, w, fpn_dim) (NLB_LAYOUT_CHANNELS_LAST); the values are the same in both.
 * taps: NULL, or two optional NCHW outputs (a NULL member = not wanted): layer1 (V, 256, h2, w2) and layer2 (V, 512, h3, w3), the outputs of the ResNet's layer1
 * and layer2 in front of the FPN.  The three outputs have the same bits whether taps are taken or not.
 * Limits: H, W >= NLB_BACKBONE_MIN_SIDE, no divisibility requirement; 1 <= V <= NLB_BACKBONE_MAX_VIEWS; V H W <= 2^24.  Anything else is NL_ERR_UNSUPPORTED and
 * nlb_backbone_workspace_bytes answers 0.  An unknown precision or layout is NL_ERR_BAD_ARG.
 * A view's bits do not depend on the other views of the call: every workgroup works on one view, and no sum's order depends on V.
 *
 * The arithmetic.  conv(k, s, p) is a k x k convolution of stride s over the input padded by p with ZEROS; its sums run in ascending k, one fused
 * multiply-add per term from 0, with k = (ky 3 + kx) Cin + in for the 3 x 3 convolutions, k = in for the 1 x 1 ones and k = (in 7 + ky) 7 + kx for conv1.
 * NLB_PRECISION_BF16X3: in the 1 x 1 and 3 x 3 convolutions both operands are split as the weights are (the activations as they are staged), and per 16 k
 * the fp32 accumulator takes w_lo x_hi, then w_hi x_lo, then w_hi x_hi on v_mfma_f32_32x32x16_bf16 (the lo lo term, 2^-16 of a product, is dropped); conv1
 * (K = 147, 3.5 % of the multiply-adds), the accumulation, every epilogue and the InstanceNorms are as in fp32.
 * BN_j(x) = x * scale_j + bias_j (one multiply, then one add) with the packed image's folded (scale, bias).  ReLU(x) = x < 0 ? 0 : x.
 *   n  = (imgs - mean_c) / std_c,  mean = (0.485, 0.456, 0.406), std = (0.229, 0.224, 0.225) rounded to fp32: applied when a pixel is loaded; a padded pixel
 *        is zero AFTER normalisation, which is why the normalisation is not folded into conv1's weights.
 *   conv1 = conv(7, 2, 3)(n)                                       3 -> 64, h1 x w1, raw sums: this is the output `conv1`
 *   p0 = maxpool(3, 2, 1)(ReLU(BN(conv1)))                         h2 x w2; the maximum runs over the window's in-range pixels; one pass over conv1
 *   Bottleneck(x; planes, s): a = ReLU(BN(conv(1, 1, 0)(x)));  b = ReLU(BN(conv(3, s, 1)(a)));  i = x, or BN(conv(1, s, 0)(x)) in the first block of a layer;
 *                             ReLU(BN(conv(1, 1, 0)(b)) + i)       planes -> planes -> 4 planes; every BN, ReLU and the add sit in the convolution's epilogue
 *   x1 = layer1(p0): 3 Bottlenecks, planes 64, s = 1               256 channels, h2 x w2   (taps.layer1)
 *   x2 = layer2(x1): 4 Bottlenecks, planes 128, s = 2 in the first 512 channels, h3 x w3   (taps.layer2)
 * IN is InstanceNorm without affine parameters per (view, channel) over the plane's n values:  mean = (sum x) / n,  var = (sum (x - mean)^2) / n  (biased; the
 * deviations are taken from the finished mean),  IN(x) = (x - mean) * (1 / sqrt(var + 1e-5)).  Both sums: thread t of 256 adds values t, t + 256, ... in
 * ascending order, the 256 sums are added in a fixed tree (stride 128, 64, ..., 1).  The FPN's convolutions have no bias.
 *   m2 = IN(conv(1, 1, 0)(x2))                                     512 -> fpn_dim          p_layer2 = IN(conv(3, 1, 1)(m2))
 *   m1 = IN(conv(1, 1, 0)(x1)) + up(m2)                            256 -> fpn_dim          p_layer1 = IN(conv(3, 1, 1)(m1))
 *   up(m2)[y][x] = m2[(y h3) / h2][(x w3) / w2] in integers: nearest neighbour, what F.interpolate(mode="nearest") takes for these sizes.
 * Launches: conv1, the BN + ReLU + max-pool pass, 10 convolutions of layer1, 13 of layer2, 4 of the FPN, one InstanceNorm launch behind each of those 4 (one
 * workgroup per plane; the one of m1 adds up(m2) as it writes), and for NLB_LAYOUT_CHANNELS_LAST one tiled transpose (32 x 32 through LDS) per FPN output:
 * NLB_BACKBONE_LAUNCHES in all for channels-last, two fewer for NCHW, where the last InstanceNorm launch of each level writes the output itself.
 * Workspace: nlb_backbone_workspace_bytes(V, H, W, fpn_dim) bytes, 256-byte aligned. */
#define NLB_BACKBONE_MIN_SIDE 16
#define NLB_BACKBONE_MAX_VIEWS 64
#define NLB_BACKBONE_MAX_PIXELS 16777216
#define NLB_BACKBONE_LAUNCHES 35
typedef struct {
  float* layer1;
  float* layer2;
} nlb_backbone_taps;
size_t nlb_backbone_workspace_bytes(int V, int H, int W, int fpn_dim);
int nlb_backbone_forward(const void* packed, const float* imgs, int V, int H, int W, int fpn_dim, int precision, int layout, float* conv1_out, float* p_layer1,
                         float* p_layer2, const nlb_backbone_taps* taps, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#pragma GCC visibility pop
#endif
