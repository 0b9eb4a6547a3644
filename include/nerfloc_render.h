/* nerfloc_render.h — C-ABI of libnerfloc_render.so (MI355X / gfx950 HIP renderer for NeRF-Loc's
 * conditional-NeRF hot path).  Plain pointers and sizes only; no torch / C++ types.
 *
 * What each entry point replaces in the reference (paths relative to /root/reference/nerf_loc/models/):
 *   nl_knn               pytorch3d.ops.knn_points == ops/knn/knn_utils.py:97-174 -> ops/knn/src/knn_api.cpp:10-14
 *                        (`knn_points_idx`), CUDA path ops/knn/src/knn.cu:131-241, CPU path knn_cpu.cpp:13-64;
 *                        call sites conditional_nerf/model.py:289,318,376-383
 *   nl_mv_aggregate      MultiviewFeatureAggregator.forward, conditional_nerf/multiview_aggregator.py:156-222
 *                        (Projector.compute ibrnet/ibrnet.py:194-231, project_points_dict depth_fusion.py:128-147,
 *                         MixtureLogisticsDistDecoder visibility_decoder.py:99-148)
 *   nl_point_mlp         ConditionalNeRF.query neighbour branch, conditional_nerf/model.py:372-427
 *                        (base_mlp :63-71, MultiHeadAttention ibrnet/ibrnet.py:69-119, aggregation :415-427)
 *   nl_ray_unet          RayUnet.forward, conditional_nerf/ray_unet.py:55-69
 *   nl_heads_composite   sigma/rgb-blend/feat heads + alpha compositing + valid mask, conditional_nerf/model.py:525-598
 *   nl_coarse_weights    MultiviewFeatureAggregator.predict_weights_from_neuray, multiview_aggregator.py:95-154
 *   nl_sample_pdf        sample_pdf + sort/merge, conditional_nerf/utils.py:73-112 and model.py:492-495
 *   nl_render_rays       ConditionalNeRF.render_rays, conditional_nerf/model.py:472-600 (eval mode), rows a2-a18 fused
 *   nl_composite_backward  autograd of model.py:544-560,597 (compositing) — first slice of the backward pass
 *   nl_point_mlp_backward  autograd of model.py:372-427 w.r.t. the sample positions / directions / query features (frozen weights)
 *   nl_knn_backward      ops/knn/src/knn.cu:449-490 (KNearestNeighborBackwardKernel), knn_cpu.cpp:68-117
 *   nl_pack_weights      (no reference counterpart: state_dict fp32 tensors -> kernel layouts; names = SURVEY App. C)
 *   nl_frame_*           per-frame caches the reference keeps on the module: `support_neural_points['fine']`
 *                        (model.py:79,180-197) and `multiview_aggregator.vis_featmaps` (multiview_aggregator.py:29,178)
 *
 * Conventions
 *   - every function returns 0 (NL_OK) or a negative nl_status; nl_strerror() names it; nothing throws.
 *   - all tensor pointers are DEVICE pointers to contiguous fp32 unless marked HOST; the library never
 *     allocates device memory: the caller passes workspaces sized by the *_bytes() queries.
 *   - `stream` is a hipStream_t (as void*); kernels are enqueued asynchronously on it, no host sync.
 *   - indices are int32 on the device side (N, M < 2^31); sizes are int64_t in the signatures.
 */
#ifndef NERFLOC_RENDER_H
#define NERFLOC_RENDER_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
/* The library is built with -fvisibility=hidden: only what this header declares is exported. */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

#define NL_ABI_VERSION 13  /* 2: nl_render_rays_ex / nl_render_opts (early termination, per-ray query centres); 3: nl_render_opts.flags,
                            * reserved fields validated, side stream owned by the nl_frame; 5: NL_PREC_F16MX; 6: nl_frame_diagnostics;
                            * 7: NL_RENDER_PRECISION_GUARD (the precision guard at the boundary), NL_DIAG_GUARD_*; 8: nl_s2d_* (the coarse matcher);
                            * 9: nl_fine_* (the fine matcher); 10: nl_sct_* (the matcher's SelfCrossTransformer);
                            * 11: nl_s2d_*_train (the coarse matcher's training step);
                            * 12: nl_fine_*_backward, nl_fine_pack_proj_train (the fine matcher's training step);
                            * 13: nl_sct_*_train, nl_sct_backward, nl_sct_layer_backward (the SelfCrossTransformer's training step); added within 13, with
                            * nothing else changed: nl_sct_*_dropout, nl_sct_dropout_mask (that step with dropout inside the kernels); nl_pnp_* (the absolute
                            * pose from the matches: P3P RANSAC + refinement) */
#define NL_MAX_VIEWS 16
#define NL_KNN_MAX_K 8

typedef enum nl_status {
  NL_OK = 0,
  NL_ERR_BAD_ARG = -1,       /* null pointer / negative size / inconsistent shapes */
  NL_ERR_UNSUPPORTED = -2,   /* shape outside what the kernels are built for (see nl_config) */
  NL_ERR_WORKSPACE = -3,     /* workspace too small; call the matching *_bytes() */
  NL_ERR_HIP = -4,           /* a HIP runtime call failed (hipGetLastError is left set) */
  NL_ERR_NO_DEVICE = -5
} nl_status;

typedef enum nl_precision {
  NL_PREC_F32 = 0,     /* f32-input MFMA (v_mfma_f32_32x32x2_f32): exact fp32 products/accumulation   */
  NL_PREC_BF16X3 = 1,  /* 3-term split-bf16 MFMA (hi*hi + hi*lo + lo*hi), fp32 accumulate: parity mode  */
  NL_PREC_BF16 = 2,    /* single bf16 MFMA, fp32 accumulate: throughput mode (does not meet 1e-4)       */
  NL_PREC_F16MX = 3    /* round 4 / 5 — parity mode, 1.5 (round 4: 2.0) instead of 3 matrix-instruction equivalents per product in the fused neural-point kernel
                        * (the MFMA-bound kernel): fp16 hi.hi (v_mfma_f32_32x32x16_f16) + the two cross terms hi.lo / lo.hi on gfx950's
                        * block-scaled instruction v_mfma_scale_f32_32x32x64_f8f6f4 — since round 5 with FP6 (e2m3) operands, 8 passes per K = 64 where FP8 takes 16
                        * (the cross terms are 2^-11 of a product: three mantissa bits leave 2^-15, whether the element is e4m3 or e2m3; what e2m3 lacks is range,
                        * which the block scales supply).  Round 6: the ray U-Net's conv_out (W = 256, S = 128: the second-largest kernel of nl_render_rays) multiplies
                        * in the same arithmetic, its B operand rebuilt per K = 64 slab in registers with a scale per 32-value block from the values themselves.
                        * Every other GEMM-shaped stage, the stage entry points and the backward passes run exactly as NL_PREC_BF16X3.
                        * RANGE: every MX block — a row's 32 values of one K half-slab — carries its own power-of-two scale 2^(floor(log2 max) - 2), taken from the
                        * values themselves: in the kernel for the activations (per row, slab and layer; the residual image uses the same scale x 2^-11), at
                        * packing time for the weights (per output row and half-slab).  No activation or weight magnitude saturates or flushes a block.  What is
                        * left is fp16's own range for the hi part: |activation| < 65504 (beyond it the value saturates, MODE.FP16_OVFL, instead of becoming inf)
                        * and >= 2^-14 for its full 11 bits.  Validated (tests/test_gpu_parity.py, tools/scale_sweep.py): feature maps x 1/64 ... 64 (activations
                        * to ~2e3), Student-t (nu = 3) weights, DepthFusionNet maps x 8.
                        * ACCURACY: a product carries ~2^-16 (NL_PREC_BF16X3: 2^-17, NL_PREC_F32: 2^-24).  On well-conditioned inputs that is 1-2.5e-5 of the
                        * outputs; where the network amplifies rounding (attention logits of |q.k / sqrt d| >> 10: see nl_frame_diagnostics) every mode's
                        * distance to the reference grows by the same factor and NL_PREC_F32 is the mode that stays at the reference's own level.          */
} nl_precision;

typedef struct nl_config {
  int32_t W;          /* model_3d_hidden_dim: multiple of 32, 32..256                      */
  int32_t C;          /* backbone2d_fpn_dim (feature channels of the support maps), 192    */
  int32_t S;          /* samples per ray seen by ray_unet (N_samples + N_importance), S%8==0, S<=256 */
  int32_t precision;  /* nl_precision for the GEMM-shaped stages                           */
} nl_config;

/* Per-frame inputs (reference `data` dict, nerf_pose_estimator.py:255-290, plus the two module caches). */
typedef struct nl_frame_desc {
  int32_t V, H, Wimg, h, w;      /* support views, full-res image size, feature-map size (H/4 fine, H/8 coarse) */
  int32_t vis_h, vis_w;          /* size of vis_featmaps (always H/4, Wimg/4: depth_fusion.py:239-282)     */
  float near_, far_;             /* data['depth_range'][0]                                             */
  const float* images;           /* (V,3,H,Wimg)   data['topk_images']                                 */
  const float* featmaps;         /* (V,h,w,C)      data['feat_fine_src'] (channels-last, as the reference stores it) */
  const float* vis_featmaps;     /* (V,32,vis_h,vis_w) multiview_aggregator.vis_featmaps                */
  const float* proj_ibr;         /* HOST (V,3,4)   rows 0..2 of  K4 @ inv(c2w)   (ibrnet.py:183)       */
  const float* proj_neuray;      /* HOST (V,3,4)   K @ inv(c2w)[:3]             (depth_fusion.py:90)   */
  const float* cam_centers;      /* HOST (V,3)     c2w[:3,3]                    (ibrnet.py:159)        */
  int64_t M;                     /* support neural points (fine level)                                 */
  const float* sp_xyz;           /* (M,3)   support_neural_points['fine']['xyz']                       */
  const float* sp_feature;       /* (M,C+3) ...['feature']  = [rgb, feat]                              */
  const float* sp_confidence;    /* (M,1)   ...['confidence']                                          */
  const float* sp_direction;     /* (M,4)   ...['direction'] = [unit view dir, depth]                  */
} nl_frame_desc;

typedef struct nl_frame nl_frame;   /* opaque: device tables + KNN grid living in caller-provided memory */

/* Outputs of render_rays (model.py:577-598).  Any pointer may be NULL to skip that output. */
typedef struct nl_render_out {
  float* rgb;                /* (R,3)  */
  float* depth;              /* (R)    */
  float* weights;            /* (R,S)  any alignment is accepted; 16-byte aligned (or null) lets the f16mx path at W = 256 fuse feat_mlp with the
                              *        compositing pass (the library falls back to the staged feature path otherwise: same results to ~1e-6) */
  uint8_t* mask;             /* (R)    0/1 */
  float* depth_uncertainty;  /* (R)    */
  float* feat;               /* (R,C)  */
  /* optional intermediates for testing / staged callers */
  float* sigma;              /* (R*S)   */
  float* feature_agg;        /* (R*S,W) */
  float* mv_feature_agg;     /* (R*S,W) */
  float* geo;                /* (R*S,W) ray_unet output */
  int32_t* knn_idx;          /* (R*S,8) */
  float* knn_d2;             /* (R*S,8) */
} nl_render_out;

/* ---- library ---------------------------------------------------------------------------------- */
int nl_abi_version(void);
const char* nl_strerror(int status);
/* Names of the state_dict tensors nl_pack_weights consumes, in the order it expects them. */
int nl_num_weights(void);
const char* nl_weight_name(int i);

/* Measurement hook (no reference counterpart): between nl_profile_begin and nl_profile_end every launch of the dominant
 * kernel (the fused neural-point kernel, rows a9-a11) made through this library is bracketed by HIP events on its own
 * stream; nl_profile_end synchronises, returns the summed device time in ms and the number of launches, and disarms.
 * bench.py uses it for roofline.dominant_kernel. */
int nl_profile_begin(void);
int nl_profile_end(float* fused_ms, int* launches);

/* Debug facility for tests (not thread-safe, process-global): with a gap set, every buffer the library carves from a caller workspace is followed by
 * `bytes` unused bytes (the *_workspace_bytes queries grow accordingly) and the carve records the regions between the buffers; a caller that filled its
 * workspace with `pattern` before a call learns from nl_debug_check_gaps how many of those regions a kernel wrote into.  0 switches it off. */
int nl_debug_bump_gap(size_t bytes);
int nl_debug_check_gaps(int pattern, int32_t* scratch /* device, 4 bytes */, int* bad_regions /* host */, int* checked_regions /* host, may be NULL */,
                        void* stream);

/* ---- weights ---------------------------------------------------------------------------------- */
size_t nl_packed_weights_bytes(const nl_config* cfg);
/* tensors[i] = DEVICE pointer of state_dict[nl_weight_name(i)] (fp32, contiguous, torch layout). */
int nl_pack_weights(const nl_config* cfg, const float* const* tensors, int n_tensors,
                    void* packed, size_t packed_bytes, void* stream);

/* ---- per-frame setup ---------------------------------------------------------- */
/* Workspace for the two setup calls below (stride = 1 for nl_cross_view_features). */
size_t nl_setup_workspace_bytes(int V, int H, int W, int stride);
/* DepthFusionNet's hand-made input (conditional_nerf/depth_fusion.py:150-227 depth2pts3d + get_diff_feats +
 * extract_depth_for_init, assembled at :269-278): cnn_in (V,12,H,W) = [rgb 3 | normalised inverse depth 1 | masked mean of the
 * cross-view colour difference 3 | its variance 3 | mean and variance of the inverse-depth difference 2].  imgs (V,3,H,W),
 * depths (V,H,W) metric, Ks (V,3,3), c2w (V,4,4), all fp32 device pointers; V <= 16.  Replaces ~60 framework ops over
 * (V, V*H*W, c) intermediates. */
int nl_cross_view_features(const float* imgs, const float* depths, const float* Ks, const float* c2w, int V, int H, int W,
                           float near_, float far_, float* cnn_in, void* workspace, size_t workspace_bytes, void* stream);
/* ConditionalNeRF.backproject_support_frame (conditional_nerf/model.py:203-265; get_rays utils.py:56-70): every pixel with
 * depth > 0 of the nearest-resized (H/stride, W/stride) depth map of every view becomes one row of the support tables, in the
 * reference's order (view, row, column).  feats (V,fh,fw,C) channels-last at the level's resolution.  Tables (capacity rows):
 * feature (.,3+C) = [rgb | feature], xyz (.,3) world, xyz_ref (.,3) in view 0's camera, direction (.,4) = unit viewing ray in
 * the world frame + depth.  *m_out (HOST) receives the number of rows; if it exceeds capacity nothing is written and
 * NL_ERR_WORKSPACE is returned (capacity = V*(H/stride)*(W/stride) always suffices).  Synchronises the stream once (the
 * reference synchronises once per view in nonzero()). */
int nl_backproject_support(const float* imgs, const float* feats, const float* depths, const float* Ks, const float* c2w,
                           int V, int H, int W, int fh, int fw, int C, int stride, int64_t capacity, float* feature, float* xyz,
                           float* xyz_ref, float* direction, int64_t* m_out, void* workspace, size_t workspace_bytes, void* stream);

/* Row a1 — get_rays (conditional_nerf/utils.py:56-70) and points_2d_to_rays (conditional_nerf/model.py:687-700): pixel ->
 * ray origin (camera centre) and unit direction in the world frame.  K (3,3) and c2w (4,4) are DEVICE pointers.  uv == NULL: the
 * whole H x W grid in row-major pixel order (R must be H*W); otherwise uv (R,2) = (x, y) pixel positions, truncated towards zero
 * like the reference's .long() look-up into the ray grid. */
int nl_get_rays(const float* K, const float* c2w, const float* uv, int H, int W, int64_t R, float* rays_o, float* rays_d, void* stream);

/* ---- per-frame state --------------------------------------------------------------------------- */
/* A frame keeps the DEVICE pointers of the descriptor (images, feature maps, support points: they must stay alive and unchanged
 * while the frame is used — call nl_frame_create again when the data changes) plus tables derived from them in frame_mem
 * (visibility maps repacked, KNN grid, and — built lazily on the first render with a given packed-weights blob and rebuilt when
 * that blob is re-packed — the per-point table T and the blend-projected feature maps; plus the scratch the training backward needs
 * per support point: d loss / d T (M, W) and (M, align32(C + 3)) staging rows, used by nl_*_backward_train / nl_render_rays_backward in
 * every mode but fp32).  A frame also owns the side stream (+ two
 * events) on which nl_render_rays runs the exact KNN beside the multi-view gather: created here, destroyed by nl_frame_destroy —
 * render calls never create streams or events (safe inside hipGraph capture from the first call on).  One frame must not be rendered
 * from two host threads / caller streams at the same time (like the reference module, a frame is not re-entrant); different frames are
 * independent. */
size_t nl_frame_bytes(const nl_config* cfg, const nl_frame_desc* desc);
int nl_frame_create(const nl_config* cfg, const nl_frame_desc* desc, void* frame_mem, size_t frame_bytes,
                    void* stream, nl_frame** out);
int nl_frame_destroy(nl_frame* frame);

/* Conditioning indicators of what has been rendered against `frame` so far (round 5), copied to HOST memory; synchronises `stream`.
 *   [NL_DIAG_TABLE_ABSMAX]  max |T| over the per-frame table T = support features x base_mlp.0's feature columns + bias (0 until the first render builds it)
 *   [NL_DIAG_LOGIT_ABSMAX]  largest |attention logit| (q.k / sqrt d_k, ibrnet.py:28-45) the neural-point branch has scored since nl_frame_create (round 6: every kernel
 *                           that scores logits reports it — the fused kernels of W = 128 / 256 and W = 64 and the staged attention kernel; a NaN logit is recorded as +inf).  The softmax over a sample's 8 neighbours turns a logit error e into a weight error ~e, and a split
 *                           product's logit error is its relative precision x |logit|: at |logit| ~ 100 NL_PREC_F16MX (2^-16) sits ~2e-4 from the fp64 result where
 *                           it sits 2e-5 at |logit| ~ 1 — and the reference's own fp32 arithmetic moves from 1e-6 to 1e-5.  The host mirror uses it to fall back to
 *                           a more exact mode (nerf_loc_amd.conditional_nerf: precision_guard).
 *   [NL_DIAG_POINT_KERNEL_GHZ]  the clock the chip ran the last fused neural-point launch at (the roofline's peak assumes 2.4 GHz; under matrix load it is ~1.7)
 *   [NL_DIAG_DENSITY_MAX]  the largest density (sigma) among the samples of the batches rendered with NL_RENDER_PRECISION_GUARD (unguarded calls do not pay for the
 *                           reduction and leave it alone): the guard's second indicator, see NL_GUARD_DENSITY_LIMIT_*
 * n: how many of the NL_DIAG_COUNT values to write. */
#define NL_DIAG_TABLE_ABSMAX 0
#define NL_DIAG_LOGIT_ABSMAX 1
#define NL_DIAG_POINT_KERNEL_GHZ 2   /* shader clock of the last fused neural-point launch (workgroup 0: s_memtime cycles / s_memrealtime): DVFS under matrix load */
#define NL_DIAG_GUARD_PRECISION 3    /* the nl_precision the last NL_RENDER_PRECISION_GUARD call against this frame produced its outputs in (-1: no guarded call yet) */
#define NL_DIAG_GUARD_ESCALATIONS 4  /* how many times a guarded call moved this frame to a more exact mode (0, 1 or 2 over a frame's life) */
#define NL_DIAG_DENSITY_MAX 5        /* largest density (sigma) of the batches rendered with NL_RENDER_PRECISION_GUARD against this frame (0 before the first; a NaN stays a NaN) */
#define NL_DIAG_COUNT 6
int nl_frame_diagnostics(const nl_frame* frame, float* host_out, int32_t n, void* stream);

/* ---- stages (each is also reachable through nl_render_rays) -------------------------------------- */
/* a8: exact K nearest support points (squared L2 in the reference's fp32 order, ascending, ties by index). */
int nl_knn(const nl_frame* frame, const float* xyz, int64_t N, int K, int32_t* idx, float* d2, void* stream);

/* a2-a3: z_vals (R,S) [given, or generated from near/far when z_vals_in==NULL] -> xyz (R*S,3), z_out (R,S). */
int nl_sample_points(const float* rays_o, const float* rays_d, int64_t R, int S, float near_, float far_,
                     const float* z_vals_in, float* z_out, float* xyz, void* stream);

size_t nl_mv_aggregate_workspace_bytes(const nl_config* cfg, int V, int64_t N);
/* a4-a7 (+ a15's per-view part): -> mv_feat (N,W), valid_s (N) = #views(in-bounds & in front) > 1, and optionally
 *   rgb_feat (N*V,196) [cols 0..194 = raw multi-view projection], vis_ang (N*V,8) = [vis, angle(4), pad]   (staged callers), and/or
 *   blend1 (N*V,32) = per-(sample,view) part of rgb_blending_mlp layer 1 (pre-activation, bias included), rgbv (N*V,4) = [r,g,b,vis]
 *   (what nl_heads_composite consumes).  query_center = data['pose'][:3,3] (HOST, 3 floats). */
int nl_mv_aggregate(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center,
                    const float* xyz, int64_t N, float* mv_feat, float* rgb_feat, float* vis_ang, int32_t* valid_s,
                    float* blend1, float* rgbv, void* ws, size_t ws_bytes, void* stream);

size_t nl_point_mlp_workspace_bytes(const nl_config* cfg, int64_t N);
/* a8-a12: xyz (N,3), dir (N,3) viewing direction per sample (NULL: nearest neighbour's, model.py:391-392),
 *         mv_feat (N,W) -> feature_agg (N,W); optional knn outputs. */
int nl_point_mlp(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* xyz, const float* dir,
                 int64_t dir_stride, const float* mv_feat, int64_t N, int K, float* feature_agg, int32_t* knn_idx, float* knn_d2,
                 void* ws, size_t ws_bytes, void* stream);

size_t nl_ray_unet_workspace_bytes(const nl_config* cfg, int64_t R);
/* a13: x (R*S,W) sample-major -> geo (R*S,W). */
int nl_ray_unet(const nl_config* cfg, const void* packed, const float* x, int64_t R, float* geo,
                void* ws, size_t ws_bytes, void* stream);

size_t nl_heads_composite_workspace_bytes(const nl_config* cfg, int V, int64_t R);
/* a14-a18.  blend1 (N*V,32) / rgbv (N*V,4) / valid_s (N) as nl_mv_aggregate writes them (valid_s may be NULL: the mask is then 0);  out: rgb, depth, weights, mask,
 * depth_uncertainty, feat, sigma — each may be NULL.  A configuration that is valid but for S > 256: NL_ERR_UNSUPPORTED (a ray is composited by one wave, four samples per lane). */
int nl_heads_composite(const nl_config* cfg, const void* packed, int V, const float* z_vals, const float* feature_agg,
                       const float* geo, const float* blend1, const float* rgbv, const int32_t* valid_s,
                       int64_t R, int white_bkgd, const nl_render_out* out, void* ws, size_t ws_bytes, void* stream);

/* a20 (hierarchical): coarse NeuRay weights (R,Sc) for z_coarse (R,Sc) along un-normalised K^-1[u,v,1] rays, Sc <= 64.
 * query_w2c_kinv HOST 12+9 floats: inv(pose)[:3] (3x4 row-major) then inv(K) (3x3).  z_coarse holds one row PER RAY (rows may differ), each strictly
 * increasing.  depth_coarse (R) = sum(weights * z_coarse) may be NULL; weights are the same bits either way.  A sample that no view sees takes the ground
 * state alpha = sigmoid(-15).  Contract, checked before the workspace is looked at: 3 <= Sc <= 64 — Sc < 3: NL_ERR_BAD_ARG, Sc > 64: NL_ERR_UNSUPPORTED;
 * R == 0: NL_OK, nothing is read; precision NL_PREC_F32 runs per-lane fp32 decoders, every other one the split-fp16 MFMA decoders. */
size_t nl_coarse_weights_workspace_bytes(int V, int64_t R, int Sc);
int nl_coarse_weights(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_w2c_kinv,
                      const float* pixel_coordinates, const float* z_coarse, int64_t R, int Sc, float* weights,
                      float* depth_coarse, void* ws, size_t ws_bytes, void* stream);
/* inverse-CDF sampling with caller-provided uniforms u (R,Ni) in [0, 1), merged with z_base (R,Sb) and sorted -> z_out (R,Sb+Ni).  The pdf is
 * weights_coarse[:, 1:-1] + 1e-5 over the Sc - 1 mid-points of z_coarse; a bin whose cdf step is below 1e-5 returns its lower mid-point (utils.py:73-112).
 * z_base needs no order; the merge is exact (the output holds the bits of z_base and of the samples, ascending); every pointer must be non-NULL, z_base too
 * when Sb == 0.  Contract, checked before any launch: Sb >= 0, Ni >= 1, Sb + Ni >= 1, Sc >= 3, else NL_ERR_BAD_ARG; Sb + Ni <= 256 and Sc <= 64, else
 * NL_ERR_UNSUPPORTED (one wave sorts a ray's keys in a 256-entry network; one coarse sample per lane).  R == 0: NL_OK, nothing is read. */
int nl_sample_pdf(const float* z_coarse, const float* weights_coarse, int Sc, const float* u, int Ni,
                  const float* z_base, int Sb, int64_t R, float* z_out, void* stream);

/* ---- the fused path ----------------------------------------------------------------------------- */
size_t nl_render_rays_workspace_bytes(const nl_config* cfg, int V, int64_t R);   /* recommended size */
size_t nl_render_rays_min_workspace_bytes(const nl_config* cfg, int V);          /* one-ray-chunk minimum */
/* Options of nl_render_rays_ex.  early_term_eps > 0 enables early-termination compositing (BASELINE.json config 5; the reference
 * has no such switch): along every ray the colour blend (model.py:528-538), feat_mlp (model.py:595) and the compositing reads of
 * the samples behind the point where the transmittance T (model.py:549-552) falls below eps are skipped; their total compositing
 * weight is < eps, so rgb / feat change by < eps * max|value| (weights, depth, depth_uncertainty and mask are computed from all
 * samples and do not change at all).  0 = off = nl_render_rays.  The density itself cannot be skipped: the ray U-Net
 * (ray_unet.py:55-69) runs along the whole ray. */
typedef struct nl_render_opts {
  float early_term_eps;      /* 0 (off) or in (0, 1): e.g. 1e-5 keeps BASELINE's 1e-4 with a wide margin; anything else (NaN too) is NL_ERR_BAD_ARG */
  uint32_t flags;            /* NL_RENDER_* bits below; unknown bits are NL_ERR_BAD_ARG */
  /* Several query frames per launch: device pointer to (R, 3) per-ray query camera centres, or NULL.  When set
   * it replaces `query_center` (which may then be NULL): rays of different query poses against the SAME support frame go down in one
   * call — the query centre is the only per-query-frame quantity the ray path reads (ibrnet.py:144-167, the view-angle features) —
   * which amortises the launch chain for small per-frame batches (PoseOptimizer-sized: 512 rays). */
  const float* ray_centers;
  int32_t reserved[4];       /* must be 0 (checked: NL_ERR_BAD_ARG otherwise) */
} nl_render_opts;
/* nl_render_opts.flags */
#define NL_RENDER_NO_SIDE_STREAM 1u   /* keep every kernel on the caller's stream: no fork of the exact KNN onto the frame's side stream
                                       * (results are bit-identical either way; for profiling one kernel at a time and for callers that
                                       * must not see a second stream) */
#define NL_RENDER_PRECISION_GUARD 2u  /* round 6 (ABI 7) — the precision guard AT the boundary: after the batch the library reads the frame's conditioning indicator
                                       * (NL_DIAG_LOGIT_ABSMAX and NL_DIAG_DENSITY_MAX: one small device-to-host copy; the call SYNCHRONISES `stream`; both are running maxima over the frame's guarded batches) and, while one lies beyond the range the
                                       * mode of the outputs was validated to — NL_GUARD_LOGIT_LIMIT_* / NL_GUARD_DENSITY_LIMIT_* below, DESIGN.md 2.3 — renders THIS batch again in the next more
                                       * exact mode (NL_PREC_F16MX -> NL_PREC_BF16X3 -> NL_PREC_F32; NL_PREC_BF16 is a throughput mode and is left alone).  The frame
                                       * then stays in that mode for every later guarded call (until nl_frame_create), so the second pass is paid once per frame;
                                       * NL_DIAG_GUARD_PRECISION / NL_DIAG_GUARD_ESCALATIONS say what happened.  A NaN logit counts as beyond every range.  Every batch
                                       * of a frame is checked, not only the first (the indicator is cumulative: a later batch with larger logits escalates when it
                                       * arrives).  Not capturable into a HIP graph (the synchronisation); NL_ERR_BAD_ARG in nl_render_rays_multi with more than one job. */
#define NL_RENDER_FLAGS_ALL 3u
#define NL_GUARD_LOGIT_LIMIT_F16MX 50.0f    /* tools/scale_sweep.py (profiles/r5_scale_sweep.txt): f16mx <= 5.1e-5 of the CPU oracle up to |logit| 64, 7.2e-5 at 95, 9.3e-5 at 142 */
#define NL_GUARD_LOGIT_LIMIT_BF16X3 500.0f  /* bf16x3 <= 4.2e-5 up to |logit| 475, 0.3-1.7e-4 at ~1000 */
/* The guard's second indicator, NL_DIAG_DENSITY_MAX (like the logit indicator a running maximum over the guarded batches of the frame): the density head multiplies
 * whatever error `geo` carries (f16mx 1.8-2.6e-5, bf16x3 0.9-1.2e-5 of max |geo|) by its gain, and behind a surface one or two samples carry a ray, so nothing averages
 * that error out.  Scenes with surfaces of tests/test_gpu_surfaces.py, worst output against the CPU oracle: f16mx 2.9-5.2e-5 at densities 17.6-21.9,
 * 2.8-6.0e-5 at 28.6-35.9, 4.9e-5 at 52.0, 1.05e-4 / 1.02e-4 (depth_uncertainty) at 48.9 / 59.8; nothing was measured between 36 and 48.9.  The worst measured error per
 * unit of density is 2.8e-6 (5.2e-5 at 18.8), which reaches 1e-4 at 36: the limit is 32, 1.5 x below the first measured miss.  bf16x3 met the bar on every one of
 * these scenes (<= 7.8e-5, densities up to 61.3) and has no density limit. */
#define NL_GUARD_DENSITY_LIMIT_F16MX 32.0f

/* rays_o, rays_d (R,3); z_vals (R,S) or NULL to generate linspace(near,far,S) (model.py:451-458,483-484). */
int nl_render_rays(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center,
                   const float* rays_o, const float* rays_d, const float* z_vals, int64_t R, int white_bkgd,
                   const nl_render_out* out, void* ws, size_t ws_bytes, void* stream);

/* nl_render_rays with options (opts == NULL: identical to nl_render_rays). */
int nl_render_rays_ex(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center,
                      const float* rays_o, const float* rays_d, const float* z_vals, int64_t R, int white_bkgd,
                      const nl_render_out* out, void* ws, size_t ws_bytes, void* stream, const nl_render_opts* opts);

/* Several FRAMES per call (replaces the reference's per-frame loop nerf_pose_estimator.py:289-290 + model.py:615-639 when a pose is scored
 * against several retrieved support sets, or several query images are rendered at once): job i renders its rays against its own nl_frame — its own support
 * views, tables and workspace — exactly as nl_render_rays_ex(cfg, packed, job.frame, ...) would (bit-identical outputs), but the jobs' launch chains are
 * issued on library-owned streams forked from `stream` and joined back into it, so that PoseOptimizer-sized batches (512 rays: a fifth of the chip) of
 * different frames fill the machine together.  Jobs that share a frame run one after the other on one stream.  The first call ON A DEVICE creates that device's
 * streams (one pool per device, keyed by hipGetDevice(): a process may render on several GPUs; that call is not capturable into a HIP graph, later ones are).  Jobs
 * of different frames run concurrently: their workspaces must not overlap (NL_ERR_BAD_ARG otherwise); jobs of one frame may share one.  A single launch over frames with different tables would need per-ray table pointers in every kernel; it is
 * not what this does. */
typedef struct nl_render_job {
  const nl_frame* frame;
  const float* query_center;   /* HOST (3), or NULL with opts->ray_centers */
  const float* rays_o; const float* rays_d; const float* z_vals;   /* as nl_render_rays */
  int64_t R;
  const nl_render_out* out;
  void* ws; size_t ws_bytes;   /* this job's workspace (jobs run concurrently: no sharing) */
  const nl_render_opts* opts;  /* or NULL */
} nl_render_job;
int nl_render_rays_multi(const nl_config* cfg, const void* packed, const nl_render_job* jobs, int32_t njobs, int32_t white_bkgd, void* stream);

/* ---- backward kernels, first slice ---------------------------------------------------- */
/* Gradient of the alpha compositing of nl_render_rays / nl_heads_composite (conditional_nerf/model.py:544-560, 597; what autograd
 * does for torch.cumprod & co. in the reference) w.r.t. its per-sample inputs.  The forward pass saves nothing: the transmittance is
 * recomputed from z_vals and sigma.  Inputs as in the forward: z_vals (R,S), sigma (R,S), rgb_s (R,S,3) per-sample colours, ft (R,S,C) the
 * per-sample rows that are composited into `feat` (or NULL).  Incoming gradients (each may be NULL = zero): g_rgb (R,3), g_depth (R),
 * g_unc (R) [depth_uncertainty], g_feat (R,C), g_weights (R,S).  Outputs: g_sigma (R,S); g_rgb_s (R,S,3) and g_ft (R,S,C) may be NULL. */
int nl_composite_backward(const float* z_vals, const float* sigma, const float* rgb_s, const float* ft, int64_t R, int S, int C, int white_bkgd,
                          const float* g_rgb, const float* g_depth, const float* g_unc, const float* g_feat, const float* g_weights, float* g_sigma,
                          float* g_rgb_s, float* g_ft, void* stream);
/* Backward of nl_knn's squared distances — replaces KNearestNeighborBackwardKernel, ops/knn/src/knn.cu:449-490 (CPU: knn_cpu.cpp:68-117):
 * g_xyz (N,3) = sum_k 2 g_d2[n,k] (xyz[n] - sp_xyz[idx[n,k]]); g_sp_xyz (M,3) or NULL receives the opposite sign by atomic adds and must be
 * zero-initialised by the caller (like the reference's at::zeros).  Padded neighbour slots (k >= M) are skipped. */
int nl_knn_backward(const float* xyz, const float* sp_xyz, const int32_t* idx, const float* g_d2, int64_t N, int K, int64_t M, float* g_xyz,
                    float* g_sp_xyz, void* stream);
/* Input gradient of nl_point_mlp (rows a8-a12; conditional_nerf/model.py:372-427, ibrnet.py:89-119) with FROZEN weights and a frozen support
 * table — the part of the backward pass PoseOptimizer needs (pose_optimizer.py:131-168 optimises the pose only) and the input-gradient half
 * of a training step: g_feature_agg (N,W) -> g_xyz (N,3) [through the positional encoding of the neighbour offsets], g_dir (N,3) [through
 * ray_diff_fc; NULL when dir is NULL] and g_mv_feat (N,W) [attention query + residual; may be NULL].  Nothing is saved by the forward call:
 * the staged forward is re-run into the workspace (KNN, neighbour encoding, base_mlp, k / v / q projections, attention), then transposed-
 * weight GEMMs and the reductions' derivatives walk back.  Arguments as nl_point_mlp (dir: one row per sample, row stride dir_stride).
 * The neighbour weights' dependence on the distances is exactly zero for this network (the normalised weights multiply K identical rows)
 * and is not propagated.  knn_idx / knn_d2 (N,K): the neighbours nl_point_mlp returned for the same xyz (both or neither; NULL: the search runs again).
 * Samples are processed in chunks that fit the workspace. */
size_t nl_point_mlp_backward_workspace_bytes(const nl_config* cfg, int64_t N);
int nl_point_mlp_backward(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* xyz, const float* dir, int64_t dir_stride,
                          const float* mv_feat, int64_t N, int K, const int32_t* knn_idx, const float* knn_d2, const float* g_feature_agg, float* g_xyz,
                          float* g_dir, float* g_mv_feat, void* ws, size_t ws_bytes, void* stream);

/* ---- training: weight gradients (compute_render_loss, conditional_nerf/model.py:641-685) ----------------------------
 * The *_train variants of the backward entry points do everything their frozen-weight counterparts do and, in the same pass over the
 * recomputed activations, ADD the gradients of the stage's parameters (and of the per-frame tables the stage reads) into caller-owned
 * buffers: the caller zero-fills them once per step, every call — and every workspace chunk inside a call — accumulates.  Weight
 * gradients are reduced in a fixed order (split-K partial tiles, no atomics); the table gradients are scatter-adds (atomics, like
 * index_add / grid_sample's backward in the reference's autograd).  `packed` must hold the CURRENT weights (nl_pack_weights after every
 * optimizer step: ~0.5 ms).  The weight-gradient products read their operands as 16-byte rows: nl_config.C must be a multiple of 4 here
 * (NL_ERR_UNSUPPORTED otherwise; the forward and the frozen-weight gradients take any C <= 192). */
typedef struct nl_train_grads {
  float* const* weights;     /* HOST array of nl_num_weights() DEVICE pointers, tensor i laid out like state_dict[nl_weight_name(i)];
                              * NULL entries (and a NULL array) = that gradient is not wanted */
  float* support_feature;    /* (M, C+3) gradient of the support table's features (knn_gather's backward), or NULL */
  float* feat_maps;          /* (V, h, w, C) gradient of the support feature maps (nl_frame_desc.featmaps, channels-last), or NULL */
  float* vis_featmaps;       /* (V, vh, vw, 32) CHANNELS-LAST gradient of the DepthFusionNet maps (nl_frame_desc.vis_featmaps is (V,32,vh,vw)), or NULL */
  float* blend_feat_maps;    /* (V, h, w, 32) gradient of the blend-projected feature maps P = featmaps . rgb_blending_mlp.0.weight[:, W+3 : W+3+C]^T
                              * (the blend taps P instead of projecting every tap, model.py:532-535 by linearity): the caller continues with
                              * d weight[:, W+3 : W+3+C] += sum P_grad^T featmaps and d featmaps += P_grad . weight[:, W+3 : W+3+C].  Or NULL */
  void* scratch;             /* split-K partial tiles: nl_train_scratch_bytes(cfg) */
  size_t scratch_bytes;
  int32_t reserved[4];       /* must be 0 */
} nl_train_grads;
size_t nl_train_scratch_bytes(const nl_config* cfg);
/* nl_point_mlp_backward + gradients of ray_diff_fc.*, base_mlp.*, base_mlp_attn.{w_qs, w_ks, w_vs, fc, layer_norm}.* and of the support
 * features.  (base_mlp_agg_weight's gradient is identically zero: its softmax runs over K identical rows, model.py:415-427.) */
size_t nl_point_mlp_backward_train_workspace_bytes(const nl_config* cfg, int64_t N);
int nl_point_mlp_backward_train(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* xyz, const float* dir, int64_t dir_stride,
                                const float* mv_feat, int64_t N, int K, const int32_t* knn_idx, const float* knn_d2, const float* g_feature_agg,
                                float* g_xyz, float* g_dir, float* g_mv_feat, const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* nl_mv_aggregate_backward + gradients of multiview_aggregator.out_fc.*, the four dist_decoder MLPs (24 tensors), the support feature maps
 * (grid_sample's backward: scatter-add of the taps) and the DepthFusionNet maps. */
size_t nl_mv_aggregate_backward_train_workspace_bytes(const nl_config* cfg, int V, int64_t N);
int nl_mv_aggregate_backward_train(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* xyz, int64_t N, const float* g_mv_feat,
                                   float* g_xyz, const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream);
/* nl_blend_backward + gradients of rgb_blending_mlp.* (layer 1: every column except the feature columns, see blend_feat_maps), the decoders,
 * the DepthFusionNet maps and the blend-projected feature maps. */
size_t nl_blend_backward_train_workspace_bytes(const nl_config* cfg, int V, int64_t N);
int nl_blend_backward_train(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center, const float* xyz,
                            const float* feature_agg, int64_t N, const float* g_rgb_s, float* g_xyz, float* g_feature_agg, float* g_query_center,
                            const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* The whole ray path backwards in ONE call (ConditionalNeRF.render_rays, model.py:472-600, as PoseOptimizer — pose_optimizer.py:131-168 — and a training
 * step — model.py:641-685 — differentiate it): cotangents of the per-ray outputs -> gradients of the rays (and, with `grads`, of all 84 parameter tensors,
 * the maps and the support features).  Equivalent to chaining the stage entry points above through compositing and the three heads, but every
 * per-frame / per-sample quantity is recomputed ONCE per call: one pass of the visibility decoders forward and one backward for the aggregation's and
 * the blend's uses of them, one geometry kernel for both sets of taps, one neighbour search.  z_vals (R,S): the sample depths the forward call used
 * (the hierarchical branch's resampled depths are constants: model.py:495 detaches them).  The query camera centre comes from the host (3 floats) or —
 * no device-to-host copy of a pose that is being optimised on the device — as per-ray rows in device memory (like nl_render_opts.ray_centers).
 * g_query_center_rows (R,3) or NULL: per-ray partial sums of
 * d/d(query camera centre) — the caller adds them up.  Rays are processed in chunks that fit the workspace. */
typedef struct nl_render_cotangents {
  const float* g_rgb;                 /* (R,3) or NULL (= zero) */
  const float* g_depth;               /* (R) */
  const float* g_depth_uncertainty;   /* (R) */
  const float* g_feat;                /* (R,C) */
  const float* g_weights;             /* (R,S) */
  const int32_t* knn_idx;             /* (R*S,8) and */
  const float* knn_d2;                /* (R*S,8): the neighbours the forward call returned for the same rays (nl_render_out.knn_idx / knn_d2), both or neither;
                                       * NULL: the search runs again */
  const void* reserved[1];            /* must be NULL */
} nl_render_cotangents;
size_t nl_render_rays_backward_workspace_bytes(const nl_config* cfg, int V, int64_t R, int train);
int nl_render_rays_backward(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center /* HOST, 3 floats, or NULL */,
                            const float* ray_centers /* DEVICE (R,3) per-ray query centres, or NULL: one of the two */,
                            const float* rays_o, const float* rays_d, const float* z_vals, int64_t R, int white_bkgd, const nl_render_cotangents* g,
                            float* g_rays_o, float* g_rays_d, float* g_query_center_rows, const nl_train_grads* grads, void* ws, size_t ws_bytes,
                            void* stream);

/* The gradient path's forward and backward as a PAIR sharing one workspace: nl_render_rays_forward_keep runs the STAGED forward (the arithmetic of the
 * backward pass's recompute: exact fp32 / split-FP16), writes the per-ray outputs and leaves every intermediate in `ws`; nl_render_rays_backward_kept walks
 * back from them — no recompute, no second neighbour search.  The caller keeps `ws` untouched in between and passes the same rays / query centre / `train`
 * flag to both.  The whole batch is one chunk: NL_ERR_WORKSPACE when it does not fit (then: nl_render_rays + nl_render_rays_backward, which chunk).
 * `out`: rgb, depth, weights, mask, depth_uncertainty required, feat optional (without it feat_mlp is not evaluated and g_feat must be NULL), the
 * optional intermediates are ignored.
 * beta (may be NULL): the training-mode uncertainty head (model.py:98,111,587-592; `render.use_render_uncertainty`, the reference configs' default):
 * beta[r] = sum_s w_s softplus(beta_mlp.0(geo_s)) + beta_min.  beta_mlp is not one of the nl_pack_weights tensors (eval-mode rendering never evaluates it):
 * its two tensors, the output, its cotangent and its gradients travel in this block; the same block goes to both calls of the pair. */
typedef struct nl_beta_head {
  const float* weight;   /* beta_mlp.0.weight (W) */
  const float* bias;     /* beta_mlp.0.bias (1) */
  float beta_min;        /* 0.1 (model.py:98) */
  float* beta;           /* forward call: (R) output */
  const float* g_beta;   /* backward call: (R) cotangent, or NULL */
  float* g_weight;       /* backward call: (W) +=, or NULL */
  float* g_bias;         /* backward call: (1) +=, or NULL */
} nl_beta_head;
size_t nl_render_rays_keep_workspace_bytes(const nl_config* cfg, int V, int64_t R, int train);
int nl_render_rays_forward_keep(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center /* HOST or NULL */,
                                const float* ray_centers /* DEVICE (R,3) or NULL */, const float* rays_o, const float* rays_d, const float* z_vals, int64_t R,
                                int white_bkgd, const nl_render_out* out, const nl_beta_head* beta, int train, void* ws, size_t ws_bytes, void* stream);
int nl_render_rays_backward_kept(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center /* HOST or NULL */,
                                 const float* ray_centers /* DEVICE (R,3) or NULL */, const float* rays_d, int64_t R, int white_bkgd,
                                 const nl_render_cotangents* g, const nl_beta_head* beta, float* g_rays_o, float* g_rays_d, float* g_query_center_rows,
                                 const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* nl_ray_unet_backward + gradients of the seven blocks' convolution weights / biases and LayerNorm([C, L]) tables (28 tensors). */
size_t nl_ray_unet_backward_train_workspace_bytes(const nl_config* cfg, int64_t R);
int nl_ray_unet_backward_train(const nl_config* cfg, const void* packed, const float* x, int64_t R, const float* g_geo, float* g_x,
                               const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream);

/* Input gradient of nl_mv_aggregate's feature rows (rows a4-a7; multiview_aggregator.py:156-222, ibrnet.py:169-231, visibility_decoder.py:64-148)
 * with frozen weights and frozen support maps: g_mv_feat (N,W) -> g_xyz (N,3).  The forward is recomputed in exact fp32; the way back goes through
 * out_fc (transposed-weight products, ELU), the visibility-weighted statistics, the bilinear taps' spatial derivative (zeros padding,
 * align_corners = True), the projection, and — for the visibility weights and the depth difference — the NeuRay decoders, the border-mode tap of
 * the visibility map and the NeuRay projection. */
size_t nl_mv_aggregate_backward_workspace_bytes(const nl_config* cfg, int V, int64_t N);
int nl_mv_aggregate_backward(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* xyz, int64_t N, const float* g_mv_feat,
                             float* g_xyz, void* ws, size_t ws_bytes, void* stream);
/* Input gradient of nl_ray_unet (row a13; ray_unet.py:55-69) with frozen weights: g_geo (R*S,W) -> g_x (R*S,W).  The unfused forward is re-run in exact
 * fp32 (every layer's pre-LayerNorm output stays in the workspace); then, layer by layer, the LayerNorm([C,L]) / ELU / MaxPool1d derivative and the
 * transposed-weight convolution, with the skip connections' gradients added where the concatenations were. */
size_t nl_ray_unet_backward_workspace_bytes(const nl_config* cfg, int64_t R);
int nl_ray_unet_backward(const nl_config* cfg, const void* packed, const float* x, int64_t R, const float* g_geo, float* g_x, void* ws, size_t ws_bytes,
                         void* stream);
/* a15 as a stage (model.py:528-538): per-sample colours rgb_s (N,3) = softmax-over-views blend of the tapped colours, from the sample positions and
 * feature_agg (N,W) (query_center HOST, 3 floats) — what nl_render_rays computes between the neural-point branch and the compositing — and its
 * input gradient: g_rgb_s (N,3) -> g_xyz (N,3), g_feature_agg (N,W) or NULL, g_query_center (N,3: per-sample contributions, the caller sums
 * them) or NULL.  One workspace size serves both. */
size_t nl_blend_workspace_bytes(const nl_config* cfg, int V, int64_t N);
int nl_blend(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center, const float* xyz, const float* feature_agg, int64_t N,
             float* rgb_s, void* ws, size_t ws_bytes, void* stream);
int nl_blend_backward(const nl_config* cfg, const void* packed, const nl_frame* frame, const float* query_center, const float* xyz, const float* feature_agg,
                      int64_t N, const float* g_rgb_s, float* g_xyz, float* g_feature_agg, float* g_query_center, void* ws, size_t ws_bytes, void* stream);

/* ---- localisation head: the sparse-to-dense coarse matcher ----------------------------------------------------------------------------
 * S2DMatching.forward in eval mode, models/matching/sparse_to_dense.py:80-151 (used by matcher.py:22,72): for N sparse 3-D descriptors desc0 (N,C) and M dense
 * 2-D descriptors desc1 (M,C), score[n,m] = sigmoid(mlps(desc0[n] * desc1[m])) with mlps = C -> 128 -> ReLU -> 128 -> ReLU -> 1, then the mutual-nearest
 * selection `mask = (s > thr) & (s == rowmax) & (s == colmax)` applied to the fp32 scores the kernel itself produced, ties included: match_j[n] is the FIRST
 * column of row n's mask (-1: none), match_score[n] that score (0: none).  The N x M x C product and the hidden activations are never written.
 * C: a multiple of 32, 32..256 (NL_ERR_UNSUPPORTED otherwise); N, M >= 1.  precision: NL_PREC_F32, NL_PREC_BF16X3 (parity modes), NL_PREC_BF16 (throughput);
 * NL_PREC_F16MX is NL_ERR_UNSUPPORTED here.  desc0, desc1 and packed must be 16-byte aligned.
 * The packed image holds mlps.0.weight (128,C), mlps.0.bias, mlps.2.weight (128,128), mlps.2.bias, mlps.4.weight (1,128), mlps.4.bias (DEVICE pointers, fp32,
 * torch layout) in the kernels' fragment order for every precision.
 * scores_out (N,M) may be NULL: the scores then live in the workspace (nl_s2d_min_workspace_bytes(.., want_scores = 0) grows by N*M*4). */
size_t nl_s2d_packed_weights_bytes(int C);
int nl_s2d_pack_weights(int C, const float* w1, const float* b1, const float* w2, const float* b2, const float* w3, const float* b3, void* packed,
                        size_t packed_bytes, void* stream);
size_t nl_s2d_min_workspace_bytes(int64_t N, int64_t M, int C, int want_scores);
int nl_s2d_match(const void* packed, int C, int precision, const float* desc0, int64_t N, const float* desc1, int64_t M, float thr, float* scores_out,
                 int32_t* match_j, float* match_score, void* workspace, size_t workspace_bytes, void* stream);

/* The coarse matcher's training step (S2DMatching.forward in train mode and its autograd backward, sparse_to_dense.py:14-78, 112-151).
 * nl_s2d_forward_train is nl_s2d_match (the same kernels, scores and selection) that also keeps the fp32 logits (N,M) and, with target (N,M) != NULL, writes the
 * reference's sigmoid focal loss (alpha 0.25, gamma 2, unit anchor weights, mean over N*M, float targets) to the DEVICE scalar loss_out, summed in a fixed order.
 * target and loss_out are given together or both NULL (no loss); scores_out and logits_out are required.
 * nl_s2d_backward_train: from the descriptors, the saved logits, the target, the loss's cotangent g_loss (a pointer to a DEVICE scalar: no host read) and an
 * optional cotangent g_score (N,M) of the scores (NULL: zero) it writes (overwrites) g_desc0 (N,C), g_desc1 (M,C) and the parameter gradients g_w1 (128,C),
 * g_b1 (128), g_w2 (128,128), g_b2 (128), g_w3 (1,128), g_b3 (1).  Each parameter-gradient pointer may be NULL (frozen weights: with all six NULL only the
 * descriptor gradients are computed, with the same bits).  target and g_loss are given together or both NULL (only g_score flows).
 * The hidden activations are recomputed from the descriptors in row chunks; the workspace holds one chunk and does not grow with N.  Sums run in a fixed
 * order and no float atomic touches a result: a call is bit-reproducible.  Gradient products are split-bf16 MFMA: three terms under NL_PREC_F32 and
 * NL_PREC_BF16X3 (parity), one under NL_PREC_BF16 (throughput); NL_PREC_F16MX is NL_ERR_UNSUPPORTED.
 * The backward pass reads the inference image (nl_s2d_pack_weights) and a second, training image with the transposed weights (nl_s2d_pack_train_weights from
 * mlps.0.weight and mlps.2.weight, DEVICE pointers).  C, alignment and error conventions as for nl_s2d_match; N * M < 2^31 and M <= 2^20
 * (NL_ERR_UNSUPPORTED / a size query of 0 otherwise).  Arguments are validated before anything is dereferenced. */
size_t nl_s2d_forward_train_workspace_bytes(int64_t N, int64_t M, int C);
int nl_s2d_forward_train(const void* packed, int C, int precision, const float* desc0, int64_t N, const float* desc1, int64_t M, float thr, const float* target,
                         float* scores_out, float* logits_out, float* loss_out, int32_t* match_j, float* match_score, void* workspace, size_t workspace_bytes,
                         void* stream);
size_t nl_s2d_train_weights_bytes(int C);
int nl_s2d_pack_train_weights(int C, const float* w1, const float* w2, void* packed, size_t packed_bytes, void* stream);
size_t nl_s2d_backward_train_workspace_bytes(int64_t N, int64_t M, int C);
int nl_s2d_backward_train(const void* packed, const void* train_packed, int C, int precision, const float* desc0, int64_t N, const float* desc1, int64_t M,
                          const float* logits, const float* target, const float* g_loss, const float* g_score, float* g_desc0, float* g_desc1, float* g_w1,
                          float* g_b1, float* g_w2, float* g_b2, float* g_w3, float* g_b3, void* workspace, size_t workspace_bytes, void* stream);

/* ---- localisation head: the fine matcher ------------------------------------------------------------------------------------------------
 * The two stages behind the coarse matches (matcher.py:101-124), models/matching/fine_matching.py.  No workspace: both calls are one launch that writes its
 * outputs only.  Cf, Cout, C: multiples of 32, 32..256.  precision as for nl_s2d_match (NL_PREC_F16MX: NL_ERR_UNSUPPORTED).  Null pointers, M < 0, unsupported
 * widths and stride < 1 are NL_ERR_BAD_ARG before anything is dereferenced; M == 0 is NL_OK with nothing launched.  packed images and the feature tensors must be
 * 16-byte aligned.
 *
 * nl_fine_windows: FinePreprocess.forward with fine_concat_coarse_feat = False (fine_matching.py:35-76): out (M,49,Cout) = proj(window), where window m is the 7 x 7
 * window l = j_ids[m] of image b_ids[m] as F.unfold(kernel 7, stride, padding 3) + 'n (c ww) l -> n l ww c' define it: Ly = (Hf-1)/stride + 1, Lx = (Wf-1)/stride + 1,
 * (ly, lx) = (l / Lx, l % Lx), cell ww = wy*7 + wx reads pixel (ly*stride + wy - 3, lx*stride + wx - 3); a pixel outside the map is a row of zeros (the output is
 * the bias).  feat_nhwc is the fine map as (B,Hf,Wf,Cf); b_ids, j_ids are int64 DEVICE arrays whose range the CALLER has checked (b in [0,B), l in [0,Ly*Lx)).
 * The packed image holds proj.weight (Cout,Cf) and proj.bias (DEVICE pointers, fp32, torch layout) for every precision.  The unfolded map is never formed.
 *
 * nl_fine_match: FineMatching.forward in eval mode (fine_matching.py:94-143, get_fine_match :145-153): for every match m the 49 logits mlps(feat_f0[m] * feat_f1[m,r])
 * (mlps = C -> 128 -> ReLU -> 128 -> ReLU -> 1, packed by nl_s2d_pack_weights: the coarse matcher's image format), heatmap = softmax(logits / sqrt(C)),
 * coords = its expectation over linspace(-1,1,7)^2 (x along the fast axis), std = sum over x, y of sqrt(max(sum(g^2 h) - coords^2, 1e-10)).
 * expec_f (M,3) = (x, y, std); mkps2d_f (M,2) = mkps2d_c + 3 * coords; heatmap (M,49) may be NULL.  Products, hidden activations and logits are never written.
 * NL_PREC_BF16X3 here is three-term split-FP16 (hi = f16(v), lo = f16(v - hi); 2^-22 per product, still three matrix instructions; the image carries fp16 planes
 * for it): the softmax multiplies a logit's error by the logit's size, and split-bf16's 2^-17 misses 1e-4 on nearly one-hot heat-maps.  RANGE of that mode: products
 * feat_f0 * feat_f1 and hidden activations saturate at 65504 (MODE.FP16_OVFL) instead of overflowing; NL_PREC_F32 and NL_PREC_BF16 have no such limit. */
size_t nl_fine_proj_packed_bytes(int Cf, int Cout);
int nl_fine_pack_proj(int Cf, int Cout, const float* w, const float* b, void* packed, size_t packed_bytes, void* stream);
int nl_fine_windows(const void* packed, int Cf, int Cout, int precision, const float* feat_nhwc, int B, int Hf, int Wf, const int64_t* b_ids, const int64_t* j_ids,
                    int64_t M, int stride, float* out, void* stream);
int nl_fine_match(const void* packed_mlp, int C, int precision, const float* feat_f0, const float* feat_f1, int64_t M, const float* mkps2d_c, float* expec_f,
                  float* mkps2d_f, float* heatmap, void* stream);

/* The fine matcher's training step (ABI 12).  The training forward is nl_fine_windows, and nl_fine_match with the heat-map requested; nothing else is kept.
 * Widths, alignment, precision and the order of the argument checks as for the forward calls; M <= NL_FINE_BACKWARD_MAX_M (NL_ERR_UNSUPPORTED / a size query
 * of 0 above): nl_fine_windows_backward places each match at its rank among the earlier matches of its window, one thread per match over all earlier ones,
 * which is quadratic in M (nothing at a frame's few thousand matches, 2 * 10^9 key reads at the limit), and both workspaces grow linearly with M.
 * A training forward should compute the window rows with NL_PREC_F32 also when the rest runs in NL_PREC_BF16X3 (as the FinePreprocess drop-in does): every
 * gradient is taken at those rows, and split-bf16's 2^-17 there shows as up to 2e-3 in the gradients (softmax gain, ReLU units near their kink).
 * Gradient products are split-bf16 MFMA: three terms under NL_PREC_F32 and NL_PREC_BF16X3, one under NL_PREC_BF16.  The hidden activations are recomputed — exact
 * fp32 in the two parity modes, with the ReLU masks of pre-activations near zero decided in fp64 as in nl_s2d_backward_train.  Every sum runs in an order that
 * depends on the shapes and the ids alone and no float atomic touches a result: two calls give the same bits.  All outputs are overwritten.
 *
 * nl_fine_match_backward: from feat_f0 (M,C), feat_f1 (M,49,C), the heatmap (M,49) nl_fine_match wrote and the cotangent g_expec (M,3) of expec_f it writes
 * g_feat_f0 (M,C), g_feat_f1 (M,49,C) and the six parameter gradients (shapes as nl_s2d_backward_train).  Each of the eight output pointers may be NULL; a NULL
 * parameter pointer (frozen weights) skips that weight-gradient work and leaves the other results' bits unchanged.  With t[r] = g_x gx[r] + g_y gy[r] +
 * g_std dstd/dh[r], dstd/dh[r] = sum over the axes with var >= 1e-10 (the clamp passes its gradient at equality, as torch's) of (g[r]^2 - 2 coord g[r]) /
 * (2 sqrt(var)), the logit's gradient is h[r] (t[r] - sum h t) / sqrt(C); a zero g_std contributes exactly nothing whatever the variance, and a match whose
 * g_expec row is zero yields exact zeros.  g_b3 is written as an exact zero: a softmax ignores a common shift of its logits, so expec_f does not depend on
 * mlps.4.bias (autograd leaves rounding noise around zero there).  packed_mlp: nl_s2d_pack_weights; train_packed: nl_s2d_pack_train_weights.  M == 0: NL_OK, nothing launched.
 * Workspace (the size query; 0 for an unsupported C or M): the operands of the weight gradients, M*49 rows of C + 3*128 floats, M*132 floats of gW3 / gb3
 * partial rows, 256 * 128 * (max(C,128) + 1) floats of split-K partial tiles and 128*256 floats — about M * 49 * (C + 384) * 4 bytes.
 *
 * nl_fine_windows_backward: from the cotangent g_out (M,49,Cout) of nl_fine_windows' output it writes g_w (Cout,Cf), g_b (Cout) and g_feat_nhwc (B,Hf,Wf,Cf);
 * each may be NULL.  g_b sums all M*49 rows (a padded cell's output is the bias), g_w sees zeros for padded cells; a pixel's gradient is the sum of
 * g_out[m,ww] . W over the matches whose window covers it, in ascending m (repeated j_ids, overlapping windows and B > 1 follow from that), and a pixel no window
 * covers is written as zero.  packed: nl_fine_pack_proj; train_packed: nl_fine_pack_proj_train (proj.weight^T in the same fragment format,
 * nl_fine_proj_train_bytes bytes, from the DEVICE pointer w).  M == 0: NL_OK, zeros are written to the pointers given.  ids as for nl_fine_windows.
 * Workspace: two (M*49,Cf) fp32 matrices (the gathered windows, the window-gradient rows), 256 * (Cout*Cf + Cout) floats of split-K partial tiles, Cout*Cf floats,
 * and (2 M + B*Ly*Lx + 1) int32 of window lists — about M * 49 * Cf * 8 bytes. */
#define NL_FINE_BACKWARD_MAX_M 65536
size_t nl_fine_proj_train_bytes(int Cf, int Cout);
int nl_fine_pack_proj_train(int Cf, int Cout, const float* w, void* packed, size_t packed_bytes, void* stream);
size_t nl_fine_match_backward_workspace_bytes(int64_t M, int C);
int nl_fine_match_backward(const void* packed_mlp, const void* train_packed, int C, int precision, const float* feat_f0, const float* feat_f1, int64_t M,
                           const float* heatmap, const float* g_expec, float* g_feat_f0, float* g_feat_f1, float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                           float* g_w3, float* g_b3, void* workspace, size_t workspace_bytes, void* stream);
size_t nl_fine_windows_backward_workspace_bytes(int Cf, int Cout, int B, int Hf, int Wf, int stride, int64_t M);
int nl_fine_windows_backward(const void* packed, const void* train_packed, int Cf, int Cout, int precision, const float* feat_nhwc, int B, int Hf, int Wf,
                             const int64_t* b_ids, const int64_t* j_ids, int64_t M, int stride, const float* g_out, float* g_w, float* g_b, float* g_feat_nhwc,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- localisation head: SelfCrossTransformer ------------------------------------------------------------------------------------------
 * models/COTR/transformer.py:17-64 in eval mode (matcher.py:68-72, :120-124): four post-norm layers on v0 (B,N0,C) and v1 (B,N1,C), batch first, fp32 —
 * layer 0: self-attention of v0 (q = k = x + pos, value = x), layer 1: the same for v1, layer 2: v0 attends to layer 1's output (q = x + pos0, k = mem + pos1,
 * value = mem), layer 3: v1 attends to layer 2's OUTPUT.  Each layer: in_proj, 8-head softmax attention (scores * (C/8)^-0.5), out_proj, + residual, LayerNorm
 * (eps 1e-5), linear2(relu(linear1)), + residual, LayerNorm.  The attention is flash-style: no Nq x Nk value is written to memory in any mode, and the F-wide hidden
 * rows stay on chip.  Every Nq, Nk >= 1.
 * Supported: nhead == 8, C in {64, 128, 192, 256}, F a multiple of 32 in 32..512 (nl_sct_packed_bytes returns 0 otherwise, the calls NL_ERR_UNSUPPORTED);
 * B * max(N0, N1) <= 2^24.  precision: NL_PREC_F32 (exact fp32 products), NL_PREC_BF16X3 (three-term split-FP16 as nl_fine_match, operands saturate at 65504),
 * NL_PREC_BF16 (throughput, no bar); NL_PREC_F16MX is NL_ERR_UNSUPPORTED.
 * nl_sct_pack_weights: `tensors` is a HOST array of the module's 52 state-dict tensors in state-dict order (DEVICE pointers, fp32, torch layout: two encoder
 * layers of 12, two decoder layers of 14 — the decoder layers' norm1 pair is taken and ignored, as the reference never applies it); one image for all modes.
 * Nothing is allocated; work is enqueued on `stream`.  Negative or zero extents, null or not 16-byte aligned pointers are NL_ERR_BAD_ARG, a missing, short or not
 * 256-byte aligned workspace NL_ERR_WORKSPACE, all before anything is dereferenced; B == 0 is NL_OK with nothing launched.
 * nl_sct_layer: one layer (0..3 in forward order) of the image, so that a deviation can be attributed: out (B,Nq,C) from x, x_pos (B,Nq,C) and, for layers 2 / 3,
 * mem, mem_pos (B,Nk,C); for layers 0 / 1 mem and mem_pos are NULL or x and x_pos, and Nk == Nq.  out may be x.
 * nl_sct_forward: the four layers; out0 (B,N0,C), out1 (B,N1,C) are distinct buffers that alias neither input of the other side (out0 may be v0, out1 may be v1). */
size_t nl_sct_packed_bytes(int C, int nhead, int F);
int nl_sct_pack_weights(int C, int nhead, int F, const float* const* tensors, int n_tensors, void* packed, size_t packed_bytes, void* stream);
size_t nl_sct_workspace_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F);
int nl_sct_layer(const void* packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos, int64_t Nq, const float* mem,
                 const float* mem_pos, int64_t Nk, int64_t B, float* out, void* ws, size_t ws_bytes, void* stream);
int nl_sct_forward(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1, const float* pos1,
                   int64_t N1, int64_t B, float* out0, float* out1, void* ws, size_t ws_bytes, void* stream);

/* ---- SelfCrossTransformer: training step (ABI 13) ---------------------------------------------------------------------------------------
 * The forward and backward of the four layers above with NO dropout in effect (dropout == 0, or the module in eval mode); with dropout: the next section.
 * No Nq x Nk value reaches memory in either direction: the backward rebuilds the probabilities tile by tile from the kept row maximum and sum (the two parts of the
 * log-sum-exp), in two passes (dQ: a wave per 32 queries over the key tiles; dK / dV: a wave per 32 keys over the query tiles), no float atomics: two calls on the
 * same inputs give the same bits.  Shapes, precisions, alignment and the order of the checks are nl_sct_forward's; every size query returns 0 for a shape or
 * configuration the calls refuse.
 * nl_sct_pack_weights_train: the second image (nl_sct_train_packed_bytes) — the transposes of the three in_proj blocks, out_proj, linear1 and linear2 of every layer
 * in the fragment planes of the inference image; `tensors` as for nl_sct_pack_weights.
 * nl_sct_forward_train: nl_sct_forward's arguments plus a caller-owned, 256-byte aligned state buffer of nl_sct_train_state_bytes(B, N0, N1, C, F) bytes (a missing or
 * short one: NL_ERR_WORKSPACE; `ws` is checked as nl_sct_forward checks it and not written: q, k, v and the attention output go to the state).  out0 / out1 are
 * bit-identical to nl_sct_forward's in the same mode.  Kept per layer: q, k, v, the attention output before out_proj,
 * (maximum, sum) per (row, head), the rows after the first LayerNorm, both LayerNorms' normalised rows and 1 / std, and the outputs of layers 0..2 — 8 (rows_q x C) +
 * 2 (rows_k x C) + 18 rows_q floats per layer; nothing of size F or Nq x Nk.
 * nl_sct_backward: from both images, the four inputs, the state and the cotangents g_out0 (B,N0,C), g_out1 (B,N1,C) — either may be NULL and then means zero — it
 * writes g_v0, g_pos0 (B,N0,C), g_v1, g_pos1 (B,N1,C) and the parameter gradients grads[0..51]: a HOST array of DEVICE pointers in state-dict order (shapes of the
 * parameters), n_grads == 52, or grads == NULL.  Every output pointer may be NULL (a frozen parameter, an input that needs no gradient); the entries of the cross
 * layers' norm1 pair (indices 32, 33, 46, 47) are ignored and never written: the reference never applies that norm and leaves its .grad None.  A NULL costs no launch
 * that only it needs and leaves the other outputs' bits unchanged.  All given outputs are overwritten.  With one key (a layer whose Nk == 1) the softmax is constant
 * and dS is an exact zero, as autograd's.  Workspace: nl_sct_backward_workspace_bytes — about 10 (B max(N0,N1) x C) floats, two (min(rows, 32768) x F) staging
 * buffers for the linear1 / linear2 weight gradients and the split-K partial tiles of wgrad.  State + workspace at (B 1, N0 1024, N1 4800, C 192, F 512) is
 * about 0.13 GB, against the 1.08 GB of softmax outputs that an eager autograd which materialises them keeps, and grows linearly with the sequences.
 * nl_sct_layer_backward: one layer (0..3), mirroring nl_sct_layer: it runs that layer's training forward on (x, x_pos, mem, mem_pos) inside its workspace
 * (nl_sct_layer_backward_workspace_bytes(B, Nq, Nk, C, F): the backward's plus that layer's state) and then its backward from g_out (B,Nq,C): g_x, g_x_pos (B,Nq,C), g_mem, g_mem_pos (B,Nk,C) and the layer's 12
 * (self) or 14 (cross) parameter gradients in state-dict order.  For layers 0 / 1 mem / mem_pos are NULL or x / x_pos, g_mem / g_mem_pos must be NULL and the
 * memory side's gradient is part of g_x / g_x_pos. */
size_t nl_sct_train_packed_bytes(int C, int nhead, int F);
int nl_sct_pack_weights_train(int C, int nhead, int F, const float* const* tensors, int n_tensors, void* packed, size_t packed_bytes, void* stream);
size_t nl_sct_train_state_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F);
int nl_sct_forward_train(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1,
                         const float* pos1, int64_t N1, int64_t B, float* out0, float* out1, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                         void* stream);
size_t nl_sct_backward_workspace_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F);
int nl_sct_backward(const void* packed, const void* train_packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0,
                    const float* v1, const float* pos1, int64_t N1, int64_t B, const void* state, size_t state_bytes, const float* g_out0, const float* g_out1,
                    float* g_v0, float* g_pos0, float* g_v1, float* g_pos1, float* const* grads, int n_grads, void* ws, size_t ws_bytes, void* stream);
size_t nl_sct_layer_backward_workspace_bytes(int64_t B, int64_t Nq, int64_t Nk, int C, int F);
int nl_sct_layer_backward(const void* packed, const void* train_packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos,
                          int64_t Nq, const float* mem, const float* mem_pos, int64_t Nk, int64_t B, const float* g_out, float* g_x, float* g_x_pos, float* g_mem,
                          float* g_mem_pos, float* const* grads, int n_grads, void* ws, size_t ws_bytes, void* stream);

/* ---- SelfCrossTransformer: training step with dropout (an addition within ABI 13: new entry points only, nothing above changes) ---------------
 * The reference's four dropout sites per layer, inside the kernels: site 0 the attention probabilities after the softmax (B*8, Nq, Nk), site 1 out_proj's output
 * before the first residual, site 2 the ReLU'd hidden rows before linear2, site 3 linear2's output before the second residual.  No mask is stored: it is a pure
 * function of (seed, p, layer 0..3, site 0..3, element), recomputed in the backward; state and workspace sizes are those of the calls above, the flash-style
 * backward keeps no Nq x Nk tensor, and two calls with one seed give the same bits.
 * The mask: Philox4x32-10 (published constants), key = (seed low word, seed high word), counter = (major >> 2, minor >> 1, group, 4 layer + site); element
 * (major, minor) is bits [16 (minor & 1), +16) of output word major & 3.  Site 0: major = key, minor = query, group = 8 batch item + head; sites 1..3: major = row
 * flattened over the batch (b * Nq + q), minor = column, group = 0.  An element is kept when its 16-bit field >= thr = round-half-even(65536 p), capped at 65535:
 * the keep probability is exactly 1 - thr / 65536 (within 2^-17 of 1 - p) and kept values are scaled by 65536 / (65536 - thr), its inverse, so the expectation is
 * exact; a p below 2^-17 drops nothing.  tests/sct_dropout_ref.py restates it in numpy.
 * `p` is a float with 0 <= p < 1; anything else (NaN included) is NL_ERR_BAD_ARG, checked after the checks of the call it extends, in their order.  With p == 0 (a
 * zero threshold) these calls run the kernels of nl_sct_forward_train / nl_sct_backward / nl_sct_layer_backward and give their bits.  The backward must be given the
 * forward's (p, seed).  The state's attention output is the DROPPED one.  `seed` is a host value read when the call is made: a call captured in a HIP graph
 * replays that one seed (and so one mask) on every replay.
 * nl_sct_dropout_mask: the keep mask (1 = kept, 0 = dropped, one byte per element, DEVICE memory) of one site by the kernels' own device function — site 0:
 * out (B*8, Nq, n) with n = Nk; sites 1..3: out (B*Nq, n) with n = the row width (C, or F for site 2).  B == 0 is NL_OK. */
int nl_sct_forward_train_dropout(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1,
                                 const float* pos1, int64_t N1, int64_t B, float* out0, float* out1, void* state, size_t state_bytes, void* ws, size_t ws_bytes,
                                 float p, uint64_t seed, void* stream);
int nl_sct_backward_dropout(const void* packed, const void* train_packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0,
                            const float* v1, const float* pos1, int64_t N1, int64_t B, const void* state, size_t state_bytes, const float* g_out0,
                            const float* g_out1, float* g_v0, float* g_pos0, float* g_v1, float* g_pos1, float* const* grads, int n_grads, void* ws, size_t ws_bytes,
                            float p, uint64_t seed, void* stream);
int nl_sct_layer_backward_dropout(const void* packed, const void* train_packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos,
                                  int64_t Nq, const float* mem, const float* mem_pos, int64_t Nk, int64_t B, const float* g_out, float* g_x, float* g_x_pos,
                                  float* g_mem, float* g_mem_pos, float* const* grads, int n_grads, void* ws, size_t ws_bytes, float p, uint64_t seed, void* stream);
int nl_sct_dropout_mask(uint64_t seed, float p, int layer, int site, int64_t B, int64_t Nq, int64_t n, uint8_t* out, void* stream);

/* ---- Absolute camera pose from 2D-3D matches: P3P RANSAC + refinement (an addition within ABI 13: new entry points only, nothing above changes) ----------
 * Replaces the external CPU solver the reference hands `mkps2d` / `mkps3d` to (pycolmap.absolute_pose_estimation, nerf_pose_estimator.py:528-540, 557-583) by
 * calls on the stream the matches were produced on: no copy to the host, no synchronisation, no allocation, and two calls give the same bits.
 * A PROBLEM is M matches — pixels pts2d (M, 2) and world points pts3d (M, 3), fp32, DEVICE — with pinhole intrinsics (fx, fy, cx, cy), a threshold thr in pixels,
 * H hypotheses and a 64-bit seed.  A CALL holds B problems with their matches concatenated; `offsets` (B + 1 int32, offsets[0] = 0, non-decreasing), `intrinsics`
 * (B x 4 doubles) and `thr` (B doubles) are HOST arrays, read when the call is made (a call captured in a HIP graph replays those values; the captured graph is a
 * plain chain of kernels).  Poses are 12 doubles, world to camera, row-major [R | t].  All arithmetic after loading the fp32 inputs is fp64.
 * The inlier rule, everywhere: a match is an inlier of (R, t) when Z > 0 and (fx X/Z + cx - x)^2 + (fy Y/Z + cy - y)^2 <= thr^2, (X, Y, Z) = R p + t.
 *  1. Samples.  Sample h of problem b is three distinct indices from ONE Philox4x32-10 call (the generator of the dropout masks above): counter (h, 0, b, 0x504E50),
 *     key = seed; i0 = (w0 M) >> 32, j1 = (w1 (M - 1)) >> 32, j2 = (w2 (M - 2)) >> 32 as 64-bit products; i1 = j1 + (j1 >= i0); i2 = j2, incremented once if
 *     >= min(i0, i1), then once more if >= max(i0, i1).  A pure function of (seed, b, h, M).  (M < 3: the three indices are -1.)
 *  2. Minimal solver.  P3P on the three unit bearings and world points: Grunert's quartic in the ratio of two depths, solved in closed form (Ferrari; the resolvent
 *     cubic's real root takes one Newton step), every real root with positive depths polished by ONE Newton step on the three law-of-cosines equations, the pose from
 *     the two congruent triangles.  Up to four solutions per sample in slots [h][0 .. nsol[h]), the other slots zero; the slot order is unspecified.  nsol = 0 for a
 *     degenerate sample (world triangle of zero area, coincident bearings), both checked; a non-finite solution is never kept.
 *  3. Score.  A candidate's score is its integer inlier count over all M matches; an invalid slot (and a pose with a non-finite entry) scores -1.
 *  4. Selection.  The highest count; among equals the LOWEST candidate index 4 h + slot.
 *  5. Local optimisation.  NL_PNP_LO_ROUNDS rounds: take the inliers of the current pose, stop if there are fewer than 4, run NL_PNP_GN_ITERS Gauss-Newton
 *     iterations on them — residuals in pixels, left perturbation R <- exp(w) R, t <- t + d, the 6 x 6 normal equations J^T J + 1e-12 I solved by Cholesky.  A failed
 *     factorisation or a non-finite step ends the optimisation and keeps the last finite pose.
 *  6. Result.  mask = the inlier set of the FINAL pose (one byte per match), num_inliers its size, success = num_inliers >= min_inliers (>= 4) with a finite pose.
 *     A problem with M < 4, or without any valid candidate, is not an error: success = 0, the identity pose, an empty mask.
 * There is no adaptive stopping: H is fixed per call (counting trials would need a synchronisation).  tests/pnp_ref.py restates all six steps in fp64 numpy.
 * info (B x 4 int32, DEVICE): success, num_inliers, best_candidate, best_count (nl_pnp_refine: the last two are -1).
 * Checks, before anything is dereferenced: a negative count, min_inliers < 4, a null pointer with work to do, offsets that do not start at 0 or decrease, fx / fy /
 * thr not finite and positive (cx, cy not finite): NL_ERR_BAD_ARG; H not a multiple of 64 in 64..65536, a problem above 2^20 matches, B above 2^20, P above 2^30:
 * NL_ERR_UNSUPPORTED; a missing, short or not 256-byte aligned workspace: NL_ERR_WORKSPACE; B == 0 (nl_pnp_score: P == 0): NL_OK, nothing launched.
 * nl_pnp_workspace_bytes: 0 for arguments the calls refuse; linear in B; nothing is kept per match, so M_total does not enter today.
 * nl_pnp_samples: step 1 alone, samples (B, H, 3) int32.  nl_pnp_hypotheses: steps 1 + 2, poses (B, H, 4, 12) doubles, nsol (B, H) int32, samples optional (NULL).
 * nl_pnp_score: step 3 for ANY P poses (P, 12) against one problem; nsol (NULL, or (P / 4) int32 with P a multiple of 4) marks slot i & 3 of sample i >> 2 invalid
 * when it is not below nsol.  nl_pnp_refine: steps 5 + 6 of one problem from pose_in.  nl_pnp_ransac: the whole; poses (B, 12), mask (offsets[B] bytes), info, and
 * optionally the (B, 4 H) counts (NULL: not wanted). */
#define NL_PNP_LO_ROUNDS 3
#define NL_PNP_GN_ITERS 5
size_t nl_pnp_workspace_bytes(int64_t M_total, int64_t B, int H);
int nl_pnp_samples(uint64_t seed, const int32_t* offsets, int64_t B, int H, int32_t* samples, void* stream);
int nl_pnp_hypotheses(const float* pts2d, const float* pts3d, const int32_t* offsets, const double* intrinsics, int64_t B, int H, uint64_t seed, int32_t* samples,
                      double* poses, int32_t* nsol, void* stream);
int nl_pnp_score(const float* pts2d, const float* pts3d, int64_t M, const double* intrinsics, double thr, const double* poses, const int32_t* nsol, int64_t P,
                 int32_t* counts, void* stream);
int nl_pnp_refine(const float* pts2d, const float* pts3d, int64_t M, const double* intrinsics, double thr, int min_inliers, const double* pose_in, double* pose_out,
                  uint8_t* mask, int32_t* info, void* stream);
int nl_pnp_ransac(const float* pts2d, const float* pts3d, const int32_t* offsets, const double* intrinsics, const double* thr, int64_t B, int H, uint64_t seed,
                  int min_inliers, double* poses, uint8_t* mask, int32_t* info, int32_t* counts, void* ws, size_t ws_bytes, void* stream);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* NERFLOC_RENDER_H */
