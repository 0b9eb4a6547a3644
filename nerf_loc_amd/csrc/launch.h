// Host-side declarations of every function that one translation unit of libnerfloc_render.so defines and another calls, grouped by the defining file, each
// declared exactly once (default arguments live here only).  Included by common.h only, as its last line (it uses the types defined there and includes nothing
// itself; no .hip file includes it directly), so every unit sees the declarations, the defining files too: a definition that
// drifts from its declaration is an ambiguous call / a redefined default argument at compile time or an undefined symbol at link time (-Wl,--no-undefined).
// The public C-ABI is declared in include/nerfloc_render.h.
#pragma once

// ---- abi.hip ---------------------------------------------------------------------------------------------
// Workgroups of a persistent kernel on the CURRENT device: its CU count rounded down to a multiple of the 8 XCDs (>= 8); cached per device id
// — a process may drive several GPUs through several HipRenderers.  < 0: NL_ERR_HIP
int nl_persistent_cus();

// ---- pack.hip --------------------------------------------------------------------------------------------
// An N x K row-major fp32 matrix (device) into fragment planes of N * K elements each (mfma.h: nl_frag16_src for the four 16-bit planes — acc_order: its
// permuted form — and nl_frag32_src for the fp32 plane); a null plane is not stored (the maps are walked all the same).  N a multiple of 32, K of 16.
// The weight images of s2d.hip, fine.hip and sct.hip.
int nl_launch_frag_pack(const float* w, int N, int K, unsigned short* bf_hi, unsigned short* bf_lo, unsigned short* f16_hi, unsigned short* f16_lo, float* f32,
                        bool acc_order, hipStream_t st);

// ---- gemm.hip --------------------------------------------------------------------------------------------
int nl_gemm_launch(const NlGemmArgs& a, int precision, hipStream_t stream);

// ---- tgemm.hip -------------------------------------------------------------------------------------------
size_t nl_tgemm_mx_image_bytes(int Kpad);
int nl_launch_sample_chain(const float* O, const float* T64, const float* wscale, const float* gamma, const float* beta, float eps, const void* wbase,
                           size_t off_g2, const float* bias_g2, size_t off_fc, size_t off_f0, size_t off_ba, const float* bias_f0, float* FA, float* fth,
                           float* blA, int64_t M, int precision, hipStream_t st, bool frag_out = false, bool frag_f16 = false);
int nl_launch_query_chain(const float* T64, const void* wbase, size_t off_g2, const float* bias_g2, size_t off_q, float* Q, int64_t M, int precision,
                          hipStream_t st);
// streaming transposed GEMM: bf16 modes, N <= 256, 16-B aligned segments
int nl_tgemm_nrt(int N);
size_t nl_tgemm_stream_bytes(int Kpad, int N);
bool nl_tgemm_supported(const NlGemmArgs& a, int precision);
int nl_tgemm_launch(const NlGemmArgs& a, int precision, hipStream_t stream);
// feat_mlp.0 + LeakyReLU + the compositing of its rows along the ray in the f16mx arithmetic (tgemm.hip: feat_comp_mx_kernel): hc (N / S, 256) from feature_agg's
// fragment image, the samples' compositing weights, G_FEAT0P's fp16 stream and its fp6 images
bool nl_feat_comp_mx_supported(int W, int S, int64_t N);
// w2 != null: feat_mlp.2 too (G_FEAT2's packed fp32 matrix [k][npad], row 256 = the bias that meets the weight sum): feat (N / S, C) is written, hc is not
int nl_launch_feat_comp_mx(const float* fa_frag, const float* wts, int64_t N, int S, const void* bsh, const void* bmx, const float* bias, float* hc, hipStream_t st,
                           const float* w2 = nullptr, int npad = 0, int C = 0, const float* wsum = nullptr, float* feat = nullptr, bool frag_f16 = false);

// ---- knn.hip ---------------------------------------------------------------------------------------------
struct NlKnnGrid {
  NlGridParams* params;  // device
  int* starts;           // device [GRID_CELLS + 1]
  int* counts;           // device [GRID_CELLS]
  int* cursor;           // device [GRID_CELLS]
  int* cell_of;          // device [M]
  float4* sorted;        // device [M]
  struct NlKnnNode* nodes;   // device [NL_KNN_NODES]: per-node range and bounding box of its points (knn_nodes.h)
  int M;
};
size_t nl_knn_grid_bytes(int64_t M);
int nl_knn_grid_build(NlKnnGrid* g, void* mem, const float* xyz, int64_t M, hipStream_t st);
int nl_knn_search(const NlKnnGrid* g, const float* xyz, int64_t N, int K, int* idx, float* d2, hipStream_t st);

// ---- mvagg.hip -------------------------------------------------------------------------------------------
int nl_launch_chw_to_hwc(const float* src, float* dst, int V, int Cc, int HW, hipStream_t st);
int nl_launch_mv_vis(const NlViews& vw, const float* visf_hwc, const float* dec_w, const float* xyz, int64_t N, float* vis_out, float* dd_out, hipStream_t st);
size_t nl_mv_decoder_pack_bytes();
int nl_pack_mv_decoder(const float* dec_valu_layout, void* out, hipStream_t st);
int nl_launch_mv_vis_mfma(const NlViews& vw, const float* visf_hwc, const void* dpack, const float* xyz, int64_t N, float* vis_out,
                          float* dd_out, bool x3, hipStream_t st);
int nl_launch_mv_stats(const NlViews& vw, const float* viewsdev, const float* images, const float* feat, int C, const float* xyz, int64_t N, const float* vis_in,
                       const float* dd_in, float* g393, int ldg, float* rgb_feat, float* vis_ang, int* valid_s, const float* pfeat, const float* blw,
                       float* bl1, float* rgbv, hipStream_t st);

// ---- mvfront.hip -----------------------------------------------------------------------------------------
size_t nl_mv_front_pack_bytes();
int nl_pack_mv_front(const float* w_outfc0, const float* b_outfc0, void* out, hipStream_t st);
bool nl_mv_front_supported(int C, int V, int64_t N);
int nl_launch_mv_front(const NlViews& vw, const float* viewsdev, const float* images, const float* feat, const float* xyz, int64_t N, const float* vis_in,
                       const float* dd_in, const void* pack, float* t64, int* valid_s, float* rgbv, hipStream_t st);

// ---- point.hip -------------------------------------------------------------------------------------------
int nl_launch_point_encode(const float* xyz, const float* dir, int dir_stride, int dir_div, int64_t N, int K, int64_t M, const int* idx, const float* d2,
                           const float* sp_xyz, const float* sp_feat, int F, const float* sp_conf, const float* sp_dir, const float* rd_w,
                           float inv_span, float* X, int ldx, float* wscale, hipStream_t st);
int nl_launch_attn(const float* Q, const float* KV, int64_t N, int K, float* O, hipStream_t st, unsigned* logit_amax = nullptr);
int nl_launch_ln_agg(const float* FC, const float* G, int64_t N, int W, const float* gamma, const float* beta, float eps, const float* wscale, float* out, hipStream_t st);

// ---- point_fused.hip -------------------------------------------------------------------------------------
size_t nl_point_stream_bytes(int W);
int nl_pack_point_stream(const float* w1, const float* w2, const float* w3, const float* wk, const float* wv, void* out, int W, int F, hipStream_t st);
int nl_pack_ptt(const float* w1, const float* b1, int W, int F, int Kpad, int Npad, float* B32, float* bias, hipStream_t st);
int nl_launch_wscale(const int* idx, const float* d2, const float* conf, int64_t N, int K, int64_t M, float* wscale, hipStream_t st);
bool nl_point_fused_supported(int W, int precision);
int nl_launch_point_fused(const NlPointFusedArgs& a, int W, int precision, hipStream_t st);

// ---- point_fused2.hip ------------------------------------------------------------------------------------
size_t nl_point_stream2_bytes(int W);
int nl_pack_point_stream2(const float* w1, const float* w2, const float* w3, const float* wk, const float* wv, const float* b2, const float* b3,
                          const float* rd_w, void* out, int W, int F, hipStream_t st, int mx = 0);
bool nl_point_fused2_supported(int W, int precision);
int nl_launch_point_fused2(const NlPointFusedArgs& a, int W, int precision, hipStream_t st, bool mx = false, float* keep_kv = nullptr, unsigned* const* keep_mk = nullptr,
                           unsigned* logit_amax = nullptr, unsigned long long* clk = nullptr);
int nl_table_absmax(const float* x, size_t n, float* out, hipStream_t st);

// ---- point_bwd.hip ---------------------------------------------------------------------------------------
bool nl_point_bwd_chain_supported(int W);
size_t nl_point_bwd_stream_bytes(int W);
int nl_pack_point_bwd_stream(const float* w1, const float* w2, const float* w3, const float* wk, const float* wv, void* out, int W, int F, hipStream_t st);
int nl_launch_point_bwd_chain(const float* gkv, const unsigned* const* mk, const void* wstream, float* gx, int64_t NK, int W, hipStream_t st, const float* q = nullptr,
                              const float* kv = nullptr, const float* go = nullptr, float* gq = nullptr);

// ---- unet.hip --------------------------------------------------------------------------------------------
int nl_launch_ln_slab_elu(const float* in, int64_t R, int L, int Cc, const float* gamma, const float* beta, float eps, float* out, float* pooled, hipStream_t st);

// ---- unet_inner.hip --------------------------------------------------------------------------------------
bool nl_unet_inner_supported(int S, int precision);
int nl_launch_unet_inner(const NlUnetInnerArgs& a, int precision, hipStream_t st);

// ---- heads.hip -------------------------------------------------------------------------------------------
int nl_launch_sample_points(const float* rays_o, const float* rays_d, int64_t R, int S, float near_, float far_, const float* z_in, float* z_out, float* xyz, hipStream_t st);
int nl_launch_sigma(const float* geo, int64_t N, int W, const float* w, const float* b, float* sigma, hipStream_t st);
int nl_launch_sigma_max(const float* sigma, int64_t N, unsigned* slot, hipStream_t st);
int nl_launch_blend(const float* hA, const float* h1, const float* rgbv, int64_t N, int V, const float* w2, const float* b2, const float* w4, const float* b4, float* rgb_s, hipStream_t st,
                    const int* n_alive = nullptr, int S = 1);
int nl_launch_blend_taps(const NlViews& vw, const float* viewsdev, const float* pfeat, const float* blw, const float* xyz, const float* hA, const float* rgbv, int64_t N,
                         const float* w2, const float* b2, const float* w4, const float* b4, float* rgb_s, hipStream_t st, const int* n_alive, int S);
int nl_launch_termination(const float* z_vals, const float* sigma, int64_t R, int S, float eps, int* n_alive, int* tile_list, int* tile_count, hipStream_t st);
int nl_launch_composite(const float* z_vals, const float* sigma, const float* rgb_s, const float* ft, const int* valid_s, int64_t R, int S, int C,
                        int white_bkgd, const nl_render_out* out, int64_t ray0, float* feat_dst, float* wsum_dst, hipStream_t st, const int* n_alive = nullptr,
                        float* w_scratch = nullptr);

// ---- hier.hip --------------------------------------------------------------------------------------------
int nl_launch_coarse_weights(const NlViews& vw, const float* w2c_kinv_host, const float* visf_hwc, const float* dec_w, const void* dpack,
                             int precision, const float* pix, const float* zc, int64_t R, int Sc, float* ws_alpha, float* ws_vis, float* ws_mask,
                             float* weights, float* depth_coarse, hipStream_t st);
int nl_launch_sample_pdf(const float* zc, const float* wc, int Sc, const float* u, int Ni, const float* zb, int Sb, int64_t R,
                         float* z_out, hipStream_t st);

// ---- backward.hip ----------------------------------------------------------------------------------------
// glue kernels of the backward passes (nl_composite_backward and nl_knn_backward, also defined there, are public: include/nerfloc_render.h)
int nl_launch_colsum(const float* Y, int ldy, int64_t rows, int M, float* out, float* scratch, hipStream_t st);
int nl_launch_sp_feat_scatter(const float* gXF, int ld, int F, const int* idx, int64_t N, int K, int64_t M, float* g_sp_feat, hipStream_t st);
int nl_launch_ln_agg_backward(const float* FC, const float* G, const float* gy, int64_t N, int W, const float* gamma, float eps, const float* wscale, float* gx,
                              float* aff, hipStream_t st);
int nl_launch_attn_backward(const float* Q, const float* KV, const float* gO, int64_t N, int K, float* gQ, float* gKV, hipStream_t st);
int nl_launch_lrelu_mask(float* g, const float* h, size_t n, hipStream_t st);
int nl_launch_add(const float* a, const float* b, float* o, size_t n, hipStream_t st);
int nl_launch_mv_geom_backward(const NlViews& vw, const float* viewsdev, const float* images, const float* feat, int C, const float* pfeat, const float* xyz,
                               int64_t N, const float* vis_in, const float* dd_in, const float* g393, int ldg, const float* g_pf, const float* g_rgbv,
                               const float* g_ang, float* g_xyz, float* g_qc, float* g_vis, float* g_dd, float* sc_feat, float* sc_pfeat, const float* stats,
                               hipStream_t st);
int nl_dec_train_row(void);
size_t nl_dec_wpart_floats(void);
int nl_launch_copy_rows(const float* src, int lds, float* dst, int ldd, int64_t rows, int cols, bool add, hipStream_t st);
int nl_launch_dec_backward(const NlViews& vw, const float* visf_hwc, const float* dec_w, const void* dpack, const float* xyz, int64_t N, const float* g_vis,
                           const float* g_dd, float* part, float* g_xyz, float* tr, float* const* decw, float* scratch, size_t scratch_floats, float* sc_vis,
                           hipStream_t st);
int nl_launch_blend_backward(const float* hA, const float* h1, const float* rgbv, int64_t N, int V, const float* w2, const float* b2, const float* w4,
                             const float* b4, const float* blw, const float* g_rgb_s, float* g_hA, float* g_pf, float* g_rgbv, float* g_ang, float* tr,
                             hipStream_t st);
int nl_launch_blend_inputs8(const NlViews& vw, const float* viewsdev, const float* xyz, int64_t N, const float* rgbv, float* x8, hipStream_t st);
int nl_launch_blw_unpack(const float* t, float* g, int W, int F, hipStream_t st);
int nl_launch_elu_mask(float* g, const float* e, size_t n, hipStream_t st);
int nl_launch_ln_slab_elu_backward(const float* x, int64_t R, int L, int Cc, const float* gamma, const float* beta, float eps, const float* g_out, int ldgo, int pool,
                                   float* g_x, float* aff, hipStream_t st);
int nl_launch_table_add_t(const float* t, float* g, int L, int Cc, hipStream_t st);
int nl_launch_colsum_tables(const float* Y, int64_t rows, int L, int Cc, float* gw, float* gb, float* scratch, hipStream_t st);
int nl_launch_ray_feat_sum(const float* z, const float* sigma, const float* ft, int64_t R, int S, int C, float* hc, float* wsum4, hipStream_t st);
int nl_launch_sigma_backward(const float* geo, int64_t N, int W, const float* w, const float* b, const float* g_sigma, float* g_geo, float* gpre4, hipStream_t st);
int nl_launch_gw_total(const float* g_wts, const float* g_feat, const float* b2, int64_t R, int S, int C, float* gw, const float* g_beta, const float* bv,
                       hipStream_t st);
int nl_launch_beta_forward(const float* wts, const float* bv, int64_t R, int S, float beta_min, float* beta, hipStream_t st);
int nl_launch_beta_backward(const float* geo, int64_t N, int S, int W, const float* wb, const float* bb, const float* wts, const float* g_beta, float* g_geo, float* gpre4,
                            hipStream_t st);
int nl_launch_ray_reduce(const float* ga, const float* gb, const float* gc, const float* g_dir, const float* g_qcN, const float* z, int64_t R, int S, float* g_o,
                         float* g_d, float* g_qc, hipStream_t st);
int nl_launch_add2d(const float* a, int lda, const float* b, int ldb, float* o, int ldo, int64_t rows, int cols, hipStream_t st);
int nl_launch_point_encode_backward(const float* xyz, const float* dir, int dir_stride, int dir_div, int64_t N, int K, int64_t M, const int* idx,
                                    const float* sp_xyz, const float* sp_dir, const float* rd_w, float inv_span, const float* gX, int ldg, float* g_xyz,
                                    float* g_dir, float* tr, hipStream_t st);

// ---- wgrad.hip -------------------------------------------------------------------------------------------
int nl_launch_wgrad(const float* dY, int ldy, int M, const float* X, int ldx, int N, int64_t rows, int shift, int period, float* gW, int ldc, int cs, int co,
                    float* gb, float* scratch, size_t scratch_floats, hipStream_t st);
size_t nl_wgrad_scratch_floats(int64_t rows, int M, int N);
int nl_launch_wgrad_multi(int nsub, const float* const* dY, int ldy, int M, const float* const* X, int ldx, int N, int64_t rows, const int* shift, int period,
                          float* gW, int ldc, int cs, const int* co, float* gb, int bias_sub, float* scratch, size_t scratch_floats, hipStream_t st);

// ---- s2d_bwd.hip -----------------------------------------------------------------------------------------
// gw3[unit] += / gb3[0] += the waves' partial rows ([items][S2D_W3P_LD], s2d_bwd.h) in a fixed order; either output may be null
int nl_launch_s2d_w3_reduce(const float* part, int items, float* gw3, float* gb3, hipStream_t st);
// wt (cols, rows) = w (rows, cols)^T
int nl_launch_transpose(const float* w, int rows, int cols, float* wt, hipStream_t st);

// ---- fine.hip --------------------------------------------------------------------------------------------
// out (M * 49, Cout) = rows (M * 49, Cin) . W^T for a proj image of W (Cout x Cin): the window kernels on dense rows, split-bf16 (three terms with x3)
int nl_launch_fine_rows(const void* img, int Cin, int Cout, bool x3, const float* rows, int64_t M, float* out, hipStream_t st);

// ---- sct.hip ---------------------------------------------------------------------------------------------
// the projections and the attention of one layer (0..3) of an nl_sct_pack_weights image with the inference kernels, into caller-owned q (B * Nq, C), k, v
// (B * Nk, C) and attention-output rows (B * Nq, C): the first half of nl_sct_layer, for the training forward (sct_bwd.hip), which keeps them.  A drop_p whose
// 16-bit threshold (sct_drop.h) is not zero takes the dropping attention kernel with the masks of (drop_seed, layer, site 0); 0 is the inference kernel
int nl_launch_sct_qkv_attn(const void* img, int C, int F, int layer, int precision, const float* x, const float* xpos, int64_t Nq, const float* mem, const float* mpos,
                           int64_t Nk, int64_t B, float* q, float* k, float* v, float* attn, float drop_p, unsigned long long drop_seed, hipStream_t st);
