// The forward path of libnerfloc_render.so: the stage drivers (do_mv, do_point, do_unet, do_heads), their entry points and the chunked render_rays
// orchestrator with its precision guard and the several-frames call.  The way back: render_bwd.hip.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include <mutex>
#include <unordered_map>
#include "common.h"
#include "host.h"
using namespace nlhost;

namespace {

void carve_mv(Bump& b, const nl_config* c, int V, int64_t N, MvBufs& m) {
  m.vis = b.take<float>((size_t)V * N); m.dd = b.take<float>((size_t)V * N);
  m.g393 = b.take<float>((size_t)N * ldg_of(c->C)); m.t64 = b.take<float>((size_t)N * 64);
}
void carve_pt(Bump& b, const nl_config* c, int64_t N, int K, PtBufs& p, bool force_generic = false) {
  const int W = c->W;
  p.idx = b.take<int>((size_t)N * K); p.d2 = b.take<float>((size_t)N * K);
  if (!force_generic && nl_point_fused_supported(W, c->precision)) { p.X = p.H1 = p.H2 = p.KV = nullptr; }
  else {
    p.X = b.take<float>((size_t)N * K * ldx_of(c->C));
    p.H1 = b.take<float>((size_t)N * K * W); p.H2 = b.take<float>((size_t)N * K * W);
    p.KV = b.take<float>((size_t)N * K * 256);
  }
  p.Q = b.take<float>((size_t)N * 128); p.O = b.take<float>((size_t)N * 128);
  p.FCo = b.take<float>((size_t)N * W); p.wscale = b.take<float>((size_t)N);
}

}  // namespace

namespace nlhost {
void carve_un(Bump& b, const nl_config* c, int64_t R, UnBufs& u) {
  const size_t N = (size_t)R * c->S;
  u.r1 = b.take<float>(N * 64); u.c1 = b.take<float>(N / 2 * 64);
  u.r2 = b.take<float>(N / 2 * 128); u.c2 = b.take<float>(N / 4 * 128);
  u.r3 = b.take<float>(N / 4 * 128); u.c3 = b.take<float>(N / 8 * 128);
  u.x0r = b.take<float>(N / 4 * 128); u.x0 = b.take<float>(N / 4 * 128);
  u.x1r = b.take<float>(N / 2 * 64); u.x1 = b.take<float>(N / 2 * 64);
  u.x2r = b.take<float>(N * 32); u.x2 = b.take<float>(N * 32);
  u.outr = b.take<float>(N * c->W);
}
}  // namespace nlhost

namespace {

void carve_hd(Bump& b, const nl_config* c, int V, int64_t R, HdBufs& h) {
  const size_t N = (size_t)R * c->S;
  h.sigma = b.take<float>(N); h.fth = b.take<float>(N * c->W); h.hc = b.take<float>((size_t)R * c->W); h.wsum = b.take<float>((size_t)R);
  h.blA = b.take<float>(N * 32); h.rgb_s = b.take<float>(N * 3);
  h.n_alive = b.take<int>((size_t)R); h.tile_list = b.take<int>(N / 32 + 2); h.tile_count = b.take<int>(1);
}

// whether the fused render path runs statistics + out_fc.0 in mv_front_kernel and recomputes the blend taps (round 4): a function of the configuration alone,
// so that workspace sizing and the render call agree
inline bool front_path(const nl_config* c, int V) {
  return c->precision != NL_PREC_F32 && nl_mv_front_supported(c->C, V, 1);
}

void carve_render(Bump& b, const nl_config* c, int V, int64_t R, RenderBufs& rb) {
  const size_t N = (size_t)R * c->S;
  rb.xyz = b.take<float>(N * 3); rb.z = b.take<float>(N);
  rb.G = b.take<float>(N * c->W);
  // the blend layer's per-(sample, view) rows exist only where mv_front_kernel + blend_taps_mfma_kernel do not apply (other feature widths, fp32 mode):
  // at config 2 that is 0.67 GB of the chunk's workspace
  rb.bl1 = front_path(c, V) ? nullptr : b.take<float>(N * V * 32);
  rb.rgbv = b.take<float>(N * V * 4);
  // (the statistics row of the old path is not needed then either, but carve_mv serves the stage API too)
  rb.valid_s = b.take<int>(N);
  rb.FA = b.take<float>(N * c->W); rb.geo = b.take<float>(N * c->W);
  carve_mv(b, c, V, N, rb.mv); carve_pt(b, c, N, 8, rb.pt); carve_un(b, c, R, rb.un); carve_hd(b, c, V, R, rb.hd);
}

// front (fused render path, C = 192, non-fp32 modes; round 4): statistics + out_fc.0 in mv_front_kernel — no statistics row, no per-(sample, view) blend rows
// (bl1 is then not written: the blend tail recomputes its taps, do_heads_pre); rgbv still carries the tapped colours + visibility
int do_mv(const Ctx& x, const nl_frame* f, const float* qc, const float* xyz, int64_t N, float* G, float* rgb_feat,
          float* vis_ang, int* valid_s, float* bl1, float* rgbv, const MvBufs& m, bool skip_g = false, const float* qrows = nullptr, int qS = 1,
          bool front = false) {
  const NlViews vw = with_query(f, qc, qrows, qS);
  if (bl1 || front) NL_TRY(ensure_pfeat(x, f));
  if (x.c->precision == NL_PREC_F32) NL_TRY(nl_launch_mv_vis(vw, f->visf_hwc, x.p<float>(x.L.dec_w), xyz, N, m.vis, m.dd, x.st));
  else NL_TRY(nl_launch_mv_vis_mfma(vw, f->visf_hwc, x.p<char>(x.L.dec_mfma), xyz, N, m.vis, m.dd, x.c->precision == NL_PREC_BF16X3, x.st));
  if (front) {
    NL_TRY(nl_launch_mv_front(vw, f->views_dev, f->images, f->feat, xyz, N, m.vis, m.dd, x.p<char>(x.L.mvf_pack), m.t64, valid_s, rgbv, x.st));
    if (skip_g) return NL_OK;
    SegSpec s1{m.t64, 64, 64, 0, 1};
    NL_TRY(run_gemm(x, G_OUTFC2, &s1, 1, N, G, x.c->W, NL_ACT_ELU));
    return NL_OK;
  }
  NL_TRY(nl_launch_mv_stats(vw, f->views_dev, f->images, f->feat, f->C, xyz, N, m.vis, m.dd, m.g393, ldg_of(f->C), rgb_feat, vis_ang, valid_s, f->pfeat,
                            x.p<float>(x.L.blw), bl1, rgbv, x.st));
  SegSpec s0{m.g393, ldg_of(f->C), ldg_of(f->C), 0, 1};
  NL_TRY(run_gemm(x, G_OUTFC0, &s0, 1, N, m.t64, 64, NL_ACT_ELU));
  if (skip_g) return NL_OK;   // the consumers recompute G from the hidden rows (sample_chain_kernel)
  SegSpec s1{m.t64, 64, 64, 0, 1};
  NL_TRY(run_gemm(x, G_OUTFC2, &s1, 1, N, G, x.c->W, NL_ACT_ELU));
  return NL_OK;
}

// knn_done != null: the caller already ran the KNN (+ the aggregation scale) on a side stream and hands over the event to wait for
// chain != null && chain->t64 != null (fused render path, W = 256, bf16 modes): the query rows before the branch and fc + LayerNorm +
// scale, feat_mlp.0 (chain->fth, may be null) and the blend projection (chain->blA) after it run as two chain kernels that recompute
// the multiview feature rows G from out_fc's hidden rows t64 (G is then not read here and need not exist); *chain->done reports it
int do_point(const Ctx& x, const nl_frame* f, const float* xyz, const float* dir, int dir_stride, int dir_div, const float* G, int64_t N, int K,
             float* FA, const PtBufs& p, SideJoin* knn_done = nullptr, const ChainOut* chain = nullptr) {
  const int W = x.c->W, F = f->C + 3;
  const bool fused_path = K == 8 && nl_point_fused_supported(W, x.c->precision);
  if (!knn_done) NL_TRY(nl_knn_search(&f->grid, xyz, N, K, p.idx, p.d2, x.st));
  const float* t64 = chain ? chain->t64 : nullptr;
  if (t64) {
    NL_TRY(nl_launch_query_chain(t64, x.pk, x.L.bst[G_OUTFC2], x.p<float>(x.L.bias[G_OUTFC2]), x.L.bst[G_QP], p.Q, N, x.c->precision, x.st));
  } else {
    SegSpec sg{G, W, W, 0, 1};
    NL_TRY(run_gemm(x, G_Q, &sg, 1, N, p.Q, 128, NL_ACT_NONE));
  }
  // (Issuing the search in parts, each under the neural-point launch of the part before it, was measured slower: profiles/r6_knn_parts_*_timeline.txt.)
  if (knn_done) NL_TRY(knn_done->join());
  if (fused_path) {
    NL_TRY(ensure_ptt(x, f));
    if (!knn_done) NL_TRY(nl_launch_wscale(p.idx, p.d2, f->sp_conf, N, K, f->M, p.wscale, x.st));
    NlPointFusedArgs a;
    a.xyz = xyz; a.dir = dir; a.dir_stride = dir_stride; a.dir_div = dir_div > 0 ? dir_div : 1;
    a.idx = p.idx; a.Q = p.Q; a.O = p.O; a.ptt = f->ptt; a.sp_xyz = f->sp_xyz; a.sp_dir = f->sp_dir;
    a.wstream = x.p<uint4>(x.L.pt_stream); a.bias = x.p<float>(x.L.pt_bias); a.rd_w = x.p<float>(x.L.rd_w);
    const bool mx = x.mx && x.c->precision == NL_PREC_BF16X3 && nl_point_fused2_supported(W, x.c->precision);
    a.wstream2 = x.p<uint4>(mx ? x.L.pt_stream2_mx : x.L.pt_stream2);
    a.N = (int)N; a.M = (int)(f->M > 0x7fffffff ? 0x7fffffff : f->M); a.inv_span = 1.f / (f->views.far_ - f->views.near_);
    hipEvent_t pe0 = nullptr, pe1 = nullptr;
    if (prof_arm(&pe0, &pe1)) NL_CHECK_HIP(hipEventRecord(pe0, x.st));
    a.logit_amax = reinterpret_cast<unsigned*>(f->views_dev + 249);   // (read by the v1 kernel; the v2 launcher takes it as a parameter)
    int rc2 = NL_ERR_UNSUPPORTED;
    if (nl_point_fused2_supported(W, x.c->precision)) rc2 = nl_launch_point_fused2(a, W, x.c->precision, x.st, mx, nullptr, nullptr, reinterpret_cast<unsigned*>(f->views_dev + 249),
                                                                                   reinterpret_cast<unsigned long long*>(f->views_dev + 250));
    if (rc2 == NL_ERR_UNSUPPORTED) rc2 = nl_launch_point_fused(a, W, x.c->precision, x.st);   // (e.g. more rows than 32-bit buffer offsets reach)
    NL_TRY(rc2);
    if (pe1) NL_CHECK_HIP(hipEventRecord(pe1, x.st));
  } else {
    if (!p.X) return NL_ERR_UNSUPPORTED;
    NL_TRY(nl_launch_point_encode(xyz, dir, dir_stride, dir_div, N, K, f->M, p.idx, p.d2, f->sp_xyz, f->sp_feat, F, f->sp_conf, f->sp_dir,
                                  x.p<float>(x.L.rd_w), 1.f / (f->views.far_ - f->views.near_), p.X, ldx_of(f->C), p.wscale, x.st));
    const int64_t MK = N * K;
    SegSpec sx{p.X, ldx_of(f->C), F + 90, 0, 1};
    NL_TRY(run_gemm(x, G_BASE0, &sx, 1, MK, p.H1, W, NL_ACT_LRELU));
    SegSpec s1{p.H1, W, W, 0, 1}, s2{p.H2, W, W, 0, 1};
    NL_TRY(run_gemm(x, G_BASE2, &s1, 1, MK, p.H2, W, NL_ACT_LRELU));
    NL_TRY(run_gemm(x, G_BASE4, &s2, 1, MK, p.H1, W, NL_ACT_LRELU));
    NL_TRY(run_gemm(x, G_KV, &s1, 1, MK, p.KV, 256, NL_ACT_NONE));
    NL_TRY(nl_launch_attn(p.Q, p.KV, N, K, p.O, x.st, reinterpret_cast<unsigned*>(f->views_dev + 249)));   // (the staged path reports the conditioning indicator too)
  }
  if (chain && chain->done) *chain->done = false;
  if (t64) {   // (the caller checked W, precision and the 32-bit offset range before leaving G unmaterialised)
    NL_TRY(nl_launch_sample_chain(p.O, t64, p.wscale, x.p<float>(x.L.ln_g), x.p<float>(x.L.ln_b), 1e-6f, x.pk, x.L.bst[G_OUTFC2],
                                  x.p<float>(x.L.bias[G_OUTFC2]), x.L.bst[G_FC], x.L.bst[G_FEAT0P], chain->fa_f16 ? x.L.bsh[G_BLENDAP] : x.L.bst[G_BLENDAP],
                                  x.p<float>(x.L.bias[G_FEAT0P]), FA, chain->fth, chain->blA, N, x.c->precision, x.st, chain->fa_frag, chain->fa_f16));
    if (chain->done) *chain->done = true;
    return NL_OK;
  }
  SegSpec so{p.O, 128, 128, 0, 1};
  // fc + residual + LayerNorm + aggregation scale: inside the GEMM's epilogue when the streaming kernel takes it
  const RowEpi ep{G, W, x.p<float>(x.L.ln_g), x.p<float>(x.L.ln_b), p.wscale, 1e-6f, FA};
  bool fused = false;
  NL_TRY(run_gemm(x, G_FC, &so, 1, N, p.FCo, W, NL_ACT_NONE, 0, 0, 0, 1, 0, &ep, &fused));
  if (!fused) NL_TRY(nl_launch_ln_agg(p.FCo, G, N, W, x.p<float>(x.L.ln_g), x.p<float>(x.L.ln_b), 1e-6f, p.wscale, FA, x.st));
  return NL_OK;
}

}  // namespace

namespace nlhost {

// sigma_out (optional): when conv_out's LayerNorm runs inside the GEMM, the density head is evaluated there too and
// *sigma_done is set; otherwise the caller runs sigma_kernel on geo
// need_geo == false: the caller only wants the density (model.py:525 is the sole consumer of the U-Net's output); when the density
// head runs inside conv_out's epilogue the (N, W) output rows are then never written (0.5 GB per config-2 batch)
// in_frag: `in` is feature_agg as the chain kernel's fragment image (NlGemmSeg::frag) instead of fp32 rows
// fuse_inner: the caller needs nothing of the five inner layers but their result (u.x2) — the inference render path; the backward passes and the stage entry
// point keep the separate launches (their pre-LayerNorm outputs and block outputs are read back)
int do_unet(const Ctx& x, const float* in, int64_t R, float* geo, const UnBufs& u, float* sigma_out, bool* sigma_done,
            bool need_geo, int in_frag, bool fuse_inner) {   // in_frag: NlGemmSeg::frag of `in` (0: fp32 rows, 1: fragment image, 3: its split-FP16 form)
  const int W = x.c->W, S = x.c->S;
  // the two phases of every transposed convolution as one launch (bf16 modes; the fp32 kernels keep the separate phases)
  const bool merged = x.c->precision != NL_PREC_F32;
  auto g = [&](int i) { return x.p<float>(x.L.un_g[i]); };
  auto b = [&](int i) { return x.p<float>(x.L.un_b[i]); };
  auto gl = [&](int i) { return x.p<float>(x.L.un_gl[i]); };   // accumulator-lane order: what the GEMM's fused LayerNorm reads
  auto bl = [&](int i) { return x.p<float>(x.L.un_bl[i]); };
  const float eps = 1e-5f;
  // feature_agg's two consumers take their weights with the channels of every 32-block in accumulator order in the bf16 modes (G_CONV1F / G_CONVOUTF, streaming
  // kernel): from the chain kernel's fragment image (in_frag) or from fp32 rows read in that order — the same products in the same order either way
  const bool korder = in_frag || ((x.c->precision == NL_PREC_BF16X3 || x.c->precision == NL_PREC_BF16) && (((size_t)in) & 15) == 0 &&
                                  ((x.has_bst >> G_CONV1F) & 1) && ((x.has_bst >> G_CONVOUTF) & 1));
  const int fa_mode = in_frag ? in_frag : (korder ? 2 : 0);
  {  // conv1: W -> 64 over S
    SegSpec s[1] = {{in, W, W, 0, 1, 3, fa_mode}};   // 3 taps, interleaved per 32-channel block
    const RowEpi ep{nullptr, 0, gl(U_CONV1), bl(U_CONV1), nullptr, eps, u.c1, NL_EPI_LNSLAB, 1};   // LN + ELU + MaxPool inside the GEMM when one workgroup = one ray
    bool fused = false;
    NL_TRY(run_gemm(x, korder ? G_CONV1F : G_CONV1, s, 1, R * S, u.r1, 64, NL_ACT_NONE, S, S, S, 1, 0, &ep, &fused));
    if (!fused) NL_TRY(nl_launch_ln_slab_elu(u.r1, R, S, 64, g(U_CONV1), b(U_CONV1), eps, nullptr, u.c1, x.st));
  }
  // conv2 ... trans_conv1 as one kernel (unet_inner.hip: a pair of rays per workgroup, every slab in LDS): S = 128, the streaming kernels' weight images
  const uint64_t inner_bits = (1ull << G_CONV2) | (1ull << G_CONV3) | (1ull << G_T3M) | (1ull << G_T2M) | (1ull << G_T1M);
  if (fuse_inner && merged && nl_unet_inner_supported(S, x.c->precision) && (x.has_bst & inner_bits) == inner_bits) {
    NlUnetInnerArgs ia;
    ia.c1 = u.c1; ia.c2 = u.c2; ia.x2 = u.x2; ia.R = (int)R; ia.eps = eps;
    const int gs[5] = {G_CONV2, G_CONV3, G_T3M, G_T2M, G_T1M}, us[5] = {U_CONV2, U_CONV3, U_T3, U_T2, U_T1};
    for (int i = 0; i < 5; ++i) { ia.w[i] = x.pk + x.L.bst[gs[i]]; ia.bias[i] = x.p<float>(x.L.bias[gs[i]]); ia.gl[i] = gl(us[i]); ia.bl[i] = bl(us[i]); }
    NL_TRY(nl_launch_unet_inner(ia, x.c->precision, x.st));
  } else {
  {  // conv2: 64 -> 128 over S/2
    SegSpec s[1] = {{u.c1, 64, 64, 0, 1, 3}};
    const RowEpi ep{nullptr, 0, gl(U_CONV2), bl(U_CONV2), nullptr, eps, u.c2, NL_EPI_LNSLAB, 1};   // two rays per workgroup at S = 128
    bool fused = false;
    NL_TRY(run_gemm(x, G_CONV2, s, 1, R * (S / 2), u.r2, 128, NL_ACT_NONE, S / 2, S / 2, S / 2, 1, 0, &ep, &fused));
    if (!fused) NL_TRY(nl_launch_ln_slab_elu(u.r2, R, S / 2, 128, g(U_CONV2), b(U_CONV2), eps, nullptr, u.c2, x.st));
  }
  {  // conv3: 128 -> 128 over S/4
    SegSpec s[1] = {{u.c2, 128, 128, 0, 1, 3}};
    const RowEpi ep{nullptr, 0, gl(U_CONV3), bl(U_CONV3), nullptr, eps, u.c3, NL_EPI_LNSLAB, 1};   // one ray per wave at S = 128
    bool fused = false;
    NL_TRY(run_gemm(x, G_CONV3, s, 1, R * (S / 4), u.r3, 128, NL_ACT_NONE, S / 4, S / 4, S / 4, 1, 0, &ep, &fused));
    if (!fused) NL_TRY(nl_launch_ln_slab_elu(u.r3, R, S / 4, 128, g(U_CONV3), b(U_CONV3), eps, nullptr, u.c3, x.st));
  }
  {  // trans_conv3: S/8 -> S/4
    const int Li = S / 8, Lo = S / 4;
    SegSpec o[2] = {{u.c3, 128, 128, 0, 1}, {u.c3, 128, 128, 1, 1}};
    bool tfused = false;
    // row m = output positions 2m, 2m+1: the (Li x 2 co) view of the merged output IS the ray's (Lo x co) slab, so LayerNorm([C, L]) + ELU
    // ride in the GEMM's epilogue (the affine tables are stored position-major: same memory either way)
    const RowEpi ept3{nullptr, 0, gl(U_T3), bl(U_T3), nullptr, eps, u.x0, NL_EPI_LNSLAB, 0};
    if (merged) NL_TRY(run_gemm(x, G_T3M, o, 2, R * Li, u.x0r, 256, NL_ACT_NONE, Li, Li, Li, 1, 0, &ept3, &tfused));
    else {
      SegSpec e[1] = {{u.c3, 128, 128, 0, 1}};
      NL_TRY(run_gemm(x, G_T3E, e, 1, R * Li, u.x0r, 128, NL_ACT_NONE, Li, Li, Lo, 2, 0));
      NL_TRY(run_gemm(x, G_T3O, o, 2, R * Li, u.x0r, 128, NL_ACT_NONE, Li, Li, Lo, 2, 1));
    }
    if (!tfused) NL_TRY(nl_launch_ln_slab_elu(u.x0r, R, Lo, 128, g(U_T3), b(U_T3), eps, u.x0, nullptr, x.st));
  }
  {  // trans_conv2 on cat[c2, x0]: S/4 -> S/2
    const int Li = S / 4, Lo = S / 2;
    SegSpec o[4] = {{u.c2, 128, 128, 0, 1}, {u.x0, 128, 128, 0, 1}, {u.c2, 128, 128, 1, 1}, {u.x0, 128, 128, 1, 1}};
    bool tfused = false;
    const RowEpi ept2{nullptr, 0, gl(U_T2), bl(U_T2), nullptr, eps, u.x1, NL_EPI_LNSLAB, 0};
    if (merged) NL_TRY(run_gemm(x, G_T2M, o, 4, R * Li, u.x1r, 128, NL_ACT_NONE, Li, Li, Li, 1, 0, &ept2, &tfused));
    else {
      SegSpec e[2] = {{u.c2, 128, 128, 0, 1}, {u.x0, 128, 128, 0, 1}};
      NL_TRY(run_gemm(x, G_T2E, e, 2, R * Li, u.x1r, 64, NL_ACT_NONE, Li, Li, Lo, 2, 0));
      NL_TRY(run_gemm(x, G_T2O, o, 4, R * Li, u.x1r, 64, NL_ACT_NONE, Li, Li, Lo, 2, 1));
    }
    if (!tfused) NL_TRY(nl_launch_ln_slab_elu(u.x1r, R, Lo, 64, g(U_T2), b(U_T2), eps, u.x1, nullptr, x.st));
  }
  {  // trans_conv1 on cat[c1, x1]: S/2 -> S
    const int Li = S / 2, Lo = S;
    SegSpec o[4] = {{u.c1, 64, 64, 0, 1}, {u.x1, 64, 64, 0, 1}, {u.c1, 64, 64, 1, 1}, {u.x1, 64, 64, 1, 1}};
    bool tfused = false;
    const RowEpi ept1{nullptr, 0, gl(U_T1), bl(U_T1), nullptr, eps, u.x2, NL_EPI_LNSLAB, 0};
    if (merged) NL_TRY(run_gemm(x, G_T1M, o, 4, R * Li, u.x2r, 64, NL_ACT_NONE, Li, Li, Li, 1, 0, &ept1, &tfused));
    else {
      SegSpec e[2] = {{u.c1, 64, 64, 0, 1}, {u.x1, 64, 64, 0, 1}};
      NL_TRY(run_gemm(x, G_T1E, e, 2, R * Li, u.x2r, 32, NL_ACT_NONE, Li, Li, Lo, 2, 0));
      NL_TRY(run_gemm(x, G_T1O, o, 4, R * Li, u.x2r, 32, NL_ACT_NONE, Li, Li, Lo, 2, 1));
    }
    if (!tfused) NL_TRY(nl_launch_ln_slab_elu(u.x2r, R, Lo, 32, g(U_T1), b(U_T1), eps, u.x2, nullptr, x.st));
  }
  }
  {  // conv_out on cat[in, x2]
    SegSpec s[2] = {{in, W, W, 0, 1, 3, fa_mode}, {u.x2, 32, 32, 0, 1, 3}};
    RowEpi ep{nullptr, 0, gl(U_OUT), bl(U_OUT), nullptr, eps, geo, NL_EPI_LNSLAB, 0};
    if (sigma_out) { ep.sig_w = x.p<float>(x.L.sig_w); ep.sig_b = x.p<float>(x.L.sig_b); ep.sig_out = sigma_out; }
    bool fused = false;
    if (!need_geo && sigma_out) ep.out = nullptr;   // (the unfused fallback below still writes `geo`)
    NL_TRY(run_gemm(x, korder ? G_CONVOUTF : G_CONVOUT, s, 2, R * S, u.outr, W, NL_ACT_NONE, S, S, S, 1, 0, &ep, &fused));
    if (!fused) NL_TRY(nl_launch_ln_slab_elu(u.outr, R, S, W, g(U_OUT), b(U_OUT), eps, geo, nullptr, x.st));
    if (sigma_done) *sigma_done = fused && sigma_out;
  }
  return NL_OK;
}

}  // namespace nlhost

namespace {

// the part of the heads that needs feature_agg only (not the density): feat_mlp.0, the per-sample blend projection, the blend tail
// term == true: n_alive / tile_list of `h` are valid (nl_launch_termination ran): dead samples are skipped
int do_heads_pre(const Ctx& x, int V, const float* FA, const float* bl1, const float* rgbv, int64_t N, bool want_feat, const HdBufs& h, int parts = 7,
                 bool term = false, const BlendTaps* bt = nullptr) {
  const int W = x.c->W;
  if (want_feat && (parts & 1)) {
    SegSpec s0{FA, W, W, 0, 1};
    const TileMap tm{h.tile_list, h.tile_count};
    NL_TRY(run_gemm(x, G_FEAT0, &s0, 1, N, h.fth, W, NL_ACT_LRELU, 0, 0, 0, 1, 0, nullptr, nullptr, term ? &tm : nullptr));
  }
  SegSpec sa{FA, W, W, 0, 1};
  if (parts & 2) NL_TRY(run_gemm(x, G_BLENDA, &sa, 1, N, h.blA, 32, NL_ACT_NONE));
  if ((parts & 4) && !bl1) {
    if (!bt) return NL_ERR_BAD_ARG;
    NL_TRY(nl_launch_blend_taps(bt->vw, bt->viewsdev, bt->pfeat, x.p<float>(x.L.blw), bt->xyz, h.blA, rgbv, N, x.p<float>(x.L.bl2_w), x.p<float>(x.L.bl2_b),
                                x.p<float>(x.L.bl4_w), x.p<float>(x.L.bl4_b), h.rgb_s, x.st, term ? h.n_alive : nullptr, x.c->S));
  } else if (parts & 4) NL_TRY(nl_launch_blend(h.blA, bl1, rgbv, N, V, x.p<float>(x.L.bl2_w), x.p<float>(x.L.bl2_b), x.p<float>(x.L.bl4_w),
                                               x.p<float>(x.L.bl4_b), h.rgb_s, x.st, term ? h.n_alive : nullptr, x.c->S));
  return NL_OK;
}

int do_heads(const Ctx& x, int V, const float* z, const float* FA, const float* geo, const float* bl1, const float* rgbv,
             const int* valid_s, int64_t R, int white, const nl_render_out* out, int64_t ray0, const HdBufs& h, bool have_sigma = false,
             bool pre_done = false, float term_eps = 0.f, int chain_parts = 0, const BlendTaps* bt = nullptr, bool feat_late = false, bool fa_f16 = false,
             unsigned* density_max = nullptr) {   // density_max: the frame's NL_DIAG_DENSITY_MAX slot (guarded calls only: one small reduction over the batch's densities)
  const int W = x.c->W, S = x.c->S, C = x.c->C;
  const int64_t N = R * S;
  if (!have_sigma) NL_TRY(nl_launch_sigma(geo, N, W, x.p<float>(x.L.sig_w), x.p<float>(x.L.sig_b), h.sigma, x.st));
  if (density_max) NL_TRY(nl_launch_sigma_max(h.sigma, N, density_max, x.st));
  const bool want_feat = out->feat != nullptr;
  const bool term = term_eps > 0.f && !pre_done;
  if (term) NL_TRY(nl_launch_termination(z, h.sigma, R, S, term_eps, h.n_alive, h.tile_list, h.tile_count, x.st));
  bool feat_done = false;
  if (feat_late) {
    // f16mx, W = 256, FA = the chain kernel's fragment image: feat_mlp.0's hidden rows are never materialised — the compositing pass leaves the samples' weights
    // (in the caller's `weights` output, or in the buffer the hidden rows would have taken) and feat_comp_mx_kernel multiplies, activates, weights and sums in one go
    if (!want_feat || term || pre_done || (chain_parts & 1)) return NL_ERR_BAD_ARG;
    NL_TRY(do_heads_pre(x, V, FA, bl1, rgbv, N, false, h, 6 & ~chain_parts, false, bt));
    float* wts = out->weights ? out->weights + ray0 * S : h.fth;
    NL_TRY(nl_launch_composite(z, h.sigma, h.rgb_s, nullptr, valid_s, R, S, W, white, out, ray0, nullptr, h.wsum, x.st, nullptr, out->weights ? nullptr : h.fth));
    // ... and applies feat_mlp.2 to the rows it has summed (the per-ray GEMM below: 33 us whatever the batch, 3 % of a 512-ray shard's step)
    const bool f2 = x.L.g[G_FEAT2].Npad <= 192;
    NL_TRY(nl_launch_feat_comp_mx(FA, wts, N, S, x.pk + x.L.bsh[G_FEAT0P], x.pk + x.L.mx_feat0, x.p<float>(x.L.bias[G_FEAT0P]), h.hc, x.st,
                                  f2 ? x.p<float>(x.L.b32[G_FEAT2]) : nullptr, x.L.g[G_FEAT2].Npad, C, h.wsum, out->feat + ray0 * C, fa_f16));
    feat_done = f2;
  } else {
  if (!pre_done) NL_TRY(do_heads_pre(x, V, FA, bl1, rgbv, N, want_feat, h, 7 & ~chain_parts, term, bt));   // chain_parts: what the chain kernel already produced
  NL_TRY(nl_launch_composite(z, h.sigma, h.rgb_s, want_feat ? h.fth : nullptr, valid_s, R, S, W, white, out, ray0,
                             want_feat ? h.hc : nullptr, want_feat ? h.wsum : nullptr, x.st, term ? h.n_alive : nullptr));
  }
  if (want_feat && !feat_done) {   // feat = W2 . (sum_s w_s hidden_s) + b2 * sum_s w_s  ==  sum_s w_s (W2 . hidden_s + b2)
    SegSpec s1[2] = {{h.hc, W, W, 0, 1}, {h.wsum, 1, 1, 0, 1}};
    NL_TRY(run_gemm(x, G_FEAT2, s1, 2, R, out->feat + ray0 * C, C, NL_ACT_NONE));
  }
  if (out->sigma) NL_CHECK_HIP(hipMemcpyAsync(out->sigma + ray0 * S, h.sigma, sizeof(float) * N, hipMemcpyDeviceToDevice, x.st));
  return NL_OK;
}

// ---- fused path ---------------------------------------------------------------------------------------------
static size_t render_bytes(const nl_config* cfg, int V, int64_t rc) {
  Bump b{nullptr, 0}; RenderBufs rb; carve_render(b, cfg, V, rc, rb); return b.off;
}

// exactness order of the precision modes (the enum's numbers are historical): BF16 < F16MX < BF16X3 < F32
int prec_rank(int p) { return p == NL_PREC_BF16 ? 0 : p == NL_PREC_F16MX ? 1 : p == NL_PREC_BF16X3 ? 2 : 3; }
// the |attention logit| up to which a mode stayed within 1e-4 of the CPU oracle on every scene of tools/scale_sweep.py; <= 0: no limit known
float guard_limit(int p) { return p == NL_PREC_F16MX ? NL_GUARD_LOGIT_LIMIT_F16MX : p == NL_PREC_BF16X3 ? NL_GUARD_LOGIT_LIMIT_BF16X3 : 0.f; }
// the density up to which a mode stayed within 1e-4 of the CPU oracle on the scenes with surfaces of tests/test_gpu_surfaces.py: the density head
// multiplies the error geo carries by its gain
// (bf16x3 met the bar on every one of those scenes, densities up to 61: it has no density limit.)  <= 0: no limit
float guard_density_limit(int p) { return p == NL_PREC_F16MX ? NL_GUARD_DENSITY_LIMIT_F16MX : 0.f; }
int guard_safer(int p) { return p == NL_PREC_F16MX ? NL_PREC_BF16X3 : NL_PREC_F32; }

int render_rays_impl(const nl_config* cfg, const void* packed, const nl_frame* f, const float* qc, const float* rays_o,
                     const float* rays_d, const float* z_vals, int64_t R, int white, const nl_render_out* out, void* ws,
                     size_t ws_bytes, void* stream, const nl_render_opts* opts) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  const float term_eps = opts ? opts->early_term_eps : 0.f;
  if (!(term_eps >= 0.f && term_eps < 1.f)) return NL_ERR_BAD_ARG;   // (written so that NaN is rejected)
  if (opts) {   // fields without a meaning in this ABI version must be zero, so that a later version can give them one
    if (opts->flags & ~(uint32_t)NL_RENDER_FLAGS_ALL) return NL_ERR_BAD_ARG;
    for (int i = 0; i < 4; ++i) if (opts->reserved[i] != 0) return NL_ERR_BAD_ARG;
  }
  const uint32_t flags = opts ? opts->flags : 0u;
  const float* ray_centers = opts ? opts->ray_centers : nullptr;
  if (!cfg_ok(cfg) || !packed || !f || (!qc && !ray_centers) || !rays_o || !rays_d || !out || !ws || R < 0) return NL_ERR_BAD_ARG;
  const int V = f->views.V, S = cfg->S, W = cfg->W;
  // largest ray chunk whose buffers fit the workspace
  int64_t RC = largest_chunk(R > 1 ? R : 1, ws_bytes, [&](int64_t r) { return render_bytes(cfg, V, r); });
  if (RC == 0) return NL_ERR_WORKSPACE;
  {   // the buffer-addressed kernels use 32-bit byte offsets: at most 2^21 samples per chunk (twice the recommended workspace's chunk)
    const int64_t cap = ((int64_t)1 << 21) / S > 0 ? ((int64_t)1 << 21) / S : 1;
    if (RC > cap) RC = cap;
  }
  Bump b{(char*)ws, 0}; RenderBufs rb; carve_render(b, cfg, V, RC, rb);
  Ctx x = make_ctx(cfg, packed, stream);
  x.mx = nl_mx_;
  const bool fork = f->side_ok && !(flags & NL_RENDER_NO_SIDE_STREAM) && nl_point_fused_supported(W, cfg->precision);
  for (int64_t r0 = 0; r0 < R; r0 += RC) {
    const int64_t rc = (R - r0 < RC) ? R - r0 : RC;
    const int64_t N = rc * S;
    NL_TRY(nl_launch_sample_points(rays_o + 3 * r0, rays_d + 3 * r0, rc, S, f->views.near_, f->views.far_,
                                   z_vals ? z_vals + r0 * S : nullptr, rb.z, rb.xyz, x.st));
    // ---- fork: exact KNN + aggregation scale on the frame's side stream, beside the multi-view gather kernels (both need xyz only).
    // `knn` joins in do_point before the neural-point kernel — or in its destructor on any earlier exit from this iteration.
    SideJoin knn;
    if (fork) {
      NL_CHECK_HIP(hipEventRecord(f->ev_fork, x.st));
      NL_CHECK_HIP(hipStreamWaitEvent(f->side, f->ev_fork, 0));
      knn.arm(x.st, f->side, f->ev_join);
      NL_TRY(nl_knn_search(&f->grid, rb.xyz, N, 8, rb.pt.idx, rb.pt.d2, f->side));
      NL_TRY(nl_launch_wscale(rb.pt.idx, rb.pt.d2, f->sp_conf, N, 8, f->M, rb.pt.wscale, f->side));
    }
    // the chain kernels recompute the multiview feature rows G (N x W) from out_fc's 64-wide hidden rows: G is only materialised for
    // the stage output or when the separate launches run instead
    const bool use_chain = W == 256 && cfg->precision != NL_PREC_F32 && N * 1024 <= 0x7fffffffll &&
                           nl_point_fused_supported(W, cfg->precision);
    const bool front = front_path(cfg, V) && f->C == cfg->C && nl_mv_front_supported(f->C, V, N) && rb.bl1 == nullptr;
    NL_TRY(do_mv(x, f, qc, rb.xyz, N, rb.G, nullptr, nullptr, rb.valid_s, front ? nullptr : rb.bl1, rb.rgbv, rb.mv, use_chain && !out->mv_feature_agg,
                 ray_centers ? ray_centers + 3 * r0 : nullptr, S, front));
    BlendTaps bt{with_query(f, qc, ray_centers ? ray_centers + 3 * r0 : nullptr, S), f->views_dev, f->pfeat, rb.xyz};
    // per-sample viewing direction = its ray's direction (model.py:501-504): row = sample / S
    // with early termination feat_mlp.0 runs later, over the live tiles only; otherwise the chain kernel produces it right here
    bool chain_done = false;
    const bool want_feat = out->feat != nullptr;
    // feature_agg has two consumers left on this path — conv1 and conv_out, three taps each: the chain kernel hands it over as the split-bf16 fragments it
    // holds anyway (same bytes in the same buffer) unless someone wants the fp32 rows: the stage output, or feat_mlp.0 over the live tiles of an early-terminated batch
    const bool fa_frag = use_chain && (N & 31) == 0 && !out->feature_agg && !(want_feat && term_eps > 0.f);
    // f16mx: feat_mlp.0 leaves the chain kernel — it runs after the density, fused with the compositing of its rows (do_heads: feat_late)
    // (the kernel reads the samples' weights as 16-byte rows: a caller's `weights` buffer that is not 16-byte aligned keeps the old path — no alignment was ever asked of it)
    const bool feat_late = want_feat && term_eps == 0.f && fa_frag && x.mx && ((x.has_bsh >> G_FEAT0P) & 1) && nl_feat_comp_mx_supported(W, S, N) &&
                           (((size_t)out->weights) & 15) == 0;
    // split-FP16 fragments where EVERY consumer of the image multiplies in fp16-based arithmetic: conv1 -> tgemm_conv1_kernel<true, true>, conv_out -> tgemm_mx_kernel,
    // feat_mlp.0 -> feat_comp_mx_kernel (or nobody), the blend projection inside the chain kernel on its fp16 stream (W = 256, S = 128, f16mx)
    const bool fa_f16 = fa_frag && x.mx && W == 256 && S == 128 && (!want_feat || feat_late) && ((x.has_bsh >> G_CONV1F) & 1) && ((x.has_bsh >> G_CONVOUTF) & 1) &&
                        ((x.has_bsh >> G_BLENDAP) & 1);
    const ChainOut chain{(want_feat && term_eps == 0.f && !feat_late) ? rb.hd.fth : nullptr, rb.hd.blA, &chain_done, use_chain ? rb.mv.t64 : nullptr, fa_frag, fa_f16};
    NL_TRY(do_point(x, f, rb.xyz, rays_d + 3 * r0, 3, S, rb.G, N, 8, rb.FA, rb.pt, fork ? &knn : nullptr, &chain));
    const int chain_parts = chain_done ? ((want_feat && term_eps == 0.f && !feat_late ? 1 : 0) | 2) : 0;
    bool have_sigma = false;
    NL_TRY(do_unet(x, rb.FA, rc, rb.geo, rb.un, rb.hd.sigma, &have_sigma, out->geo != nullptr, fa_frag ? (fa_f16 ? 3 : 1) : 0, true));
    // (The colour-blend taps on the frame's side stream beside the ray U-Net's kernels — they need the chain kernel's projection rows, not the density — built and
    // traced: conv1 stretches by what the taps take (conv1 399 us with the taps' 369 us inside it = a 403-us span against 192 + 222 us one after the other;
    // profiles/r6_blend_side_stream.txt).  Not kept.)
    NL_TRY(do_heads(x, V, rb.z, rb.FA, rb.geo, front ? nullptr : rb.bl1, rb.rgbv, rb.valid_s, rc, white, out, r0, rb.hd, have_sigma, false, term_eps, chain_parts, &bt,
                    feat_late && chain_done, fa_f16, (flags & NL_RENDER_PRECISION_GUARD) ? reinterpret_cast<unsigned*>(f->views_dev + 254) : nullptr));
    if (out->feature_agg) NL_CHECK_HIP(hipMemcpyAsync(out->feature_agg + r0 * S * W, rb.FA, sizeof(float) * N * W, hipMemcpyDeviceToDevice, x.st));
    if (out->mv_feature_agg) NL_CHECK_HIP(hipMemcpyAsync(out->mv_feature_agg + r0 * S * W, rb.G, sizeof(float) * N * W, hipMemcpyDeviceToDevice, x.st));
    if (out->geo) NL_CHECK_HIP(hipMemcpyAsync(out->geo + r0 * S * W, rb.geo, sizeof(float) * N * W, hipMemcpyDeviceToDevice, x.st));
    if (out->knn_idx) NL_CHECK_HIP(hipMemcpyAsync(out->knn_idx + r0 * S * 8, rb.pt.idx, sizeof(int) * N * 8, hipMemcpyDeviceToDevice, x.st));
    if (out->knn_d2) NL_CHECK_HIP(hipMemcpyAsync(out->knn_d2 + r0 * S * 8, rb.pt.d2, sizeof(float) * N * 8, hipMemcpyDeviceToDevice, x.st));
  }
  return NL_OK;
}

// ---- several frames per call: fork / join over library-owned streams -----------------------------------------------------------------------
// One pool of lane streams / events PER DEVICE (keyed by hipGetDevice(): streams and events belong to the device that was current when they were
// created — a process that renders on cuda:0 and later on cuda:1 must not launch cuda:1's work on cuda:0's streams)
struct MultiPool { std::vector<hipStream_t> st; std::vector<hipEvent_t> ev; hipEvent_t fork = nullptr; };
std::mutex g_multi_mu;
std::unordered_map<int, MultiPool> g_multi;

}  // namespace

extern "C" {

// ---- stages ----------------------------------------------------------------------------------------------
int nl_knn(const nl_frame* f, const float* xyz, int64_t N, int K, int32_t* idx, float* d2, void* stream) {
  if (N == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (!f || !xyz || !idx || !d2 || N < 0 || K < 1 || K > NL_KNN_MAX_K) return NL_ERR_BAD_ARG;
  return nl_knn_search(&f->grid, xyz, N, K, idx, d2, (hipStream_t)stream);
}

int nl_sample_points(const float* o, const float* d, int64_t R, int S, float near_, float far_, const float* z_in, float* z_out,
                     float* xyz, void* stream) {
  if (R == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (!o || !d || !xyz || R < 0 || S < 1) return NL_ERR_BAD_ARG;
  return nl_launch_sample_points(o, d, R, S, near_, far_, z_in, z_out, xyz, (hipStream_t)stream);
}

size_t nl_mv_aggregate_workspace_bytes(const nl_config* cfg, int V, int64_t N) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  Bump b{nullptr, 0}; MvBufs m; carve_mv(b, cfg, V, N, m); return b.off;
}

int nl_mv_aggregate(const nl_config* cfg, const void* packed, const nl_frame* f, const float* qc, const float* xyz, int64_t N,
                    float* mv_feat, float* rgb_feat, float* vis_ang, int32_t* valid_s, float* blend1, float* rgbv, void* ws,
                    size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (N == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (!cfg_ok(cfg) || !packed || !f || !xyz || !mv_feat || !valid_s || !ws || N < 0 || (blend1 && !rgbv)) return NL_ERR_BAD_ARG;
  if (ws_bytes < nl_mv_aggregate_workspace_bytes(cfg, f->views.V, N)) return NL_ERR_WORKSPACE;
  Bump b{(char*)ws, 0}; MvBufs m; carve_mv(b, cfg, f->views.V, N, m);
  Ctx x = make_ctx(cfg, packed, stream);
  return do_mv(x, f, qc, xyz, N, mv_feat, rgb_feat, vis_ang, valid_s, blend1, rgbv, m);
}

size_t nl_point_mlp_workspace_bytes(const nl_config* cfg, int64_t N) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  Bump b{nullptr, 0}; PtBufs p; carve_pt(b, cfg, N, 8, p, true); return b.off;
}

int nl_point_mlp(const nl_config* cfg, const void* packed, const nl_frame* f, const float* xyz, const float* dir, int64_t dir_stride,
                 const float* mv_feat, int64_t N, int K, float* feature_agg, int32_t* knn_idx, float* knn_d2, void* ws, size_t ws_bytes,
                 void* stream) {
  NL_EFF_CFG(cfg);
  if (N == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (!cfg_ok(cfg) || !packed || !f || !xyz || !mv_feat || !feature_agg || !ws || N < 0 || K < 1 || K > 8) return NL_ERR_BAD_ARG;
  if (ws_bytes < nl_point_mlp_workspace_bytes(cfg, N)) return NL_ERR_WORKSPACE;
  Bump b{(char*)ws, 0}; PtBufs p; carve_pt(b, cfg, N, 8, p, true);
  Ctx x = make_ctx(cfg, packed, stream);
  NL_TRY(do_point(x, f, xyz, dir, (int)dir_stride, 1, mv_feat, N, K, feature_agg, p));
  if (knn_idx) NL_CHECK_HIP(hipMemcpyAsync(knn_idx, p.idx, sizeof(int) * N * K, hipMemcpyDeviceToDevice, x.st));
  if (knn_d2) NL_CHECK_HIP(hipMemcpyAsync(knn_d2, p.d2, sizeof(float) * N * K, hipMemcpyDeviceToDevice, x.st));
  return NL_OK;
}

size_t nl_ray_unet_workspace_bytes(const nl_config* cfg, int64_t R) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  Bump b{nullptr, 0}; UnBufs u; carve_un(b, cfg, R, u); return b.off;
}

int nl_ray_unet(const nl_config* cfg, const void* packed, const float* xin, int64_t R, float* geo, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (!cfg_ok(cfg) || !packed || !xin || !geo || !ws || R < 0) return NL_ERR_BAD_ARG;
  if (ws_bytes < nl_ray_unet_workspace_bytes(cfg, R)) return NL_ERR_WORKSPACE;
  Bump b{(char*)ws, 0}; UnBufs u; carve_un(b, cfg, R, u);
  Ctx x = make_ctx(cfg, packed, stream);
  return do_unet(x, xin, R, geo, u);
}

size_t nl_heads_composite_workspace_bytes(const nl_config* cfg, int V, int64_t R) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  Bump b{nullptr, 0}; HdBufs h; carve_hd(b, cfg, V, R, h); return b.off;
}

int nl_heads_composite(const nl_config* cfg, const void* packed, int V, const float* z, const float* FA, const float* geo,
                       const float* blend1, const float* rgbv, const int32_t* valid_s, int64_t R, int white,
                       const nl_render_out* out, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (cfg && cfg->S > 256 && cfg->S % 8 == 0) return NL_ERR_UNSUPPORTED;   // composite_kernel holds a ray in one wave, four samples per lane at the most: nothing is launched beyond that
  if (!cfg_ok(cfg) || !packed || !z || !FA || !geo || !blend1 || !rgbv || !out || !ws || R < 0 || V < 1 || V > NL_MAX_VIEWS) return NL_ERR_BAD_ARG;
  if (ws_bytes < nl_heads_composite_workspace_bytes(cfg, V, R)) return NL_ERR_WORKSPACE;
  Bump b{(char*)ws, 0}; HdBufs h; carve_hd(b, cfg, V, R, h);
  Ctx x = make_ctx(cfg, packed, stream);
  return do_heads(x, V, z, FA, geo, blend1, rgbv, valid_s, R, white, out, 0, h);
}

size_t nl_render_rays_min_workspace_bytes(const nl_config* cfg, int V) {
  NL_EFF_CFG(cfg); return cfg_ok(cfg) ? render_bytes(cfg, V, 1) : 0; }

size_t nl_render_rays_workspace_bytes(const nl_config* cfg, int V, int64_t R) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  int64_t rc = R < 1 ? 1 : R;
  const int64_t cap = (1 << 20) / cfg->S > 0 ? (1 << 20) / cfg->S : 1;  // ~1M samples per chunk (~12 GB of workspace at W=256, V=10): small grids in the U-Net fill the chip only at this size
  if (rc > cap) rc = cap;
  return render_bytes(cfg, V, rc);
}

int nl_render_rays(const nl_config* cfg, const void* packed, const nl_frame* f, const float* qc, const float* rays_o,
                   const float* rays_d, const float* z_vals, int64_t R, int white, const nl_render_out* out, void* ws,
                   size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  return nl_render_rays_ex(cfg, packed, f, qc, rays_o, rays_d, z_vals, R, white, out, ws, ws_bytes, stream, nullptr);
}

int nl_render_rays_ex(const nl_config* cfg, const void* packed, const nl_frame* f, const float* qc, const float* rays_o,
                      const float* rays_d, const float* z_vals, int64_t R, int white, const nl_render_out* out, void* ws,
                      size_t ws_bytes, void* stream, const nl_render_opts* opts) {
  if (!opts || !(opts->flags & NL_RENDER_PRECISION_GUARD) || !cfg || !f || R <= 0)
    return render_rays_impl(cfg, packed, f, qc, rays_o, rays_d, z_vals, R, white, out, ws, ws_bytes, stream, opts);
  // ---- NL_RENDER_PRECISION_GUARD: render, read the frame's two conditioning indicators (largest |attention logit|, largest density: one 24-byte copy + a stream
  // synchronisation), and while one is beyond the validated range of the mode the outputs were produced in, render THIS batch again in the next more exact mode.
  // Both are running maxima over the frame's life, and the frame stays in that mode for every later guarded call (a frame whose attention logits or densities are
  // large once has them large in every batch), so the extra pass is paid once per frame.
  nl_config c = *cfg;
  if (f->guard_prec >= 0 && prec_rank(f->guard_prec) > prec_rank(c.precision)) c.precision = f->guard_prec;
  for (;;) {
    const int rc = render_rays_impl(&c, packed, f, qc, rays_o, rays_d, z_vals, R, white, out, ws, ws_bytes, stream, opts);
    if (rc != NL_OK) return rc;
    f->guard_last_prec = c.precision;
    const float limit = guard_limit(c.precision);
    if (limit <= 0.f) return NL_OK;
    float diag[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};   // floats 249 .. 254: [0] max |attention logit|, [5] max density
    NL_CHECK_HIP(hipMemcpyAsync(diag, f->views_dev + 249, sizeof(diag), hipMemcpyDeviceToHost, (hipStream_t)stream));
    NL_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
    const float dlimit = guard_density_limit(c.precision);
    if (diag[0] <= limit && (dlimit <= 0.f ? diag[5] == diag[5] : diag[5] <= dlimit)) return NL_OK;   // (a NaN logit is recorded as +inf, a NaN density as itself: both escalate)
    c.precision = guard_safer(c.precision);
    f->guard_prec = c.precision;
    ++f->guard_escalations;
  }
}

int nl_render_rays_multi(const nl_config* cfg, const void* packed, const nl_render_job* jobs, int32_t njobs, int32_t white, void* stream) {
  if (njobs == 0) return NL_OK;
  if (!cfg || !packed || !jobs || njobs < 0) return NL_ERR_BAD_ARG;
  for (int i = 0; i < njobs; ++i) if (!jobs[i].frame || !jobs[i].out || !jobs[i].ws) return NL_ERR_BAD_ARG;
  if (njobs == 1) return nl_render_rays_ex(cfg, packed, jobs[0].frame, jobs[0].query_center, jobs[0].rays_o, jobs[0].rays_d, jobs[0].z_vals, jobs[0].R, white,
                                           jobs[0].out, jobs[0].ws, jobs[0].ws_bytes, stream, jobs[0].opts);
  // the precision guard synchronises its stream after every job: with concurrent lanes it would serialise them — callers check nl_frame_diagnostics per frame instead
  for (int i = 0; i < njobs; ++i) if (jobs[i].opts && (jobs[i].opts->flags & NL_RENDER_PRECISION_GUARD)) return NL_ERR_BAD_ARG;
  // a lane (stream) per distinct frame: a frame's side stream and events serve one render call at a time
  std::vector<int> lane_of(njobs);
  std::vector<const nl_frame*> lanes;
  for (int i = 0; i < njobs; ++i) {
    int l = -1;
    for (size_t k = 0; k < lanes.size(); ++k) if (lanes[k] == jobs[i].frame) { l = (int)k; break; }
    if (l < 0) { l = (int)lanes.size(); lanes.push_back(jobs[i].frame); }
    lane_of[i] = l;
  }
  // jobs on DIFFERENT lanes run concurrently: their workspaces must not overlap (jobs of one lane run one after the other and may share one)
  for (int i = 0; i < njobs; ++i)
    for (int k = i + 1; k < njobs; ++k) {
      if (lane_of[i] == lane_of[k]) continue;
      const char *a0 = (const char*)jobs[i].ws, *a1 = a0 + jobs[i].ws_bytes, *b0 = (const char*)jobs[k].ws, *b1 = b0 + jobs[k].ws_bytes;
      if (a0 < b1 && b0 < a1) return NL_ERR_BAD_ARG;
    }
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return NL_ERR_HIP;
  std::lock_guard<std::mutex> lk(g_multi_mu);
  MultiPool& mp = g_multi[dev];
  while (mp.st.size() < lanes.size()) {
    hipStream_t s; hipEvent_t e;
    if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) return NL_ERR_HIP;
    mp.st.push_back(s); mp.ev.push_back(e);
  }
  if (!mp.fork && hipEventCreateWithFlags(&mp.fork, hipEventDisableTiming) != hipSuccess) return NL_ERR_HIP;
  hipStream_t main = (hipStream_t)stream;
  NL_CHECK_HIP(hipEventRecord(mp.fork, main));
  for (size_t k = 0; k < lanes.size(); ++k) NL_CHECK_HIP(hipStreamWaitEvent(mp.st[k], mp.fork, 0));
  int rc = NL_OK;
  for (int i = 0; i < njobs && rc == NL_OK; ++i)
    rc = nl_render_rays_ex(cfg, packed, jobs[i].frame, jobs[i].query_center, jobs[i].rays_o, jobs[i].rays_d, jobs[i].z_vals, jobs[i].R, white, jobs[i].out,
                           jobs[i].ws, jobs[i].ws_bytes, mp.st[lane_of[i]], jobs[i].opts);
  // join unconditionally: whatever was enqueued must be ordered before the caller's next work (and an active capture must stay well-formed)
  for (size_t k = 0; k < lanes.size(); ++k) {
    if (hipEventRecord(mp.ev[k], mp.st[k]) != hipSuccess || hipStreamWaitEvent(main, mp.ev[k], 0) != hipSuccess) rc = rc == NL_OK ? NL_ERR_HIP : rc;
  }
  return rc;
}

size_t nl_coarse_weights_workspace_bytes(int V, int64_t R, int Sc) {
  return 3 * nl_align_up((size_t)(V > 0 ? V : 1) * (R > 0 ? R : 1) * (Sc > 0 ? Sc : 1) * 4, 256);
}

int nl_coarse_weights(const nl_config* cfg, const void* packed, const nl_frame* f, const float* w2c_kinv, const float* pix,
                      const float* zc, int64_t R, int Sc, float* weights, float* depth_coarse, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (!cfg_ok(cfg) || !packed || !f || !w2c_kinv || !pix || !zc || !weights || !ws || R < 0) return NL_ERR_BAD_ARG;
  if (Sc < 3) return NL_ERR_BAD_ARG;           // the resampling drops both ends of a row: fewer than 3 samples leave no bin
  if (Sc > 64) return NL_ERR_UNSUPPORTED;      // coarse_ray_kernel: one sample per lane
  if (ws_bytes < nl_coarse_weights_workspace_bytes(f->views.V, R, Sc)) return NL_ERR_WORKSPACE;
  const size_t part = nl_align_up((size_t)f->views.V * R * Sc * 4, 256);
  float* wa = (float*)ws; float* wv = (float*)((char*)ws + part); float* wm = (float*)((char*)ws + 2 * part);
  const Layout L = make_layout(cfg);
  return nl_launch_coarse_weights(f->views, w2c_kinv, f->visf_hwc, (const float*)((const char*)packed + L.dec_w), (const char*)packed + L.dec_mfma,
                                  cfg->precision, pix, zc, R, Sc, wa, wv, wm, weights, depth_coarse, (hipStream_t)stream);
}

int nl_sample_pdf(const float* zc, const float* wc, int Sc, const float* u, int Ni, const float* zb, int Sb, int64_t R, float* z_out,
                  void* stream) {
  if (R == 0) return NL_OK;   // empty batch: nothing to do, data pointers may be null
  if (!zc || !wc || !u || !zb || !z_out || R < 0) return NL_ERR_BAD_ARG;
  // before any launch: sample_pdf_kernel writes s_sort[Sb + i], a negative Sb would land below the array
  if (Sb < 0 || Ni < 1 || (int64_t)Sb + Ni < 1 || Sc < 3) return NL_ERR_BAD_ARG;
  if ((int64_t)Sb + Ni > 256 || Sc > 64) return NL_ERR_UNSUPPORTED;   // one wave sorts a ray's 256 keys in LDS; one coarse sample per lane
  return nl_launch_sample_pdf(zc, wc, Sc, u, Ni, zb, Sb, R, z_out, (hipStream_t)stream);
}

}  // extern "C"
