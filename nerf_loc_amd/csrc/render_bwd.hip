// Everything of libnerfloc_render.so that exists for gradients: the stage backwards (neural-point branch, multi-view aggregation, colour blend, ray U-Net),
// the whole ray path backwards, and the training entry points that add weight gradients.  The forward path: render.hip.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
#include "host.h"
using namespace nlhost;

namespace {

// ---- input gradient of the neural-point branch (frozen weights) ---------------------------------------------------------------------
// gW[tw] += dY^T X (and gb[tb] += column sums of dY) for whichever of the two the caller asked for
int wgrad_to(const TrainOut* tg, hipStream_t st, int tw, int tb, const float* dY, int ldy, int Mo, const float* X, int ldxx, int Ni, int64_t rows) {
  if (!tg || (!tg->w[tw] && (tb < 0 || !tg->w[tb]))) return NL_OK;
  if (!tg->w[tw]) return nl_launch_colsum(dY, ldy, rows, Mo, tg->w[tb], tg->scratch, st);
  return nl_launch_wgrad(dY, ldy, Mo, X, ldxx, Ni, rows, 0, 0, tg->w[tw], Ni, 1, 0, tb >= 0 ? tg->w[tb] : nullptr, tg->scratch, tg->scratch_floats, st);
}
void carve_ptb(Bump& b, const nl_config* c, int64_t N, int K, PtBwdBufs& p, bool train = false) {
  const int W = c->W;
  const size_t NK = (size_t)N * K;
  p.idx = b.take<int>(NK); p.d2 = b.take<float>(NK);
  p.X = b.take<float>(NK * ldx_of(c->C));
  p.H1 = b.take<float>(NK * W); p.H2 = b.take<float>(NK * W); p.H3 = b.take<float>(NK * W);
  p.KV = b.take<float>(NK * 256);
  p.Q = b.take<float>((size_t)N * 128); p.O = b.take<float>((size_t)N * 128); p.FCo = b.take<float>((size_t)N * W); p.wscale = b.take<float>((size_t)N);
  p.gpre = b.take<float>((size_t)N * W); p.gO = b.take<float>((size_t)N * 128); p.gQ = b.take<float>((size_t)N * 128);
  p.gKV = b.take<float>(NK * 256); p.gA = b.take<float>(NK * W); p.gB = b.take<float>(NK * W); p.gX = b.take<float>(NK * 96);
  for (int i = 0; i < 3; ++i) p.mk[i] = b.take<unsigned>((NK / 32 + 8) * 256);   // LeakyReLU sign bits of the three base_mlp layers: 32 bytes per row
  p.aff = p.tr = p.gXF = nullptr;
  if (train) {
    p.aff = b.take<float>((size_t)N * 2 * W); p.tr = b.take<float>(NK * 68);
    if (c->precision == NL_PREC_F32) p.gXF = b.take<float>(NK * ldf_of(c->C));   // (otherwise the support features' gradient goes through the table: pt_backward_only)
  }
}

// dX = (dY . W) * LeakyReLU'(h): the mask inside the streaming GEMM's epilogue where that kernel runs, a separate pass otherwise (fp32 mode)
// the layers' sign bits exist when the forward layers ran on the streaming kernel (every mode but fp32: pt_forward_staged checks it)
inline bool pt_mask_bits(const Ctx& x) { return x.c->precision != NL_PREC_F32; }
inline bool pt_table(const Ctx& x) { return x.c->precision != NL_PREC_F32; }   // base_mlp.0 through the per-frame table (pt_forward_staged)
int gemm_lrelu_masked(const Ctx& x, int g, const SegSpec& s, int64_t M, float* out, int ld, const float* h, const unsigned* bits = nullptr) {
  if (x.c->precision != NL_PREC_F32 && (s.k & 31) == 0 && (((size_t)s.ptr) & 15) == 0 && (s.ld & 3) == 0 && (ld & 3) == 0 && (((size_t)h) & 15) == 0 && x.L.g[g].N <= 256) {
    RowEpi ep{h, ld, nullptr, nullptr, nullptr, 0.f, out, NL_EPI_NONE};
    ep.maskin = bits;
    bool streamed = false;
    NL_TRY(run_gemm(x, g, &s, 1, M, out, ld, NL_ACT_LRELU_MASK, 0, 0, 0, 1, 0, &ep, &streamed));
    return streamed ? NL_OK : NL_ERR_UNSUPPORTED;   // (the generic kernels do not know this activation)
  }
  NL_TRY(run_gemm(x, g, &s, 1, M, out, ld, NL_ACT_NONE));
  return nl_launch_lrelu_mask(out, h, (size_t)M * ld, x.st);
}

// Re-runs the staged forward (point.hip kernels + segment GEMMs in the configured precision) into the workspace, then walks back:
// g_FA -> LayerNorm/scale -> {residual -> g_G ; fc^T -> attention -> {w_qs^T -> g_G ; [w_ks; w_vs]^T -> base_mlp^T x 3 with LeakyReLU masks ->
// posenc / ray_diff_fc -> g_xyz, g_dir}}.  The aggregation scale sum_k w_k is a constant of the backward pass: it is identically 1 (or 0)
// whatever the distances are (model.py:419-427 normalises the weights; the K rows they multiply are identical, see point.hip).
// the staged forward of the branch into the workspace (everything the way back reads); dir: one row per dir_div samples
int pt_forward_staged(const Ctx& x, const nl_frame* f, const float* xyz, const float* dir, int dir_stride, int dir_div, const float* G, int64_t N, int K,
                      const PtBwdBufs& p, const int* idx_in, const float* d2_in) {
  const int W = x.c->W, F = f->C + 3, ldx = ldx_of(f->C);
  const int64_t NK = N * K;
  const float inv_span = 1.f / (f->views.far_ - f->views.near_);
  const int64_t M = f->M;
  const int* idx = idx_in && d2_in ? idx_in : p.idx;
  const float* d2 = idx_in && d2_in ? d2_in : p.d2;
  if (idx == p.idx) NL_TRY(nl_knn_search(&f->grid, xyz, N, K, p.idx, p.d2, x.st));   // (the caller may hand over the forward call's neighbours)
  // every mode but fp32: base_mlp.0 on the per-frame table T like the fused kernel — the encoded rows are the 96 posenc + ray_diff_fc columns only (the 195
  // gathered feature columns per row are never written: 400 MB per 65 k samples), the layer's K is 96 instead of 288, and its epilogue adds T[neighbour]
  const bool tab = pt_table(x);
  if (tab) NL_TRY(ensure_ptt(x, f));
  NL_TRY(nl_launch_point_encode(xyz, dir, dir_stride, dir_div, N, K, M, idx, d2, f->sp_xyz, f->sp_feat, tab ? 0 : F, f->sp_conf, f->sp_dir, x.p<float>(x.L.rd_w),
                                inv_span, p.X, tab ? 96 : ldx, p.wscale, x.st));
  // (the encoded rows' pad columns are zero and so are the weights' pad rows: taking all ldx columns keeps the streaming kernel applicable)
  SegSpec sx{p.X, ldx, ldx, 0, 1}, s1{p.H1, W, W, 0, 1}, s2{p.H2, W, W, 0, 1}, s3{p.H3, W, W, 0, 1}, sg{G, W, W, 0, 1}, so{p.O, 128, 128, 0, 1};
  if (tab) sx = SegSpec{p.X, 96, 96, 0, 1};
  if (pt_mask_bits(x)) {   // the layers also leave their outputs' signs as bits: the way back reads 32 bytes per row instead of the 1 KB activation row
    const int gs[3] = {tab ? G_BASE0_S : G_BASE0, G_BASE2, G_BASE4};
    const SegSpec* ss[3] = {&sx, &s1, &s2};
    float* hs[3] = {p.H1, p.H2, p.H3};
    for (int i = 0; i < 3; ++i) {
      RowEpi ep{nullptr, 0, nullptr, nullptr, nullptr, 0.f, hs[i], NL_EPI_NONE};
      ep.maskout = p.mk[i];
      if (i == 0 && tab) { ep.tab = f->ptt; ep.tabidx = idx; ep.ldtab = W; ep.tabK = K; ep.tabM = (int)(M > 0x7fffffff ? 0x7fffffff : M); }
      bool streamed = false;
      NL_TRY(run_gemm(x, gs[i], ss[i], 1, NK, hs[i], W, NL_ACT_LRELU, 0, 0, 0, 1, 0, &ep, &streamed));
      if (!streamed) return NL_ERR_UNSUPPORTED;
    }
  } else {
    NL_TRY(run_gemm(x, G_BASE0, &sx, 1, NK, p.H1, W, NL_ACT_LRELU));
    NL_TRY(run_gemm(x, G_BASE2, &s1, 1, NK, p.H2, W, NL_ACT_LRELU));
    NL_TRY(run_gemm(x, G_BASE4, &s2, 1, NK, p.H3, W, NL_ACT_LRELU));
  }
  NL_TRY(run_gemm(x, G_KV, &s3, 1, NK, p.KV, 256, NL_ACT_NONE));
  NL_TRY(run_gemm(x, G_Q, &sg, 1, N, p.Q, 128, NL_ACT_NONE));
  NL_TRY(nl_launch_attn(p.Q, p.KV, N, K, p.O, x.st));
  return run_gemm(x, G_FC, &so, 1, N, p.FCo, W, NL_ACT_NONE);
}
// Frozen weights (pose refinement: no weight gradient wants the layers' activations), W = 128 / 256, K = 8, non-fp32 modes: the branch's forward as ONE launch of the
// fused neural-point kernel in split-FP16 (point_fused2_kernel<NRT, true, false, F16, KEEP>) that also leaves the k / v rows and the three layers' sign bits — what
// pt_backward_only reads — instead of an encode kernel, four (N x 8)-row GEMMs through HBM and an attention kernel (round 4: 1.7 -> 0.6 ms of a 512-ray step).
bool pt_keep_fused_ok(const Ctx& x, const nl_frame* f, int64_t N, int K) {
  return K == 8 && x.c->precision == NL_PREC_F16X3_INTERNAL && nl_point_fused2_supported(x.c->W, NL_PREC_BF16X3) && f->M >= 1 &&
         N * 8 * 1024 <= 0x7fffffffll && ((int64_t)f->M + 1) * x.c->W * 4 <= 0x7fffffffll;
}
int pt_forward_keep_fused(const Ctx& x, const nl_frame* f, const float* xyz, const float* dir, int dir_stride, int dir_div, const float* G, int64_t N,
                          const PtBwdBufs& p, const int* idx_in, const float* d2_in) {
  const int W = x.c->W, K = 8;
  const int* idx = idx_in && d2_in ? idx_in : p.idx;
  const float* d2 = idx_in && d2_in ? d2_in : p.d2;
  if (idx == p.idx) NL_TRY(nl_knn_search(&f->grid, xyz, N, K, p.idx, p.d2, x.st));
  NL_TRY(ensure_ptt(x, f));
  NL_TRY(nl_launch_wscale(idx, d2, f->sp_conf, N, K, f->M, p.wscale, x.st));
  SegSpec sg{G, W, W, 0, 1}, so{p.O, 128, 128, 0, 1};
  NL_TRY(run_gemm(x, G_Q, &sg, 1, N, p.Q, 128, NL_ACT_NONE));
  NlPointFusedArgs a;
  memset(&a, 0, sizeof(a));
  a.xyz = xyz; a.dir = dir; a.dir_stride = dir_stride; a.dir_div = dir_div > 0 ? dir_div : 1;
  a.idx = idx; a.Q = p.Q; a.O = p.O; a.ptt = f->ptt; a.sp_xyz = f->sp_xyz; a.sp_dir = f->sp_dir;
  a.wstream = nullptr; a.bias = x.p<float>(x.L.pt_bias); a.rd_w = x.p<float>(x.L.rd_w);
  a.wstream2 = x.p<uint4>(x.L.pt_stream2_f16);
  a.N = (int)N; a.M = (int)(f->M > 0x7fffffff ? 0x7fffffff : f->M); a.inv_span = 1.f / (f->views.far_ - f->views.near_);
  unsigned* mk[3] = {p.mk[0], p.mk[1], p.mk[2]};
  NL_TRY(nl_launch_point_fused2(a, W, NL_PREC_BF16X3, x.st, false, p.KV, mk));
  return run_gemm(x, G_FC, &so, 1, N, p.FCo, W, NL_ACT_NONE);
}

int pt_backward_only(const Ctx& xb, const Ctx& x, const nl_frame* f, const float* xyz, const float* dir, int dir_stride, int dir_div, const float* G, int64_t N,
                     int K, const float* gFA, float* g_xyz, float* g_dir, float* g_G, const PtBwdBufs& p, const int* idx_in, const float* d2_in,
                     const TrainOut* tg) {
  const int W = x.c->W, F = f->C + 3, ldx = ldx_of(f->C);
  // training: gW += dY^T X right after each dY exists (its buffer is reused by the next layer's)
  auto wg = [&](int tw, int tb, const float* dY, int ldy, int Mo, const float* X, int ldxx, int Ni, int64_t rows) -> int {
    return wgrad_to(tg, x.st, tw, tb, dY, ldy, Mo, X, ldxx, Ni, rows);
  };
  const int64_t NK = N * K;
  const float inv_span = 1.f / (f->views.far_ - f->views.near_);
  const int64_t M = f->M;
  const int* idx = idx_in && d2_in ? idx_in : p.idx;
  const bool aff = tg && (tg->w[T_LNW] || tg->w[T_LNB]);
  NL_TRY(nl_launch_ln_agg_backward(p.FCo, G, gFA, N, W, x.p<float>(x.L.ln_g), 1e-6f, p.wscale, p.gpre, aff ? p.aff : nullptr, x.st));
  if (aff) {
    if (tg->w[T_LNW]) NL_TRY(nl_launch_colsum(p.aff, 2 * W, N, W, tg->w[T_LNW], tg->scratch, x.st));
    if (tg->w[T_LNB]) NL_TRY(nl_launch_colsum(p.aff + W, 2 * W, N, W, tg->w[T_LNB], tg->scratch, x.st));
  }
  NL_TRY(wg(T_FC, -1, p.gpre, W, W, p.O, 128, 128, N));
  SegSpec sp{p.gpre, W, W, 0, 1}, sgq{p.gQ, 128, 128, 0, 1}, skv{p.gKV, 256, 256, 0, 1}, sa{p.gA, W, W, 0, 1}, sb{p.gB, W, W, 0, 1};
  NL_TRY(run_gemm(xb, G_FC_T, &sp, 1, N, p.gO, 128, NL_ACT_NONE));
  // frozen weights, W = 128 / 256, K = 8: the attention's way back, the four (N x 8)-row products and the LeakyReLU masks in between as ONE launch that keeps the rows
  // in registers (point_bwd.hip); d query comes back from it
  const bool chain = !tg && K == 8 && pt_mask_bits(x) && pt_table(x) && nl_point_bwd_chain_supported(W) && NK * 1024 <= 0x7fffffffll;
  if (chain) {
    const unsigned* mk[3] = {p.mk[0], p.mk[1], p.mk[2]};
    NL_TRY(nl_launch_point_bwd_chain(nullptr, mk, x.p<char>(x.L.pt_bwd_stream), p.gX, NK, W, x.st, p.Q, p.KV, p.gO, p.gQ));
    if (g_G) {   // residual path + query projection
      NL_TRY(run_gemm(xb, G_Q_T, &sgq, 1, N, p.FCo, W, NL_ACT_NONE));   // (FCo is free from here on)
      NL_TRY(nl_launch_add(p.gpre, p.FCo, g_G, (size_t)N * W, x.st));
    }
    return nl_launch_point_encode_backward(xyz, dir, dir_stride, dir_div, N, K, M, idx, f->sp_xyz, f->sp_dir, x.p<float>(x.L.rd_w), inv_span, p.gX, 96, g_xyz, g_dir,
                                           nullptr, x.st);
  }
  NL_TRY(nl_launch_attn_backward(p.Q, p.KV, p.gO, N, K, p.gQ, p.gKV, x.st));
  NL_TRY(wg(T_WQ, -1, p.gQ, 128, 128, G, W, W, N));
  NL_TRY(wg(T_WK, -1, p.gKV, 256, 128, p.H3, W, W, NK));
  NL_TRY(wg(T_WV, -1, p.gKV + 128, 256, 128, p.H3, W, W, NK));
  if (g_G) {   // residual path + query projection
    NL_TRY(run_gemm(xb, G_Q_T, &sgq, 1, N, p.FCo, W, NL_ACT_NONE));   // (FCo is free from here on)
    NL_TRY(nl_launch_add(p.gpre, p.FCo, g_G, (size_t)N * W, x.st));
  }
  const bool bits = pt_mask_bits(x);
  NL_TRY(gemm_lrelu_masked(xb, G_KV_T, skv, NK, p.gA, W, p.H3, bits ? p.mk[2] : nullptr));
  NL_TRY(wg(T_B4W, T_B4B, p.gA, W, W, p.H2, W, W, NK));
  NL_TRY(gemm_lrelu_masked(xb, G_BASE4_T, sa, NK, p.gB, W, p.H2, bits ? p.mk[1] : nullptr));
  NL_TRY(wg(T_B2W, T_B2B, p.gB, W, W, p.H1, W, W, NK));
  NL_TRY(gemm_lrelu_masked(xb, G_BASE2_T, sb, NK, p.gA, W, p.H1, bits ? p.mk[0] : nullptr));
  const bool tab = pt_table(x);
  if (!tab) NL_TRY(wg(T_B0W, T_B0B, p.gA, W, W, p.X, ldx, F + 90, NK));
  else if (tg) {
    // base_mlp.0 on the table: its posenc / ray_diff_fc columns and the bias from the 96-wide rows; the feature columns and the support features through
    // d T = the rows' gradients summed per support point (M, W): d W[:, :F] = d T^T . sp_feature, d sp_feature = d T . W[:, :F]
    if (tg->w[T_B0W]) NL_TRY(nl_launch_wgrad(p.gA, W, W, p.X, 96, 90, NK, 0, 0, tg->w[T_B0W] + F, F + 90, 1, 0, tg->w[T_B0B], tg->scratch, tg->scratch_floats, x.st));
    else if (tg->w[T_B0B]) NL_TRY(nl_launch_colsum(p.gA, W, NK, W, tg->w[T_B0B], tg->scratch, x.st));
    if ((tg->w[T_B0W] || tg->sp_feat) && M > 0) {
      const int ldf = ldf_of(f->C);
      NL_CHECK_HIP(hipMemsetAsync(f->tr_gT, 0, sizeof(float) * (size_t)M * W, x.st));
      NL_TRY(nl_launch_sp_feat_scatter(p.gA, W, W, idx, N, K, M, f->tr_gT, x.st));
      if (tg->w[T_B0W]) {
        NL_TRY(nl_launch_copy_rows(f->sp_feat, F, f->tr_tmp, ldf, M, F, false, x.st));   // (rows of 195 floats are not 16-byte aligned)
        NL_TRY(nl_launch_wgrad(f->tr_gT, W, W, f->tr_tmp, ldf, F, M, 0, 0, tg->w[T_B0W], F + 90, 1, 0, nullptr, tg->scratch, tg->scratch_floats, x.st));
      }
      if (tg->sp_feat) {
        SegSpec st_{f->tr_gT, W, W, 0, 1};
        NL_TRY(run_gemm(xb, G_BASE0_TF, &st_, 1, M, f->tr_tmp, ldf, NL_ACT_NONE));
        NL_TRY(nl_launch_copy_rows(f->tr_tmp, ldf, tg->sp_feat, F, M, F, true, x.st));
      }
    }
  }
  NL_TRY(run_gemm(xb, G_BASE0_T, &sa, 1, NK, p.gX, 96, NL_ACT_NONE));
  const bool rdw = tg && (tg->w[T_RD0W] || tg->w[T_RD0B] || tg->w[T_RD2W] || tg->w[T_RD2B]);
  NL_TRY(nl_launch_point_encode_backward(xyz, dir, dir_stride, dir_div, N, K, M, idx, f->sp_xyz, f->sp_dir, x.p<float>(x.L.rd_w), inv_span, p.gX, 96, g_xyz,
                                         g_dir, rdw ? p.tr : nullptr, x.st));
  if (rdw) {   // ray_diff_fc (model.py:36-39): rows [input 4 | hidden 16 | d hidden 16 | d output 32]
    NL_TRY(wg(T_RD2W, T_RD2B, p.tr + 36, 68, 27, p.tr + 4, 68, 16, NK));
    NL_TRY(wg(T_RD0W, T_RD0B, p.tr + 20, 68, 16, p.tr, 68, 4, NK));
  }
  if (tg && tg->sp_feat && !tab) {   // the gathered support features (columns 0 .. F-1 of the encoded rows)
    const int ldf = ldf_of(f->C);
    NL_TRY(run_gemm(xb, G_BASE0_TF, &sa, 1, NK, p.gXF, ldf, NL_ACT_NONE));
    NL_TRY(nl_launch_sp_feat_scatter(p.gXF, ldf, F, idx, N, K, M, tg->sp_feat, x.st));
  }
  return NL_OK;
}
int do_point_backward(const Ctx& xb, const Ctx& x, const nl_frame* f, const float* xyz, const float* dir, int dir_stride, const float* G, int64_t N, int K,
                      const float* gFA, float* g_xyz, float* g_dir, float* g_G, const PtBwdBufs& p, const int* idx_in = nullptr, const float* d2_in = nullptr,
                      const TrainOut* tg = nullptr) {
  if (!tg && dir && pt_keep_fused_ok(x, f, N, K)) NL_TRY(pt_forward_keep_fused(x, f, xyz, dir, dir_stride, 1, G, N, p, idx_in, d2_in));
  else NL_TRY(pt_forward_staged(x, f, xyz, dir, dir_stride, 1, G, N, K, p, idx_in, d2_in));
  return pt_backward_only(xb, x, f, xyz, dir, dir_stride, 1, G, N, K, gFA, g_xyz, g_dir, g_G, p, idx_in, d2_in, tg);
}

// ---- input gradients of the multi-view aggregation and of the colour blend (frozen weights) ------------------------------------------
void carve_mvb(Bump& b, const nl_config* c, int V, int64_t N, bool blend, MvBwdBufs& m, bool train = false) {
  const int W = c->W, ldg = ldg_of(c->C);
  m.vis = b.take<float>((size_t)V * N); m.dd = b.take<float>((size_t)V * N); m.gvis = b.take<float>((size_t)V * N); m.gdd = b.take<float>((size_t)V * N);
  m.gpart = b.take<float>((size_t)V * N * 3);
  m.g393 = b.take<float>((size_t)N * ldg); m.valid_s = b.take<int>((size_t)N);
  if (!blend) {
    m.t64 = b.take<float>((size_t)N * 64); m.G = b.take<float>((size_t)N * W); m.gA = b.take<float>((size_t)N * W);
    m.gt64 = b.take<float>((size_t)N * 64); m.gg393 = b.take<float>((size_t)N * ldg);
    m.bl1 = m.rgbv = m.blA = m.ghA = m.gpf = m.grgbv = m.gang = nullptr;
  } else {
    m.bl1 = b.take<float>((size_t)N * V * 32); m.rgbv = b.take<float>((size_t)N * V * 4); m.blA = b.take<float>((size_t)N * 32);
    m.ghA = b.take<float>((size_t)N * 32); m.gpf = b.take<float>((size_t)N * V * 32); m.grgbv = b.take<float>((size_t)N * V * 4);
    m.gang = b.take<float>((size_t)N * V * 4);
    m.t64 = m.G = m.gA = m.gt64 = m.gg393 = nullptr;
  }
  m.dtr = m.btr = m.ang = nullptr;
  if (train) {
    if (c->precision == NL_PREC_F32) m.dtr = b.take<float>((size_t)V * N * nl_dec_train_row());   // (the MFMA decoder backward needs no rows)
    if (blend) { m.btr = b.take<float>((size_t)V * N * 68); m.ang = b.take<float>((size_t)V * N * 8 + 256); }
  }
}

// the recomputed forward both need: visibility / depth difference (exact fp32 decoders: the backward kernel differentiates those) and the
// statistics rows (+ the blend's per-(sample, view) layer-1 part when bl1 != null)
int mv_recompute(const Ctx& x32, const nl_frame* f, const NlViews& vw, const float* xyz, int64_t N, const MvBwdBufs& m) {
  if (m.bl1) NL_TRY(ensure_pfeat(x32, f));
  if (x32.c->precision == NL_PREC_F32) NL_TRY(nl_launch_mv_vis(vw, f->visf_hwc, x32.p<float>(x32.L.dec_w), xyz, N, m.vis, m.dd, x32.st));
  else NL_TRY(nl_launch_mv_vis_mfma(vw, f->visf_hwc, x32.p<char>(x32.L.dec_mfma), xyz, N, m.vis, m.dd, true, x32.st));   // split-FP16 decoders (§2)
  return nl_launch_mv_stats(vw, f->views_dev, f->images, f->feat, f->C, xyz, N, m.vis, m.dd, m.g393, ldg_of(f->C), nullptr, nullptr, m.valid_s, f->pfeat,
                            x32.p<float>(x32.L.blw), m.bl1, m.rgbv, x32.st);
}

// the 24 decoder tensors from the rows the decoder backward kernels emit (backward.hip: [x 32 | per decoder: h1 32, h2 32, d a1 32, d a2 32, d out 2, pad 2])
int dec_wgrads(const TrainOut* tg, hipStream_t st, const float* tr, int64_t rows) {
  const int ld = nl_dec_train_row();
  for (int d = 0; d < 4; ++d) {
    const float* q = tr + 32 + 132 * d;
    const int t0 = T_DEC + 6 * d;
    NL_TRY(wgrad_to(tg, st, t0, t0 + 1, q + 64, ld, 32, tr, ld, 32, rows));
    NL_TRY(wgrad_to(tg, st, t0 + 2, t0 + 3, q + 96, ld, 32, q, ld, 32, rows));
    NL_TRY(wgrad_to(tg, st, t0 + 4, t0 + 5, q + 128, ld, d < 2 ? 2 : 1, q + 32, ld, 32, rows));
  }
  return NL_OK;
}

// g_G (N, W) -> g_xyz (N, 3): out_fc backwards (two transposed-weight products, ELU masks), the visibility-weighted statistics, the bilinear taps'
// spatial derivative, the IBRNet projection; visibility / depth difference through the NeuRay decoders and the NeuRay projection.
// out_fc on the recomputed statistics rows -> m.t64, m.G
int mv_outfc_forward(const Ctx& x32, const nl_frame* f, int64_t N, const MvBwdBufs& m) {
  const int W = x32.c->W, ldg = ldg_of(f->C);
  SegSpec s0{m.g393, ldg, ldg, 0, 1}, s1{m.t64, 64, 64, 0, 1};
  NL_TRY(run_gemm(x32, G_OUTFC0, &s0, 1, N, m.t64, 64, NL_ACT_ELU));
  return run_gemm(x32, G_OUTFC2, &s1, 1, N, m.G, W, NL_ACT_ELU);
}
// gG (N, W) -> m.gg393 (the statistics rows' gradient) + out_fc's weight gradients
int mv_outfc_backward(const Ctx& xb, const Ctx& x32, const nl_frame* f, int64_t N, const float* gG, const MvBwdBufs& m, const TrainOut* tg) {
  const int W = x32.c->W, ldg = ldg_of(f->C);
  NL_CHECK_HIP(hipMemcpyAsync(m.gA, gG, sizeof(float) * (size_t)N * W, hipMemcpyDeviceToDevice, x32.st));
  NL_TRY(nl_launch_elu_mask(m.gA, m.G, (size_t)N * W, x32.st));
  NL_TRY(wgrad_to(tg, x32.st, T_OUT2W, T_OUT2B, m.gA, W, W, m.t64, 64, 64, N));
  SegSpec sa{m.gA, W, W, 0, 1}, st{m.gt64, 64, 64, 0, 1};
  NL_TRY(run_gemm(xb, G_OUTFC2_T, &sa, 1, N, m.gt64, 64, NL_ACT_NONE));
  NL_TRY(nl_launch_elu_mask(m.gt64, m.t64, (size_t)N * 64, x32.st));
  NL_TRY(wgrad_to(tg, x32.st, T_OUT0W, T_OUT0B, m.gt64, 64, 64, m.g393, ldg, 2 * (f->C + 3) + 3, N));
  return run_gemm(xb, G_OUTFC0_T, &st, 1, N, m.gg393, ldg, NL_ACT_NONE);
}
// gradients of the tapped values (statistics rows: gg393; blend: g_pf / g_rgbv / g_ang; either may be null) -> g_xyz (written), g_qc, the maps' scatter-adds;
// then visibility / depth difference back through the decoders (ONE pass for whatever consumers contributed) -> += g_xyz, the decoders' gradients
int mv_geom_dec_backward(const Ctx& x32, const nl_frame* f, const NlViews& vw, const float* xyz, int64_t N, const float* gg393, bool blend, float* g_xyz,
                         float* g_qc, const MvBwdBufs& m, const TrainOut* tg) {
  NL_TRY(nl_launch_mv_geom_backward(vw, f->views_dev, f->images, f->feat, f->C, blend ? f->pfeat : nullptr, xyz, N, m.vis, m.dd, gg393, ldg_of(f->C),
                                    blend ? m.gpf : nullptr, blend ? m.grgbv : nullptr, blend ? m.gang : nullptr, g_xyz, g_qc, m.gvis, m.gdd,
                                    tg ? tg->feat_maps : nullptr, tg && blend ? tg->pfeat_maps : nullptr, gg393 ? m.g393 : nullptr, x32.st));
  const bool decw = tg && tg->any(T_DEC, T_DEC + 24);
  const bool f32 = x32.c->precision == NL_PREC_F32;   // fp32: rows for dec_wgrads; otherwise the MFMA kernel accumulates the 24 tensors' gradients itself
  NL_TRY(nl_launch_dec_backward(vw, f->visf_hwc, x32.p<float>(x32.L.dec_w), f32 ? nullptr : x32.p<char>(x32.L.dec_mfma), xyz, N, m.gvis, m.gdd, m.gpart, g_xyz,
                                decw && f32 ? m.dtr : nullptr, decw && !f32 ? tg->w + T_DEC : nullptr, tg ? tg->scratch : nullptr, tg ? tg->scratch_floats : 0,
                                tg ? tg->vis_maps : nullptr, x32.st));
  return decw && f32 ? dec_wgrads(tg, x32.st, m.dtr, (int64_t)vw.V * N) : NL_OK;
}
int do_mv_backward(const Ctx& xb, const Ctx& x32, const nl_frame* f, const float* xyz, int64_t N, const float* gG, float* g_xyz, const MvBwdBufs& m,
                   const TrainOut* tg = nullptr) {
  const NlViews vw = with_query(f, nullptr);
  NL_TRY(mv_recompute(x32, f, vw, xyz, N, m));
  NL_TRY(mv_outfc_forward(x32, f, N, m));
  NL_TRY(mv_outfc_backward(xb, x32, f, N, gG, m, tg));
  return mv_geom_dec_backward(x32, f, vw, xyz, N, m.gg393, false, g_xyz, nullptr, m, tg);
}

// rgb_s = blend(feature_agg, per-view taps) forward (staged) and its input gradient
int do_blend_forward(const Ctx& x, const nl_frame* f, const float* qc, const float* xyz, const float* FA, int64_t N, float* rgb_s, const MvBwdBufs& m) {
  const int W = x.c->W;
  const NlViews vw = with_query(f, qc);
  nl_config c32 = *x.c;   // the same arithmetic as the backward call's recomputed forward
  c32.precision = x.c->precision == NL_PREC_F32 ? NL_PREC_F32 : NL_PREC_F16X3_INTERNAL;
  Ctx x32 = x; x32.c = &c32;
  NL_TRY(mv_recompute(x32, f, vw, xyz, N, m));
  SegSpec sa{FA, W, W, 0, 1};
  NL_TRY(run_gemm(x32, G_BLENDA, &sa, 1, N, m.blA, 32, NL_ACT_NONE));
  return nl_launch_blend(m.blA, m.bl1, m.rgbv, N, vw.V, x.p<float>(x.L.bl2_w), x.p<float>(x.L.bl2_b), x.p<float>(x.L.bl4_w), x.p<float>(x.L.bl4_b), rgb_s, x.st);
}

// g_rgb_s -> m.ghA / m.gpf / m.grgbv / m.gang (+ rgb_blending_mlp's weight gradients) and g_FA (may be null); needs m.blA, m.bl1, m.rgbv of the forward
int blend_tail_backward(const Ctx& xb, const Ctx& x32, const nl_frame* f, const NlViews& vw, const float* xyz, const float* FA, int64_t N, const float* g_rgb_s,
                        float* g_FA, const MvBwdBufs& m, const TrainOut* tg) {
  const int W = x32.c->W;
  SegSpec sg{m.ghA, 32, 32, 0, 1};
  const bool blw = tg && (tg->any(T_BL0W, T_BL4B + 1));
  NL_TRY(nl_launch_blend_backward(m.blA, m.bl1, m.rgbv, N, vw.V, x32.p<float>(x32.L.bl2_w), x32.p<float>(x32.L.bl2_b), x32.p<float>(x32.L.bl4_w),
                                  x32.p<float>(x32.L.bl4_b), x32.p<float>(x32.L.blw), g_rgb_s, m.ghA, m.gpf, m.grgbv, m.gang, blw ? m.btr : nullptr, x32.st));
  if (blw) {   // rgb_blending_mlp (model.py:84-93, 532-535)
    const int64_t NV = N * vw.V;
    const int F = f->C + 3;
    NL_TRY(wgrad_to(tg, x32.st, T_BL2W, T_BL2B, m.btr + 32, 68, 16, m.btr, 68, 32, NV));
    NL_TRY(wgrad_to(tg, x32.st, T_BL4W, T_BL4B, m.btr + 64, 68, 1, m.btr + 48, 68, 16, NV));
    if (tg->w[T_BL0W]) {
      // layer 1 by linearity: the feature_agg columns (per sample), the [rgb | visibility | view angles] columns (per sample and view); the feature
      // columns multiply the per-frame projected maps, whose gradient goes back as a map (nl_train_grads.blend_feat_maps)
      NL_TRY(nl_launch_wgrad(m.ghA, 32, 32, FA, W, W, N, 0, 0, tg->w[T_BL0W], W + F + 5, 1, 0, nullptr, tg->scratch, tg->scratch_floats, x32.st));
      float* t8 = m.ang + (size_t)NV * 8;
      NL_CHECK_HIP(hipMemsetAsync(t8, 0, sizeof(float) * 256, x32.st));
      NL_TRY(nl_launch_blend_inputs8(vw, f->views_dev, xyz, N, m.rgbv, m.ang, x32.st));
      NL_TRY(nl_launch_wgrad(m.gpf, 32, 32, m.ang, 8, 8, NV, 0, 0, t8, 8, 1, 0, nullptr, tg->scratch, tg->scratch_floats, x32.st));
      NL_TRY(nl_launch_blw_unpack(t8, tg->w[T_BL0W], W, F, x32.st));
    }
    if (tg->w[T_BL0B]) NL_TRY(nl_launch_colsum(m.gpf, 32, NV, 32, tg->w[T_BL0B], tg->scratch, x32.st));
  }
  if (g_FA) NL_TRY(run_gemm(xb, G_BLENDA_T, &sg, 1, N, g_FA, W, NL_ACT_NONE));
  return NL_OK;
}
int do_blend_backward(const Ctx& xb, const Ctx& x32, const nl_frame* f, const float* qc, const float* xyz, const float* FA, int64_t N, const float* g_rgb_s,
                      float* g_xyz, float* g_FA, float* g_qc, const MvBwdBufs& m, const TrainOut* tg = nullptr) {
  const int W = x32.c->W;
  const NlViews vw = with_query(f, qc);
  NL_TRY(mv_recompute(x32, f, vw, xyz, N, m));
  SegSpec sa{FA, W, W, 0, 1};
  NL_TRY(run_gemm(x32, G_BLENDA, &sa, 1, N, m.blA, 32, NL_ACT_NONE));
  NL_TRY(blend_tail_backward(xb, x32, f, vw, xyz, FA, N, g_rgb_s, g_FA, m, tg));
  return mv_geom_dec_backward(x32, f, vw, xyz, N, nullptr, true, g_xyz, g_qc, m, tg);
}

// ---- input gradient of the ray U-Net (frozen weights) -------------------------------------------------------------------------------
void carve_unb(Bump& b, const nl_config* c, int64_t R, UnBwdBufs& q, bool train = false) {
  const size_t N = (size_t)R * c->S;
  const int W = c->W;
  carve_un(b, c, R, q.u);
  q.geo = b.take<float>(N * W); q.gout = b.take<float>(N * W);
  q.gx2 = b.take<float>(N * 32); q.gx2r = b.take<float>(N * 32);
  q.gcat1 = b.take<float>(N / 2 * 128); q.gx1r = b.take<float>(N / 2 * 64);
  q.gcat2 = b.take<float>(N / 4 * 256); q.gx0r = b.take<float>(N / 4 * 128);
  q.gc3 = b.take<float>(N / 8 * 128); q.gr3 = b.take<float>(N / 4 * 128);
  q.gc2 = b.take<float>(N / 4 * 128); q.gr2 = b.take<float>(N / 2 * 128);
  q.gc1 = b.take<float>(N / 2 * 64); q.gr1 = b.take<float>(N * 64);
  q.tmp = b.take<float>(N * W);
  q.aff = train ? b.take<float>(2 * N * (W > 64 ? W : 64)) : nullptr;   // the largest slab per ray (conv_out: S x W; conv1: S x 64; conv2: S/2 x 128), [d y * xhat | d y]
}

// (the forward's pre-LayerNorm outputs and block outputs are in q.u)
int unet_backward_only(const Ctx& xb, const Ctx& x32, const float* in, int64_t R, const float* g_geo, float* g_in, const UnBwdBufs& q, const TrainOut* tg) {
  const int W = x32.c->W, S = x32.c->S;
  const UnBufs& u = q.u;
  auto g = [&](int i) { return x32.p<float>(x32.L.un_g[i]); };
  auto b = [&](int i) { return x32.p<float>(x32.L.un_b[i]); };
  const float eps = 1e-5f;
  hipStream_t st = x32.st;
  // LayerNorm / ELU / MaxPool backward of block `li`; training: + its affine tables' gradients (column sums over the rays, transposed into the
  // state_dict's (C, L) layout)
  auto ln_bwd = [&](int li, const float* x, int L, int Cc, const float* go, int ldgo, int pool, float* gx) -> int {
    float* gw = tg ? tg->w[T_UNET + 4 * li + 2] : nullptr;
    float* gb = tg ? tg->w[T_UNET + 4 * li + 3] : nullptr;
    const bool aff = gw || gb;
    NL_TRY(nl_launch_ln_slab_elu_backward(x, R, L, Cc, g(li), b(li), eps, go, ldgo, pool, gx, aff ? q.aff : nullptr, st));
    if (!aff) return NL_OK;
    return nl_launch_colsum_tables(q.aff, R, L, Cc, gw, gb, tg->scratch, st);   // sums over the rays, straight into the channel-major tables
  };
  // Conv1d(k = 3, padding 1) weight (co, ci_total, 3): one product per tap, the input rows shifted by tap - 1 inside each ray
  auto conv_wg = [&](int li, const float* dY, int co, const float* X, int ci, int ci_total, int ci0, int L, bool bias) -> int {
    float* gw = tg ? tg->w[T_UNET + 4 * li] : nullptr;
    float* gb = tg && bias ? tg->w[T_UNET + 4 * li + 1] : nullptr;
    if (!gw && gb) return nl_launch_colsum(dY, co, R * L, co, gb, tg->scratch, st);
    if (!gw) return NL_OK;
    const float* dys[3] = {dY, dY, dY};
    const float* xs[3] = {X, X, X};
    const int sh[3] = {-1, 0, 1}, cos_[3] = {ci0 * 3, ci0 * 3 + 1, ci0 * 3 + 2};
    return nl_launch_wgrad_multi(3, dys, co, co, xs, ci, ci, R * L, sh, L, gw, ci_total * 3, 3, cos_, gb, 1, tg->scratch, tg->scratch_floats, st);   // the three taps
  };
  // ConvTranspose1d(k = 3, stride 2, padding 1, output_padding 1) weight (ci_total, co, 3): y[2m] = x[m] w1, y[2m+1] = x[m] w2 + x[m+1] w0;
  // gy = the merged rows (R Li, 2 co) [even | odd]
  auto convT_wg = [&](int li, const float* X, int ci, int ci0, const float* gy, int co, int Li) -> int {
    float* gw = tg ? tg->w[T_UNET + 4 * li] : nullptr;
    if (!gw) return NL_OK;
    float* base = gw + (size_t)ci0 * co * 3;
    const float* dys[3] = {X, X, X};                       // (operand roles swapped: the weight's rows are the INPUT channels)
    const float* xs[3] = {gy, gy + co, gy + co};
    const int sh[3] = {0, 0, -1}, cos_[3] = {1, 2, 0};
    return nl_launch_wgrad_multi(3, dys, ci, ci, xs, 2 * co, co, R * Li, sh, Li, base, co * 3, 3, cos_, nullptr, -1, tg->scratch, tg->scratch_floats, st);
  };
  auto convT_bias = [&](int li, const float* gy, int co, int Lo) -> int {
    float* gb = tg ? tg->w[T_UNET + 4 * li + 1] : nullptr;
    return gb ? nl_launch_colsum(gy, co, R * Lo, co, gb, tg->scratch, st) : NL_OK;
  };
  // conv_out
  NL_TRY(ln_bwd(U_OUT, u.outr, S, W, g_geo, W, 0, q.gout));
  NL_TRY(conv_wg(U_OUT, q.gout, W, in, W, W + 32, 0, S, true));
  NL_TRY(conv_wg(U_OUT, q.gout, W, u.x2, 32, W + 32, W, S, false));
  { SegSpec s[1] = {{q.gout, W, W, 0, 1, 3}};
    NL_TRY(run_gemm(xb, G_UB_OUTA, s, 1, R * S, g_in, W, NL_ACT_NONE, S, S, S, 1, 0));
    NL_TRY(run_gemm(xb, G_UB_OUTB, s, 1, R * S, q.gx2, 32, NL_ACT_NONE, S, S, S, 1, 0)); }
  // trans_conv1: slab (S x 32) = merged rows (S/2 x 64)
  NL_TRY(ln_bwd(U_T1, u.x2r, S, 32, q.gx2, 32, 0, q.gx2r));
  NL_TRY(convT_wg(U_T1, u.c1, 64, 0, q.gx2r, 32, S / 2));
  NL_TRY(convT_wg(U_T1, u.x1, 64, 64, q.gx2r, 32, S / 2));
  NL_TRY(convT_bias(U_T1, q.gx2r, 32, S));
  { SegSpec s[2] = {{q.gx2r, 64, 64, 0, 1}, {q.gx2r + 32, 64, 32, -1, 1}};
    NL_TRY(run_gemm(xb, G_UB_T1, s, 2, R * (S / 2), q.gcat1, 128, NL_ACT_NONE, S / 2, S / 2, S / 2, 1, 0)); }
  // trans_conv2: output x1 = columns 64..127 of cat[c1, x1]'s gradient
  NL_TRY(ln_bwd(U_T2, u.x1r, S / 2, 64, q.gcat1 + 64, 128, 0, q.gx1r));
  NL_TRY(convT_wg(U_T2, u.c2, 128, 0, q.gx1r, 64, S / 4));
  NL_TRY(convT_wg(U_T2, u.x0, 128, 128, q.gx1r, 64, S / 4));
  NL_TRY(convT_bias(U_T2, q.gx1r, 64, S / 2));
  { SegSpec s[2] = {{q.gx1r, 128, 128, 0, 1}, {q.gx1r + 64, 128, 64, -1, 1}};
    NL_TRY(run_gemm(xb, G_UB_T2, s, 2, R * (S / 4), q.gcat2, 256, NL_ACT_NONE, S / 4, S / 4, S / 4, 1, 0)); }
  // trans_conv3: output x0 = columns 128..255 of cat[c2, x0]'s gradient
  NL_TRY(ln_bwd(U_T3, u.x0r, S / 4, 128, q.gcat2 + 128, 256, 0, q.gx0r));
  NL_TRY(convT_wg(U_T3, u.c3, 128, 0, q.gx0r, 128, S / 8));
  NL_TRY(convT_bias(U_T3, q.gx0r, 128, S / 4));
  { SegSpec s[2] = {{q.gx0r, 256, 256, 0, 1}, {q.gx0r + 128, 256, 128, -1, 1}};
    NL_TRY(run_gemm(xb, G_UB_T3, s, 2, R * (S / 8), q.gc3, 128, NL_ACT_NONE, S / 8, S / 8, S / 8, 1, 0)); }
  // conv3 (+ MaxPool): gradient of its pooled output c3
  NL_TRY(ln_bwd(U_CONV3, u.r3, S / 4, 128, q.gc3, 128, 1, q.gr3));
  NL_TRY(conv_wg(U_CONV3, q.gr3, 128, u.c2, 128, 128, 0, S / 4, true));
  { SegSpec s[1] = {{q.gr3, 128, 128, 0, 1, 3}};
    NL_TRY(run_gemm(xb, G_UB_C3, s, 1, R * (S / 4), q.tmp, 128, NL_ACT_NONE, S / 4, S / 4, S / 4, 1, 0)); }
  NL_TRY(nl_launch_add2d(q.gcat2, 256, q.tmp, 128, q.gc2, 128, R * (S / 4), 128, st));
  // conv2 (+ MaxPool)
  NL_TRY(ln_bwd(U_CONV2, u.r2, S / 2, 128, q.gc2, 128, 1, q.gr2));
  NL_TRY(conv_wg(U_CONV2, q.gr2, 128, u.c1, 64, 64, 0, S / 2, true));
  { SegSpec s[1] = {{q.gr2, 128, 128, 0, 1, 3}};
    NL_TRY(run_gemm(xb, G_UB_C2, s, 1, R * (S / 2), q.tmp, 64, NL_ACT_NONE, S / 2, S / 2, S / 2, 1, 0)); }
  NL_TRY(nl_launch_add2d(q.gcat1, 128, q.tmp, 64, q.gc1, 64, R * (S / 2), 64, st));
  // conv1 (+ MaxPool)
  NL_TRY(ln_bwd(U_CONV1, u.r1, S, 64, q.gc1, 64, 1, q.gr1));
  NL_TRY(conv_wg(U_CONV1, q.gr1, 64, in, W, W, 0, S, true));
  { SegSpec s[1] = {{q.gr1, 64, 64, 0, 1, 3}};
    NL_TRY(run_gemm(xb, G_UB_C1, s, 1, R * S, q.tmp, W, NL_ACT_NONE, S, S, S, 1, 0)); }
  return nl_launch_add2d(g_in, W, q.tmp, W, g_in, W, R * S, W, st);
}
// Unfused forward in exact fp32 (every layer's pre-LayerNorm output stays in the workspace), then layer by layer backwards: LayerNorm / ELU /
// MaxPool derivative (one block per ray) -> transposed-weight convolution (segment GEMM over the gradient rows' taps), the skip connections'
// gradients added where the concatenations were.
int do_unet_backward(const Ctx& xb, const Ctx& x32, const float* in, int64_t R, const float* g_geo, float* g_in, const UnBwdBufs& q, const TrainOut* tg = nullptr) {
  NL_TRY(do_unet(x32, in, R, q.geo, q.u));   // fp32: separate GEMM + ln_slab_elu launches
  return unet_backward_only(xb, x32, in, R, g_geo, g_in, q, tg);
}

// ---- the whole ray path backwards in one call (nl_render_rays_backward) ----------------------------------------------------------------
// = the four stage backwards above + the heads + compositing, sharing what the separate autograd nodes each recompute: ONE pass of the visibility
// decoders forward and ONE backward for the aggregation's and the blend's uses of visibility / depth difference, one geometry kernel for
// both sets of taps, one neighbour search.
void carve_rb(Bump& b, const nl_config* c, int V, int64_t R, RbBufs& a, bool train) {
  const int W = c->W, S = c->S;
  const size_t N = (size_t)R * S;
  // multi-view buffers: the union of the aggregation's and the blend's sets
  carve_mvb(b, c, V, (int64_t)N, true, a.m, train);
  a.m.t64 = b.take<float>(N * 64); a.m.G = b.take<float>(N * W); a.m.gA = b.take<float>(N * W);
  a.m.gt64 = b.take<float>(N * 64); a.m.gg393 = b.take<float>(N * ldg_of(c->C));
  carve_ptb(b, c, (int64_t)N, 8, a.p, train);
  carve_unb(b, c, R, a.q, train);
  a.xyz = b.take<float>(N * 3); a.zc = b.take<float>(N); a.FA = b.take<float>(N * W); a.sigma = b.take<float>(N); a.Hf = b.take<float>(N * W);
  a.rgb_s = b.take<float>(N * 3); a.hc = b.take<float>((size_t)R * W); a.wsum4 = b.take<float>((size_t)R * 4); a.ghc = b.take<float>((size_t)R * W);
  a.gw = b.take<float>(N); a.g_sigma = b.take<float>(N); a.g_rgb_s = b.take<float>(N * 3); a.gFA = b.take<float>(N * W); a.gtmp = b.take<float>(N * W);
  a.gpre4 = b.take<float>(N * 4); a.gxyz_m = b.take<float>(N * 3); a.gxyz_p = b.take<float>(N * 3); a.gdir = b.take<float>(N * 3);
  a.gG = b.take<float>(N * W); a.gqcN = b.take<float>(N * 3);
  a.wts = b.take<float>(N); a.bv = b.take<float>(N); a.gpre4b = b.take<float>(N * 4);   // the uncertainty head (keep / kept pair)
}
struct RbCot { const float *g_rgb, *g_depth, *g_unc, *g_feat, *g_wts; const int* idx; const float* d2; };
// the staged forward of the whole path into the workspace (everything the way back reads).  want_feat: feat_mlp.0's hidden rows too
int render_forward_staged(const Ctx& x32, const nl_frame* f, const float* qc, const float* qrows, const float* rays_o, const float* rays_d, const float* z, int64_t R,
                          bool want_feat, const int* knn_idx, const float* knn_d2, const RbBufs& a, bool frozen = false) {
  const int W = x32.c->W, S = x32.c->S;
  const int64_t N = R * S;
  hipStream_t st = x32.st;
  const NlViews vw = with_query(f, qc, qrows, S);
  const float eps_ln = 1e-6f;
  NL_TRY(nl_launch_sample_points(rays_o, rays_d, R, S, f->views.near_, f->views.far_, z, a.zc, a.xyz, st));
  NL_TRY(mv_recompute(x32, f, vw, a.xyz, N, a.m));                       // visibility / depth difference, statistics rows, the blend's per-view part
  NL_TRY(mv_outfc_forward(x32, f, N, a.m));                              // -> G
  if (frozen && pt_keep_fused_ok(x32, f, N, 8)) NL_TRY(pt_forward_keep_fused(x32, f, a.xyz, rays_d, 3, S, a.m.G, N, a.p, knn_idx, knn_d2));
  else NL_TRY(pt_forward_staged(x32, f, a.xyz, rays_d, 3, S, a.m.G, N, 8, a.p, knn_idx, knn_d2));
  NL_TRY(nl_launch_ln_agg(a.p.FCo, a.m.G, N, W, x32.p<float>(x32.L.ln_g), x32.p<float>(x32.L.ln_b), eps_ln, a.p.wscale, a.FA, st));
  NL_TRY(do_unet(x32, a.FA, R, a.q.geo, a.q.u));
  NL_TRY(nl_launch_sigma(a.q.geo, N, W, x32.p<float>(x32.L.sig_w), x32.p<float>(x32.L.sig_b), a.sigma, st));
  SegSpec sfa{a.FA, W, W, 0, 1};
  if (want_feat) NL_TRY(run_gemm(x32, G_FEAT0, &sfa, 1, N, a.Hf, W, NL_ACT_LRELU));
  NL_TRY(run_gemm(x32, G_BLENDA, &sfa, 1, N, a.m.blA, 32, NL_ACT_NONE));
  return nl_launch_blend(a.m.blA, a.m.bl1, a.m.rgbv, N, vw.V, x32.p<float>(x32.L.bl2_w), x32.p<float>(x32.L.bl2_b), x32.p<float>(x32.L.bl4_w),
                         x32.p<float>(x32.L.bl4_b), a.rgb_s, st);
}
// the way back from the staged forward's workspace
int render_backward_staged(const Ctx& xb, const Ctx& x32, const nl_frame* f, const float* qc, const float* qrows, const float* rays_d, int64_t R, int white,
                           const RbCot& ct, float* g_o, float* g_d, float* g_qc_rows, const RbBufs& a, const TrainOut* tg, const nl_beta_head* bh = nullptr) {
  const int W = x32.c->W, S = x32.c->S, C = x32.c->C;
  const int64_t N = R * S;
  hipStream_t st = x32.st;
  const NlViews vw = with_query(f, qc, qrows, S);
  const bool want_feat = ct.g_feat != nullptr;
  // ---------------------------------------------------------------- compositing backwards (feat = W2 . sum_s w_s hidden_s + b2 sum_s w_s)
  const float* b2 = x32.p<float>(x32.L.b32[G_FEAT2]) + (size_t)W * x32.L.g[G_FEAT2].Npad;   // the bias row of G_FEAT2's fp32 weights (K row W)
  if (want_feat) {
    SegSpec sgf{ct.g_feat, C, C, 0, 1};
    NL_TRY(run_gemm(xb, G_FEAT2_T, &sgf, 1, R, a.ghc, W, NL_ACT_NONE));
  }
  const bool beta = bh && bh->g_beta;
  // (the uncertainty head's share of the weights' cotangent has to be in before compositing is differentiated; its share of d/d geo joins the density
  // head's below)
  NL_TRY(nl_launch_gw_total(ct.g_wts, ct.g_feat, b2, R, S, C, a.gw, beta ? bh->g_beta : nullptr, a.bv, st));
  NL_TRY(nl_composite_backward(a.zc, a.sigma, a.rgb_s, want_feat ? a.Hf : nullptr, R, S, want_feat ? W : 0, white, ct.g_rgb, ct.g_depth, ct.g_unc,
                               want_feat ? a.ghc : nullptr, a.gw, a.g_sigma, a.g_rgb_s, want_feat ? a.gtmp : nullptr, st));
  // ---------------------------------------------------------------- heads
  bool have_gfa = false;
  if (want_feat) {   // feat_mlp: gtmp = d/d hidden -> LeakyReLU mask -> feat_mlp.0^T
    NL_TRY(nl_launch_lrelu_mask(a.gtmp, a.Hf, (size_t)N * W, st));
    NL_TRY(wgrad_to(tg, st, T_F0W, T_F0B, a.gtmp, W, W, a.FA, W, W, N));
    SegSpec sg{a.gtmp, W, W, 0, 1};
    NL_TRY(run_gemm(xb, G_FEAT0_T, &sg, 1, N, a.gFA, W, NL_ACT_NONE));
    have_gfa = true;
    if (tg && (tg->w[T_F2W] || tg->w[T_F2B])) {
      NL_TRY(nl_launch_ray_feat_sum(a.zc, a.sigma, a.Hf, R, S, W, a.hc, a.wsum4, st));
      if (tg->w[T_F2W]) NL_TRY(nl_launch_wgrad(ct.g_feat, C, C, a.hc, W, W, R, 0, 0, tg->w[T_F2W], W, 1, 0, nullptr, tg->scratch, tg->scratch_floats, st));
      if (tg->w[T_F2B]) NL_TRY(nl_launch_wgrad(ct.g_feat, C, C, a.wsum4, 4, 1, R, 0, 0, tg->w[T_F2B], 1, 1, 0, nullptr, tg->scratch, tg->scratch_floats, st));
    }
  }
  // density head -> g_geo (in q.gout's neighbour: reuse a.gG as scratch is not possible yet; g_geo lives in a.Hf, free from here on)
  float* g_geo = a.Hf;
  NL_TRY(nl_launch_sigma_backward(a.q.geo, N, W, x32.p<float>(x32.L.sig_w), x32.p<float>(x32.L.sig_b), a.g_sigma, g_geo, a.gpre4, st));
  NL_TRY(wgrad_to(tg, st, T_SIGW, T_SIGB, a.gpre4, 4, 1, a.q.geo, W, W, N));
  if (beta) {
    NL_TRY(nl_launch_beta_backward(a.q.geo, N, S, W, bh->weight, bh->bias, a.wts, bh->g_beta, g_geo, a.gpre4b, st));
    if (bh->g_weight) NL_TRY(nl_launch_wgrad(a.gpre4b, 4, 1, a.q.geo, W, W, N, 0, 0, bh->g_weight, W, 1, 0, bh->g_bias, tg ? tg->scratch : nullptr,
                                            tg ? tg->scratch_floats : 0, st));
  }
  // ---------------------------------------------------------------- ray U-Net, colour blend: their shares of d/d feature_agg
  NL_TRY(unet_backward_only(xb, x32, a.FA, R, g_geo, a.gtmp, a.q, tg));
  if (have_gfa) NL_TRY(nl_launch_add(a.gFA, a.gtmp, a.gFA, (size_t)N * W, st));
  else NL_CHECK_HIP(hipMemcpyAsync(a.gFA, a.gtmp, sizeof(float) * (size_t)N * W, hipMemcpyDeviceToDevice, st));
  NL_TRY(blend_tail_backward(xb, x32, f, vw, a.xyz, a.FA, N, a.g_rgb_s, a.gtmp, a.m, tg));
  NL_TRY(nl_launch_add(a.gFA, a.gtmp, a.gFA, (size_t)N * W, st));
  // ---------------------------------------------------------------- neural-point branch, aggregation, geometry + decoders
  NL_TRY(pt_backward_only(xb, x32, f, a.xyz, rays_d, 3, S, a.m.G, N, 8, a.gFA, a.gxyz_p, a.gdir, a.gG, a.p, ct.idx, ct.d2, tg));
  NL_TRY(mv_outfc_backward(xb, x32, f, N, a.gG, a.m, tg));
  NL_TRY(mv_geom_dec_backward(x32, f, vw, a.xyz, N, a.m.gg393, true, a.gxyz_m, g_qc_rows ? a.gqcN : nullptr, a.m, tg));
  return nl_launch_ray_reduce(a.gxyz_m, a.gxyz_p, nullptr, a.gdir, g_qc_rows ? a.gqcN : nullptr, a.zc, R, S, g_o, g_d, g_qc_rows, st);
}
int do_render_backward(const Ctx& xb, const Ctx& x32, const nl_frame* f, const float* qc, const float* qrows, const float* rays_o, const float* rays_d, const float* z,
                       int64_t R, int white, const RbCot& ct, float* g_o, float* g_d, float* g_qc_rows, const RbBufs& a, const TrainOut* tg) {
  NL_TRY(render_forward_staged(x32, f, qc, qrows, rays_o, rays_d, z, R, ct.g_feat != nullptr, ct.idx, ct.d2, a, tg == nullptr));
  return render_backward_staged(xb, x32, f, qc, qrows, rays_d, R, white, ct, g_o, g_d, g_qc_rows, a, tg);
}
// the per-ray outputs from the staged forward's workspace (the gradient path's forward values: split-FP16 arithmetic in the bf16 modes)
int render_outputs_staged(const Ctx& x32, const nl_frame* f, int64_t R, int white, const nl_render_out* out, const RbBufs& a, const nl_beta_head* bh = nullptr) {
  const int W = x32.c->W, S = x32.c->S, C = x32.c->C;
  const bool want_feat = out->feat != nullptr;
  NL_TRY(nl_launch_composite(a.zc, a.sigma, a.rgb_s, want_feat ? a.Hf : nullptr, a.m.valid_s, R, S, W, white, out, 0, want_feat ? a.hc : nullptr,
                             want_feat ? a.gw : nullptr, x32.st));   // (a.gw: R floats of scratch for the weight sums; the way back rewrites it)
  if (want_feat) {
    SegSpec s1[2] = {{a.hc, W, W, 0, 1}, {a.gw, 1, 1, 0, 1}};
    NL_TRY(run_gemm(x32, G_FEAT2, s1, 2, R, out->feat, C, NL_ACT_NONE));
  }
  if (bh) {   // the uncertainty head: softplus(beta_mlp.0(geo)) per sample (the density head's kernel), composited with the weights; both stay for the way back
    NL_TRY(nl_launch_sigma(a.q.geo, R * S, W, bh->weight, bh->bias, a.bv, x32.st));
    NL_CHECK_HIP(hipMemcpyAsync(a.wts, out->weights, sizeof(float) * (size_t)R * S, hipMemcpyDeviceToDevice, x32.st));
    NL_TRY(nl_launch_beta_forward(a.wts, a.bv, R, S, bh->beta_min, bh->beta, x32.st));
  }
  return NL_OK;
}

}  // namespace

struct BwdCtx { nl_config c32, cbw; Ctx x32, xb; };
static void make_bwd_ctx(BwdCtx& B, const nl_config* cfg, const void* packed, void* stream) {
  B.c32 = *cfg; B.cbw = *cfg;
  // recomputed forward: exact fp32 in the fp32 mode, three-term split-FP16 (products good to ~2^-22, the speed of split-bf16) otherwise — see
  // nl_point_mlp_backward for why split-bf16 is not enough there; the way back: split-bf16
  B.c32.precision = cfg->precision == NL_PREC_F32 ? NL_PREC_F32 : NL_PREC_F16X3_INTERNAL;
  if (B.cbw.precision == NL_PREC_BF16) B.cbw.precision = NL_PREC_BF16X3;
  B.x32 = make_ctx(&B.c32, packed, stream); B.xb = make_ctx(&B.cbw, packed, stream);
}

static size_t point_bwd_bytes(const nl_config* cfg, int64_t n, bool train = false) { Bump b{nullptr, 0}; PtBwdBufs p; carve_ptb(b, cfg, n, 8, p, train); return b.off; }
// nl_train_grads -> TrainOut (validated)
static int resolve_train(const nl_config* cfg, const nl_train_grads* g, TrainOut& t) {
  memset(&t, 0, sizeof(t));
  if (!g) return NL_OK;
  for (int i = 0; i < 4; ++i) if (g->reserved[i] != 0) return NL_ERR_BAD_ARG;
  if (g->weights) for (int i = 0; i < kNumWeights; ++i) t.w[i] = g->weights[i];
  t.sp_feat = g->support_feature;
  t.feat_maps = g->feat_maps; t.pfeat_maps = g->blend_feat_maps; t.vis_maps = g->vis_featmaps;
  if (!g->scratch || g->scratch_bytes < nl_train_scratch_bytes(cfg) || ((uintptr_t)g->scratch & 15)) return NL_ERR_WORKSPACE;
  t.scratch = (float*)g->scratch; t.scratch_floats = g->scratch_bytes / sizeof(float);
  return NL_OK;
}
static size_t mv_bwd_bytes(const nl_config* cfg, int V, int64_t n, bool blend, bool train = false) {
  Bump b{nullptr, 0}; MvBwdBufs m; carve_mvb(b, cfg, V, n, blend, m, train); return b.off;
}
static int64_t mv_bwd_chunk(const nl_config* cfg, int V, int64_t N, bool blend, size_t ws_bytes, bool train = false) {
  const int64_t fit = largest_chunk(N, ws_bytes, [&](int64_t n) { return mv_bwd_bytes(cfg, V, n, blend, train); });
  return fit < (1 << 18) ? fit : (1 << 18);
}
static size_t unet_bwd_bytes(const nl_config* cfg, int64_t r, bool train = false) { Bump b{nullptr, 0}; UnBwdBufs q; carve_unb(b, cfg, r, q, train); return b.off; }
static size_t render_bwd_bytes(const nl_config* cfg, int V, int64_t r, bool train) { Bump b{nullptr, 0}; RbBufs a; carve_rb(b, cfg, V, r, a, train); return b.off; }

extern "C" {

size_t nl_point_mlp_backward_workspace_bytes(const nl_config* cfg, int64_t N) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  const int64_t n = N < 1 ? 1 : (N > (1 << 14) ? (1 << 14) : N);   // recommended: chunks of <= 16 384 samples (131 072 neighbour rows, ~1.1 GB at W = 256)
  return point_bwd_bytes(cfg, n);
}

size_t nl_train_scratch_bytes(const nl_config* cfg) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  const int F = cfg->C + 3;
  // the largest weight the split-K kernel is asked for: conv_out (W, 3 (W + 32)) is done one tap at a time -> W x (W + 32); out_fc.0 64 x (2F + 3); base_mlp.0 W x (F + 90)
  size_t mx = (size_t)cfg->W * (F + 90);
  if ((size_t)64 * (2 * F + 3) > mx) mx = (size_t)64 * (2 * F + 3);
  if ((size_t)128 * 128 > mx) mx = (size_t)128 * 128;                       // the U-Net's fixed-width layers (one tap / one phase at a time)
  if ((size_t)cfg->C * cfg->W > mx) mx = (size_t)cfg->C * cfg->W;           // feat_mlp.2
  size_t fl = nl_wgrad_scratch_floats(0, 1, (int)(mx + 256));
  const size_t ln = (size_t)258 * 2 * cfg->S * (cfg->W > 64 ? cfg->W : 64);   // the U-Net's LayerNorm tables: 2 S max(W, 64) sums + up to 256 partial rows of them
  if (ln > fl) fl = ln;
  if (nl_dec_wpart_floats() > fl) fl = nl_dec_wpart_floats();   // the decoder backward's per-wave partial sets
  return sizeof(float) * fl;
}
size_t nl_point_mlp_backward_train_workspace_bytes(const nl_config* cfg, int64_t N) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg)) return 0;
  const int64_t n = N < 1 ? 1 : (N > (1 << 15) ? (1 << 15) : N);
  return point_bwd_bytes(cfg, n, true);
}
int nl_point_mlp_backward(const nl_config* cfg, const void* packed, const nl_frame* f, const float* xyz, const float* dir, int64_t dir_stride,
                          const float* mv_feat, int64_t N, int K, const int32_t* knn_idx, const float* knn_d2, const float* g_feature_agg, float* g_xyz,
                          float* g_dir, float* g_mv_feat, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  return nl_point_mlp_backward_train(cfg, packed, f, xyz, dir, dir_stride, mv_feat, N, K, knn_idx, knn_d2, g_feature_agg, g_xyz, g_dir, g_mv_feat, nullptr, ws,
                                     ws_bytes, stream);
}
int nl_point_mlp_backward_train(const nl_config* cfg, const void* packed, const nl_frame* f, const float* xyz, const float* dir, int64_t dir_stride,
                                const float* mv_feat, int64_t N, int K, const int32_t* knn_idx, const float* knn_d2, const float* g_feature_agg, float* g_xyz,
                                float* g_dir, float* g_mv_feat, const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (N == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !f || !xyz || !mv_feat || !g_feature_agg || !g_xyz || !ws || N < 0 || K < 1 || K > 8 || (g_dir && !dir)) return NL_ERR_BAD_ARG;
  const bool train = grads != nullptr;
  TrainOut T;
  NL_TRY(resolve_train(cfg, grads, T));   // (validated before anything is dereferenced)
  if (f->M < 1) return NL_ERR_UNSUPPORTED;
  const int64_t fit = largest_chunk(N, ws_bytes, [&](int64_t n) { return point_bwd_bytes(cfg, n, train); });   // largest sample chunk whose buffers fit the workspace
  if (fit == 0) return NL_ERR_WORKSPACE;
  // Precision of the two halves (measured):
  //  * the RECOMPUTED FORWARD must be much better than split-bf16: the derivative of a LeakyReLU network is piecewise constant, and a forward that
  //    is 1e-5 off flips the sign of a few pre-activations near zero — every flip changes that neighbour row's gradient by a few percent (2e-2 in
  //    the max-norm of g_xyz with a split-bf16 recompute against 4e-6 with exact fp32; plain fp32 autograd is 4e-3 from the fp64 gradient for the
  //    same reason).  Exact fp32 in the fp32 mode; three-term split-FP16 (~2^-22) otherwise: 40x fewer flips than split-bf16 at the same speed;
  //  * the transposed-weight products of the way back are linear in the incoming gradient and run in split-bf16 (1e-5, no discontinuity).
  const int64_t NC = fit < (1 << 17) ? fit : (1 << 17);
  BwdCtx B; make_bwd_ctx(B, cfg, packed, stream);
  const Ctx &xf = B.x32, &xb = B.xb;   // recomputed forward / way back
  const int W = cfg->W;
  for (int64_t n0 = 0; n0 < N; n0 += NC) {
    const int64_t nc = N - n0 < NC ? N - n0 : NC;
    Bump b{(char*)ws, 0}; PtBwdBufs p; carve_ptb(b, cfg, nc, 8, p, train);
    NL_TRY(do_point_backward(xb, xf, f, xyz + 3 * n0, dir ? dir + dir_stride * n0 : nullptr, (int)dir_stride, mv_feat + n0 * W, nc, K, g_feature_agg + n0 * W,
                             g_xyz + 3 * n0, g_dir ? g_dir + 3 * n0 : nullptr, g_mv_feat ? g_mv_feat + n0 * W : nullptr, p,
                             knn_idx ? knn_idx + n0 * K : nullptr, knn_d2 ? knn_d2 + n0 * K : nullptr, train ? &T : nullptr));
  }
  return NL_OK;
}

size_t nl_mv_aggregate_backward_train_workspace_bytes(const nl_config* cfg, int V, int64_t N) {
  NL_EFF_CFG(cfg);
  return cfg_ok(cfg) && V >= 1 && V <= NL_MAX_VIEWS ? mv_bwd_bytes(cfg, V, N < 1 ? 1 : (N > (1 << 15) ? (1 << 15) : N), false, true) : 0;
}
size_t nl_blend_backward_train_workspace_bytes(const nl_config* cfg, int V, int64_t N) {
  NL_EFF_CFG(cfg);
  return cfg_ok(cfg) && V >= 1 && V <= NL_MAX_VIEWS ? mv_bwd_bytes(cfg, V, N < 1 ? 1 : (N > (1 << 15) ? (1 << 15) : N), true, true) : 0;
}
size_t nl_mv_aggregate_backward_workspace_bytes(const nl_config* cfg, int V, int64_t N) {
  NL_EFF_CFG(cfg);
  return cfg_ok(cfg) && V >= 1 && V <= NL_MAX_VIEWS ? mv_bwd_bytes(cfg, V, N < 1 ? 1 : (N > (1 << 16) ? (1 << 16) : N), false) : 0;
}
int nl_mv_aggregate_backward(const nl_config* cfg, const void* packed, const nl_frame* f, const float* xyz, int64_t N, const float* g_mv_feat, float* g_xyz,
                             void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  return nl_mv_aggregate_backward_train(cfg, packed, f, xyz, N, g_mv_feat, g_xyz, nullptr, ws, ws_bytes, stream);
}
int nl_mv_aggregate_backward_train(const nl_config* cfg, const void* packed, const nl_frame* f, const float* xyz, int64_t N, const float* g_mv_feat, float* g_xyz,
                                   const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (N == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !f || !xyz || !g_mv_feat || !g_xyz || !ws || N < 0) return NL_ERR_BAD_ARG;
  const bool train = grads != nullptr;
  TrainOut T;
  NL_TRY(resolve_train(cfg, grads, T));
  const int V = f->views.V, W = cfg->W;
  const int64_t NC = mv_bwd_chunk(cfg, V, N, false, ws_bytes, train);
  if (NC == 0) return NL_ERR_WORKSPACE;
  BwdCtx B; make_bwd_ctx(B, cfg, packed, stream);
  for (int64_t n0 = 0; n0 < N; n0 += NC) {
    const int64_t nc = N - n0 < NC ? N - n0 : NC;
    Bump b{(char*)ws, 0}; MvBwdBufs m; carve_mvb(b, cfg, V, nc, false, m, train);
    NL_TRY(do_mv_backward(B.xb, B.x32, f, xyz + 3 * n0, nc, g_mv_feat + n0 * W, g_xyz + 3 * n0, m, train ? &T : nullptr));
  }
  return NL_OK;
}

size_t nl_blend_workspace_bytes(const nl_config* cfg, int V, int64_t N) {
  NL_EFF_CFG(cfg);
  return cfg_ok(cfg) && V >= 1 && V <= NL_MAX_VIEWS ? mv_bwd_bytes(cfg, V, N < 1 ? 1 : (N > (1 << 16) ? (1 << 16) : N), true) : 0;
}
int nl_blend(const nl_config* cfg, const void* packed, const nl_frame* f, const float* qc, const float* xyz, const float* feature_agg, int64_t N, float* rgb_s,
             void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (N == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !f || !qc || !xyz || !feature_agg || !rgb_s || !ws || N < 0) return NL_ERR_BAD_ARG;
  const int V = f->views.V, W = cfg->W;
  const int64_t NC = mv_bwd_chunk(cfg, V, N, true, ws_bytes);
  if (NC == 0) return NL_ERR_WORKSPACE;
  Ctx x = make_ctx(cfg, packed, stream);
  for (int64_t n0 = 0; n0 < N; n0 += NC) {
    const int64_t nc = N - n0 < NC ? N - n0 : NC;
    Bump b{(char*)ws, 0}; MvBwdBufs m; carve_mvb(b, cfg, V, nc, true, m);
    NL_TRY(do_blend_forward(x, f, qc, xyz + 3 * n0, feature_agg + n0 * W, nc, rgb_s + 3 * n0, m));
  }
  return NL_OK;
}
int nl_blend_backward(const nl_config* cfg, const void* packed, const nl_frame* f, const float* qc, const float* xyz, const float* feature_agg, int64_t N,
                      const float* g_rgb_s, float* g_xyz, float* g_feature_agg, float* g_query_center, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  return nl_blend_backward_train(cfg, packed, f, qc, xyz, feature_agg, N, g_rgb_s, g_xyz, g_feature_agg, g_query_center, nullptr, ws, ws_bytes, stream);
}
int nl_blend_backward_train(const nl_config* cfg, const void* packed, const nl_frame* f, const float* qc, const float* xyz, const float* feature_agg, int64_t N,
                            const float* g_rgb_s, float* g_xyz, float* g_feature_agg, float* g_query_center, const nl_train_grads* grads, void* ws,
                            size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (N == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !f || !qc || !xyz || !feature_agg || !g_rgb_s || !g_xyz || !ws || N < 0) return NL_ERR_BAD_ARG;
  const bool train = grads != nullptr;
  TrainOut T;
  NL_TRY(resolve_train(cfg, grads, T));
  const int V = f->views.V, W = cfg->W;
  const int64_t NC = mv_bwd_chunk(cfg, V, N, true, ws_bytes, train);
  if (NC == 0) return NL_ERR_WORKSPACE;
  BwdCtx B; make_bwd_ctx(B, cfg, packed, stream);
  for (int64_t n0 = 0; n0 < N; n0 += NC) {
    const int64_t nc = N - n0 < NC ? N - n0 : NC;
    Bump b{(char*)ws, 0}; MvBwdBufs m; carve_mvb(b, cfg, V, nc, true, m, train);
    NL_TRY(do_blend_backward(B.xb, B.x32, f, qc, xyz + 3 * n0, feature_agg + n0 * W, nc, g_rgb_s + 3 * n0, g_xyz + 3 * n0,
                             g_feature_agg ? g_feature_agg + n0 * W : nullptr, g_query_center ? g_query_center + 3 * n0 : nullptr, m, train ? &T : nullptr));
  }
  return NL_OK;
}

size_t nl_render_rays_backward_workspace_bytes(const nl_config* cfg, int V, int64_t R, int train) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg) || V < 1 || V > NL_MAX_VIEWS) return 0;
  const int64_t cap = (1 << 16) / cfg->S > 1 ? (1 << 16) / cfg->S : 1;   // recommended chunk: ~64 k samples (~70 KB of workspace per sample at W = 256)
  return render_bwd_bytes(cfg, V, R < 1 ? 1 : (R > cap ? cap : R), train != 0);
}
int nl_render_rays_backward(const nl_config* cfg, const void* packed, const nl_frame* f, const float* query_center, const float* ray_centers, const float* rays_o,
                            const float* rays_d, const float* z_vals, int64_t R, int white_bkgd, const nl_render_cotangents* g, float* g_rays_o, float* g_rays_d,
                            float* g_query_center_rows, const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !f || (!query_center && !ray_centers) || !rays_o || !rays_d || !z_vals || !g || !g_rays_o || !g_rays_d || !ws || R < 0) return NL_ERR_BAD_ARG;
  if (g->reserved[0] != nullptr || (g->knn_idx == nullptr) != (g->knn_d2 == nullptr)) return NL_ERR_BAD_ARG;
  const bool train = grads != nullptr;
  TrainOut T;
  NL_TRY(resolve_train(cfg, grads, T));
  if (f->M < 1) return NL_ERR_UNSUPPORTED;
  const int V = f->views.V, S = cfg->S, C = cfg->C;
  const int64_t RC = largest_chunk(R, ws_bytes, [&](int64_t r) { return render_bwd_bytes(cfg, V, r, train); });
  if (RC == 0) return NL_ERR_WORKSPACE;
  BwdCtx B; make_bwd_ctx(B, cfg, packed, stream);
  for (int64_t r0 = 0; r0 < R; r0 += RC) {
    const int64_t rc = R - r0 < RC ? R - r0 : RC;
    Bump b{(char*)ws, 0}; RbBufs a; carve_rb(b, cfg, V, rc, a, train);
    RbCot ct{g->g_rgb ? g->g_rgb + 3 * r0 : nullptr, g->g_depth ? g->g_depth + r0 : nullptr, g->g_depth_uncertainty ? g->g_depth_uncertainty + r0 : nullptr,
             g->g_feat ? g->g_feat + r0 * C : nullptr, g->g_weights ? g->g_weights + r0 * S : nullptr,
             g->knn_idx ? g->knn_idx + r0 * S * 8 : nullptr, g->knn_d2 ? g->knn_d2 + r0 * S * 8 : nullptr};
    NL_TRY(do_render_backward(B.xb, B.x32, f, query_center, ray_centers ? ray_centers + 3 * r0 : nullptr, rays_o + 3 * r0, rays_d + 3 * r0, z_vals + r0 * S, rc,
                              white_bkgd, ct, g_rays_o + 3 * r0,
                              g_rays_d + 3 * r0, g_query_center_rows ? g_query_center_rows + 3 * r0 : nullptr, a, train ? &T : nullptr));
  }
  return NL_OK;
}

// The gradient path's forward and backward as a PAIR that shares one workspace: the forward call leaves the staged activations there, the backward call
// walks back from them without recomputing.  The whole batch must fit the workspace as one chunk (NL_ERR_WORKSPACE otherwise: use nl_render_rays +
// nl_render_rays_backward, which chunk).
size_t nl_render_rays_keep_workspace_bytes(const nl_config* cfg, int V, int64_t R, int train) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg) || V < 1 || V > NL_MAX_VIEWS || R < 1) return 0;
  return render_bwd_bytes(cfg, V, R, train != 0);
}
int nl_render_rays_forward_keep(const nl_config* cfg, const void* packed, const nl_frame* f, const float* query_center, const float* ray_centers, const float* rays_o,
                                const float* rays_d, const float* z_vals, int64_t R, int white_bkgd, const nl_render_out* out, const nl_beta_head* beta, int train,
                                void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !f || (!query_center && !ray_centers) || !rays_o || !rays_d || !z_vals || !out || !ws || R < 0) return NL_ERR_BAD_ARG;
  if (beta && (!beta->weight || !beta->bias || !beta->beta)) return NL_ERR_BAD_ARG;
  if (!out->rgb || !out->depth || !out->weights || !out->mask || !out->depth_uncertainty) return NL_ERR_BAD_ARG;
  if (f->M < 1) return NL_ERR_UNSUPPORTED;
  const int V = f->views.V;
  if (ws_bytes < render_bwd_bytes(cfg, V, R, train != 0)) return NL_ERR_WORKSPACE;
  BwdCtx B; make_bwd_ctx(B, cfg, packed, stream);
  Bump b{(char*)ws, 0}; RbBufs a; carve_rb(b, cfg, V, R, a, train != 0);
  NL_TRY(render_forward_staged(B.x32, f, query_center, ray_centers, rays_o, rays_d, z_vals, R, out->feat != nullptr, nullptr, nullptr, a, train == 0));
  return render_outputs_staged(B.x32, f, R, white_bkgd, out, a, beta);
}
int nl_render_rays_backward_kept(const nl_config* cfg, const void* packed, const nl_frame* f, const float* query_center, const float* ray_centers, const float* rays_d,
                                 int64_t R, int white_bkgd, const nl_render_cotangents* g, const nl_beta_head* beta, float* g_rays_o, float* g_rays_d,
                                 float* g_query_center_rows, const nl_train_grads* grads, void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !f || (!query_center && !ray_centers) || !rays_d || !g || !g_rays_o || !g_rays_d || !ws || R < 0) return NL_ERR_BAD_ARG;
  if (beta && (!beta->weight || !beta->bias || (beta->g_weight && !grads))) return NL_ERR_BAD_ARG;   // (the weight gradient's split-K scratch comes with `grads`)
  if (g->reserved[0] != nullptr || g->knn_idx || g->knn_d2) return NL_ERR_BAD_ARG;   // (the neighbours are in the workspace)
  const bool train = grads != nullptr;
  TrainOut T;
  NL_TRY(resolve_train(cfg, grads, T));
  if (f->M < 1) return NL_ERR_UNSUPPORTED;
  const int V = f->views.V;
  if (ws_bytes < render_bwd_bytes(cfg, V, R, train)) return NL_ERR_WORKSPACE;
  BwdCtx B; make_bwd_ctx(B, cfg, packed, stream);
  Bump b{(char*)ws, 0}; RbBufs a; carve_rb(b, cfg, V, R, a, train);
  RbCot ct{g->g_rgb, g->g_depth, g->g_depth_uncertainty, g->g_feat, g->g_weights, nullptr, nullptr};
  return render_backward_staged(B.xb, B.x32, f, query_center, ray_centers, rays_d, R, white_bkgd, ct, g_rays_o, g_rays_d, g_query_center_rows, a, train ? &T : nullptr,
                                beta);
}

size_t nl_ray_unet_backward_train_workspace_bytes(const nl_config* cfg, int64_t R) {
  NL_EFF_CFG(cfg);
  return cfg_ok(cfg) ? unet_bwd_bytes(cfg, R < 1 ? 1 : (R > 1024 ? 1024 : R), true) : 0;
}
size_t nl_ray_unet_backward_workspace_bytes(const nl_config* cfg, int64_t R) {
  NL_EFF_CFG(cfg);
  return cfg_ok(cfg) ? unet_bwd_bytes(cfg, R < 1 ? 1 : (R > 1024 ? 1024 : R)) : 0;   // recommended: chunks of <= 1024 rays
}
int nl_ray_unet_backward(const nl_config* cfg, const void* packed, const float* xin, int64_t R, const float* g_geo, float* g_x, void* ws, size_t ws_bytes,
                         void* stream) {
  NL_EFF_CFG(cfg);
  return nl_ray_unet_backward_train(cfg, packed, xin, R, g_geo, g_x, nullptr, ws, ws_bytes, stream);
}
int nl_ray_unet_backward_train(const nl_config* cfg, const void* packed, const float* xin, int64_t R, const float* g_geo, float* g_x, const nl_train_grads* grads,
                               void* ws, size_t ws_bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (R == 0) return NL_OK;
  if (!cfg_ok(cfg) || !packed || !xin || !g_geo || !g_x || !ws || R < 0) return NL_ERR_BAD_ARG;
  const bool train = grads != nullptr;
  TrainOut T;
  NL_TRY(resolve_train(cfg, grads, T));
  const int64_t RC = largest_chunk(R, ws_bytes, [&](int64_t r) { return unet_bwd_bytes(cfg, r, train); });
  if (RC == 0) return NL_ERR_WORKSPACE;
  BwdCtx B; make_bwd_ctx(B, cfg, packed, stream);
  const size_t row = (size_t)cfg->S * cfg->W;
  for (int64_t r0 = 0; r0 < R; r0 += RC) {
    const int64_t rc = R - r0 < RC ? R - r0 : RC;
    Bump b{(char*)ws, 0}; UnBwdBufs q; carve_unb(b, cfg, rc, q, train);
    NL_TRY(do_unet_backward(B.xb, B.x32, xin + r0 * row, rc, g_geo + r0 * row, g_x + r0 * row, q, train ? &T : nullptr));
  }
  return NL_OK;
}


}  // extern "C"
