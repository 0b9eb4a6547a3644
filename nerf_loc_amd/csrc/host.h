// Shared header of the HOST units of libnerfloc_render.so — abi.hip, pack.hip, render.hip and render_bwd.hip.  common.h does not include it, and of the kernel
// files only the localisation head's (s2d.hip, fine.hip, sct.hip) do, for the two entry-point helpers at its top (nl_prec_status_no_mx, nl_allow_dynamic_lds).
// It holds the types the drivers hand to each other (packed-blob layout, per-stage buffer sets, GEMM descriptors, the frame) and ONE declaration of every host
// function that one of the four units defines and another calls, grouped by the defining file (default arguments live here only), all in namespace nlhost
// (hidden visibility like everything else; exports.map lists the C-ABI alone).  The defining unit includes it too, so a definition that drifts from its
// declaration is an ambiguous call / a redefined default argument at compile time or an undefined symbol at link time (-Wl,--no-undefined). What only one unit
// uses stays static / in an anonymous namespace of that unit.  Kernel launchers shared with the kernel files: launch.h.
#pragma once
#include <atomic>
#include "common.h"

// ---- entry-point helpers of the units whose kernels have no NL_PREC_F16MX form (s2d.hip, fine.hip, sct.hip) -------------------------------------------
// NL_OK / NL_ERR_UNSUPPORTED (F16MX) / NL_ERR_BAD_ARG (no precision at all) for a precision argument
inline int nl_prec_status_no_mx(int precision) {
  if (precision == NL_PREC_F16MX) return NL_ERR_UNSUPPORTED;
  if (precision != NL_PREC_F32 && precision != NL_PREC_BF16X3 && precision != NL_PREC_BF16) return NL_ERR_BAD_ARG;
  return NL_OK;
}
// A kernel whose dynamic LDS may exceed the 64 KB a kernel can use unasked: raise its limit to `bytes`, the largest supported configuration's need, once per device
// and kernel (`done`: one static per kernel; bit d = device d; two threads that race both set the same value).  Each launch still asks for its own size.
inline int nl_allow_dynamic_lds(const void* kernel, size_t bytes, std::atomic<unsigned long long>& done) {
  int dev = 0;
  NL_CHECK_HIP(hipGetDevice(&dev));
  const unsigned long long bit = 1ull << (dev & 63);
  if (dev < 64 && (done.load(std::memory_order_acquire) & bit)) return NL_OK;
  NL_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  if (dev < 64) done.fetch_or(bit, std::memory_order_release);
  return NL_OK;
}

struct nl_frame {
  NlViews views;
  int C;
  const float* images; const float* feat; float* visf_hwc;
  const float* sp_xyz; const float* sp_feat; const float* sp_conf; const float* sp_dir;
  int64_t M;
  NlKnnGrid grid;
  float* ptt;               // [(M+1)][W] table T (see G_PTT), built lazily per (frame, weights); row M = bias
  const void* ptt_for; uint64_t ptt_gen;
  float* pfeat;             // (V,h,w,32) feature maps projected through the blend layer's feature columns
  const void* pfeat_for; uint64_t pfeat_gen;   // packed weights (address + pack generation) pfeat was computed with (lazily, first render of the frame)
  float* views_dev;         // device copy of the per-view matrices: [16][12] proj_ibr rows, then [16][3] camera centres
  float *tr_gT, *tr_tmp;    // training scratch sized by the table: d loss / d T (M, W) and (M, ldf_of(C)) staging rows (pt_backward_only)
  float views_host[16 * 15];
  // side stream of the fused render path (exact KNN beside the multi-view gather): owned by the frame, created in nl_frame_create —
  // never lazily inside a render call (stream / event creation is illegal during graph capture) and never shared between frames, so two
  // renderers on two caller streams do not record into each other's events.  side_ok == false: everything runs on the caller's stream.
  hipStream_t side; hipEvent_t ev_fork, ev_join; bool side_ok;
  // precision guard (NL_RENDER_PRECISION_GUARD): the mode guarded calls render this frame in once one of them found the conditioning indicator beyond the
  // configured mode's validated range (-1: none yet), how often that happened, and the mode the last guarded call's outputs were produced in.  Host-side
  // state of a frame that is documented as not re-entrant; mutable because render calls take the frame as const.
  mutable int guard_prec = -1; mutable int guard_escalations = 0; mutable int guard_last_prec = -1;
};

namespace nlhost {

// ------------------------------------------------------------------------------------------ weight table (pack.hip: kWeightNames)
constexpr int kNumWeights = 84;
extern const char* kWeightNames[];
enum {
  T_RD0W = 0, T_RD0B, T_RD2W, T_RD2B, T_DEC = 4,  // 24 decoder tensors
  T_OUT0W = 28, T_OUT0B, T_OUT2W, T_OUT2B, T_B0W, T_B0B, T_B2W, T_B2B, T_B4W, T_B4B,
  T_WQ, T_WK, T_WV, T_FC, T_LNW, T_LNB, T_UNET = 44,  // 7 x {conv w, conv b, ln w, ln b}
  T_SIGW = 72, T_SIGB, T_F0W, T_F0B, T_F2W, T_F2B, T_BL0W, T_BL0B, T_BL2W, T_BL2B, T_BL4W, T_BL4B
};

// ------------------------------------------------------------------------------------------ GEMM layer table
enum {
  G_OUTFC0 = 0, G_OUTFC2, G_BASE0, G_BASE2, G_BASE4, G_KV, G_Q, G_FC, G_CONV1, G_CONV2, G_CONV3,
  G_T3E, G_T3O, G_T2E, G_T2O, G_T1E, G_T1O, G_T3M, G_T2M, G_T1M, G_FEAT0P, G_BLENDAP, G_QP, G_CONVOUT, G_FEAT0, G_FEAT2, G_BLENDA, G_BLENDP, G_PTT,
  G_FC_T, G_Q_T, G_KV_T, G_BASE4_T, G_BASE2_T, G_BASE0_T,   // transposed weights: input gradients of the neural-point branch (do_point_backward)
  G_OUTFC2_T, G_OUTFC0_T, G_BLENDA_T,                         // ... of the multi-view aggregation's out_fc and of the blend's per-sample projection
  G_UB_OUTA, G_UB_OUTB, G_UB_T1, G_UB_T2, G_UB_T3, G_UB_C3, G_UB_C2, G_UB_C1,   // ... of the ray U-Net's seven convolutions (do_unet_backward)
  G_BASE0_TF,                                                                    // training: base_mlp.0 towards its support-feature columns
  G_FEAT0_T, G_FEAT2_T,                                                          // whole-path backward: feat_mlp's two layers towards their inputs
  G_BASE0_S,                                                                     // base_mlp.0's posenc + ray_diff_fc columns (the staged forward on the table T)
  G_CONV1F, G_CONVOUTF,   // conv1 / conv_out with the feature_agg channels of every 32-block in ACCUMULATOR order: their input is the chain kernel's fragment image
  G_COUNT
};
enum { U_CONV1 = 0, U_CONV2, U_CONV3, U_T3, U_T2, U_T1, U_OUT, U_COUNT };

struct GemmDim { int K, N, Kpad, Npad; bool bias; };

struct Layout {
  GemmDim g[G_COUNT];
  size_t b32[G_COUNT], bhi[G_COUNT], blo[G_COUNT], bst[G_COUNT], bsh[G_COUNT], bias[G_COUNT];   // bsh: the weight stream in fp16 hi / lo (split-FP16 arithmetic)
  size_t rd_w, dec_w, sig_w, sig_b, bl2_w, bl2_b, bl4_w, bl4_b, ln_g, ln_b;
  size_t pt_stream, pt_stream2, pt_stream2_mx, pt_stream2_f16, pt_bwd_stream, mvf_pack, pt_bias, blw, dec_mfma, zeros;   // blw: [32][8] rgb/vis/angle columns of rgb_blending_mlp.0 + bias[32]  // fused point-branch weight stream (W in {64,128,256}) and its 3 bias rows
  size_t mx_convout;   // NL_PREC_F16MX (round 6): fp6 images + block scales of G_CONVOUTF for tgemm_mx_kernel (W = 256)
  size_t mx_feat0;     // ... and of G_FEAT0P for feat_comp_mx_kernel (feat_mlp.0 + compositing in one kernel)
  size_t un_g[U_COUNT], un_b[U_COUNT];     // LayerNorm([C, L]) affine tables, position-major (L, C)
  size_t un_gl[U_COUNT], un_bl[U_COUNT];   // the same tables in the accumulator-lane order of the GEMM that fuses the LayerNorm (un_n x un_so)
  int un_c[U_COUNT], un_l[U_COUNT], un_n[U_COUNT], un_so[U_COUNT];
  size_t total;
};

struct PackInfo { uint64_t gen, bst, bsh; };

// ---- workspace carving ---------------------------------------------------------------------------
// Debug facility (nl_debug_bump_gap / nl_debug_check_gaps, used by the test-suite's guarded workspaces): with a gap size set, every buffer carved from a
// workspace is followed by that many untouched bytes, and the carve records [exact end of the buffer, start of the next one) — the caller fills the workspace
// with a pattern before the call and the check finds any byte a kernel wrote outside its buffer, also BETWEEN two buffers of one workspace.
// The gap size and the recorded regions are state of abi.hip alone (nl_debug_*); this template reaches them through bump_gap_after (abi.hip), one small function
// rather than two extern variables: no other unit can then write them, and a carve is a handful of calls per entry point, not a hot path.
// bump_gap_after(end, pad): the gap size in force (0: facility off); when it is non-zero and end != null it records [end, end + pad + gap), where pad is
// what alignment leaves behind the buffer's exact end.
size_t bump_gap_after(char* end, size_t pad);
struct Bump {
  char* base; size_t off;
  template <class T> T* take(size_t count) {
    size_t o = off;
    const size_t al = nl_align_up(count * sizeof(T), 256);
    off += al + bump_gap_after(base ? base + o + count * sizeof(T) : nullptr, al - count * sizeof(T));
    return base ? (T*)(base + o) : nullptr;
  }
};
// "largest chunk whose buffers fit the workspace": the largest n in [1, n_max] with bytes_of(n) <= ws_bytes (bytes_of grows with n); 0 when not even one row fits
template <class F> int64_t largest_chunk(int64_t n_max, size_t ws_bytes, F bytes_of) {
  if (bytes_of(1) > ws_bytes) return 0;
  int64_t lo = 1, hi = n_max;
  while (lo < hi) { const int64_t mid = (lo + hi + 1) / 2; if (bytes_of(mid) <= ws_bytes) lo = mid; else hi = mid - 1; }
  return lo;
}

// ---- per-stage buffers ---------------------------------------------------------------------------
struct MvBufs { float *vis, *dd, *g393, *t64; };
struct PtBufs { int* idx; float *d2, *X, *H1, *H2, *KV, *Q, *O, *FCo, *wscale; };
struct UnBufs { float *r1, *c1, *r2, *c2, *r3, *c3, *x0r, *x0, *x1r, *x1, *x2r, *x2, *outr; };
struct HdBufs { float *sigma, *fth, *hc, *wsum, *blA, *rgb_s; int *n_alive, *tile_list, *tile_count; };

// leading dimensions of the two feature-width-dependent staging rows (416 and 288 at C = 192).  LDG: mv_stats zero-fills columns
// 2F+3 .. LDG-1, so out_fc's K is a whole number of 32-wide chunks; LDX: [posenc 63 | ray_diff 27 | F] padded likewise
inline int ldg_of(int C) { return (int)nl_align_up(2 * (C + 3) + 3, 32); }
inline int ldx_of(int C) { return (int)nl_align_up(C + 3 + 90, 32); }
inline int ldf_of(int C) { return (int)nl_align_up(C + 3, 32); }

struct RenderBufs {
  float *xyz, *z, *G, *bl1, *rgbv, *FA, *geo; int* valid_s;
  MvBufs mv; PtBufs pt; UnBufs un; HdBufs hd;
};
struct PtBwdBufs { int* idx; float *d2, *X, *H1, *H2, *H3, *KV, *Q, *O, *FCo, *wscale, *gpre, *gO, *gQ, *gKV, *gA, *gB, *gX, *aff, *tr, *gXF; unsigned* mk[3]; };
struct MvBwdBufs { float *vis, *dd, *g393, *t64, *G, *gA, *gt64, *gg393, *gvis, *gdd, *gpart, *bl1, *rgbv, *blA, *ghA, *gpf, *grgbv, *gang, *dtr, *btr, *ang; int* valid_s; };
struct UnBwdBufs { UnBufs u; float *geo, *gout, *gx2, *gx2r, *gcat1, *gx1r, *gcat2, *gx0r, *gc3, *gr3, *gc2, *gr2, *gc1, *gr1, *tmp, *aff; };
struct RbBufs {
  MvBwdBufs m; PtBwdBufs p; UnBwdBufs q;
  float *xyz, *zc, *FA, *sigma, *Hf, *rgb_s, *hc, *wsum4, *ghc, *gw, *g_sigma, *g_rgb_s, *gFA, *gtmp, *gpre4, *gxyz_m, *gxyz_p, *gdir, *gG, *gqcN, *wts, *bv, *gpre4b;
};

// ---- GEMM helper ----------------------------------------------------------------------------------
struct Ctx {
  const nl_config* c; Layout L; const char* pk; hipStream_t st;
  uint64_t has_bst = ~0ull, has_bsh = ~0ull;   // layers whose streaming-kernel images exist in pk (pack_info)
  bool mx = false;                             // NL_PREC_F16MX: the fused neural-point kernel multiplies as fp16 hi.hi + two MX-FP6 cross terms (everything else: BF16X3)
  template <class T> const T* p(size_t off) const { return (const T*)(pk + off); }
};

struct SegSpec { const float* ptr; int ld; int k; int ioff; int rdiv; int ntap = 1; int frag = 0; };   // frag: NlGemmSeg::frag

struct TileMap { const int* map; const int* count; };
struct RowEpi { const float* res; int ldres; const float* gamma; const float* beta; const float* scale; float eps; float* out; int kind = NL_EPI_LNROW; int pool = 0;
                const float* sig_w = nullptr; const float* sig_b = nullptr; float* sig_out = nullptr;
                unsigned* maskout = nullptr; const unsigned* maskin = nullptr;
                const float* tab = nullptr; const int* tabidx = nullptr; int ldtab = 0, tabK = 0, tabM = 0; };   // out: destination when fused; mask*: sign bits (common.h: ep_maskout / ep_maskin)

// do_point (render.hip)
struct ChainOut { float* fth; float* blA; bool* done; const float* t64 = nullptr; bool fa_frag = false; bool fa_f16 = false; };   // fa_frag: FA leaves the chain kernel as a fragment image (fa_f16: in split-FP16)
// do_heads_pre (render.hip)
struct BlendTaps { NlViews vw; const float* viewsdev; const float* pfeat; const float* xyz; };   // bl1 == null: the blend tail recomputes its per-(sample, view) rows
// Where a training step's backward calls ADD the gradients of the weights and of the per-frame tables (nl_train_grads, resolved)
struct TrainOut {
  float* w[kNumWeights];
  float* sp_feat;
  float *feat_maps, *pfeat_maps, *vis_maps;   // (V,h,w,C), (V,h,w,32), (V,vh,vw,32)
  float* scratch; size_t scratch_floats;
  bool any(int a, int b) const { for (int i = a; i < b; ++i) if (w[i]) return true; return false; }
};

// ---- fork / join of the fused render path's side stream ------------------------------------------------------------------
// The exact KNN (+ the aggregation scale) only needs the sample positions, like the multi-view gather kernels: nl_render_rays forks it
// onto the frame's side stream and joins before the neural-point kernel (events: graph-capturable).  SideJoin makes the join
// unconditional: whatever path leaves the scope after the fork — including an error return — the caller's stream waits for the
// side stream first, so no kernel is left writing the caller's workspace behind its back and an active capture stays well-formed.
struct SideJoin {
  hipStream_t main = nullptr, side = nullptr; hipEvent_t ev = nullptr; bool armed = false;
  void arm(hipStream_t m, hipStream_t s_, hipEvent_t e) { main = m; side = s_; ev = e; armed = true; }
  int join() {
    if (!armed) return NL_OK;
    armed = false;
    if (hipEventRecord(ev, side) != hipSuccess || hipStreamWaitEvent(main, ev, 0) != hipSuccess) return NL_ERR_HIP;
    return NL_OK;
  }
  ~SideJoin() { (void)join(); }
};

#define NL_TRY(e) do { int _rc = (e); if (_rc != NL_OK) return _rc; } while (0)
// First statement of every entry point that takes an nl_config: NL_PREC_F16MX is BF16X3 everywhere but in the fused neural-point kernel of the render path,
// so the library works on a BF16X3 copy of the configuration and remembers the request in nl_mx_ (nl_render_rays_ex passes it on as Ctx::mx)
#define NL_EFF_CFG(cfg)                                                                 \
  nl_config nl_eff_cfg_;                                                                 \
  bool nl_mx_ = false;                                                                   \
  if ((cfg) && (cfg)->precision == NL_PREC_F16MX) { nl_eff_cfg_ = *(cfg); nl_eff_cfg_.precision = NL_PREC_BF16X3; (cfg) = &nl_eff_cfg_; nl_mx_ = true; } \
  (void)nl_mx_

// ---- pack.hip --------------------------------------------------------------------------------------------
bool cfg_ok(const nl_config* c);
Layout make_layout(const nl_config* c);
// the generation stamp of a packed blob (0: not packed by this process) and which of its layers have streaming images (pack.hip: g_pack_gen)
uint64_t pack_generation(const void* pk);
PackInfo pack_info(const void* pk);

// ---- abi.hip ---------------------------------------------------------------------------------------------
// fills the launch descriptor; *fused says whether the optional row epilogue will run inside the GEMM (else the caller runs it)
int run_gemm(const Ctx& x, int g, const SegSpec* segs, int nseg, int64_t M, float* C, int ldc, int act,
             int So = 0, int Li = 0, int Lo = 0, int ostride = 1, int ooff = 0, const RowEpi* epi = nullptr, bool* fused = nullptr,
             const TileMap* tiles = nullptr);
Ctx make_ctx(const nl_config* c, const void* packed, void* stream);
// qrows != null: per-ray query centres (device, row = sample / S) instead of the one host-side centre qc
NlViews with_query(const nl_frame* f, const float* qc, const float* qrows = nullptr, int S = 1);
// per-frame tables derived from the weights, built once per (frame, pack generation)
int ensure_pfeat(const Ctx& x, const nl_frame* fc);
int ensure_ptt(const Ctx& x, const nl_frame* fc);
// nl_profile_begin / nl_profile_end: a pair of events for the caller to record around the dominant kernel (false: profiling is off)
bool prof_arm(hipEvent_t* e0, hipEvent_t* e1);

// ---- render.hip ------------------------------------------------------------------------------------------
void carve_un(Bump& b, const nl_config* c, int64_t R, UnBufs& u);
int do_unet(const Ctx& x, const float* in, int64_t R, float* geo, const UnBufs& u, float* sigma_out = nullptr, bool* sigma_done = nullptr,
            bool need_geo = true, int in_frag = 0, bool fuse_inner = false);

}  // namespace nlhost
