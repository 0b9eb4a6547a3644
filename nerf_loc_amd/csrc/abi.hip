// C-ABI of libnerfloc_render.so, the core: version / status strings, the debug and profile hooks, per-frame state, and the helpers every driver calls
// (run_gemm, make_ctx, the per-frame tables).  Weight packing: pack.hip; the stage entry points and the chunked render_rays orchestrator: render.hip;
// everything that exists for gradients: render_bwd.hip (include/nerfloc_render.h documents which reference code each entry point replaces).
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <new>
#include <vector>
#include <mutex>
#include "common.h"
#include "host.h"
using namespace nlhost;

// CU count for persistent kernels, per device id (launch.h)
int nl_persistent_cus() {
  static std::mutex mu;
  static int cus[64] = {0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return NL_ERR_HIP;
  std::lock_guard<std::mutex> lk(mu);
  if (dev < 64 && cus[dev] > 0) return cus[dev];
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) != hipSuccess) return NL_ERR_HIP;
  const int n = prop.multiProcessorCount > 8 ? prop.multiProcessorCount / 8 * 8 : 8;
  if (dev < 64) cus[dev] = n;
  return n;
}

namespace {

// the debug-gap facility's state (host.h: Bump)
size_t g_bump_gap = 0;
std::vector<std::pair<char*, size_t>> g_bump_gaps;

__global__ void gap_check_kernel(const unsigned char* __restrict__ p, size_t n, unsigned char pat, int* __restrict__ bad) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && p[i] != pat) atomicAdd(bad, 1);
}

// ---- measurement hook: HIP events around the dominant kernel (nl_profile_begin / nl_profile_end) -----------------
struct ProfState { bool on = false; std::vector<hipEvent_t> ev; int used = 0; };
ProfState g_prof;

static bool desc_ok(const nl_config* c, const nl_frame_desc* d) {
  return cfg_ok(c) && d && d->V >= 1 && d->V <= NL_MAX_VIEWS && d->H > 1 && d->Wimg > 1 && d->h > 1 && d->w > 1 && d->vis_h > 1 && d->vis_w > 1 && d->M >= 0 &&
         d->images && d->featmaps && d->vis_featmaps && d->proj_ibr && d->proj_neuray && d->cam_centers &&
         (d->M == 0 || (d->sp_xyz && d->sp_feature && d->sp_confidence && d->sp_direction));
}

}  // namespace

namespace nlhost {

size_t bump_gap_after(char* end, size_t pad) {
  if (g_bump_gap && end && g_bump_gaps.size() < (1u << 16)) g_bump_gaps.push_back({end, pad + g_bump_gap});
  return g_bump_gap;
}

bool prof_arm(hipEvent_t* e0, hipEvent_t* e1) {
  if (!g_prof.on) return false;
  if (g_prof.used + 2 > (int)g_prof.ev.size()) {
    hipEvent_t a, b;
    if (hipEventCreate(&a) != hipSuccess || hipEventCreate(&b) != hipSuccess) return false;
    g_prof.ev.push_back(a); g_prof.ev.push_back(b);
  }
  *e0 = g_prof.ev[g_prof.used]; *e1 = g_prof.ev[g_prof.used + 1];
  g_prof.used += 2;
  return true;
}

int run_gemm(const Ctx& x, int g, const SegSpec* segs, int nseg, int64_t M, float* C, int ldc, int act,
             int So, int Li, int Lo, int ostride, int ooff, const RowEpi* epi, bool* fused,
             const TileMap* tiles) {
  NlGemmArgs a;
  memset(&a, 0, sizeof(a));
  if (tiles) { a.tile_map = tiles->map; a.tile_count = tiles->count; }
  int ksum = 0;
  for (int i = 0; i < NL_GEMM_MAX_SEG; ++i) a.kstart[i] = 0x7fffffff;
  for (int i = 0; i < nseg; ++i) {
    a.kstart[i] = ksum;
    a.seg[i].ptr = segs[i].ptr; a.seg[i].ld = segs[i].ld; a.seg[i].k = segs[i].k; a.seg[i].ioff = segs[i].ioff;
    a.seg[i].rdiv = segs[i].rdiv > 0 ? segs[i].rdiv : 1;
    a.seg[i].vec = ((((size_t)segs[i].ptr) & 15) == 0 && (segs[i].ld & 3) == 0) ? 1 : 0;
    a.seg[i].ntap = segs[i].ntap > 1 ? segs[i].ntap : 1;
    a.seg[i].frag = segs[i].frag;
    if (a.seg[i].ntap > 1 && (segs[i].k & 31)) return NL_ERR_BAD_ARG;
    ksum += ((segs[i].k + 31) & ~31) * a.seg[i].ntap;   // every segment occupies round_up(k, 32) slots of K-space (one k-tile = one segment)
  }
  const GemmDim& d = x.L.g[g];
  if (ksum != ((d.K + 31) & ~31)) return NL_ERR_BAD_ARG;
  a.nseg = nseg; a.M = (int)M; a.K = d.K; a.N = d.N; a.Kpad = d.Kpad; a.Npad = d.Npad;
  int prec = x.c->precision;
  if (prec == NL_PREC_F16X3_INTERNAL) {   // split-FP16 where the streaming kernel applies (its only implementation), exact fp32 elsewhere
    a.Bst = x.pk + x.L.bsh[g];
    a.zeros = x.p<float>(x.L.zeros); a.C = C; a.ldc = ldc; a.N = d.N; a.M = (int)M;
    a.epi = NL_EPI_NONE;
    if (tiles || d.N > 256 || !((x.has_bsh >> g) & 1) || !nl_tgemm_supported(a, prec)) { prec = NL_PREC_F32; a.Bst = nullptr; }   // (a requested fused epilogue is simply not fused)
  }
  if (prec == NL_PREC_F32) a.B = x.pk + x.L.b32[g];
  else if (prec != NL_PREC_F16X3_INTERNAL) { a.B = x.pk + x.L.bhi[g]; a.Blo = x.pk + x.L.blo[g]; a.Bst = ((x.has_bst >> g) & 1) ? x.pk + x.L.bst[g] : nullptr; }
  // NL_PREC_F16MX: conv_out multiplies as fp16 hi.hi + two MX-FP6 cross terms too (tgemm_mx_kernel) when its images exist
  if (x.mx && g == G_CONVOUTF && prec == NL_PREC_BF16X3 && x.c->W == 256 && ((x.has_bsh >> g) & 1)) {
    a.Bsh_mx = x.pk + x.L.bsh[g]; a.Bmx = x.pk + x.L.mx_convout;
  }
  for (int i = 0; i < nseg; ++i) if (segs[i].frag == 3 && ((x.has_bsh >> g) & 1)) a.Bsh16 = x.pk + x.L.bsh[g];   // split-FP16 fragments: the layer's fp16 stream (conv1)
  a.zeros = x.p<float>(x.L.zeros);
  a.bias = d.bias ? x.p<float>(x.L.bias[g]) : nullptr;
  a.C = C; a.ldc = ldc; a.act = act;
  a.So = So; a.Li = Li; a.Lo = Lo; a.ostride = ostride; a.ooff = ooff;
  if (fused) *fused = false;
  if (epi) {
    a.epi = epi->kind; a.ep_pool = epi->pool; a.ep_res = epi->res; a.ep_ldres = epi->ldres; a.ep_gamma = epi->gamma; a.ep_beta = epi->beta;
    a.ep_scale = epi->scale; a.ep_eps = epi->eps;
    a.ep_sig_w = epi->sig_w; a.ep_sig_b = epi->sig_b; a.ep_sig_out = epi->sig_out;
    a.ep_maskout = epi->maskout; a.ep_maskin = epi->maskin;
    a.ep_tab = epi->tab; a.ep_tabidx = epi->tabidx; a.ep_ldtab = epi->ldtab; a.ep_tabK = epi->tabK; a.ep_tabM = epi->tabM;
    if (nl_tgemm_supported(a, prec)) { a.C = epi->out; if (fused) *fused = true; }
    else if (epi->tab) return NL_ERR_UNSUPPORTED;   // (no other kernel knows the table: the caller checks *fused first or keeps the full-width layer)
    else { a.epi = NL_EPI_NONE; a.ep_maskout = nullptr; a.ep_maskin = nullptr; }
  }
  if (tiles && !nl_tgemm_supported(a, prec)) { a.tile_map = nullptr; a.tile_count = nullptr; }   // generic kernels compute every row
  return nl_gemm_launch(a, prec, x.st);
}

Ctx make_ctx(const nl_config* c, const void* packed, void* stream) {
  Ctx x;
  x.c = c; x.L = make_layout(c); x.pk = (const char*)packed; x.st = (hipStream_t)stream;
  const PackInfo pi = pack_info(packed);
  x.has_bst = pi.bst; x.has_bsh = pi.bsh;
  return x;
}

NlViews with_query(const nl_frame* f, const float* qc, const float* qrows, int S) {
  NlViews v = f->views;
  v.qcam[0] = qc ? qc[0] : 0.f; v.qcam[1] = qc ? qc[1] : 0.f; v.qcam[2] = qc ? qc[2] : 0.f;
  v.qrows = qrows; v.qS = S > 0 ? S : 1;
  return v;
}

// per-frame projection of the support feature maps through the blend layer (exact fp32 MFMA), done once per (frame, weights)
int ensure_pfeat(const Ctx& x, const nl_frame* fc) {
  nl_frame* f = const_cast<nl_frame*>(fc);
  const uint64_t gen = pack_generation(x.pk);
  if (f->pfeat_for == (const void*)x.pk && f->pfeat_gen == gen) return NL_OK;
  nl_config c32 = *x.c;
  c32.precision = NL_PREC_F32;
  Ctx x32 = x;
  x32.c = &c32;
  SegSpec s{f->feat, f->C, f->C, 0, 1};
  NL_TRY(run_gemm(x32, G_BLENDP, &s, 1, (int64_t)f->views.V * f->views.h * f->views.w, f->pfeat, 32, NL_ACT_NONE));
  f->pfeat_for = (const void*)x.pk; f->pfeat_gen = gen;
  return NL_OK;
}

// per-frame table T for the fused point kernel (exact fp32 MFMA), once per (frame, weights)
int ensure_ptt(const Ctx& x, const nl_frame* fc) {
  nl_frame* f = const_cast<nl_frame*>(fc);
  const uint64_t gen = pack_generation(x.pk);
  if (f->ptt_for == (const void*)x.pk && f->ptt_gen == gen) return NL_OK;
  const int W = x.c->W, F = f->C + 3;
  nl_config c32 = *x.c;
  c32.precision = NL_PREC_F32;
  Ctx x32 = x;
  x32.c = &c32;
  if (f->M > 0) {
    SegSpec s{f->sp_feat, F, F, 0, 1};
    NL_TRY(run_gemm(x32, G_PTT, &s, 1, f->M, f->ptt, W, NL_ACT_NONE));
  }
  NL_CHECK_HIP(hipMemcpyAsync(f->ptt + (size_t)f->M * W, x.pk + x.L.bias[G_PTT], sizeof(float) * W, hipMemcpyDeviceToDevice, x.st));
  // max |T| (bias row included): what the f16mx kernel bounds base_mlp.0's outputs with; kept in the slack behind the per-view matrices (float 248 of that 1-KB block)
  NL_TRY(nl_table_absmax(f->ptt, (size_t)(f->M + 1) * W, f->views_dev + 248, x.st));
  f->ptt_for = (const void*)x.pk; f->ptt_gen = gen;
  return NL_OK;
}

}  // namespace nlhost

// =====================================================================================================
extern "C" {

static_assert(sizeof(nl_render_opts) == 32, "nl_render_opts is part of the C-ABI: 32 bytes");
static_assert(sizeof(nl_train_grads) == 72 && sizeof(nl_render_cotangents) == 64, "training / cotangent blocks are part of the C-ABI");
static_assert(offsetof(nl_render_opts, flags) == 4 && offsetof(nl_render_opts, ray_centers) == 8, "nl_render_opts layout");
int nl_abi_version(void) { return NL_ABI_VERSION; }

int nl_debug_bump_gap(size_t bytes) { g_bump_gap = nl_align_up(bytes, 256); g_bump_gaps.clear(); return NL_OK; }
// counts the recorded gap regions (since the last nl_debug_bump_gap / nl_debug_check_gaps) that hold anything but `pattern`; scratch: 4 device bytes
int nl_debug_check_gaps(int pattern, int* scratch, int* bad_regions, int* checked_regions, void* stream) {
  if (!scratch || !bad_regions) return NL_ERR_BAD_ARG;
  if (checked_regions) *checked_regions = (int)g_bump_gaps.size();
  hipStream_t st = (hipStream_t)stream;
  int bad = 0;
  for (const auto& g : g_bump_gaps) {
    NL_CHECK_HIP(hipMemsetAsync(scratch, 0, sizeof(int), st));
    hipLaunchKernelGGL(gap_check_kernel, dim3((unsigned)nl_cdiv((int64_t)g.second, 256)), dim3(256), 0, st, (const unsigned char*)g.first, g.second, (unsigned char)pattern,
                       scratch);
    int h = 0;
    NL_CHECK_HIP(hipMemcpyAsync(&h, scratch, sizeof(int), hipMemcpyDeviceToHost, st));
    NL_CHECK_HIP(hipStreamSynchronize(st));
    if (h) ++bad;
  }
  *bad_regions = bad;
  g_bump_gaps.clear();
  return NL_OK;
}

int nl_profile_begin(void) { g_prof.on = true; g_prof.used = 0; return NL_OK; }
int nl_profile_end(float* fused_ms, int* launches) {
  float tot = 0.f;
  for (int i = 0; i + 1 < g_prof.used; i += 2) {
    float ms = 0.f;
    if (hipEventSynchronize(g_prof.ev[i + 1]) != hipSuccess || hipEventElapsedTime(&ms, g_prof.ev[i], g_prof.ev[i + 1]) != hipSuccess) return NL_ERR_HIP;
    tot += ms;
  }
  if (fused_ms) *fused_ms = tot;
  if (launches) *launches = g_prof.used / 2;
  g_prof.on = false; g_prof.used = 0;
  return NL_OK;
}

const char* nl_strerror(int s) {
  switch (s) {
    case NL_OK: return "ok";
    case NL_ERR_BAD_ARG: return "bad argument";
    case NL_ERR_UNSUPPORTED: return "unsupported shape or option";
    case NL_ERR_WORKSPACE: return "workspace too small";
    case NL_ERR_HIP: return "HIP runtime error";
    case NL_ERR_NO_DEVICE: return "no HIP device";
    default: return "unknown status";
  }
}

// ---- frame ---------------------------------------------------------------------------------------------
size_t nl_frame_bytes(const nl_config* cfg, const nl_frame_desc* d) {
  NL_EFF_CFG(cfg);
  if (!desc_ok(cfg, d)) return 0;
  return nl_align_up((size_t)d->V * d->vis_h * d->vis_w * 32 * 4, 256) + nl_knn_grid_bytes(d->M) + nl_align_up((size_t)(d->M + 1) * cfg->W * 4, 256) +
         nl_align_up((size_t)d->V * d->h * d->w * 32 * 4, 256) + 1024 + nl_align_up((size_t)d->M * cfg->W * 4, 256) +
         nl_align_up((size_t)d->M * nl_align_up(cfg->C + 3, 32) * 4, 256);
}

int nl_frame_create(const nl_config* cfg, const nl_frame_desc* d, void* mem, size_t bytes, void* stream, nl_frame** out) {
  NL_EFF_CFG(cfg);
  if (!desc_ok(cfg, d) || !mem || !out) return NL_ERR_BAD_ARG;
  if (bytes < nl_frame_bytes(cfg, d)) return NL_ERR_WORKSPACE;
  nl_frame* f = new (std::nothrow) nl_frame;
  if (!f) return NL_ERR_BAD_ARG;
  memset(&f->views, 0, sizeof(NlViews));
  f->views.V = d->V; f->views.H = d->H; f->views.Wimg = d->Wimg; f->views.h = d->h; f->views.w = d->w;
  f->views.vh = d->vis_h; f->views.vw = d->vis_w;
  f->views.near_ = d->near_; f->views.far_ = d->far_;
  for (int v = 0; v < d->V; ++v) {
    memcpy(f->views.P1[v], d->proj_ibr + 12 * v, 48);
    memcpy(f->views.P2[v], d->proj_neuray + 12 * v, 48);
    memcpy(f->views.cam[v], d->cam_centers + 3 * v, 12);
  }
  f->C = cfg->C;
  f->images = d->images; f->feat = d->featmaps;
  f->sp_xyz = d->sp_xyz; f->sp_feat = d->sp_feature; f->sp_conf = d->sp_confidence; f->sp_dir = d->sp_direction;
  f->M = d->M;
  hipStream_t st = (hipStream_t)stream;
  f->visf_hwc = (float*)mem;
  int rc = nl_launch_chw_to_hwc(d->vis_featmaps, f->visf_hwc, d->V, 32, d->vis_h * d->vis_w, st);
  if (rc == NL_OK) rc = nl_knn_grid_build(&f->grid, (char*)mem + nl_align_up((size_t)d->V * d->vis_h * d->vis_w * 32 * 4, 256), d->sp_xyz, d->M, st);
  {
    char* p = (char*)mem + nl_align_up((size_t)d->V * d->vis_h * d->vis_w * 32 * 4, 256) + nl_knn_grid_bytes(d->M);
    f->ptt = (float*)p;
    f->ptt_for = nullptr; f->ptt_gen = 0;
    f->pfeat = (float*)(p + nl_align_up((size_t)(d->M + 1) * cfg->W * 4, 256));
    f->pfeat_for = nullptr; f->pfeat_gen = 0;
    f->views_dev = (float*)((char*)f->pfeat + nl_align_up((size_t)d->V * d->h * d->w * 32 * 4, 256));
    f->tr_gT = (float*)((char*)f->views_dev + 1024);
    f->tr_tmp = (float*)((char*)f->tr_gT + nl_align_up((size_t)d->M * cfg->W * 4, 256));
    memset(f->views_host, 0, sizeof(f->views_host));
    for (int v = 0; v < d->V; ++v) {
      memcpy(f->views_host + 12 * v, d->proj_ibr + 12 * v, 48);
      memcpy(f->views_host + 192 + 3 * v, d->cam_centers + 3 * v, 12);
    }
    if (rc == NL_OK && hipMemcpyAsync(f->views_dev, f->views_host, sizeof(f->views_host), hipMemcpyHostToDevice, st) != hipSuccess) rc = NL_ERR_HIP;
    // the 16 floats of slack behind the matrices hold the frame's diagnostics (nl_frame_diagnostics): [248] max |T|, [249] max |attention logit|, [250 .. 253] two
    // clock counters, [254] max density of the guarded batches
    if (rc == NL_OK && hipMemsetAsync(f->views_dev + 240, 0, 64, st) != hipSuccess) rc = NL_ERR_HIP;
  }
  if (rc != NL_OK) { delete f; return rc; }
  // the side stream and its two events (see nl_frame): failure to create them only disables the fork
  f->side = nullptr; f->ev_fork = f->ev_join = nullptr;
  f->side_ok = hipStreamCreateWithFlags(&f->side, hipStreamNonBlocking) == hipSuccess &&
               hipEventCreateWithFlags(&f->ev_fork, hipEventDisableTiming) == hipSuccess &&
               hipEventCreateWithFlags(&f->ev_join, hipEventDisableTiming) == hipSuccess;
  if (!f->side_ok) (void)hipGetLastError();
  *out = f;
  return NL_OK;
}

int nl_frame_destroy(nl_frame* f) {
  if (!f) return NL_OK;
  if (f->side) { (void)hipStreamSynchronize(f->side); (void)hipStreamDestroy(f->side); }
  if (f->ev_fork) (void)hipEventDestroy(f->ev_fork);
  if (f->ev_join) (void)hipEventDestroy(f->ev_join);
  delete f;
  return NL_OK;
}

int nl_frame_diagnostics(const nl_frame* f, float* host_out, int32_t n, void* stream) {
  if (!f || !host_out || n < 1) return NL_ERR_BAD_ARG;
  struct { float tmax, lmax; unsigned long long cyc, ref; float dmax, pad; } tmp = {0.f, 0.f, 0ull, 0ull, 0.f, 0.f};   // floats 248, 249; two 64-bit counters at floats 250 .. 253; 254
  static_assert(sizeof(tmp) == 32, "diagnostics block");
  NL_CHECK_HIP(hipMemcpyAsync(&tmp, f->views_dev + 248, sizeof(tmp), hipMemcpyDeviceToHost, (hipStream_t)stream));
  NL_CHECK_HIP(hipStreamSynchronize((hipStream_t)stream));
  const float vals[NL_DIAG_COUNT] = {tmp.tmax, tmp.lmax, tmp.ref ? (float)((double)tmp.cyc / ((double)tmp.ref * 10.0)) : 0.f,   // cycles per ns = GHz
                                     (float)f->guard_last_prec, (float)f->guard_escalations, tmp.dmax};
  for (int i = 0; i < n; ++i) host_out[i] = i < NL_DIAG_COUNT ? vals[i] : 0.f;
  return NL_OK;
}

}  // extern "C"
