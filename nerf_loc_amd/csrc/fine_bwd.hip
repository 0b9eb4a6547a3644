// Training step of the fine matcher (fine.hip is the forward: nl_fine_windows, and nl_fine_match with the heat-map requested): the gradients of expec_f (M, 3) with
// respect to the centre descriptors, the window rows and the MLP (nl_fine_match_backward), and of the window rows with respect to proj.* and the fine map
// (nl_fine_windows_backward).  Nothing per pair is kept by the forward: the hidden activations are recomputed.
//
// nl_fine_match_backward: fine_match_bwd_kernel, one wave per match, the tile of fine_match_*_kernel (49 cells in two 32-column tiles), weight fragments from L2
//   for the reason fine.hip gives (M is a few thousand at most).  From the saved heat-map h and the cotangent (g_x, g_y, g_std) of expec_f, per cell r
//     t[r] = g_x gx[r] + g_y gy[r] + g_std dstd/dh[r],   dstd/dh[r] = sum over the axes with var >= 1e-10 of (g[r]^2 - 2 coord g[r]) / (2 sqrt(var)),
//     g_logit[r] = h[r] (t[r] - sum h t) / sqrt(C)
//   (DPP sums of the one wave; a zero g_std skips its term, so 0 x inf cannot arise).  Then s2d_bwd.h's chain — layers 1 and 2 again (exact fp32 in the parity modes,
//   masks near zero decided in fp64), g_a2, W2^T, g_a1 — and g_x = W1^T g_a1 one 32-channel block at a time, which never reaches memory:
//     g_feat_f1[m, r] = g_x[r] * feat_f0[m],   g_feat_f0[m] = sum_r g_x[r] * feat_f1[m, r]  (the lane's two cells, then a butterfly over the 32 lanes of a half-wave).
//   The operands of the weight gradients go to the workspace as rows m * 49 + r — the 15 padding columns of a match's 64 are not stored — and wgrad.hip's split-K
//   kernel multiplies them; gW3 / gb3 are the waves' partial rows added in order (s2d_bwd.hip's reduction).
// nl_fine_windows_backward:
//   1. X = the gathered windows (M * 49, Cf), zeros outside the map; gW = g_out^T X and gb = the column sums of g_out over all M * 49 rows (wgrad.hip).
//   2. R = g_out . W (M * 49, Cf): the forward's window kernels on dense rows with the training image of proj.weight^T (fine.hip: nl_launch_fine_rows).
//   3. the map's gradient is a gather: per image and window a list of its matches in ascending m (integer work only: a count per window, one scan, and each match
//      placed at its rank among the earlier matches of the same window); a thread per (pixel, four channels) walks the at most ceil(7 / stride)^2 windows that cover
//      its pixel and adds their matches' rows in ascending m (each step takes the smallest m above the last one: a binary search per window).  A pixel no window covers
//      is written as zero.
// Every sum has an order that depends on the shapes and the ids alone and no float atomic touches a result: two calls give the same bits.
#include <algorithm>
#include "common.h"
#include "compact.h"
#include "mfma.h"
#include "s2d.h"
#include "s2d_bwd.h"
#include "fine.h"
#include "host.h"
#include "s2d_bwd_host.h"

namespace {

// rank placement is quadratic in the matches of a call and the operands grow with M: far above what a frame yields (a few thousand)
constexpr int64_t FINE_BWD_MAX_M = NL_FINE_BACKWARD_MAX_M;

// ------------------------------------------------------------------------------------------ match
struct FineMatchBwdArgs {
  const unsigned char* img; const unsigned char* timg;
  const float* f0; const float* f1; const float* heat; const float* g_expec;
  float *x, *h1, *ga2, *ga1;   // rows m * 49 + r of the weight gradients' operands; each may be null
  float* w3part;               // [M][S2D_W3P_LD] or null
  float* g_f0; float* g_f1;    // may be null
  int M, C;
  float temp;
};

// the logit's gradient of cell `lane` (0 for lanes 49..63) from the heat-map and the cotangent of (x, y, std): the derivative of fine.hip's fine_finish
__device__ __forceinline__ float fine_logit_grad(const FineMatchBwdArgs& a, int m, int lane) {
  const bool valid = lane < FINE_WW;
  const float h = valid ? a.heat[(size_t)m * FINE_WW + lane] : 0.f;
  const int wy = lane / FINE_W, wx = lane - wy * FINE_W;
  const float gx = (float)(wx - 3) / 3.f, gy = (float)(wy - 3) / 3.f;
  const float gcx = a.g_expec[(size_t)m * 3 + 0], gcy = a.g_expec[(size_t)m * 3 + 1], gsd = a.g_expec[(size_t)m * 3 + 2];
  float t = gcx * gx + gcy * gy;
  if (gsd != 0.f) {   // wave-uniform
    const float cx = wave_sum(h * gx), cy = wave_sum(h * gy);
    const float vx = wave_sum(gx * gx * h) - cx * cx, vy = wave_sum(gy * gy * h) - cy * cy;
    float ds = 0.f;
    if (vx >= 1e-10f) ds += (gx * gx - 2.f * cx * gx) / (2.f * sqrtf(vx));   // the clamp passes its gradient at equality, as torch's
    if (vy >= 1e-10f) ds += (gy * gy - 2.f * cy * gy) / (2.f * sqrtf(vy));
    t += gsd * ds;
  }
  const float s = wave_sum(h * t);
  return valid ? h * (t - s) * a.temp : 0.f;
}

template <bool EXACT>
__global__ __launch_bounds__(256) void fine_match_bwd_kernel(const FineMatchBwdArgs a) {
  constexpr bool X3 = EXACT;
  extern __shared__ __attribute__((aligned(16))) float fine_bwd_hidden[];   // EXACT: S2D_F32_LDS bytes, lane-private columns (s2d.h: s2d_f32_layer2)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5, col = lane & 31;
  const int m = blockIdx.x * 4 + wave;
  if (m >= a.M) return;   // wave-uniform; the kernel has no barrier
  const int C = a.C, nrb1 = C >> 5;
  const S2dLayout L = s2d_layout(C);
  const S2dTrainLayout T = s2d_train_layout(C);
  const int cell1 = min(32 + col, FINE_WW - 1);   // columns 49 .. 63 of tile 1 repeat cell 48; their gradient is zero and nothing of them is stored
  const bool ok[2] = {true, 32 + col < FINE_WW};
  const size_t prow[2] = {(size_t)m * FINE_WW + col, (size_t)m * FINE_WW + cell1};
  nl_f32x16 acc[2][4];
  nl_acc_zero(acc);
  // ---- layer 1 again (fine.hip's walks); the products are also the X operand of gW1
  if constexpr (EXACT) {
    const float* w1f = (const float*)(a.img + L.f32w1);
    const float* xp = a.f0 + (size_t)m * C + 4 * hh;
    const float* ya = a.f1 + prow[0] * C + 4 * hh;
    const float* yb = a.f1 + prow[1] * C + 4 * hh;
    for (int g = 0; g < (C >> 3); ++g) {
      const float4 x = *(const float4*)(xp + 8 * g), va = *(const float4*)(ya + 8 * g), vb = *(const float4*)(yb + 8 * g);
      const float pa[4] = {x.x * va.x, x.y * va.y, x.z * va.z, x.w * va.w};
      const float pb[4] = {x.x * vb.x, x.y * vb.y, x.z * vb.z, x.w * vb.w};
      if (a.x) {
        *(float4*)(a.x + prow[0] * C + 8 * g + 4 * hh) = make_float4(pa[0], pa[1], pa[2], pa[3]);
        if (ok[1]) *(float4*)(a.x + prow[1] * C + 8 * g + 4 * hh) = make_float4(pb[0], pb[1], pb[2], pb[3]);
      }
      s2d_f32_layer1_group(acc, w1f, g, lane, pa, pb);
    }
  } else {
    const uint4* w1hi = (const uint4*)(a.img + L.w1hi);
    const uint4* w1lo = (const uint4*)(a.img + L.w1lo);
    const float* xp = a.f0 + (size_t)m * C + 8 * hh;
    const float* ya = a.f1 + prow[0] * C + 8 * hh;
    const float* yb = a.f1 + prow[1] * C + 8 * hh;
    for (int s = 0; s < (C >> 4); ++s) {
      const float4 x0 = *(const float4*)(xp + 16 * s), x1 = *(const float4*)(xp + 16 * s + 4);
      const float4 ya0 = *(const float4*)(ya + 16 * s), ya1 = *(const float4*)(ya + 16 * s + 4);
      const float4 yb0 = *(const float4*)(yb + 16 * s), yb1 = *(const float4*)(yb + 16 * s + 4);
      const float4 pa0 = make_float4(x0.x * ya0.x, x0.y * ya0.y, x0.z * ya0.z, x0.w * ya0.w), pa1 = make_float4(x1.x * ya1.x, x1.y * ya1.y, x1.z * ya1.z, x1.w * ya1.w);
      const float4 pb0 = make_float4(x0.x * yb0.x, x0.y * yb0.y, x0.z * yb0.z, x0.w * yb0.w), pb1 = make_float4(x1.x * yb1.x, x1.y * yb1.y, x1.z * yb1.z, x1.w * yb1.w);
      if (a.x) {
        { float* p = a.x + prow[0] * C + 16 * s + 8 * hh; *(float4*)p = pa0; *(float4*)(p + 4) = pa1; }
        if (ok[1]) { float* p = a.x + prow[1] * C + 16 * s + 8 * hh; *(float4*)p = pb0; *(float4*)(p + 4) = pb1; }
      }
      unsigned ph[2][4], pl[2][4];
      nl_split_bf16_pair(pa0.x, pa0.y, ph[0][0], pl[0][0]);
      nl_split_bf16_pair(pa0.z, pa0.w, ph[0][1], pl[0][1]);
      nl_split_bf16_pair(pa1.x, pa1.y, ph[0][2], pl[0][2]);
      nl_split_bf16_pair(pa1.z, pa1.w, ph[0][3], pl[0][3]);
      nl_split_bf16_pair(pb0.x, pb0.y, ph[1][0], pl[1][0]);
      nl_split_bf16_pair(pb0.z, pb0.w, ph[1][1], pl[1][1]);
      nl_split_bf16_pair(pb1.x, pb1.y, ph[1][2], pl[1][2]);
      nl_split_bf16_pair(pb1.z, pb1.w, ph[1][3], pl[1][3]);
      s2d_layer1_step<X3>(acc, w1hi, w1lo, s, lane, ph, pl);
    }
  }
  // ---- the way back to g_a1 (s2d_bwd.h)
  unsigned hi[2][4][8], lo[2][4][8];
  const S2dBwdStores stores = {a.h1, a.ga2, a.ga1, a.w3part ? a.w3part + (size_t)m * S2D_W3P_LD : nullptr};
  s2d_bwd_chain<EXACT>(
      acc, a.img, a.timg, C, ok, prow, stores, fine_bwd_hidden + wave * (128 * 64) + lane, lane,
      [&](float (&gl)[2]) {
        const float g = fine_logit_grad(a, m, lane);   // of cell `lane`
        gl[0] = __shfl(g, col);
        gl[1] = __shfl(g, 32 + col);                   // lanes 49 .. 63 hold zero
      },
      [&](int t, int c, const float*& pd0, const float*& pd1) {
        pd0 = a.f0 + (size_t)m * C;
        pd1 = a.f1 + ((size_t)m * FINE_WW + 32 * t + c) * C;   // only flagged for an existing cell
      },
      hi, lo);
  // ---- g_x = W1^T g_a1, 32 channels at a time, straight into the two feature gradients
  const uint4* w1thi = (const uint4*)(a.timg + T.w1t_hi);
  const uint4* w1tlo = (const uint4*)(a.timg + T.w1t_lo);
  for (int rb = 0; rb < nrb1; ++rb) {
    nl_f32x16 o[2];
    nl_acc_zero(o);
    bwd_mult<X3>(o[0], o[1], hi, lo, w1thi, w1tlo, nrb1, rb, lane);
#pragma unroll
    for (int r4 = 0; r4 < 4; ++r4) {
      const int ch = 32 * rb + 8 * r4 + 4 * hh;
      const float4 g0 = make_float4(o[0][4 * r4], o[0][4 * r4 + 1], o[0][4 * r4 + 2], o[0][4 * r4 + 3]);
      const float4 g1 = make_float4(o[1][4 * r4], o[1][4 * r4 + 1], o[1][4 * r4 + 2], o[1][4 * r4 + 3]);   // exact zeros where the cell does not exist
      if (a.g_f1) {
        const float4 x = *(const float4*)(a.f0 + (size_t)m * C + ch);
        *(float4*)(a.g_f1 + prow[0] * C + ch) = make_float4(g0.x * x.x, g0.y * x.y, g0.z * x.z, g0.w * x.w);
        if (ok[1]) *(float4*)(a.g_f1 + prow[1] * C + ch) = make_float4(g1.x * x.x, g1.y * x.y, g1.z * x.z, g1.w * x.w);
      }
      if (a.g_f0) {
        const float4 y0 = *(const float4*)(a.f1 + prow[0] * C + ch), y1 = *(const float4*)(a.f1 + prow[1] * C + ch);
        float s[4] = {g0.x * y0.x + g1.x * y1.x, g0.y * y0.y + g1.y * y1.y, g0.z * y0.z + g1.z * y1.z, g0.w * y0.w + g1.w * y1.w};
#pragma unroll
        for (int x = 16; x >= 1; x >>= 1)
#pragma unroll
          for (int e = 0; e < 4; ++e) s[e] += __shfl_xor(s[e], x);
        if (col == 0) *(float4*)(a.g_f0 + (size_t)m * C + ch) = make_float4(s[0], s[1], s[2], s[3]);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ windows
struct FineMapArgs {
  const long long* b_ids; const long long* j_ids;
  int* key;     // [M]: b * L + l, or -1 for ids outside the grid (the forward reads zeros there)
  int* start;   // [K + 1], K = B * L: counts, then their exclusive scan
  int* list;    // [M]: the matches of each window in ascending m
  const float* rows; float* g_feat;
  int B, Hf, Wf, Cf, M, stride, Lx, Ly, L, K;
};

__global__ __launch_bounds__(256) void fine_key_count_kernel(const FineMapArgs a) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= a.M) return;
  const long long b = a.b_ids[m], l = a.j_ids[m];
  const bool ok = b >= 0 && b < a.B && l >= 0 && l < a.L;
  const int key = ok ? (int)(b * a.L + l) : -1;
  a.key[m] = key;
  if (ok) atomicAdd(a.start + key, 1);   // an integer count: its value does not depend on the order
}
// start[0 .. K] = exclusive scan of the counts in place (start[K] = the number of placed matches); one workgroup (compact.h)
__global__ __launch_bounds__(1024) void fine_scan_kernel(int* start, int K) {
  __shared__ int part[1024];
  const int total = nl_scan_exclusive<1024>(start, K, part);
  if (threadIdx.x == 1023) start[K] = total;
}
// match m goes to its window's list at its rank among the earlier matches of that window
__global__ __launch_bounds__(256) void fine_place_kernel(const FineMapArgs a) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m >= a.M) return;
  const int key = a.key[m];
  if (key < 0) return;
  int rank = 0;
  for (int i = 0; i < m; ++i) rank += a.key[i] == key;
  a.list[a.start[key] + rank] = m;
}
// X[m * 49 + r] = window cell r of match m, zeros outside the map
__global__ __launch_bounds__(256) void fine_gather_kernel(const FineWinArgs a, float* X) {
  const int c4n = a.Cf >> 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.M * FINE_WW * c4n) return;
  const long long row = e / c4n;
  const int c4 = (int)(e - row * c4n), m = (int)(row / FINE_WW), cell = (int)(row - (long long)m * FINE_WW);
  const float* src = fine_cell_row(a, m, cell);
  *(float4*)(X + (size_t)row * a.Cf + 4 * c4) = src ? *(const float4*)(src + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
}
// g_feat[b, py, px] = the rows of the matches whose window covers the pixel, added in ascending m
__global__ __launch_bounds__(256) void fine_map_gather_kernel(const FineMapArgs a) {
  const int c4n = a.Cf >> 2;
  const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
  if (e >= (long long)a.B * a.Hf * a.Wf * c4n) return;
  const long long pix = e / c4n;
  const int c4 = (int)(e - pix * c4n);
  const int b = (int)(pix / ((long long)a.Hf * a.Wf));
  const int rem = (int)(pix - (long long)b * a.Hf * a.Wf), py = rem / a.Wf, px = rem - py * a.Wf;
  const int s = a.stride, half = FINE_W / 2;
  const int ly0 = py <= half ? 0 : (py - half + s - 1) / s, ly1 = min(a.Ly - 1, (py + half) / s);
  const int lx0 = px <= half ? 0 : (px - half + s - 1) / s, lx1 = min(a.Lx - 1, (px + half) / s);
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  int last = -1;
  for (;;) {
    int best = 0x7fffffff, bcell = 0;
    for (int ly = ly0; ly <= ly1; ++ly)
      for (int lx = lx0; lx <= lx1; ++lx) {
        const int key = b * a.L + ly * a.Lx + lx;
        int lo = a.start[key];
        const int end = a.start[key + 1];
        int hi = end;
        while (lo < hi) {   // the first entry above `last`
          const int mid = (lo + hi) >> 1;
          if (a.list[mid] > last) hi = mid; else lo = mid + 1;
        }
        if (lo < end) {
          const int mm = a.list[lo];
          if (mm < best) { best = mm; bcell = (py - ly * s + half) * FINE_W + (px - lx * s + half); }
        }
      }
    if (best == 0x7fffffff) break;
    const float4 v = *(const float4*)(a.rows + ((size_t)best * FINE_WW + bcell) * a.Cf + 4 * c4);
    sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
    last = best;
  }
  *(float4*)(a.g_feat + (size_t)pix * a.Cf + 4 * c4) = sum;
}

// ------------------------------------------------------------------------------------------ workspaces
// the shared operand block (s2d_bwd_host.h): 49 operand rows and one partial row of gW3 per match
S2dMlpBwdWs match_bwd_ws(int64_t M, int C) { return S2dMlpBwdWs((size_t)M * FINE_WW, (size_t)M, C); }
struct WinBwdWs { size_t X, rows, wg, dummy, key, start, list, total; size_t wg_floats; };
WinBwdWs win_bwd_ws(int Cf, int Cout, int64_t K, int64_t M) {
  WinBwdWs w;
  const size_t P = (size_t)M * FINE_WW;
  size_t o = 0;
  auto take = [&](size_t bytes) { const size_t at = o; o += nl_align_up(bytes, 256); return at; };
  w.X = take(P * Cf * 4);
  w.rows = take(P * Cf * 4);
  w.wg_floats = nl_wgrad_scratch_floats((int64_t)P, Cout, Cf);
  w.wg = take(w.wg_floats * 4);
  w.dummy = take((size_t)Cout * Cf * 4);
  w.key = take((size_t)M * 4);
  w.start = take((size_t)(K + 1) * 4);
  w.list = take((size_t)M * 4);
  w.total = o;
  return w;
}
// windows per call (B images of Ly x Lx), or 0 when the shape is refused
int64_t win_keys(int B, int Hf, int Wf, int stride) {
  if (B < 1 || Hf < 1 || Wf < 1 || stride < 1) return 0;
  const int64_t K = (int64_t)B * ((Hf - 1) / stride + 1) * ((Wf - 1) / stride + 1);
  return K < ((int64_t)1 << 30) && (int64_t)B * Hf * Wf < ((int64_t)1 << 31) ? K : 0;
}

}  // namespace

extern "C" {

size_t nl_fine_proj_train_bytes(int Cf, int Cout) { return fine_c_ok(Cf) && fine_c_ok(Cout) ? nl_align_up(fine_proj_layout(Cout, Cf).total, 16) : 0; }

int nl_fine_pack_proj_train(int Cf, int Cout, const float* w, void* packed, size_t packed_bytes, void* stream) {
  if (!fine_c_ok(Cf) || !fine_c_ok(Cout)) return NL_ERR_BAD_ARG;
  if (!w || !packed || ((uintptr_t)packed & 15) != 0 || ((uintptr_t)w & 3) != 0) return NL_ERR_BAD_ARG;
  if (packed_bytes < nl_fine_proj_train_bytes(Cf, Cout)) return NL_ERR_WORKSPACE;
  const FineProjLayout L = fine_proj_layout(Cout, Cf);   // of proj.weight^T: Cf rows of Cout
  unsigned char* img = (unsigned char*)packed;
  hipStream_t st = (hipStream_t)stream;
  float* wt = (float*)(img + L.f32);
  if (const int e = nl_launch_transpose(w, Cout, Cf, wt, st)) return e;
  if (const int e = nl_launch_frag_pack(wt, Cf, Cout, (unsigned short*)(img + L.hi), (unsigned short*)(img + L.lo), nullptr, nullptr, nullptr, false, st)) return e;
  NL_CHECK_HIP(hipMemsetAsync(img + L.bias, 0, (size_t)Cf * 4, st));
  return NL_OK;
}

size_t nl_fine_match_backward_workspace_bytes(int64_t M, int C) {
  if (!fine_c_ok(C) || M < 0 || M > FINE_BWD_MAX_M) return 0;
  return match_bwd_ws(std::max<int64_t>(M, 1), C).total;
}

int nl_fine_match_backward(const void* packed_mlp, const void* train_packed, int C, int precision, const float* feat_f0, const float* feat_f1, int64_t M,
                           const float* heatmap, const float* g_expec, float* g_feat_f0, float* g_feat_f1, float* g_w1, float* g_b1, float* g_w2, float* g_b2,
                           float* g_w3, float* g_b3, void* workspace, size_t workspace_bytes, void* stream) {
  if (M < 0 || !fine_c_ok(C)) return NL_ERR_BAD_ARG;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (M > FINE_BWD_MAX_M) return NL_ERR_UNSUPPORTED;
  if (M == 0) return NL_OK;
  if (!packed_mlp || !train_packed || !feat_f0 || !feat_f1 || !heatmap || !g_expec) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)packed_mlp | (uintptr_t)train_packed | (uintptr_t)feat_f0 | (uintptr_t)feat_f1 | (uintptr_t)g_feat_f0 | (uintptr_t)g_feat_f1) & 15) != 0)
    return NL_ERR_BAD_ARG;   // read / written as 16-byte pieces
  const S2dMlpGrads g{g_w1, g_b1, g_w2, g_b2, g_w3, g_b3};
  if ((((uintptr_t)heatmap | (uintptr_t)g_expec | g.addr_bits()) & 3) != 0) return NL_ERR_BAD_ARG;
  const S2dMlpBwdWs w = match_bwd_ws(M, C);
  if (!workspace || workspace_bytes < w.total || ((uintptr_t)workspace & 15) != 0) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned char* ws = (unsigned char*)workspace;
  const int64_t P = M * FINE_WW;

  if (const int e = s2d_mlp_grads_zero(g, C, st)) return e;

  FineMatchBwdArgs a;
  a.img = (const unsigned char*)packed_mlp; a.timg = (const unsigned char*)train_packed;
  a.f0 = feat_f0; a.f1 = feat_f1; a.heat = heatmap; a.g_expec = g_expec;
  w.operands(ws, g, a.x, a.ga1, a.h1, a.ga2);
  a.w3part = g_w3 ? (float*)(ws + w.w3part) : nullptr;
  a.g_f0 = g_feat_f0; a.g_f1 = g_feat_f1;
  a.M = (int)M; a.C = C;
  a.temp = (float)(1.0 / sqrt((double)C));
  float* wg = (float*)(ws + w.wg);
  float* dummy = (float*)(ws + w.dummy);

  static std::atomic<unsigned long long> lds_set{0};
  // (named ahead of <true>: the two kernels lie in the code object in the order of their first use, and tools/kernel_identity.py holds the device code fixed)
  const auto bf16_kernel = fine_match_bwd_kernel<false>;
  if (const int e = s2d_mlp_bwd_launch(fine_match_bwd_kernel<true>, bf16_kernel, dim3((unsigned)nl_cdiv(M, 4)), a, precision, lds_set, st)) return e;
  if (const int e = s2d_mlp_wgrad(a.x, a.ga1, a.h1, a.ga2, C, P, g, dummy, wg, w.wg_floats, st)) return e;
  // gb3 stays the zero written above: the softmax ignores a common shift of a match's 49 logits, so expec_f does not depend on b3 at all (the sum of the
  // logit gradients that autograd forms there is rounding noise around zero)
  if (g_w3)
    if (const int e = nl_launch_s2d_w3_reduce(a.w3part, (int)M, g_w3, nullptr, st)) return e;
  return NL_OK;
}

size_t nl_fine_windows_backward_workspace_bytes(int Cf, int Cout, int B, int Hf, int Wf, int stride, int64_t M) {
  const int64_t K = win_keys(B, Hf, Wf, stride);
  if (!fine_c_ok(Cf) || !fine_c_ok(Cout) || K == 0 || M < 0 || M > FINE_BWD_MAX_M) return 0;
  return win_bwd_ws(Cf, Cout, K, std::max<int64_t>(M, 1)).total;
}

int nl_fine_windows_backward(const void* packed, const void* train_packed, int Cf, int Cout, int precision, const float* feat_nhwc, int B, int Hf, int Wf,
                             const int64_t* b_ids, const int64_t* j_ids, int64_t M, int stride, const float* g_out, float* g_w, float* g_b, float* g_feat_nhwc,
                             void* workspace, size_t workspace_bytes, void* stream) {
  if (M < 0 || stride < 1 || B < 1 || Hf < 1 || Wf < 1 || !fine_c_ok(Cf) || !fine_c_ok(Cout)) return NL_ERR_BAD_ARG;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  const int64_t K = win_keys(B, Hf, Wf, stride);
  if (M > FINE_BWD_MAX_M || K == 0) return NL_ERR_UNSUPPORTED;
  if ((((uintptr_t)g_feat_nhwc) & 15) != 0 || (((uintptr_t)g_w | (uintptr_t)g_b) & 3) != 0) return NL_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  const size_t map_bytes = (size_t)B * Hf * Wf * Cf * 4;
  if (M == 0) {   // no window: every gradient is zero
    if (g_w) NL_CHECK_HIP(hipMemsetAsync(g_w, 0, (size_t)Cout * Cf * 4, st));
    if (g_b) NL_CHECK_HIP(hipMemsetAsync(g_b, 0, (size_t)Cout * 4, st));
    if (g_feat_nhwc) NL_CHECK_HIP(hipMemsetAsync(g_feat_nhwc, 0, map_bytes, st));
    return NL_OK;
  }
  if (!packed || !train_packed || !feat_nhwc || !b_ids || !j_ids || !g_out) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)packed | (uintptr_t)train_packed | (uintptr_t)feat_nhwc | (uintptr_t)g_out) & 15) != 0 || (((uintptr_t)b_ids | (uintptr_t)j_ids) & 7) != 0)
    return NL_ERR_BAD_ARG;
  const WinBwdWs w = win_bwd_ws(Cf, Cout, K, M);
  if (!workspace || workspace_bytes < w.total || ((uintptr_t)workspace & 15) != 0) return NL_ERR_WORKSPACE;
  unsigned char* ws = (unsigned char*)workspace;
  const int64_t P = M * FINE_WW;

  if (g_w || g_b) {
    FineWinArgs a;
    a.img = (const unsigned char*)packed;
    a.feat = feat_nhwc;
    a.b_ids = (const long long*)b_ids; a.j_ids = (const long long*)j_ids;
    a.out = nullptr;
    a.B = B; a.Hf = Hf; a.Wf = Wf; a.Cf = Cf; a.Cout = Cout; a.M = (int)M; a.stride = stride;
    a.Lx = (Wf - 1) / stride + 1;
    a.L = ((Hf - 1) / stride + 1) * a.Lx;
    a.Q = 0; a.dense = 0;
    float* X = (float*)(ws + w.X);
    hipLaunchKernelGGL(fine_gather_kernel, dim3((unsigned)nl_cdiv(P * (Cf >> 2), 256)), dim3(256), 0, st, a, X);
    NL_LAUNCH_CHECK();
    float* gw = g_w ? g_w : (float*)(ws + w.dummy);
    if (g_w) NL_CHECK_HIP(hipMemsetAsync(g_w, 0, (size_t)Cout * Cf * 4, st));
    if (g_b) NL_CHECK_HIP(hipMemsetAsync(g_b, 0, (size_t)Cout * 4, st));
    if (const int e = nl_launch_wgrad(g_out, Cout, Cout, X, Cf, Cf, P, 0, 0, gw, Cf, 1, 0, g_b, (float*)(ws + w.wg), w.wg_floats, st)) return e;
  }
  if (g_feat_nhwc) {
    float* rows = (float*)(ws + w.rows);
    if (const int e = nl_launch_fine_rows(train_packed, Cout, Cf, precision != NL_PREC_BF16, g_out, M, rows, st)) return e;
    FineMapArgs m;
    m.b_ids = (const long long*)b_ids; m.j_ids = (const long long*)j_ids;
    m.key = (int*)(ws + w.key); m.start = (int*)(ws + w.start); m.list = (int*)(ws + w.list);
    m.rows = rows; m.g_feat = g_feat_nhwc;
    m.B = B; m.Hf = Hf; m.Wf = Wf; m.Cf = Cf; m.M = (int)M; m.stride = stride;
    m.Lx = (Wf - 1) / stride + 1; m.Ly = (Hf - 1) / stride + 1; m.L = m.Ly * m.Lx; m.K = (int)K;
    NL_CHECK_HIP(hipMemsetAsync(m.start, 0, (size_t)(K + 1) * 4, st));
    const dim3 mgrid((unsigned)nl_cdiv(M, 256));
    hipLaunchKernelGGL(fine_key_count_kernel, mgrid, dim3(256), 0, st, m);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(fine_scan_kernel, dim3(1), dim3(1024), 0, st, m.start, m.K);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(fine_place_kernel, mgrid, dim3(256), 0, st, m);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(fine_map_gather_kernel, dim3((unsigned)nl_cdiv((int64_t)B * Hf * Wf * (Cf >> 2), 256)), dim3(256), 0, st, m);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

}  // extern "C"
