// libnerfloc_geom.so (include/nerfloc_geom.h states the contracts; tests/geom_ref.py restates them in numpy): the keypoint geometry around the localisation head.
//   nlg_select_visible   vis_mask_kernel   one workgroup per chunk of 256 points: the V combined 3 x 4 matrices once in LDS, mask[i], the chunk's count
//                        scan_kernel<1>    one workgroup: exclusive scan of the chunk counts, info
//                        vis_emit_kernel   one thread per max(N, cap): idx[rank] for the visible points, the zeros behind the count
//   nlg_build_pairs      pair_project_kernel / scan_kernel<2> / pair_emit_kernel: the same chain with two counted sets (valid, pos) and the fallback decided in the scan
//   nlg_conf_target      one launch, every value written once, 16-byte stores over the aligned part
//   nlg_cell_grid        one launch
// The order of a compaction comes from compact.h: ballot / popcount per wave, the CHUNK / 64 wave totals added in wave order, the chunk's scanned offset.
// No atomics, no kernel that waits on another workgroup; fp64 from the loaded inputs to every decision (-ffp-contract=off: no fused multiply-add, so
// tests/geom_ref.py's numpy sees the same roundings).
#include "common.h"
#include "compact.h"
#include "../../include/nerfloc_geom.h"

namespace {

constexpr int CHUNK = NLG_CHUNK;
constexpr int SCAN_THREADS = 1024;
constexpr int64_t MAX_CAP = 1 << 24;
constexpr int64_t MAX_TARGET_DIM = 1 << 24;
static_assert(NLG_MAX_POINTS / CHUNK <= 4 * SCAN_THREADS, "the scan owns at most four chunks per thread");

// P (3 x 4, row-major) = K [R | t] with [R | t] the inverse of the affine map of `pose` (its top three rows), as the header writes it
template <typename T>
__device__ void combined_matrix(const T* __restrict__ pose, const float* __restrict__ K, double* __restrict__ P) {
  double A[3][3], c[3], k[3][3];
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) { A[r][q] = (double)pose[r * 4 + q]; k[r][q] = (double)K[r * 3 + q]; }
    c[r] = (double)pose[r * 4 + 3];
  }
  double C[3][3];   // cofactors: C[i][j] of A[i][j]
  C[0][0] = A[1][1] * A[2][2] - A[1][2] * A[2][1];
  C[0][1] = A[1][2] * A[2][0] - A[1][0] * A[2][2];
  C[0][2] = A[1][0] * A[2][1] - A[1][1] * A[2][0];
  C[1][0] = A[0][2] * A[2][1] - A[0][1] * A[2][2];
  C[1][1] = A[0][0] * A[2][2] - A[0][2] * A[2][0];
  C[1][2] = A[0][1] * A[2][0] - A[0][0] * A[2][1];
  C[2][0] = A[0][1] * A[1][2] - A[0][2] * A[1][1];
  C[2][1] = A[0][2] * A[1][0] - A[0][0] * A[1][2];
  C[2][2] = A[0][0] * A[1][1] - A[0][1] * A[1][0];
  const double det = A[0][0] * C[0][0] + A[0][1] * C[0][1] + A[0][2] * C[0][2];
  double R[3][3], t[3];
  for (int r = 0; r < 3; ++r)
    for (int q = 0; q < 3; ++q) R[r][q] = C[q][r] / det;   // the adjugate is the transposed cofactor matrix
  for (int r = 0; r < 3; ++r) t[r] = -(R[r][0] * c[0] + R[r][1] * c[1] + R[r][2] * c[2]);
  for (int r = 0; r < 3; ++r) {
    for (int q = 0; q < 3; ++q) P[r * 4 + q] = k[r][0] * R[0][q] + k[r][1] * R[1][q] + k[r][2] * R[2][q];
    P[r * 4 + 3] = k[r][0] * t[0] + k[r][1] * t[1] + k[r][2] * t[2];
  }
}

__device__ __forceinline__ void load_matrices(const void* __restrict__ poses, int V, bool f64, const float* __restrict__ K, double* __restrict__ P) {
  if ((int)threadIdx.x < V) {
    if (f64) combined_matrix((const double*)poses + (size_t)threadIdx.x * 16, K, P + threadIdx.x * 12);
    else combined_matrix((const float*)poses + (size_t)threadIdx.x * 16, K, P + threadIdx.x * 12);
  }
  __syncthreads();
}

__device__ __forceinline__ bool project(const double* __restrict__ P, double p0, double p1, double p2, double Wd, double Hd, double& u, double& v, double& z) {
  const double x0 = P[0] * p0 + P[1] * p1 + P[2] * p2 + P[3];
  const double x1 = P[4] * p0 + P[5] * p1 + P[6] * p2 + P[7];
  z = P[8] * p0 + P[9] * p1 + P[10] * p2 + P[11];
  u = x0 / z;
  v = x1 / z;
  return (u >= 0.0) && (v >= 0.0) && (u < Wd) && (v < Hd) && (z > 0.0);
}

__global__ __launch_bounds__(CHUNK) void vis_mask_kernel(const float* __restrict__ pts, int N, const void* __restrict__ poses, int V, int f64,
                                                         const float* __restrict__ K, int H, int W, unsigned char* __restrict__ mask, int* __restrict__ chunk_cnt) {
  __shared__ double P[NLG_MAX_VIEWS * 12];
  __shared__ int wtot[CHUNK / 64];
  load_matrices(poses, V, f64 != 0, K, P);
  const int i = blockIdx.x * CHUNK + threadIdx.x;
  bool vis = false;
  if (i < N) {
    const double p0 = (double)pts[(size_t)i * 3], p1 = (double)pts[(size_t)i * 3 + 1], p2 = (double)pts[(size_t)i * 3 + 2];
    for (int w = 0; w < V && !vis; ++w) {
      double u, v, z;
      vis = project(P + w * 12, p0, p1, p2, (double)W, (double)H, u, v, z);
    }
    mask[i] = vis ? 1 : 0;
  }
  nl_wave_rank(vis, wtot);
  __syncthreads();
  if (threadIdx.x == 0) chunk_cnt[blockIdx.x] = nl_group_total<CHUNK / 64>(wtot);
}

// SETS arrays of nchunks counts, one after the other in `cnt`, each turned into its exclusive scan in place (compact.h).
// SETS == 2 (valid, then pos): the positive set is pos unless fewer than NLG_MIN_POSITIVES rows are pos.
template <int SETS>
__global__ __launch_bounds__(SCAN_THREADS) void scan_kernel(int* __restrict__ cnt, int nchunks, int cap, int* __restrict__ info) {
  __shared__ int part[SCAN_THREADS];
  int total[SETS];
#pragma unroll
  for (int s = 0; s < SETS; ++s) total[s] = nl_scan_exclusive<SCAN_THREADS>(cnt + (size_t)s * nchunks, nchunks, part);
  if (threadIdx.x == 0) {
    const int fallback = SETS == 2 && total[SETS - 1] < NLG_MIN_POSITIVES ? 1 : 0;
    const int tot = fallback ? total[0] : total[SETS - 1];
    info[0] = min(tot, cap); info[1] = tot; info[2] = tot > cap ? 1 : 0; info[3] = fallback;
  }
}

__global__ __launch_bounds__(CHUNK) void vis_emit_kernel(const unsigned char* __restrict__ mask, int N, int cap, const int* __restrict__ chunk_off,
                                                         const int* __restrict__ info, long long* __restrict__ idx) {
  __shared__ int wtot[CHUNK / 64];
  const int i = blockIdx.x * CHUNK + threadIdx.x;   // i < max(N, cap) rounded up to a chunk: at most 2^24 + 255
  const bool f = i < N && mask[i] != 0;
  const int rank = nl_wave_rank(f, wtot);
  __syncthreads();
  if (f) {
    const int k = chunk_off[blockIdx.x] + nl_group_rank(rank, wtot);   // f implies blockIdx.x < nchunks
    if (k < cap) idx[k] = i;
  }
  if (i < cap && i >= info[0]) idx[i] = 0;           // k < count for every emitted row: the two stores never meet
}

__global__ __launch_bounds__(CHUNK) void pair_project_kernel(const float* __restrict__ pts, int N, const void* __restrict__ pose, int f64, const float* __restrict__ K,
                                                             int H, int W, double stride, double thr, const float* __restrict__ depth, int depth_points,
                                                             float* __restrict__ proj, float* __restrict__ zout, unsigned char* __restrict__ valid,
                                                             unsigned char* __restrict__ pos, int* __restrict__ cell, int* __restrict__ cnt, int nchunks) {
  __shared__ double P[12];
  __shared__ int wv[CHUNK / 64], wp[CHUNK / 64];
  load_matrices(pose, 1, f64 != 0, K, P);
  const int i = blockIdx.x * CHUNK + threadIdx.x;
  bool ok = false, good = false;
  if (i < N) {
    const double p0 = (double)pts[(size_t)i * 3], p1 = (double)pts[(size_t)i * 3 + 1], p2 = (double)pts[(size_t)i * 3 + 2];
    double u, v, z;
    ok = project(P, p0, p1, p2, (double)W, (double)H, u, v, z);
    const double us = u / stride, vs = v / stride;
    int j = -1;
    if (ok) {   // 0 <= u < W and 0 <= v < H: the map read and the cell index are in range
      const double d = (double)(depth_points ? depth[i] : depth[(size_t)(int)v * W + (int)u]);
      good = fabs(d - z) < thr;
      j = (int)us + (int)vs * (W / (int)stride);
    }
    proj[(size_t)i * 2] = (float)us; proj[(size_t)i * 2 + 1] = (float)vs;
    zout[i] = (float)z;
    valid[i] = ok ? 1 : 0; pos[i] = good ? 1 : 0;
    cell[i] = j;   // of every valid row for now: pair_emit_kernel knows the positive set
  }
  nl_wave_rank(ok, wv);
  nl_wave_rank(good, wp);
  __syncthreads();
  if (threadIdx.x == 0) {
    cnt[blockIdx.x] = nl_group_total<CHUNK / 64>(wv);
    cnt[nchunks + blockIdx.x] = nl_group_total<CHUNK / 64>(wp);
  }
}

__global__ __launch_bounds__(CHUNK) void pair_emit_kernel(const unsigned char* __restrict__ valid, const unsigned char* __restrict__ pos, int N, int cap,
                                                          const int* __restrict__ off, int nchunks, const int* __restrict__ info, int* __restrict__ gt_j,
                                                          long long* __restrict__ pairs) {
  __shared__ int wtot[CHUNK / 64];
  const int i = blockIdx.x * CHUNK + threadIdx.x;
  const bool fallback = info[3] != 0;
  const bool f = i < N && (fallback ? valid[i] : pos[i]) != 0;
  const int rank = nl_wave_rank(f, wtot);
  __syncthreads();
  if (i < N) {
    const int j = f ? gt_j[i] : -1;
    if (!f) gt_j[i] = -1;
    if (f) {
      const int k = off[(fallback ? 0 : nchunks) + blockIdx.x] + nl_group_rank(rank, wtot);
      if (k < cap) { pairs[k] = i; pairs[(size_t)cap + k] = j; }
    }
  }
  if (i < cap && i >= info[0]) { pairs[i] = 0; pairs[(size_t)cap + i] = 0; }
}

// PER values of type T per store (16 bytes; PER == 1: the scalar path of a misaligned `out`).  Elements [lo, hi) of the flat (N, M) matrix; vectors [v0, v1),
// v0 <= v1, cover the aligned part, the first 2 (PER - 1) threads of the grid also take the at most PER - 1 values before and after it.
template <typename T, int PER>
__global__ __launch_bounds__(256) void conf_target_kernel(const int* __restrict__ gt_j, long long M, long long lo, long long hi, long long v0, long long v1,
                                                          T* __restrict__ out) {
  struct alignas(sizeof(T) * PER) Vec { T x[PER]; };
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g < v1 - v0) {
    const long long e = (v0 + g) * PER;
    long long n = e / M, m = e - n * M;
    int j = gt_j[n];
    Vec val;
#pragma unroll
    for (int q = 0; q < PER; ++q) {
      val.x[q] = (T)(m == (long long)j ? 1 : 0);
      if (++m == M && q + 1 < PER) { m = 0; ++n; j = n * M < hi ? gt_j[n] : -1; }
    }
    *reinterpret_cast<Vec*>(out + e) = val;
  }
  if (g < 2 * (PER - 1)) {
    const long long head_end = v0 * PER < hi ? v0 * PER : hi, tail_begin = v1 * PER;   // v1 >= v0: the tail starts at or behind the head's end
    const long long e = g < PER - 1 ? lo + g : tail_begin + (g - (PER - 1));
    if (g < PER - 1 ? e < head_end : e < hi) {
      const long long n = e / M, m = e - n * M;
      out[e] = (T)(m == (long long)gt_j[n] ? 1 : 0);
    }
  }
}

__global__ __launch_bounds__(256) void cell_grid_kernel(int Wc, long long cells, float scale, int vec, float* __restrict__ out) {
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (vec) {   // two cells per 16-byte store, the odd last cell alone
    const long long m = 2 * g;
    if (m + 1 < cells) {
      const float x0 = (float)(int)(m % Wc) * scale, y0 = (float)(int)(m / Wc) * scale;
      const float x1 = (float)(int)((m + 1) % Wc) * scale, y1 = (float)(int)((m + 1) / Wc) * scale;
      reinterpret_cast<float4*>(out)[g] = make_float4(x0, y0, x1, y1);
    } else if (m < cells) {
      out[2 * m] = (float)(int)(m % Wc) * scale; out[2 * m + 1] = (float)(int)(m / Wc) * scale;
    }
  } else if (g < cells) {
    out[2 * g] = (float)(int)(g % Wc) * scale; out[2 * g + 1] = (float)(int)(g / Wc) * scale;
  }
}

size_t scan_bytes(int64_t N, int sets) {
  if (N < 1 || N > NLG_MAX_POINTS) return 0;
  return nl_align_up((size_t)nl_cdiv(N, CHUNK) * sets * sizeof(int), 256);
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

template <typename T, int PER>
int launch_conf_target(const int32_t* gt_j, int64_t M, int64_t lo, int64_t hi, void* out, hipStream_t st) {
  if (PER > 1 && misaligned(out, 16)) return launch_conf_target<T, 1>(gt_j, M, lo, hi, out, st);
  int64_t v0 = nl_cdiv(lo, PER), v1 = hi / PER;
  if (v1 < v0) v1 = v0;
  const int64_t threads = (v1 - v0) > 2 * (PER - 1) ? (v1 - v0) : 2 * (PER - 1);
  hipLaunchKernelGGL((conf_target_kernel<T, PER>), dim3((unsigned)nl_cdiv(threads, 256)), dim3(256), 0, st, (const int*)gt_j, (long long)M, (long long)lo,
                     (long long)hi, (long long)v0, (long long)v1, (T*)out);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // namespace

extern "C" {

int nlg_abi_version(void) { return NLG_ABI_VERSION; }

size_t nlg_select_visible_workspace_bytes(int64_t N) { return scan_bytes(N, 1); }
size_t nlg_build_pairs_workspace_bytes(int64_t N) { return scan_bytes(N, 2); }

int nlg_select_visible(const float* pts, int64_t N, const void* poses, int V, const float* K, int H, int W, unsigned flags, int64_t cap, uint8_t* mask,
                       int64_t* idx, int32_t* info, void* ws, size_t ws_bytes, void* stream) {
  if (N < 1 || V < 1 || H < 1 || W < 1 || cap < 1 || (flags & ~NLG_POSE_F64)) return NL_ERR_BAD_ARG;
  if (!pts || !poses || !K || !mask || !idx || !info) return NL_ERR_BAD_ARG;
  if (N > NLG_MAX_POINTS || V > NLG_MAX_VIEWS || H > NLG_MAX_IMAGE || W > NLG_MAX_IMAGE || cap > MAX_CAP) return NL_ERR_UNSUPPORTED;
  const bool f64 = (flags & NLG_POSE_F64) != 0;
  if (misaligned(pts, 4) || misaligned(K, 4) || misaligned(poses, f64 ? 8 : 4) || misaligned(idx, 8) || misaligned(info, 4)) return NL_ERR_BAD_ARG;
  if (!ws || misaligned(ws, 256) || ws_bytes < nlg_select_visible_workspace_bytes(N)) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nchunks = (int)nl_cdiv(N, CHUNK);
  int* cnt = (int*)ws;
  hipLaunchKernelGGL(vis_mask_kernel, dim3(nchunks), dim3(CHUNK), 0, st, pts, (int)N, poses, V, (int)f64, K, H, W, (unsigned char*)mask, cnt);
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_kernel<1>, dim3(1), dim3(SCAN_THREADS), 0, st, cnt, nchunks, (int)cap, (int*)info);
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(vis_emit_kernel, dim3((unsigned)nl_cdiv(N > cap ? N : cap, CHUNK)), dim3(CHUNK), 0, st, (const unsigned char*)mask, (int)N, (int)cap,
                     (const int*)cnt, (const int*)info, (long long*)idx);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlg_build_pairs(const float* pts, int64_t N, const void* pose, const float* K, int H, int W, int stride, double thr, const float* depth, unsigned flags,
                    int64_t cap, float* proj, float* z, uint8_t* valid, uint8_t* pos, int32_t* gt_j, int64_t* pairs, int32_t* info, void* ws, size_t ws_bytes,
                    void* stream) {
  if (N < 1 || H < 1 || W < 1 || stride < 1 || cap < 1 || (flags & ~(NLG_POSE_F64 | NLG_DEPTH_POINTS))) return NL_ERR_BAD_ARG;
  if (H % stride != 0 || W % stride != 0) return NL_ERR_BAD_ARG;
  if (!pts || !pose || !K || !depth || !proj || !z || !valid || !pos || !gt_j || !pairs || !info) return NL_ERR_BAD_ARG;
  if (N > NLG_MAX_POINTS || H > NLG_MAX_IMAGE || W > NLG_MAX_IMAGE || cap > MAX_CAP) return NL_ERR_UNSUPPORTED;
  const bool f64 = (flags & NLG_POSE_F64) != 0;
  if (misaligned(pts, 4) || misaligned(K, 4) || misaligned(pose, f64 ? 8 : 4) || misaligned(depth, 4) || misaligned(proj, 4) || misaligned(z, 4) ||
      misaligned(gt_j, 4) || misaligned(pairs, 8) || misaligned(info, 4))
    return NL_ERR_BAD_ARG;
  if (!ws || misaligned(ws, 256) || ws_bytes < nlg_build_pairs_workspace_bytes(N)) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nchunks = (int)nl_cdiv(N, CHUNK);
  int* cnt = (int*)ws;
  hipLaunchKernelGGL(pair_project_kernel, dim3(nchunks), dim3(CHUNK), 0, st, pts, (int)N, pose, (int)f64, K, H, W, (double)stride, thr, depth,
                     (int)((flags & NLG_DEPTH_POINTS) != 0), proj, z, (unsigned char*)valid, (unsigned char*)pos, (int*)gt_j, cnt, nchunks);
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(scan_kernel<2>, dim3(1), dim3(SCAN_THREADS), 0, st, cnt, nchunks, (int)cap, (int*)info);
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(pair_emit_kernel, dim3((unsigned)nl_cdiv(N > cap ? N : cap, CHUNK)), dim3(CHUNK), 0, st, (const unsigned char*)valid,
                     (const unsigned char*)pos, (int)N, (int)cap, (const int*)cnt, nchunks, (const int*)info, (int*)gt_j, (long long*)pairs);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlg_conf_target(const int32_t* gt_j, int64_t N, int64_t M, int dtype, int64_t row_begin, int64_t row_end, void* out, void* stream) {
  if (N < 1 || M < 1 || row_begin < 0 || row_end < row_begin || row_end > N || (dtype != NLG_TARGET_F32 && dtype != NLG_TARGET_I64)) return NL_ERR_BAD_ARG;
  if (N > MAX_TARGET_DIM || M > MAX_TARGET_DIM) return NL_ERR_UNSUPPORTED;
  if (row_end == row_begin) return NL_OK;
  if (!gt_j || !out || misaligned(gt_j, 4) || misaligned(out, dtype == NLG_TARGET_F32 ? 4 : 8)) return NL_ERR_BAD_ARG;
  const int64_t lo = row_begin * M, hi = row_end * M;
  if (nl_cdiv(hi - lo, 256) + 1 > INT32_MAX) return NL_ERR_UNSUPPORTED;   // the grid of one launch
  return dtype == NLG_TARGET_F32 ? launch_conf_target<float, 4>(gt_j, M, lo, hi, out, (hipStream_t)stream)
                                 : launch_conf_target<long long, 2>(gt_j, M, lo, hi, out, (hipStream_t)stream);
}

int nlg_cell_grid(int Hc, int Wc, float scale, float* out, void* stream) {
  if (Hc < 1 || Wc < 1 || !out || misaligned(out, 8)) return NL_ERR_BAD_ARG;
  if (Hc > NLG_MAX_IMAGE || Wc > NLG_MAX_IMAGE) return NL_ERR_UNSUPPORTED;
  const int64_t cells = (int64_t)Hc * Wc;
  const int vec = misaligned(out, 16) ? 0 : 1;
  hipLaunchKernelGGL(cell_grid_kernel, dim3((unsigned)nl_cdiv(vec ? nl_cdiv(cells, 2) : cells, 256)), dim3(256), 0, (hipStream_t)stream, Wc, (long long)cells, scale,
                     vec, out);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // extern "C"
