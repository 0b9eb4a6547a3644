// libnerfloc_head.so, part 1 (include/nerfloc_head.h states the contracts; tests/head_ref.py restates them in numpy): the glue of the localisation head that has to
// stay on the device for "descriptors in, pose out" to be queued without a host round trip.
//   nlh_select_matches   the ordered, fixed-capacity match lists of the coarse stage with a DEVICE-side count.  Three launches, a plain chain (compact.h):
//     sel_scan_kernel    one workgroup: matched rows per chunk of 256 (ballot + popcount per wave), then the exclusive scan of the chunk counts and `info`
//     sel_write_kernel   one workgroup per chunk: rank inside the wave from the ballot, the four wave totals added in wave order, + the chunk's offset = k;
//                        ids and points of the rows with k < cap
//     sel_rows_kernel    one wave per OUTPUT row k: the optional table rows of i_ids[k] for k < count, zeros (ids, points, rows) for count <= k < cap
//   nlh_pos_sine_grid    PositionEmbeddingSine(C / 2, normalize=True, 'lin_sine') of an (H, W) map: one thread per output value
//   nlh_embed_points     the NeRF embedder sin / cos(x 2^l): one thread per (point, frequency, coordinate)
// Integers only where order could matter (no atomics at all): two calls give the same bits.  The sines are ocml's full-range sinf / cosf (Payne-Hanek reduction
// for large arguments), never the hardware v_sin_f32: the embedder's arguments reach 2^31 |x|.
#include "common.h"
#include "compact.h"
#include "../../include/nerfloc_head.h"

namespace {

constexpr int SEL_CHUNK = 256;             // rows per workgroup of sel_write_kernel
constexpr int SEL_SCAN_THREADS = 1024;
constexpr int64_t SEL_MAX_N = 1 << 20;     // 4096 chunks: four per thread of the scan
constexpr int64_t SEL_MAX_CAP = 1 << 24;
constexpr int SEL_MAX_C = 512;

__device__ __forceinline__ bool sel_matched(const int* __restrict__ match_j, int i, int N, int Mc) {
  if (i >= N) return false;
  const int j = match_j[i];
  return j >= 0 && j < Mc;
}

__global__ __launch_bounds__(SEL_SCAN_THREADS) void sel_scan_kernel(const int* __restrict__ match_j, int N, int Mc, int cap, int nchunks, int* __restrict__ chunk_off,
                                                                    int* __restrict__ info) {
  __shared__ int part[SEL_SCAN_THREADS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int c = wave; c < nchunks; c += SEL_SCAN_THREADS / 64) {   // wave-uniform
    int cnt = 0;
#pragma unroll
    for (int q = 0; q < SEL_CHUNK / 64; ++q) cnt += __popcll(__ballot(sel_matched(match_j, c * SEL_CHUNK + q * 64 + lane, N, Mc)));
    if (lane == 0) chunk_off[c] = cnt;
  }
  __syncthreads();   // the counts, written by other waves, are what the scan reads
  const int total = nl_scan_exclusive<SEL_SCAN_THREADS>(chunk_off, nchunks, part);
  if (tid == SEL_SCAN_THREADS - 1) { info[0] = min(total, cap); info[1] = total; info[2] = total > cap ? 1 : 0; info[3] = 0; }
}

__global__ __launch_bounds__(SEL_CHUNK) void sel_write_kernel(const int* __restrict__ match_j, int N, int Mc, int cap, const int* __restrict__ chunk_off,
                                                              const float* __restrict__ kps3d, const float* __restrict__ kps2d, long long* __restrict__ i_ids,
                                                              long long* __restrict__ j_ids, long long* __restrict__ b_ids, float* __restrict__ mkps3d,
                                                              float* __restrict__ mkps2d_c) {
  __shared__ int wtot[SEL_CHUNK / 64];
  const int i = blockIdx.x * SEL_CHUNK + threadIdx.x;
  const bool f = sel_matched(match_j, i, N, Mc);
  const int rank = nl_wave_rank(f, wtot);   // matched lanes below this one
  __syncthreads();
  const int k = chunk_off[blockIdx.x] + nl_group_rank(rank, wtot);
  if (f && k < cap) {
    const int j = match_j[i];
    i_ids[k] = i; j_ids[k] = j; b_ids[k] = 0;
    mkps3d[(size_t)k * 3] = kps3d[(size_t)i * 3]; mkps3d[(size_t)k * 3 + 1] = kps3d[(size_t)i * 3 + 1]; mkps3d[(size_t)k * 3 + 2] = kps3d[(size_t)i * 3 + 2];
    mkps2d_c[(size_t)k * 2] = kps2d[(size_t)j * 2]; mkps2d_c[(size_t)k * 2 + 1] = kps2d[(size_t)j * 2 + 1];
  }
}

// blockDim (64, 4): wave y of workgroup x is output row k = 4 x + y.  rows_a / rows_b and their outputs are 16-byte aligned with C % 4 == 0 (checked by the host).
__global__ __launch_bounds__(256) void sel_rows_kernel(int cap, int C4, const int* __restrict__ info, const float4* __restrict__ rows_a, const float4* __restrict__ rows_b,
                                                       long long* __restrict__ i_ids, long long* __restrict__ j_ids, long long* __restrict__ b_ids,
                                                       float* __restrict__ mkps3d, float* __restrict__ mkps2d_c, float4* __restrict__ out_a, float4* __restrict__ out_b) {
  const int k = blockIdx.x * 4 + threadIdx.y, lane = threadIdx.x;
  if (k >= cap) return;
  const bool live = k < info[0];
  if (!live && lane == 0) {
    i_ids[k] = 0; j_ids[k] = 0; b_ids[k] = 0;
    mkps3d[(size_t)k * 3] = 0.f; mkps3d[(size_t)k * 3 + 1] = 0.f; mkps3d[(size_t)k * 3 + 2] = 0.f;
    mkps2d_c[(size_t)k * 2] = 0.f; mkps2d_c[(size_t)k * 2 + 1] = 0.f;
  }
  const size_t src = live ? (size_t)i_ids[k] * C4 : 0, dst = (size_t)k * C4;   // i_ids[k] < N: written by sel_write_kernel from a row index
  for (int c = lane; c < C4; c += 64) {
    float4 va = make_float4(0.f, 0.f, 0.f, 0.f), vb = va;
    if (live && rows_a) va = rows_a[src + c];
    if (live && rows_b) vb = rows_b[src + c];
    if (rows_a) out_a[dst + c] = va;
    if (rows_b) out_b[dst + c] = vb;
  }
}

// channel c of (h, w): c < C / 2 a sine, else a cosine; inside a half, frequency (c' / 2) + 1 and x (c' even) or y (c' odd).  fp32 throughout, in the order of the
// eager formulation: (cumsum - 0.5) / (size + 1e-6), then the product with float(i * pi) (-ffp-contract=off keeps the operations apart)
__global__ __launch_bounds__(256) void pos_sine_kernel(int H, int W, int C, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = (long long)H * W * C;
  if (idx >= total) return;
  const int c = (int)(idx % C);
  const long long hw = idx / C;
  const int w = (int)(hw % W), h = (int)(hw / W);
  const int half = C / 2, cc = c < half ? c : c - half;
  const int freq = cc / 2 + 1;
  const bool is_y = cc & 1;
  const float e = is_y ? ((float)(h + 1) - 0.5f) / ((float)H + 1e-6f) : ((float)(w + 1) - 0.5f) / ((float)W + 1e-6f);
  const float arg = (float)((double)freq * 3.141592653589793) * e;
  out[idx] = c < half ? sinf(arg) : cosf(arg);
}

// out[n][(2 l + s) D + d] = s ? cos : sin of x[n][d] 2^l; the product is exact (a power of two), so the argument is the reference's
__global__ __launch_bounds__(256) void embed_points_kernel(const float* __restrict__ x, long long N, int D, int L, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  const long long total = N * D * L;
  if (idx >= total) return;
  const int d = (int)(idx % D);
  const long long nl = idx / D;
  const int l = (int)(nl % L);
  const long long n = nl / L;
  const float arg = x[n * D + d] * ldexpf(1.f, l);
  float* o = out + n * (2ll * D * L) + (2ll * l) * D + d;
  o[0] = sinf(arg);
  o[D] = cosf(arg);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int nlh_abi_version(void) { return NLH_ABI_VERSION; }

size_t nlh_select_workspace_bytes(int64_t N) {
  if (N < 1 || N > SEL_MAX_N) return 0;
  return nl_align_up((size_t)nl_cdiv(N, SEL_CHUNK) * sizeof(int), 256);
}

int nlh_select_matches(const int32_t* match_j, int64_t N, int64_t cap, int64_t Mc, int C, const float* kps3d, const float* kps2d, const float* rows_a, const float* rows_b,
                       int64_t* i_ids, int64_t* j_ids, int64_t* b_ids, float* mkps3d, float* mkps2d_c, float* out_a, float* out_b, int32_t* info, void* ws,
                       size_t ws_bytes, void* stream) {
  if (N < 1 || cap < 1 || Mc < 0) return NL_ERR_BAD_ARG;
  if (!match_j || !kps3d || (Mc > 0 && !kps2d) || !i_ids || !j_ids || !b_ids || !mkps3d || !mkps2d_c || !info) return NL_ERR_BAD_ARG;
  if ((rows_a && !out_a) || (rows_b && !out_b)) return NL_ERR_BAD_ARG;
  const bool rows = rows_a || rows_b;
  if (rows && (C < 4 || C % 4 != 0)) return NL_ERR_BAD_ARG;
  if (N > SEL_MAX_N || cap > SEL_MAX_CAP || Mc > INT32_MAX || (rows && C > SEL_MAX_C)) return NL_ERR_UNSUPPORTED;
  if (rows && (!aligned16(rows_a) || !aligned16(rows_b) || !aligned16(out_a) || !aligned16(out_b))) return NL_ERR_BAD_ARG;
  if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < nlh_select_workspace_bytes(N)) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const int nchunks = (int)nl_cdiv(N, SEL_CHUNK);
  int* chunk_off = (int*)ws;
  hipLaunchKernelGGL(sel_scan_kernel, dim3(1), dim3(SEL_SCAN_THREADS), 0, st, match_j, (int)N, (int)Mc, (int)cap, nchunks, chunk_off, info);
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(sel_write_kernel, dim3(nchunks), dim3(SEL_CHUNK), 0, st, match_j, (int)N, (int)Mc, (int)cap, (const int*)chunk_off, kps3d, kps2d,
                     (long long*)i_ids, (long long*)j_ids, (long long*)b_ids, mkps3d, mkps2d_c);
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(sel_rows_kernel, dim3((unsigned)nl_cdiv(cap, 4)), dim3(64, 4), 0, st, (int)cap, rows ? C / 4 : 0, (const int*)info, (const float4*)rows_a,
                     (const float4*)rows_b, (long long*)i_ids, (long long*)j_ids, (long long*)b_ids, mkps3d, mkps2d_c, (float4*)out_a, (float4*)out_b);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlh_pos_sine_grid(int H, int W, int C, float* out, void* stream) {
  if (H < 1 || W < 1 || C < 4 || C % 4 != 0 || !out) return NL_ERR_BAD_ARG;
  const int64_t total = (int64_t)H * W * C;
  if (H > (1 << 15) || W > (1 << 15) || C > 4096 || total > ((int64_t)1 << 31)) return NL_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(pos_sine_kernel, dim3((unsigned)nl_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, H, W, C, out);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlh_embed_points(const float* x, int64_t N, int D, int L, float* out, void* stream) {
  if (N < 0 || D < 1 || L < 1) return NL_ERR_BAD_ARG;
  if (L > 32 || D > 64 || N > ((int64_t)1 << 24)) return NL_ERR_UNSUPPORTED;   // 2^(L - 1) must be an fp32 power of two the product cannot overflow in practice
  if (N == 0) return NL_OK;
  if (!x || !out) return NL_ERR_BAD_ARG;
  const int64_t total = N * D * L;
  hipLaunchKernelGGL(embed_points_kernel, dim3((unsigned)nl_cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, (long long)N, D, L, out);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // extern "C"
