// libnerfloc_counted.so (include/nerfloc_counted.h, nlk_*): the coarse matching stage with the number of 3-D points in DEVICE memory.
//
// nlk_sct_forward_counted / nlk_sct_layer_counted are nl_sct_forward / nl_sct_layer (sct.hip) on the shared kernels of sct_kernels.h: the projection and chain
// kernels are launched as they are (rows are independent), the attention kernel in its counted instantiation (a trailing SctCount) wherever sequence 0 is the key
// side.  The grids are sized for the capacity; the kernel derives the key geometry from the count (sct_kernels.h).
// nlk_s2d_select_counted is the selection of s2d.hip on a score matrix in memory: s2d_select_kernel's rule, with the row and column maxima — which nl_s2d_match's
// score kernel reduces on the fly over ALL rows — taken here over the rows below the count, by unsigned integer max on the float bits.
#include "sct_kernels.h"
#include "../../include/nerfloc_counted.h"

namespace {

__device__ __forceinline__ int nlk_count(const int32_t* n_dev, int cap) {   // wave-uniform: the address is a kernel argument
  if (!n_dev) return cap;
  const int raw = __builtin_amdgcn_readfirstlane(*n_dev);
  return raw < 0 ? 0 : raw < cap ? raw : cap;
}

// the maxima start from zero: a kernel, not a memset node (s2d.hip says why)
__global__ __launch_bounds__(256) void nlk_zero_kernel(unsigned* p, long long words) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < words) p[i] = 0u;
}

// A workgroup owns 64 rows x 64 columns; wave w takes rows 16 w .. 16 w + 15, lane l column l: coalesced 256-byte row pieces.  Row maxima meet across the lanes,
// column maxima stay in the lane; both reach memory by integer atomic max on the bits (scores >= +0).  Rows at and beyond the count are not read.
__global__ __launch_bounds__(256) void nlk_maxima_kernel(const float* scores, int N, int M, const int32_t* n_dev, unsigned* rowmax, unsigned* colmax) {
  const int n = nlk_count(n_dev, N);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned ct = (unsigned)((M + 63) >> 6), by = blockIdx.x / ct;   // column tiles fastest
  const int j = (int)(blockIdx.x - by * ct) * 64 + lane;
  const int r0 = (int)by * 64 + wave * 16;
  if (r0 >= n) return;   // wave-uniform
  const int r1 = r0 + 16 < n ? r0 + 16 : n;
  unsigned cm = 0u;
  for (int i = r0; i < r1; ++i) {
    unsigned s = j < M ? __float_as_uint(scores[(size_t)i * M + j]) : 0u;
    cm = max(cm, s);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s = max(s, (unsigned)__shfl_xor((int)s, o));
    if (lane == 0 && s != 0u) atomicMax(rowmax + i, s);
  }
  if (j < M && cm != 0u) atomicMax(colmax + j, cm);
}

// one wave per row: s2d_select_kernel's search (s2d.hip) for rows below the count, -1 / 0 for the others
__global__ __launch_bounds__(256) void nlk_select_kernel(const float* scores, const unsigned* rowmax, const unsigned* colmax, int N, int M, const int32_t* n_dev,
                                                         float thr, int32_t* match_j, float* match_score) {
  const int cnt = nlk_count(n_dev, N);
  const int lane = threadIdx.x & 63;
  const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (n >= N) return;
  int found = -1;
  unsigned rm = 0u;
  if (n < cnt) {   // wave-uniform
    rm = rowmax[n];
    if (__uint_as_float(rm) > thr) {
      const float* row = scores + (size_t)n * M;
      for (int j0 = 0; j0 < M; j0 += 64) {
        const int j = j0 + lane;
        bool hit = false;
        if (j < M) {
          const unsigned s = __float_as_uint(row[j]);
          hit = s == rm && s == colmax[j];
        }
        const unsigned long long bal = __ballot(hit);
        if (bal) { found = j0 + __builtin_ctzll(bal); break; }
      }
    }
  }
  if (lane == 0) {
    match_j[n] = found;
    match_score[n] = found >= 0 ? __uint_as_float(rm) : 0.f;
  }
}

struct NlkSelWs { size_t rowmax, colmax, total; };
NlkSelWs nlk_sel_ws(int64_t N, int64_t M) {
  NlkSelWs w;
  w.rowmax = 0;
  w.colmax = nl_align_up((size_t)N * 4, 256);
  w.total = w.colmax + nl_align_up((size_t)M * 4, 256);
  return w;
}
// ... and the 64 x 64 tiles of the matrix fit a one-dimensional grid of 256-thread workgroups (2^24 tiles = 2^32 threads, the most a launch takes)
bool nlk_sel_shape_ok(int64_t N, int64_t M) { return N >= 1 && M >= 1 && N <= (1 << 30) && M <= (1 << 30) && nl_cdiv(N, 64) * nl_cdiv(M, 64) <= (1 << 24); }

}  // namespace

extern "C" {

int nlk_abi_version(void) { return NLK_ABI_VERSION; }

size_t nlk_sct_workspace_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F) {
  (void)F;   // the hidden rows never leave LDS
  if (!sct_counts_ok(B, N0, N1) || C < 1 || !sct_counts_fit(B, N0, N1, N0 > N1 ? N0 : N1)) return 0;
  return 4 * sct_ws_part(B ? B : 1, N0, N1, C);
}

int nlk_sct_layer_counted(const void* packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos, int64_t Nq, const float* mem,
                          const float* mem_pos, int64_t Nk, const int32_t* nk_dev, int64_t B, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (layer < 0 || layer >= SCT_LAYERS) return NL_ERR_BAD_ARG;
  if (layer < 2) {   // self layers: the memory side is the target side
    if ((mem && mem != x) || (mem_pos && mem_pos != x_pos) || Nk != Nq) return NL_ERR_BAD_ARG;
    mem = x; mem_pos = x_pos;
  }
  if (((uintptr_t)nk_dev & 3) != 0) return NL_ERR_BAD_ARG;
  const void* ptrs[5] = {x, x_pos, mem, mem_pos, out};
  bool empty;
  if (const int s = sct_check(packed, C, nhead, F, precision, B, Nq, Nk, ptrs, 5, ws, ws_bytes, &empty)) return s;
  if (empty) return NL_OK;
  SctRun r{(const unsigned char*)packed, C, F, layer, x, x_pos, Nq, mem, mem_pos, Nk, B, out, (unsigned char*)ws, sct_ws_part(B, Nq, Nk, C)};
  r.nk_dev = nk_dev;
  return sct_run<true>(r, precision, (hipStream_t)stream);
}

int nlk_sct_forward_counted(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const int32_t* n0_dev,
                            const float* v1, const float* pos1, int64_t N1, int64_t B, float* out0, float* out1, void* ws, size_t ws_bytes, void* stream) {
  if (((uintptr_t)n0_dev & 3) != 0) return NL_ERR_BAD_ARG;
  const void* ptrs[6] = {v0, pos0, v1, pos1, out0, out1};
  bool empty;
  if (const int s = sct_check(packed, C, nhead, F, precision, B, N0, N1, ptrs, 6, ws, ws_bytes, &empty)) return s;
  if (empty) return NL_OK;
  if (out0 == out1) return NL_ERR_BAD_ARG;
  const unsigned char* img = (const unsigned char*)packed;
  unsigned char* w = (unsigned char*)ws;
  const size_t part = sct_ws_part(B, N0, N1, C);
  hipStream_t st = (hipStream_t)stream;
  // nl_sct_forward's four layers; sequence 0 is the key side of layers 0 and 3
  SctRun r[SCT_LAYERS] = {{img, C, F, 0, v0, pos0, N0, v0, pos0, N0, B, out0, w, part},
                          {img, C, F, 1, v1, pos1, N1, v1, pos1, N1, B, out1, w, part},
                          {img, C, F, 2, out0, pos0, N0, out1, pos1, N1, B, out0, w, part},
                          {img, C, F, 3, out1, pos1, N1, out0, pos0, N0, B, out1, w, part}};
  r[0].nk_dev = r[3].nk_dev = n0_dev;
  for (int l = 0; l < SCT_LAYERS; ++l)
    if (const int s = sct_run<true>(r[l], precision, st)) return s;
  return NL_OK;
}

size_t nlk_s2d_select_workspace_bytes(int64_t N, int64_t M) { return nlk_sel_shape_ok(N, M) ? nlk_sel_ws(N, M).total : 0; }

int nlk_s2d_select_counted(const float* scores, int64_t N, int64_t M, const int32_t* n_dev, float thr, int32_t* match_j, float* match_score, void* ws,
                           size_t ws_bytes, void* stream) {
  if (N < 1 || M < 1) return NL_ERR_BAD_ARG;
  if (!nlk_sel_shape_ok(N, M)) return NL_ERR_UNSUPPORTED;
  if (!scores || !match_j || !match_score) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)scores | (uintptr_t)match_j | (uintptr_t)match_score | (uintptr_t)n_dev) & 3) != 0) return NL_ERR_BAD_ARG;
  const NlkSelWs w = nlk_sel_ws(N, M);
  if (!ws || ws_bytes < w.total || ((uintptr_t)ws & 255) != 0) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  unsigned* rowmax = (unsigned*)((unsigned char*)ws + w.rowmax);
  unsigned* colmax = (unsigned*)((unsigned char*)ws + w.colmax);
  hipLaunchKernelGGL(nlk_zero_kernel, dim3((unsigned)nl_cdiv((int64_t)(w.total / 4), 256)), dim3(256), 0, st, (unsigned*)ws, (long long)(w.total / 4));
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nlk_maxima_kernel, dim3((unsigned)(nl_cdiv(M, 64) * nl_cdiv(N, 64))), dim3(256), 0, st, scores, (int)N, (int)M, n_dev, rowmax, colmax);
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(nlk_select_kernel, dim3((unsigned)nl_cdiv(N, 4)), dim3(256), 0, st, scores, (const unsigned*)rowmax, (const unsigned*)colmax, (int)N, (int)M, n_dev,
                     thr, match_j, match_score);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // extern "C"
