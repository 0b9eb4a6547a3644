// libnerfloc_head.so, part 2: nlh_pnp_ransac_counted = nl_pnp_ransac (csrc/pnp.hip) with each problem's match count read from DEVICE memory.  The kernels are
// csrc/pnp_kernels.h, shared with pnp.hip: their grids never depended on the count, so the count enters each of them in one place (pnp_m).  The host offsets give
// each problem's capacity and its place in the arrays; what the host checks of them is what nl_pnp_ransac checks.
#include "pnp_kernels.h"
#include "../../include/nerfloc_head.h"

extern "C" {

size_t nlh_pnp_workspace_bytes(int64_t cap_total, int64_t B, int H) {
  if (cap_total < 0 || B < 0 || B > PNP_MAX_B || !pnp_h_ok(H)) return 0;
  return pnp_carve(nullptr, B, H).total;
}

int nlh_pnp_ransac_counted(const float* pts2d, const float* pts3d, const int32_t* offsets, const int32_t* counts_dev, const double* intrinsics, const double* thr,
                           int64_t B, int H, uint64_t seed, int min_inliers, double* poses, uint8_t* mask, int32_t* info, int32_t* counts, void* ws, size_t ws_bytes,
                           void* stream) {
  if (B < 0 || min_inliers < 4) return NL_ERR_BAD_ARG;
  if (!pnp_h_ok(H) || B > PNP_MAX_B) return NL_ERR_UNSUPPORTED;
  if (B == 0) return NL_OK;
  if (!thr || !counts_dev) return NL_ERR_BAD_ARG;
  if (const int s = pnp_check_problems(offsets, intrinsics, thr, B)) return s;
  if (!poses || !info || (offsets[B] > 0 && (!pts2d || !pts3d || !mask))) return NL_ERR_BAD_ARG;
  if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < nlh_pnp_workspace_bytes(offsets[B], B, H)) return NL_ERR_WORKSPACE;
  const PnpWs w = pnp_carve(ws, B, H);
  int* cnt = counts ? counts : w.counts;
  hipStream_t st = (hipStream_t)stream;
  const long long P = 4ll * H;
  for (int64_t b0 = 0; b0 < B; b0 += PNP_CHUNK) {
    const int n = (int)(B - b0 < PNP_CHUNK ? B - b0 : PNP_CHUNK);
    const PnpBatch pb = pnp_batch(offsets, intrinsics, thr, b0, n, counts_dev);
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3(H / 64, n), dim3(64), 0, st, pb, H, (unsigned)seed, (unsigned)(seed >> 32), pts2d, pts3d, (int*)nullptr, w.poses, w.nsol);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pnp_score_kernel, dim3((unsigned)(P / 64), n), dim3(256), 0, st, pb, P, pts2d, pts3d, (const double*)w.poses, (const int*)w.nsol, cnt);
    NL_LAUNCH_CHECK();
    hipLaunchKernelGGL(pnp_lo_kernel, dim3(n), dim3(PNP_LO_THREADS), 0, st, pb, P, min_inliers, pts2d, pts3d, (const double*)w.poses, (const int*)cnt, poses, mask,
                       info);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

}  // extern "C"
