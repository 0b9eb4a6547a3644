// The nl_pnp_* entry points of libnerfloc_render.so (include/nerfloc_render.h states the algorithm).  The kernels and the host helpers are csrc/pnp_kernels.h, which
// head_pnp.hip (libnerfloc_head.so: the same solver with the match counts in device memory) includes too.
#include "pnp_kernels.h"

extern "C" {

size_t nl_pnp_workspace_bytes(int64_t M_total, int64_t B, int H) {
  if (M_total < 0 || B < 0 || B > PNP_MAX_B || !pnp_h_ok(H)) return 0;
  return pnp_carve(nullptr, B, H).total;   // candidates, solutions per sample, counts: nothing is kept per match (the mask output is the local optimisation's scratch)
}

int nl_pnp_samples(uint64_t seed, const int32_t* offsets, int64_t B, int H, int32_t* samples, void* stream) {
  if (B < 0) return NL_ERR_BAD_ARG;
  if (!pnp_h_ok(H) || B > PNP_MAX_B) return NL_ERR_UNSUPPORTED;
  if (B == 0) return NL_OK;
  if (!offsets || offsets[0] != 0 || !samples) return NL_ERR_BAD_ARG;
  for (int64_t b = 0; b < B; ++b)
    if (offsets[b + 1] < offsets[b]) return NL_ERR_BAD_ARG;
  for (int64_t b = 0; b < B; ++b)
    if (offsets[b + 1] - offsets[b] > PNP_MAX_M) return NL_ERR_UNSUPPORTED;
  for (int64_t b0 = 0; b0 < B; b0 += PNP_CHUNK) {
    const int n = (int)(B - b0 < PNP_CHUNK ? B - b0 : PNP_CHUNK);
    const PnpBatch pb = pnp_batch(offsets, nullptr, nullptr, b0, n);   // no intrinsics: the indices depend on (seed, b, h, M) alone
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3(H / 64, n), dim3(64), 0, (hipStream_t)stream, pb, H, (unsigned)seed, (unsigned)(seed >> 32), (const float*)nullptr,
                       (const float*)nullptr, samples, (double*)nullptr, (int*)nullptr);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

int nl_pnp_hypotheses(const float* pts2d, const float* pts3d, const int32_t* offsets, const double* intrinsics, int64_t B, int H, uint64_t seed, int32_t* samples,
                      double* poses, int32_t* nsol, void* stream) {
  if (B < 0) return NL_ERR_BAD_ARG;
  if (!pnp_h_ok(H) || B > PNP_MAX_B) return NL_ERR_UNSUPPORTED;
  if (B == 0) return NL_OK;
  if (const int s = pnp_check_problems(offsets, intrinsics, nullptr, B)) return s;
  if (!poses || !nsol || (offsets[B] > 0 && (!pts2d || !pts3d))) return NL_ERR_BAD_ARG;
  for (int64_t b0 = 0; b0 < B; b0 += PNP_CHUNK) {
    const int n = (int)(B - b0 < PNP_CHUNK ? B - b0 : PNP_CHUNK);
    const PnpBatch pb = pnp_batch(offsets, intrinsics, nullptr, b0, n);
    hipLaunchKernelGGL(pnp_hyp_kernel, dim3(H / 64, n), dim3(64), 0, (hipStream_t)stream, pb, H, (unsigned)seed, (unsigned)(seed >> 32), pts2d, pts3d, samples, poses,
                       nsol);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

int nl_pnp_score(const float* pts2d, const float* pts3d, int64_t M, const double* intrinsics, double thr, const double* poses, const int32_t* nsol, int64_t P,
                 int32_t* counts, void* stream) {
  if (M < 0 || P < 0 || (nsol && P % 4 != 0)) return NL_ERR_BAD_ARG;
  if (M > PNP_MAX_M || P > (int64_t)1 << 30) return NL_ERR_UNSUPPORTED;
  if (P == 0) return NL_OK;
  const int32_t offsets[2] = {0, (int32_t)M};
  if (const int s = pnp_check_problems(offsets, intrinsics, &thr, 1)) return s;
  if (!poses || !counts || (M > 0 && (!pts2d || !pts3d))) return NL_ERR_BAD_ARG;
  const PnpBatch pb = pnp_batch(offsets, intrinsics, &thr, 0, 1);
  hipLaunchKernelGGL(pnp_score_kernel, dim3((unsigned)nl_cdiv(P, 64), 1), dim3(256), 0, (hipStream_t)stream, pb, (long long)P, pts2d, pts3d, poses, nsol, counts);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nl_pnp_refine(const float* pts2d, const float* pts3d, int64_t M, const double* intrinsics, double thr, int min_inliers, const double* pose_in, double* pose_out,
                  uint8_t* mask, int32_t* info, void* stream) {
  if (M < 0 || min_inliers < 4) return NL_ERR_BAD_ARG;
  if (M > PNP_MAX_M) return NL_ERR_UNSUPPORTED;
  const int32_t offsets[2] = {0, (int32_t)M};
  if (const int s = pnp_check_problems(offsets, intrinsics, &thr, 1)) return s;
  if (!pose_in || !pose_out || !info || (M > 0 && (!pts2d || !pts3d || !mask))) return NL_ERR_BAD_ARG;
  const PnpBatch pb = pnp_batch(offsets, intrinsics, &thr, 0, 1);
  hipLaunchKernelGGL(pnp_lo_kernel, dim3(1), dim3(PNP_LO_THREADS), 0, (hipStream_t)stream, pb, 1ll, min_inliers, pts2d, pts3d, pose_in, (const int*)nullptr, pose_out,
                     mask, info);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nl_pnp_ransac(const float* pts2d, const float* pts3d, const int32_t* offsets, const double* intrinsics, const double* thr, int64_t B, int H, uint64_t seed,
                  int min_inliers, double* poses, uint8_t* mask, int32_t* info, int32_t* counts, void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || min_inliers < 4) return NL_ERR_BAD_ARG;
  if (!pnp_h_ok(H) || B > PNP_MAX_B) return NL_ERR_UNSUPPORTED;
  if (B == 0) return NL_OK;
  if (!thr) return NL_ERR_BAD_ARG;
  if (const int s = pnp_check_problems(offsets, intrinsics, thr, B)) return s;
  if (!poses || !info || (offsets[B] > 0 && (!pts2d || !pts3d || !mask))) return NL_ERR_BAD_ARG;
  if (!ws || ((uintptr_t)ws & 255) != 0 || ws_bytes < nl_pnp_workspace_bytes(offsets[B], B, H)) return NL_ERR_WORKSPACE;
  const PnpWs w = pnp_carve(ws, B, H);
  int* cnt = counts ? counts : w.counts;
  hipStream_t st = (hipStream_t)stream;
  const long long P = 4ll * H;
  for (int64_t b0 = 0; b0 < B; b0 += PNP_CHUNK) {
    const int n = (int)(B - b0 < PNP_CHUNK ? B - b0 : PNP_CHUNK);
    const PnpBatch pb = pnp_batch(offsets, intrinsics, thr, b0, n);
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
