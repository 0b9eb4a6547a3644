// Absolute camera pose from 2D-3D matches (nl_pnp_*): P3P RANSAC with a fixed number of hypotheses, an integer inlier score, a fixed-order selection and a
// Gauss-Newton local optimisation, all on the caller's stream.  include/nerfloc_render.h states the algorithm (the contract); tests/pnp_ref.py restates it in fp64
// numpy with the expressions in THIS file's order of operations (-ffp-contract=off: the two agree to rounding, libm's cos / acos / cbrt / sin aside).
// Everything after loading the fp32 matches is fp64.  No float atomics and no order-dependent float sum: the score is an integer count per candidate, the normal
// equations are summed per thread over its strided inliers and then by a fixed tree through LDS.  A problem's bits depend on (seed, problem index, its own matches,
// intrinsics, threshold, H) alone.
//
// Three kernels, one launch each per chunk of PNP_CHUNK problems (the per-problem host values — offsets, intrinsics, thresholds — travel as a kernel argument, so a
// call makes no copy, allocates nothing and can be captured in a graph as a plain chain):
//   pnp_hyp_kernel     one lane per sample: Philox indices (sct_drop.h's generator), bearings, Grunert's quartic in closed form, up to four poses
//   pnp_score_kernel   one lane per candidate with its pose in registers; 256 matches at a time staged in LDS, each of the workgroup's four waves takes a quarter of
//                      them and reads them by broadcast; the four integer partial counts are added at the end
//   pnp_lo_kernel      one workgroup per problem: arg-max (highest count, lowest index), NL_PNP_LO_ROUNDS x NL_PNP_GN_ITERS Gauss-Newton, the final mask
//
// This header holds the kernels and the host helpers both libraries need: pnp.hip (nl_pnp_*, libnerfloc_render.so) and head_pnp.hip (nlh_pnp_ransac_counted,
// libnerfloc_head.so).  The second differs in ONE value: a problem's match count M comes from device memory (PnpBatch::cnt) instead of the host offsets, which
// then give the problem's capacity.  cnt == NULL (every nl_pnp_* call) is the code as it was: pnp_m() returns the capacity.
#pragma once
#include <cmath>
#include <climits>
#include "common.h"
#include "sct_drop.h"

namespace {

constexpr int PNP_CHUNK = 16;          // problems per launch: their host-side values are one kernel argument of 0.7 KB
constexpr unsigned PNP_TAG = 0x504E50; // the sampler's counter word ("PNP")
constexpr double PNP_DAMP = 1e-12;
constexpr int PNP_MAX_M = 1 << 20;
constexpr int PNP_LO_THREADS = 256;

struct PnpBatch {
  int n, b0;                 // problems of this launch, index of the first in the call
  int off[PNP_CHUNK + 1];    // match offsets
  double fx[PNP_CHUNK], fy[PNP_CHUNK], cx[PNP_CHUNK], cy[PNP_CHUNK], thr2[PNP_CHUNK];
  const int* cnt;            // NULL, or the call's per-problem match counts in DEVICE memory (B int32): the offsets then give capacities
};
// the number of matches of problem bl of the launch: its capacity, or the first min(capacity, max(cnt[b], 0)) of them
__device__ __forceinline__ int pnp_m(const PnpBatch& pb, int bl) {
  const int cap = pb.off[bl + 1] - pb.off[bl];
  return pb.cnt ? min(cap, max(pb.cnt[pb.b0 + bl], 0)) : cap;
}

struct PnpCam { double fx, fy, cx, cy, thr2; };
__device__ __forceinline__ PnpCam pnp_cam(const PnpBatch& pb, int bl) { return PnpCam{pb.fx[bl], pb.fy[bl], pb.cx[bl], pb.cy[bl], pb.thr2[bl]}; }

__device__ __forceinline__ bool pnp_finite12(const double* p) {
  bool ok = true;
#pragma unroll
  for (int k = 0; k < 12; ++k) ok = ok && isfinite(p[k]);
  return ok;
}

// the inlier rule: z > 0 and e^2 <= thr^2
__device__ __forceinline__ bool pnp_inlier(const double* p, const PnpCam& c, double x, double y, double X, double Y, double Z) {
  const double xc = p[0] * X + p[1] * Y + p[2] * Z + p[3];
  const double yc = p[4] * X + p[5] * Y + p[6] * Z + p[7];
  const double zc = p[8] * X + p[9] * Y + p[10] * Z + p[11];
  const double du = c.fx * (xc / zc) + c.cx - x, dv = c.fy * (yc / zc) + c.cy - y;
  return zc > 0.0 && du * du + dv * dv <= c.thr2;
}

// ---- 1. samples: three distinct indices of [0, M), M >= 3, from one generator call
__device__ __forceinline__ void pnp_sample(unsigned k0, unsigned k1, unsigned b, unsigned h, int M, int& i0, int& i1, int& i2) {
  const uint4 w = sct_philox4x32_10(h, 0u, b, PNP_TAG, k0, k1);
  i0 = (int)(((unsigned long long)w.x * (unsigned long long)M) >> 32);
  const int j1 = (int)(((unsigned long long)w.y * (unsigned long long)(M - 1)) >> 32);
  const int j2 = (int)(((unsigned long long)w.z * (unsigned long long)(M - 2)) >> 32);
  i1 = j1 + (j1 >= i0 ? 1 : 0);
  const int lo = min(i0, i1), hi = max(i0, i1);
  i2 = j2 + (j2 >= lo ? 1 : 0);
  i2 = i2 + (i2 >= hi ? 1 : 0);
}

__device__ __forceinline__ void pnp_bearing(const PnpCam& c, double x, double y, double* j) {
  const double bx = (x - c.cx) / c.fx, by = (y - c.cy) / c.fy;
  const double inv = 1.0 / sqrt(bx * bx + by * by + 1.0);
  j[0] = bx * inv; j[1] = by * inv; j[2] = inv;
}
__device__ __forceinline__ void pnp_cross(const double* a, const double* b, double* o) {
  o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
__device__ __forceinline__ double pnp_dot(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }

// the largest real root of m^3 + c2 m^2 + c1 m + c0 (Cardano's or the trigonometric formula), then one Newton step
__device__ __forceinline__ double pnp_cubic_root(double c2, double c1, double c0) {
  const double sh = c2 / 3.0;
  const double P = c1 - c2 * sh;
  const double Q = 2.0 * sh * sh * sh - sh * c1 + c0;
  const double hq = -0.5 * Q;
  const double D = hq * hq + P * P * P / 27.0;
  double t;
  if (D > 0.0) {
    const double sD = sqrt(D);
    t = cbrt(hq + sD) + cbrt(hq - sD);
  } else {
    const double rr = sqrt(P < 0.0 ? -P / 3.0 : 0.0);
    double arg = hq / (rr * rr * rr);
    arg = arg < -1.0 ? -1.0 : arg > 1.0 ? 1.0 : arg;   // a NaN (rr = 0) passes through and is not used
    t = rr > 0.0 ? 2.0 * rr * cos(acos(arg) / 3.0) : 0.0;
  }
  const double m = t - sh;
  const double f = ((m + c2) * m + c1) * m + c0;
  const double df = (3.0 * m + 2.0 * c2) * m + c1;
  const double step = f / df;
  return isfinite(step) ? m - step : m;
}

// ---- 1 + 2: one lane per sample.  samples / poses / nsol may each be null (nl_pnp_samples wants the indices alone, nl_pnp_ransac not at all)
__global__ __launch_bounds__(64) void pnp_hyp_kernel(const PnpBatch pb, int H, unsigned k0, unsigned k1, const float* __restrict__ p2, const float* __restrict__ p3,
                                                     int* __restrict__ samples, double* __restrict__ poses, int* __restrict__ nsol) {
  const int bl = blockIdx.y, b = pb.b0 + bl;
  const int h = blockIdx.x * 64 + threadIdx.x;   // H is a multiple of 64
  const int off = pb.off[bl], M = pnp_m(pb, bl);
  const size_t row = (size_t)b * H + h;
  int id[3] = {-1, -1, -1};
  if (M >= 3) pnp_sample(k0, k1, (unsigned)b, (unsigned)h, M, id[0], id[1], id[2]);
  if (samples) { samples[row * 3] = id[0]; samples[row * 3 + 1] = id[1]; samples[row * 3 + 2] = id[2]; }
  if (!poses) return;
  double* out = poses + row * 48;
  int ns = 0;
  if (M >= 4) {
    const PnpCam cam = pnp_cam(pb, bl);
    double j[3][3], X[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const size_t i = (size_t)off + id[k];
      pnp_bearing(cam, (double)p2[i * 2], (double)p2[i * 2 + 1], j[k]);
      X[k][0] = (double)p3[i * 3]; X[k][1] = (double)p3[i * 3 + 1]; X[k][2] = (double)p3[i * 3 + 2];
    }
    double e1[3], e2[3], e3[3], n[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { e1[k] = X[1][k] - X[0][k]; e2[k] = X[2][k] - X[0][k]; e3[k] = X[2][k] - X[1][k]; }
    const double c2r = pnp_dot(e1, e1), b2r = pnp_dot(e2, e2), a2r = pnp_dot(e3, e3);
    pnp_cross(e1, e2, n);
    const double nn = pnp_dot(n, n);
    const double cg = pnp_dot(j[0], j[1]), cb = pnp_dot(j[0], j[2]), ca = pnp_dot(j[1], j[2]);
    // degenerate sample: world triangle of zero area (or a zero side), coincident bearings
    const bool ok = nn > 1e-12 * c2r * b2r && a2r > 0.0 && 1.0 - cg * cg > 1e-14 && 1.0 - cb * cb > 1e-14 && 1.0 - ca * ca > 1e-14;
    if (ok) {
      const double a2 = a2r / b2r, c2 = c2r / b2r;
      const double k = c2 - a2;
      const double n0 = k - 1.0, n1 = -2.0 * cb * k, n2 = 1.0 + k;
      const double d0 = -2.0 * cg, d1 = 2.0 * ca;
      const double g0 = 1.0 - c2, g1 = 2.0 * c2 * cb, g2 = -c2;
      const double D0 = d0 * d0, D1 = 2.0 * d0 * d1, D2 = d1 * d1;
      const double tc = 2.0 * cg;
      const double A0 = n0 * n0 - tc * (n0 * d0) + g0 * D0;
      const double A1 = 2.0 * n0 * n1 - tc * (n0 * d1 + n1 * d0) + (g0 * D1 + g1 * D0);
      const double A2 = (2.0 * n0 * n2 + n1 * n1) - tc * (n1 * d1 + n2 * d0) + (g0 * D2 + g1 * D1 + g2 * D0);
      const double A3 = 2.0 * n1 * n2 - tc * (n2 * d1) + (g1 * D2 + g2 * D1);
      const double A4 = n2 * n2 + g2 * D2;
      // the quartic, monic and depressed: v = y - a / 4, y^4 + p y^2 + q y + r
      const double qa = A3 / A4, qb = A2 / A4, qc = A1 / A4, qd = A0 / A4;
      const double a4 = 0.25 * qa;
      const double p = qb - 6.0 * a4 * a4;
      const double q = qc - 2.0 * a4 * qb + 8.0 * a4 * a4 * a4;
      const double r = qd - a4 * qc + a4 * a4 * qb - 3.0 * a4 * a4 * a4 * a4;
      const double m = pnp_cubic_root(p, 0.25 * p * p - r, -0.125 * q * q);
      // Ferrari (m > 0): y^2 + s y + (base - hq) = 0 and y^2 - s y + (base + hq) = 0;  else the biquadratic: y^2 = (-p +- sqrt(p^2 - 4 r)) / 2
      const bool ferrari = m > 0.0;
      const double s = sqrt(ferrari ? 2.0 * m : 1.0);
      const double hq = q / (2.0 * s);
      const double base = 0.5 * p + m;
      const double q1 = s * s - 4.0 * (base - hq), q2 = s * s - 4.0 * (base + hq);
      const double db = p * p - 4.0 * r;
      const double sdb = sqrt(db >= 0.0 ? db : 0.0);
      const double z1 = 0.5 * (-p + sdb), z2 = 0.5 * (-p - sdb);
      const double sd1 = sqrt(q1 >= 0.0 ? q1 : 0.0), sd2 = sqrt(q2 >= 0.0 ? q2 : 0.0);
      const double sz1 = sqrt(z1 >= 0.0 ? z1 : 0.0), sz2 = sqrt(z2 >= 0.0 ? z2 : 0.0);
      double r1[3], r2[3], r3[3];
      pnp_cross(e2, n, r1);
      pnp_cross(n, e1, r2);
#pragma unroll
      for (int c = 0; c < 3; ++c) { r1[c] = r1[c] / nn; r2[c] = r2[c] / nn; r3[c] = n[c] / nn; }
#pragma unroll 1
      for (int kk = 0; kk < 4; ++kk) {
        double y;
        bool real;
        if (ferrari) {
          const double sb = kk < 2 ? -s : s;
          const double sg = kk == 0 ? sd1 : kk == 1 ? -sd1 : kk == 2 ? sd2 : -sd2;
          y = 0.5 * (sb + sg);
          real = kk < 2 ? q1 >= 0.0 : q2 >= 0.0;
        } else {
          y = kk == 0 ? sz1 : kk == 1 ? -sz1 : kk == 2 ? sz2 : -sz2;
          real = db >= 0.0 && (kk < 2 ? z1 >= 0.0 : z2 >= 0.0);
        }
        const double v = y - a4;
        const double qv = 1.0 + v * v - 2.0 * cb * v;
        double s1 = sqrt(b2r / qv);
        const double u = ((n2 * v + n1) * v + n0) / (d1 * v + d0);
        double s2 = u * s1, s3 = v * s1;
        // one Newton step on the three law-of-cosines equations, by Cramer's rule
        const double F1 = s1 * s1 + s2 * s2 - 2.0 * s1 * s2 * cg - c2r;
        const double F2 = s1 * s1 + s3 * s3 - 2.0 * s1 * s3 * cb - b2r;
        const double F3 = s2 * s2 + s3 * s3 - 2.0 * s2 * s3 * ca - a2r;
        const double J11 = 2.0 * (s1 - s2 * cg), J12 = 2.0 * (s2 - s1 * cg);
        const double J21 = 2.0 * (s1 - s3 * cb), J23 = 2.0 * (s3 - s1 * cb);
        const double J32 = 2.0 * (s2 - s3 * ca), J33 = 2.0 * (s3 - s2 * ca);
        const double det = -J11 * (J23 * J32) - J12 * (J21 * J33);
        const double ds1 = (-F1 * (J23 * J32) - J12 * (F2 * J33 - J23 * F3)) / det;
        const double ds2 = (J11 * (F2 * J33 - J23 * F3) - F1 * (J21 * J33)) / det;
        const double ds3 = (J11 * (-F2 * J32) - J12 * (J21 * F3) + F1 * (J21 * J32)) / det;
        if (isfinite(ds1) && isfinite(ds2) && isfinite(ds3)) { s1 = s1 - ds1; s2 = s2 - ds2; s3 = s3 - ds3; }
        // the pose from the two congruent triangles: R = [y1 y2 y1 x y2] [e1 e2 e1 x e2]^-1, t = Y1 - R X1
        double y1[3], y2[3], ny[3], pose[12];
#pragma unroll
        for (int c = 0; c < 3; ++c) { const double Y1 = s1 * j[0][c]; y1[c] = s2 * j[1][c] - Y1; y2[c] = s3 * j[2][c] - Y1; }
        pnp_cross(y1, y2, ny);
#pragma unroll
        for (int rr = 0; rr < 3; ++rr) {
#pragma unroll
          for (int c = 0; c < 3; ++c) pose[rr * 4 + c] = y1[rr] * r1[c] + y2[rr] * r2[c] + ny[rr] * r3[c];
          pose[rr * 4 + 3] = s1 * j[0][rr] - (pose[rr * 4] * X[0][0] + pose[rr * 4 + 1] * X[0][1] + pose[rr * 4 + 2] * X[0][2]);
        }
        // kept: a real root with positive depths and a finite pose (a non-finite result is never kept)
        if (real && v > 0.0 && u > 0.0 && s1 > 0.0 && s2 > 0.0 && s3 > 0.0 && pnp_finite12(pose)) {
#pragma unroll
          for (int c = 0; c < 12; ++c) out[ns * 12 + c] = pose[c];
          ++ns;
        }
      }
    }
  }
  for (int c = ns * 12; c < 48; ++c) out[c] = 0.0;
  if (nsol) nsol[row] = ns;
}

// ---- 3. score: candidate `cand` of problem b is poses[(b P + cand) 12 ..]; with nsol, slot cand & 3 of sample cand >> 2 is valid when it is below nsol.
// An invalid slot and a pose with a non-finite entry score -1.
__global__ __launch_bounds__(256) void pnp_score_kernel(const PnpBatch pb, long long P, const float* __restrict__ p2, const float* __restrict__ p3,
                                                        const double* __restrict__ poses, const int* __restrict__ nsol, int* __restrict__ counts) {
  __shared__ float sx[256], sy[256], sX[256], sY[256], sZ[256];
  __shared__ int part[4][64];
  const int bl = blockIdx.y, b = pb.b0 + bl;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int off = pb.off[bl], M = pnp_m(pb, bl);
  const PnpCam cam = pnp_cam(pb, bl);
  const long long cand = (long long)blockIdx.x * 64 + lane;
  const bool live = cand < P;
  const size_t at = (size_t)b * (size_t)P + (size_t)(live ? cand : 0);
  double pose[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) pose[k] = poses[at * 12 + k];
  bool valid = live && pnp_finite12(pose);
  if (nsol && valid) valid = (int)(cand & 3) < nsol[at >> 2];   // P is a multiple of 4 where nsol is given
  int cnt = 0;
  for (int base = 0; base < M; base += 256) {
    __syncthreads();
    const int i = base + tid;
    if (i < M) {
      const size_t g = (size_t)off + i;
      sx[tid] = p2[g * 2]; sy[tid] = p2[g * 2 + 1];
      sX[tid] = p3[g * 3]; sY[tid] = p3[g * 3 + 1]; sZ[tid] = p3[g * 3 + 2];
    }
    __syncthreads();
    const int lo = wave * 64, hi = min(lo + 64, M - base);
    for (int m = lo; m < hi; ++m)   // every lane reads the same address: a broadcast
      cnt += pnp_inlier(pose, cam, (double)sx[m], (double)sy[m], (double)sX[m], (double)sY[m], (double)sZ[m]) ? 1 : 0;
  }
  part[wave][lane] = cnt;
  __syncthreads();
  if (wave == 0 && live) counts[at] = valid ? part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane] : -1;
}

// ---- 4 - 6: one workgroup per problem
// the inlier mask of `pose` into mask[0 .. M) and its size (every thread returns it)
__device__ __forceinline__ int pnp_mask_pass(const double* pose, const PnpCam& cam, const float* p2, const float* p3, int M, unsigned char* mask, int* ired) {
  const int tid = threadIdx.x;
  int cnt = 0;
  for (int i = tid; i < M; i += PNP_LO_THREADS) {
    const bool in = pnp_inlier(pose, cam, (double)p2[(size_t)i * 2], (double)p2[(size_t)i * 2 + 1], (double)p3[(size_t)i * 3], (double)p3[(size_t)i * 3 + 1],
                               (double)p3[(size_t)i * 3 + 2]);
    mask[i] = in ? 1 : 0;
    cnt += in ? 1 : 0;
  }
  __syncthreads();   // ired may still be read from the pass before
  ired[tid] = cnt;
  __syncthreads();
  for (int s = PNP_LO_THREADS / 2; s > 0; s >>= 1) {
    if (tid < s) ired[tid] += ired[tid + s];
    __syncthreads();
  }
  return ired[0];
}

// thread 0: solve (A + damp I) d = -g by Cholesky from the 27 reduced sums and apply the step; false: failed factorisation or non-finite step / pose
__device__ bool pnp_gn_solve(const double* sums, const double* pose, double* out) {
  double L[6][6], g[6], d[6];
  int k = 0;
  for (int i = 0; i < 6; ++i)
    for (int jj = i; jj < 6; ++jj) L[jj][i] = sums[k++];   // the lower triangle holds A until the factor overwrites it
  for (int i = 0; i < 6; ++i) { g[i] = sums[21 + i]; L[i][i] += PNP_DAMP; }
  for (int jj = 0; jj < 6; ++jj) {
    double s = L[jj][jj];
    for (int c = 0; c < jj; ++c) s -= L[jj][c] * L[jj][c];
    if (!(s > 0.0)) return false;
    L[jj][jj] = sqrt(s);
    for (int i = jj + 1; i < 6; ++i) {
      double a = L[i][jj];
      for (int c = 0; c < jj; ++c) a -= L[i][c] * L[jj][c];
      L[i][jj] = a / L[jj][jj];
    }
  }
  for (int i = 0; i < 6; ++i) {
    double a = -g[i];
    for (int c = 0; c < i; ++c) a -= L[i][c] * d[c];
    d[i] = a / L[i][i];
  }
  for (int i = 5; i >= 0; --i) {
    double a = d[i];
    for (int c = i + 1; c < 6; ++c) a -= L[c][i] * d[c];
    d[i] = a / L[i][i];
  }
  bool ok = true;
  for (int i = 0; i < 6; ++i) ok = ok && isfinite(d[i]);
  if (!ok) return false;
  // R <- exp(w) R (Rodrigues), t <- t + delta
  const double wx = d[0], wy = d[1], wz = d[2];
  const double th2 = wx * wx + wy * wy + wz * wz;
  double A = 1.0, B = 0.5;
  if (!(th2 < 1e-16)) { const double th = sqrt(th2); A = sin(th) / th; B = (1.0 - cos(th)) / th2; }
  const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double E[3][3];
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) E[r][c] = (r == c ? 1.0 : 0.0) + A * K[r][c] + B * (K[r][0] * K[0][c] + K[r][1] * K[1][c] + K[r][2] * K[2][c]);
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) out[r * 4 + c] = E[r][0] * pose[c] + E[r][1] * pose[4 + c] + E[r][2] * pose[8 + c];
    out[r * 4 + 3] = pose[r * 4 + 3] + d[3 + r];
  }
  for (int i = 0; i < 12; ++i) ok = ok && isfinite(out[i]);
  return ok;
}

// counts != null: selection over the P candidates of each problem, poses = the candidates (B, P, 12); counts == null: poses = one starting pose per problem (B, 12)
__global__ __launch_bounds__(PNP_LO_THREADS) void pnp_lo_kernel(const PnpBatch pb, long long P, int min_inliers, const float* __restrict__ p2g,
                                                                const float* __restrict__ p3g, const double* __restrict__ poses, const int* __restrict__ counts,
                                                                double* __restrict__ pose_out, unsigned char* __restrict__ maskg, int* __restrict__ info) {
  __shared__ double red[27][PNP_LO_THREADS];
  __shared__ double spose[12];
  __shared__ int ired[PNP_LO_THREADS], iidx[PNP_LO_THREADS];
  __shared__ int sflag;
  const int bl = blockIdx.x, b = pb.b0 + bl, tid = threadIdx.x;
  const int off = pb.off[bl], M = pnp_m(pb, bl);
  const PnpCam cam = pnp_cam(pb, bl);
  const float* p2 = p2g + (size_t)off * 2;
  const float* p3 = p3g + (size_t)off * 3;
  unsigned char* mask = maskg + off;
  // ---- 4. the highest count, among equals the lowest candidate index: per thread in ascending order, then a fixed tree
  int best = -1, best_count = -1;
  if (counts) {
    int bc = INT_MIN, bi = INT_MAX;
    for (long long i = tid; i < P; i += PNP_LO_THREADS) {
      const int c = counts[(size_t)b * (size_t)P + (size_t)i];
      if (c > bc) { bc = c; bi = (int)i; }
    }
    ired[tid] = bc; iidx[tid] = bi;
    __syncthreads();
    for (int s = PNP_LO_THREADS / 2; s > 0; s >>= 1) {
      if (tid < s) {
        const int c = ired[tid + s], i = iidx[tid + s];
        if (c > ired[tid] || (c == ired[tid] && i < iidx[tid])) { ired[tid] = c; iidx[tid] = i; }
      }
      __syncthreads();
    }
    best = iidx[0]; best_count = ired[0];
    __syncthreads();
  }
  double pose[12];
  const double* src = poses + (counts ? ((size_t)b * (size_t)P + (size_t)(best >= 0 ? best : 0)) * 12 : (size_t)b * 12);
#pragma unroll
  for (int k = 0; k < 12; ++k) pose[k] = src[k];
  const bool start_ok = M >= 4 && (!counts || best_count >= 0) && pnp_finite12(pose);
  int n_in = 0;
  if (!start_ok) {   // no usable start: the identity, an empty mask
#pragma unroll
    for (int k = 0; k < 12; ++k) pose[k] = (k == 0 || k == 5 || k == 10) ? 1.0 : 0.0;
    for (int i = tid; i < M; i += PNP_LO_THREADS) mask[i] = 0;
  } else {
    // ---- 5. local optimisation (the control flow is uniform: every decision is a value all threads hold)
    bool stop = false;
    for (int round = 0; round < NL_PNP_LO_ROUNDS && !stop; ++round) {
      if (pnp_mask_pass(pose, cam, p2, p3, M, mask, ired) < 4) break;
      for (int it = 0; it < NL_PNP_GN_ITERS; ++it) {
        double acc[27];
#pragma unroll
        for (int k = 0; k < 27; ++k) acc[k] = 0.0;
        for (int i = tid; i < M; i += PNP_LO_THREADS) {
          if (!mask[i]) continue;   // this thread wrote mask[i] itself
          const double X = (double)p3[(size_t)i * 3], Y = (double)p3[(size_t)i * 3 + 1], Z = (double)p3[(size_t)i * 3 + 2];
          const double yx = pose[0] * X + pose[1] * Y + pose[2] * Z, yy = pose[4] * X + pose[5] * Y + pose[6] * Z, yz = pose[8] * X + pose[9] * Y + pose[10] * Z;
          const double xc = yx + pose[3], yc = yy + pose[7], zc = yz + pose[11];
          const double ru = cam.fx * (xc / zc) + cam.cx - (double)p2[(size_t)i * 2];
          const double rv = cam.fy * (yc / zc) + cam.cy - (double)p2[(size_t)i * 2 + 1];
          const double ja = cam.fx / zc, jb = -cam.fx * xc / (zc * zc);
          const double jc = cam.fy / zc, jd = -cam.fy * yc / (zc * zc);
          const double Ju[6] = {jb * yy, ja * yz - jb * yx, -ja * yy, ja, 0.0, jb};
          const double Jv[6] = {jd * yy - jc * yz, -jd * yx, jc * yx, 0.0, jc, jd};
          int k = 0;
#pragma unroll
          for (int r = 0; r < 6; ++r)
#pragma unroll
            for (int c = r; c < 6; ++c) { acc[k] += Ju[r] * Ju[c] + Jv[r] * Jv[c]; ++k; }
#pragma unroll
          for (int r = 0; r < 6; ++r) acc[21 + r] += Ju[r] * ru + Jv[r] * rv;
        }
#pragma unroll
        for (int k = 0; k < 27; ++k) red[k][tid] = acc[k];
        __syncthreads();
        for (int s = PNP_LO_THREADS / 2; s > 0; s >>= 1) {
          if (tid < s) {
#pragma unroll
            for (int k = 0; k < 27; ++k) red[k][tid] += red[k][tid + s];
          }
          __syncthreads();
        }
        if (tid == 0) {
          double sums[27], next[12];
          for (int k = 0; k < 27; ++k) sums[k] = red[k][0];
          const bool ok = pnp_gn_solve(sums, pose, next);
          sflag = ok ? 1 : 0;
          if (ok)
            for (int k = 0; k < 12; ++k) spose[k] = next[k];
        }
        __syncthreads();
        const bool ok = sflag != 0;
        if (ok) {
#pragma unroll
          for (int k = 0; k < 12; ++k) pose[k] = spose[k];
        }
        __syncthreads();   // spose / sflag / red are rewritten by the next iteration
        if (!ok) { stop = true; break; }   // the last finite pose is kept
      }
    }
    // ---- 6. the mask of the final pose
    n_in = pnp_mask_pass(pose, cam, p2, p3, M, mask, ired);
  }
  for (int i = M + tid; i < pb.off[bl + 1] - off; i += PNP_LO_THREADS) mask[i] = 0;   // a device count below the capacity: the bytes at and beyond it (none otherwise)
  if (tid == 0) {
#pragma unroll
    for (int k = 0; k < 12; ++k) pose_out[(size_t)b * 12 + k] = pose[k];
    info[(size_t)b * 4] = (start_ok && n_in >= min_inliers) ? 1 : 0;
    info[(size_t)b * 4 + 1] = n_in;
    info[(size_t)b * 4 + 2] = best;
    info[(size_t)b * 4 + 3] = best_count;
  }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------------------------------------
bool pnp_pos(double v) { return std::isfinite(v) && v > 0.0; }
bool pnp_h_ok(int H) { return H >= 64 && H <= 65536 && H % 64 == 0; }
// the per-problem host arrays of a call with B > 0: NL_ERR_BAD_ARG (a null array, offsets that do not start at 0 or decrease, intrinsics / thresholds that are not
// finite and positive) before NL_ERR_UNSUPPORTED (a problem above 2^20 matches); thr == null: no thresholds in this call
int pnp_check_problems(const int32_t* offsets, const double* intr, const double* thr, int64_t B) {
  if (!offsets || !intr) return NL_ERR_BAD_ARG;
  if (offsets[0] != 0) return NL_ERR_BAD_ARG;
  for (int64_t b = 0; b < B; ++b) {
    if (offsets[b + 1] < offsets[b]) return NL_ERR_BAD_ARG;
    if (!pnp_pos(intr[b * 4]) || !pnp_pos(intr[b * 4 + 1]) || !std::isfinite(intr[b * 4 + 2]) || !std::isfinite(intr[b * 4 + 3])) return NL_ERR_BAD_ARG;
    if (thr && !pnp_pos(thr[b])) return NL_ERR_BAD_ARG;
  }
  for (int64_t b = 0; b < B; ++b)
    if (offsets[b + 1] - offsets[b] > PNP_MAX_M) return NL_ERR_UNSUPPORTED;
  return NL_OK;
}
PnpBatch pnp_batch(const int32_t* offsets, const double* intr, const double* thr, int64_t b0, int n, const int32_t* cnt_dev = nullptr) {
  PnpBatch pb = {};
  pb.n = n; pb.b0 = (int)b0; pb.cnt = cnt_dev;
  for (int i = 0; i <= n; ++i) pb.off[i] = offsets[b0 + i];
  for (int i = 0; i < n && intr; ++i) {   // intr == null: a launch that computes the indices alone
    const double* k = intr + (b0 + i) * 4;
    pb.fx[i] = k[0]; pb.fy[i] = k[1]; pb.cx[i] = k[2]; pb.cy[i] = k[3];
    pb.thr2[i] = thr ? thr[b0 + i] * thr[b0 + i] : 0.0;
  }
  return pb;
}
constexpr int64_t PNP_MAX_B = 1 << 20;
struct PnpWs { double* poses; int* nsol; int* counts; size_t total; };
PnpWs pnp_carve(void* ws, int64_t B, int H) {
  char* base = (char*)ws;
  PnpWs w;
  size_t o = 0;
  w.poses = (double*)(base + o); o += nl_align_up((size_t)B * H * 48 * sizeof(double), 256);
  w.nsol = (int*)(base + o); o += nl_align_up((size_t)B * H * sizeof(int), 256);
  w.counts = (int*)(base + o); o += nl_align_up((size_t)B * H * 4 * sizeof(int), 256);
  w.total = o;
  return w;
}

}  // namespace
