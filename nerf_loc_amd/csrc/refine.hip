// libnerfloc_refine.so (include/nerfloc_refine.h states the contracts; tests/refine_ref.py restates them in numpy): pose refinement around the renderer's
// forward / backward pair.
//   nlr_se3_exp / _backward / _log   one thread per matrix
//   nlr_init            init_kernel         one thread per pose: params = log(pose), the rest of the record zero, pose0 as given
//   nlr_pose_rays       pose_rays_kernel    one workgroup per 256 pixels: the B matrices once in LDS, then every pixel for every pose
//   nlr_sample_target   sample_kernel       one thread per (pixel, channel)
//   nlr_loss            loss_kernel<VEC>    one wave per ray row, 16-byte loads where the rows allow
//   nlr_step            step_kernel         one workgroup per pose: loss, latch, the twelve cotangents of [R | t], exp backward, Adam
//   nlr_finish          finish_kernel       one thread per pose
// fp64 from the loaded inputs on (-ffp-contract=off: no fused multiply-add, so the numpy restatement sees the same roundings up to the device library's
// sin / cos / acos / pow); no atomics, no kernel that waits on another workgroup, every reduction in a fixed order.
#include "common.h"
#include "../../include/nerfloc_refine.h"

namespace {

constexpr int TPB = 256;
constexpr int SD = NLR_STATE_DOUBLES;
constexpr int S_P = 0, S_M = 6, S_V = 12, S_G = 18, S_LI = 24, S_LL = 25, S_POSE0 = 26, S_T = 42, S_NAN = 43;
constexpr double SE3_EPS = 1e-4, COS_BOUND = 1e-4;
constexpr int64_t MAX_MATS = 1 << 20;

struct Coef { double th, f1, f2, a, b; double K[3][3], K2[3][3]; };

__device__ void hat2(const double* w, double K[3][3], double K2[3][3]) {
  K[0][0] = 0.0; K[0][1] = -w[2]; K[0][2] = w[1];
  K[1][0] = w[2]; K[1][1] = 0.0; K[1][2] = -w[0];
  K[2][0] = -w[1]; K[2][1] = w[0]; K[2][2] = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) K2[i][j] = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
}

__device__ void coef_of(const double* w, Coef& c) {
  const double n = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  c.th = sqrt(n < SE3_EPS ? SE3_EPS : n);
  const double inv = 1.0 / c.th, s = sin(c.th), co = cos(c.th);
  c.f1 = inv * s;
  c.f2 = inv * inv * (1.0 - co);
  c.a = (1.0 - co) / (c.th * c.th);
  c.b = (c.th - s) / (c.th * c.th * c.th);
  hat2(w, c.K, c.K2);
}

// T (row-major 4 x 4) = exp(p)
__device__ void se3_exp(const double* p, double* T) {
  Coef c;
  coef_of(p + 3, c);
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) T[i * 4 + j] = ((i == j ? 1.0 : 0.0) - c.f1 * c.K[i][j]) + c.f2 * c.K2[i][j];
    double t = 0.0;
    for (int j = 0; j < 3; ++j) t += (((i == j ? 1.0 : 0.0) + c.a * c.K[i][j]) + c.b * c.K2[i][j]) * p[j];
    T[i * 4 + 3] = t;
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}

// g (6) = d sum(G * exp(p)) / d p;  G row-major 4 x 4, its bottom row is not read
__device__ void se3_exp_backward(const double* p, const double* G, double* g) {
  Coef c;
  const double* w = p + 3;
  coef_of(w, c);
  double GR[3][3], gt[3];
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j) GR[i][j] = G[i * 4 + j];
    gt[i] = G[i * 4 + 3];
  }
  // u: t = V u, V = I + a K + b K2 -> g_u = V^T g_t
  for (int j = 0; j < 3; ++j) {
    double s = 0.0;
    for (int i = 0; i < 3; ++i) s += (((i == j ? 1.0 : 0.0) + c.a * c.K[i][j]) + c.b * c.K2[i][j]) * gt[i];
    g[j] = s;
  }
  // the four scalars
  double g_f1 = 0.0, g_f2 = 0.0, g_a = 0.0, g_b = 0.0;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      g_f1 -= GR[i][j] * c.K[i][j];
      g_f2 += GR[i][j] * c.K2[i][j];
      g_a += gt[i] * c.K[i][j] * p[j];
      g_b += gt[i] * c.K2[i][j] * p[j];
    }
  // the two matrices: GK2 first, then K2 = K K carries it to K
  double GK2[3][3], GK[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      GK2[i][j] = c.f2 * GR[i][j] + c.b * (gt[i] * p[j]);
      GK[i][j] = c.a * (gt[i] * p[j]) - c.f1 * GR[i][j];
    }
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      double s = 0.0;
      for (int k = 0; k < 3; ++k) s += GK2[i][k] * c.K[j][k] + c.K[k][i] * GK2[k][j];   // GK2 K^T + K^T GK2
      GK[i][j] += s;
    }
  double gw[3] = {GK[2][1] - GK[1][2], GK[0][2] - GK[2][0], GK[1][0] - GK[0][1]};
  // the angle: zero gradient below the clamp
  const double n = w[0] * w[0] + w[1] * w[1] + w[2] * w[2];
  if (n >= SE3_EPS) {
    const double th = c.th, s = sin(th), co = cos(th), th2 = th * th, th3 = th2 * th, th4 = th2 * th2;
    const double d_f1 = co / th - s / th2;
    const double d_f2 = s / th2 - 2.0 * (1.0 - co) / th3;
    const double d_b = (1.0 - co) / th3 - 3.0 * (th - s) / th4;
    const double g_th = g_f1 * d_f1 + (g_f2 + g_a) * d_f2 + g_b * d_b;
    const double g_n = g_th / (2.0 * th);
    for (int k = 0; k < 3; ++k) gw[k] += 2.0 * w[k] * g_n;
  }
  g[3] = gw[0]; g[4] = gw[1]; g[5] = gw[2];
}

// p (6) = log(T);  T row-major 4 x 4 of element type E, its bottom row is not read
template <typename E>
__device__ void se3_log(const E* T, double* p) {
  double R[3][3];   // the transposed top-left block
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i][j] = (double)T[j * 4 + i];
  const double cosphi = ((R[0][0] + R[1][1] + R[2][2]) - 1.0) * 0.5;
  const double bound = 1.0 - COS_BOUND;
  double phi;
  if (cosphi <= -bound) phi = (cosphi - (-bound)) * (-1.0 / sqrt(1.0 - bound * bound)) + acos(-bound);
  else if (cosphi >= bound) phi = (cosphi - bound) * (-1.0 / sqrt(1.0 - bound * bound)) + acos(bound);
  else phi = acos(cosphi);
  const double s = sin(phi);
  const double fac = fabs(s) > 0.5 * SE3_EPS ? phi / (2.0 * s) : 0.5 + phi * phi * (1.0 / 12);
  double w[3] = {fac * (R[2][1] - R[1][2]), fac * (R[0][2] - R[2][0]), fac * (R[1][0] - R[0][1])};
  Coef c;
  coef_of(w, c);
  double V[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) V[i][j] = ((i == j ? 1.0 : 0.0) + c.a * c.K[i][j]) + c.b * c.K2[i][j];
  const double t0 = (double)T[3], t1 = (double)T[7], t2 = (double)T[11];
  const double C00 = V[1][1] * V[2][2] - V[1][2] * V[2][1], C01 = V[1][2] * V[2][0] - V[1][0] * V[2][2], C02 = V[1][0] * V[2][1] - V[1][1] * V[2][0];
  const double C10 = V[0][2] * V[2][1] - V[0][1] * V[2][2], C11 = V[0][0] * V[2][2] - V[0][2] * V[2][0], C12 = V[0][1] * V[2][0] - V[0][0] * V[2][1];
  const double C20 = V[0][1] * V[1][2] - V[0][2] * V[1][1], C21 = V[0][2] * V[1][0] - V[0][0] * V[1][2], C22 = V[0][0] * V[1][1] - V[0][1] * V[1][0];
  const double det = V[0][0] * C00 + V[0][1] * C01 + V[0][2] * C02;
  p[0] = (C00 * t0 + C10 * t1 + C20 * t2) / det;   // the adjugate is the transposed cofactor matrix
  p[1] = (C01 * t0 + C11 * t1 + C21 * t2) / det;
  p[2] = (C02 * t0 + C12 * t1 + C22 * t2) / det;
  p[3] = w[0]; p[4] = w[1]; p[5] = w[2];
}

__global__ __launch_bounds__(TPB) void exp_kernel(const double* __restrict__ p, long long N, double* __restrict__ T) {
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= N) return;
  double pp[6], t[16];
  for (int k = 0; k < 6; ++k) pp[k] = p[i * 6 + k];
  se3_exp(pp, t);
  for (int k = 0; k < 16; ++k) T[i * 16 + k] = t[k];
}

__global__ __launch_bounds__(TPB) void exp_backward_kernel(const double* __restrict__ p, const double* __restrict__ G, long long N, double* __restrict__ g) {
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= N) return;
  double pp[6], gg[16], out[6];
  for (int k = 0; k < 6; ++k) pp[k] = p[i * 6 + k];
  for (int k = 0; k < 16; ++k) gg[k] = G[i * 16 + k];
  se3_exp_backward(pp, gg, out);
  for (int k = 0; k < 6; ++k) g[i * 6 + k] = out[k];
}

__global__ __launch_bounds__(TPB) void log_kernel(const double* __restrict__ T, long long N, double* __restrict__ p) {
  const long long i = (long long)blockIdx.x * TPB + threadIdx.x;
  if (i >= N) return;
  double t[16], pp[6];
  for (int k = 0; k < 16; ++k) t[k] = T[i * 16 + k];
  se3_log(t, pp);
  for (int k = 0; k < 6; ++k) p[i * 6 + k] = pp[k];
}

__global__ __launch_bounds__(64) void init_kernel(const void* __restrict__ poses, int f64, int B, double* __restrict__ state) {
  const int b = threadIdx.x;
  if (b >= B) return;
  double* s = state + (size_t)b * SD;
  double t[16], pp[6];
  for (int k = 0; k < 16; ++k) t[k] = f64 ? ((const double*)poses)[(size_t)b * 16 + k] : (double)((const float*)poses)[(size_t)b * 16 + k];
  se3_log(t, pp);
  for (int k = 0; k < 6; ++k) s[S_P + k] = pp[k];
  for (int k = S_M; k < S_POSE0; ++k) s[k] = 0.0;
  for (int k = 0; k < 16; ++k) s[S_POSE0 + k] = t[k];
  ((long long*)s)[S_T] = 0;
  ((long long*)s)[S_NAN] = 0;
}

// cam = ((x - cx) / fx, (y - cy) / fy, 1) of a pixel, its coordinates truncated towards zero
__device__ __forceinline__ void pixel_cam(const float* __restrict__ K, const float* __restrict__ uv, int i, double cam[3]) {
  const double x = (double)(int)uv[(size_t)i * 2], y = (double)(int)uv[(size_t)i * 2 + 1];
  cam[0] = (x - (double)K[2]) / (double)K[0];
  cam[1] = (y - (double)K[5]) / (double)K[4];
  cam[2] = 1.0;
}

__global__ __launch_bounds__(TPB) void pose_rays_kernel(const double* __restrict__ state, const float* __restrict__ K, const float* __restrict__ uv, int B, int Rp,
                                                        float* __restrict__ pose32, float* __restrict__ rays_o, float* __restrict__ rays_d,
                                                        float* __restrict__ centres) {
  __shared__ double T[NLR_MAX_POSES][16];
  if ((int)threadIdx.x < B) {
    double pp[6];
    for (int k = 0; k < 6; ++k) pp[k] = state[(size_t)threadIdx.x * SD + S_P + k];
    se3_exp(pp, T[threadIdx.x]);
    if (blockIdx.x == 0 && pose32)
      for (int k = 0; k < 16; ++k) pose32[(size_t)threadIdx.x * 16 + k] = (float)T[threadIdx.x][k];
  }
  __syncthreads();
  const int i = blockIdx.x * TPB + threadIdx.x;
  if (i >= Rp) return;
  double cam[3];
  pixel_cam(K, uv, i, cam);
  for (int b = 0; b < B; ++b) {
    const double* t = T[b];
    double v[3];
    for (int k = 0; k < 3; ++k) v[k] = cam[0] * t[k * 4] + cam[1] * t[k * 4 + 1] + cam[2] * t[k * 4 + 2];
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const size_t r = ((size_t)b * Rp + i) * 3;
    for (int k = 0; k < 3; ++k) {
      const float c = (float)t[k * 4 + 3];
      rays_d[r + k] = (float)(v[k] / len);
      rays_o[r + k] = c;
      centres[r + k] = c;
    }
  }
}

// the two neighbours and weights of one axis: src = (x + 0.5)(n_in / n_out) - 0.5, negative -> 0
__device__ __forceinline__ void axis_taps(int x, int n_in, int n_out, int& i0, int& i1, double& l0, double& l1) {
  double src = ((double)x + 0.5) * ((double)n_in / (double)n_out) - 0.5;
  if (src < 0.0) src = 0.0;
  i0 = (int)src;
  if (i0 > n_in - 1) i0 = n_in - 1;
  i1 = i0 + 1 < n_in - 1 ? i0 + 1 : n_in - 1;
  l1 = src - (double)i0;
  l0 = 1.0 - l1;
}

__global__ __launch_bounds__(TPB) void sample_kernel(const float* __restrict__ map, int nhwc, int C, int h, int w, int H, int W, const float* __restrict__ uv,
                                                     long long total, float* __restrict__ out) {
  const long long g = (long long)blockIdx.x * TPB + threadIdx.x;
  if (g >= total) return;
  const int i = (int)(g / C), c = (int)(g - (long long)i * C);
  int x = (int)uv[(size_t)i * 2], y = (int)uv[(size_t)i * 2 + 1];
  x = x < 0 ? 0 : (x > W - 1 ? W - 1 : x);
  y = y < 0 ? 0 : (y > H - 1 ? H - 1 : y);
  int x0, x1, y0, y1;
  double lx0, lx1, ly0, ly1;
  axis_taps(x, w, W, x0, x1, lx0, lx1);
  axis_taps(y, h, H, y0, y1, ly0, ly1);
  const size_t sy = nhwc ? (size_t)w * C : (size_t)w, sx = nhwc ? (size_t)C : 1, base = nhwc ? (size_t)c : (size_t)c * h * w;
  const double m00 = (double)map[base + y0 * sy + x0 * sx], m01 = (double)map[base + y0 * sy + x1 * sx];
  const double m10 = (double)map[base + y1 * sy + x0 * sx], m11 = (double)map[base + y1 * sy + x1 * sx];
  out[g] = (float)(ly0 * (lx0 * m00 + lx1 * m01) + ly1 * (lx0 * m10 + lx1 * m11));
}

// the sum of `v` over the 64 lanes by a fixed butterfly (every lane ends with the same bits)
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int VEC>
__global__ __launch_bounds__(TPB) void loss_kernel(const float* __restrict__ out, const unsigned char* __restrict__ mask, const float* __restrict__ target, int R, int Rp,
                                                   int C, float* __restrict__ g_out, double* __restrict__ row_loss) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * (TPB / 64) + (threadIdx.x >> 6);   // wave-uniform
  if (r >= R) return;
  const double m = (double)mask[r];
  const double scale = (double)Rp * (double)C;
  const float* o = out + (size_t)r * C;
  const float* t = target + (size_t)(r % Rp) * C;
  float* g = g_out + (size_t)r * C;
  double acc = 0.0;
  if (VEC == 4) {
    for (int c = lane * 4; c < C; c += 256) {   // C % 4 == 0: a vector never crosses the row's end
      const float4 ov = *reinterpret_cast<const float4*>(o + c), tv = *reinterpret_cast<const float4*>(t + c);
      const double e0 = ((double)ov.x - (double)tv.x) * m, e1 = ((double)ov.y - (double)tv.y) * m;
      const double e2 = ((double)ov.z - (double)tv.z) * m, e3 = ((double)ov.w - (double)tv.w) * m;
      acc += e0 * e0; acc += e1 * e1; acc += e2 * e2; acc += e3 * e3;
      *reinterpret_cast<float4*>(g + c) = make_float4((float)(2.0 * m * e0 / scale), (float)(2.0 * m * e1 / scale), (float)(2.0 * m * e2 / scale),
                                                      (float)(2.0 * m * e3 / scale));
    }
  } else {
    for (int c = lane; c < C; c += 64) {
      const double e = ((double)o[c] - (double)t[c]) * m;
      acc += e * e;
      g[c] = (float)(2.0 * m * e / scale);
    }
  }
  acc = wave_sum_d(acc);
  if (lane == 0) row_loss[r] = acc;
}

__global__ __launch_bounds__(TPB) void step_kernel(double* __restrict__ state, const double* __restrict__ row_loss, const float* __restrict__ g_o,
                                                   const float* __restrict__ g_d, const float* __restrict__ g_c, const float* __restrict__ K,
                                                   const float* __restrict__ uv, int Rp, int C, double lr, double beta1, double beta2, double eps) {
  __shared__ double T[16];
  __shared__ double part[TPB][12];
  __shared__ double G[16];
  __shared__ int stop;
  const int b = blockIdx.x, q = threadIdx.x;
  double* s = state + (size_t)b * SD;
  long long* si = (long long*)s;
  if (q == 0) {
    int st = si[S_NAN] != 0 ? 1 : 0;
    if (!st) {
      double sum = 0.0;
      for (int i = 0; i < Rp; ++i) sum += row_loss[(size_t)b * Rp + i];
      const double loss = sum / ((double)Rp * (double)C);
      if (si[S_T] == 0) s[S_LI] = loss;
      s[S_LL] = loss;
      if (loss != loss) { si[S_NAN] = 1; st = 1; }
    }
    stop = st;
    if (!st) {
      double pp[6];
      for (int k = 0; k < 6; ++k) pp[k] = s[S_P + k];
      se3_exp(pp, T);
    }
  }
  __syncthreads();
  if (stop) return;   // block-uniform
  double acc[12];
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  for (int i = q; i < Rp; i += TPB) {
    double cam[3], v[3], gd[3];
    pixel_cam(K, uv, i, cam);
    const size_t r = ((size_t)b * Rp + i) * 3;
    for (int k = 0; k < 3; ++k) {
      v[k] = cam[0] * T[k * 4] + cam[1] * T[k * 4 + 1] + cam[2] * T[k * 4 + 2];
      gd[k] = (double)g_d[r + k];
    }
    const double len = sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    const double d0 = v[0] / len, d1 = v[1] / len, d2 = v[2] / len;
    const double dot = d0 * gd[0] + d1 * gd[1] + d2 * gd[2];
    const double gv[3] = {(gd[0] - d0 * dot) / len, (gd[1] - d1 * dot) / len, (gd[2] - d2 * dot) / len};
    for (int k = 0; k < 3; ++k) {
      for (int j = 0; j < 3; ++j) acc[k * 4 + j] += gv[k] * cam[j];
      acc[k * 4 + 3] += (double)g_o[r + k] + (double)g_c[r + k];
    }
  }
  for (int k = 0; k < 12; ++k) part[q][k] = acc[k];
  __syncthreads();
  if (q < 12) {
    double sum = 0.0;
    for (int i = 0; i < TPB; ++i) sum += part[i][q];
    G[q] = sum;
  }
  if (q >= 12 && q < 16) G[q] = 0.0;
  __syncthreads();
  if (q == 0) {
    double pp[6], gg[16], g[6];
    for (int k = 0; k < 6; ++k) pp[k] = s[S_P + k];
    for (int k = 0; k < 16; ++k) gg[k] = G[k];
    se3_exp_backward(pp, gg, g);
    const long long t = si[S_T] + 1;
    si[S_T] = t;
    const double bc1 = 1.0 - pow(beta1, (double)t), bc2 = 1.0 - pow(beta2, (double)t);
    const double step_size = lr / bc1, bc2_sqrt = sqrt(bc2);
    for (int k = 0; k < 6; ++k) {
      const double m = s[S_M + k] + (g[k] - s[S_M + k]) * (1.0 - beta1);
      const double v = s[S_V + k] * beta2 + (1.0 - beta2) * g[k] * g[k];
      const double denom = sqrt(v) / bc2_sqrt + eps;
      s[S_M + k] = m; s[S_V + k] = v; s[S_G + k] = g[k];
      s[S_P + k] = pp[k] + (-step_size) * (m / denom);
    }
  }
}

__global__ __launch_bounds__(64) void finish_kernel(const double* __restrict__ state, int B, double* __restrict__ T64, float* __restrict__ T32, double* __restrict__ info) {
  const int b = threadIdx.x;
  if (b >= B) return;
  const double* s = state + (size_t)b * SD;
  const long long latch = ((const long long*)s)[S_NAN];
  const bool accepted = !(latch != 0 || s[S_LL] > s[S_LI]);
  double t[16];
  if (accepted) {
    double pp[6];
    for (int k = 0; k < 6; ++k) pp[k] = s[S_P + k];
    se3_exp(pp, t);
  } else {
    for (int k = 0; k < 16; ++k) t[k] = s[S_POSE0 + k];
  }
  for (int k = 0; k < 16; ++k) {
    if (T64) T64[(size_t)b * 16 + k] = t[k];
    if (T32) T32[(size_t)b * 16 + k] = (float)t[k];
  }
  info[b * 4] = s[S_LI]; info[b * 4 + 1] = s[S_LL]; info[b * 4 + 2] = accepted ? 1.0 : 0.0; info[b * 4 + 3] = latch != 0 ? 1.0 : 0.0;
}

bool misaligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) != 0; }

// NL_OK with `go` false: nothing to do
int batch_args(int B, int Rp, bool& go) {
  go = false;
  if (B < 0 || Rp < 0) return NL_ERR_BAD_ARG;
  if (B > NLR_MAX_POSES || Rp > NLR_MAX_RAYS) return NL_ERR_UNSUPPORTED;
  go = B > 0 && Rp > 0;
  return NL_OK;
}

}  // namespace

extern "C" {

int nlr_abi_version(void) { return NLR_ABI_VERSION; }

int nlr_se3_exp(const double* p, int64_t N, double* T, void* stream) {
  if (N < 0) return NL_ERR_BAD_ARG;
  if (N > MAX_MATS) return NL_ERR_UNSUPPORTED;
  if (N == 0) return NL_OK;
  if (!p || !T || misaligned(p, 8) || misaligned(T, 8)) return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(exp_kernel, dim3((unsigned)nl_cdiv(N, TPB)), dim3(TPB), 0, (hipStream_t)stream, p, (long long)N, T);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlr_se3_exp_backward(const double* p, const double* G, int64_t N, double* g_p, void* stream) {
  if (N < 0) return NL_ERR_BAD_ARG;
  if (N > MAX_MATS) return NL_ERR_UNSUPPORTED;
  if (N == 0) return NL_OK;
  if (!p || !G || !g_p || misaligned(p, 8) || misaligned(G, 8) || misaligned(g_p, 8)) return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(exp_backward_kernel, dim3((unsigned)nl_cdiv(N, TPB)), dim3(TPB), 0, (hipStream_t)stream, p, G, (long long)N, g_p);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlr_se3_log(const double* T, int64_t N, double* p, void* stream) {
  if (N < 0) return NL_ERR_BAD_ARG;
  if (N > MAX_MATS) return NL_ERR_UNSUPPORTED;
  if (N == 0) return NL_OK;
  if (!T || !p || misaligned(T, 8) || misaligned(p, 8)) return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(log_kernel, dim3((unsigned)nl_cdiv(N, TPB)), dim3(TPB), 0, (hipStream_t)stream, T, (long long)N, p);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

size_t nlr_state_bytes(int B) { return B < 1 || B > NLR_MAX_POSES ? 0 : (size_t)B * SD * sizeof(double); }

int nlr_init(const void* poses, unsigned pose_flags, int B, void* state, void* stream) {
  if (B < 0 || (pose_flags & ~NLR_POSE_F64)) return NL_ERR_BAD_ARG;
  if (B > NLR_MAX_POSES) return NL_ERR_UNSUPPORTED;
  if (B == 0) return NL_OK;
  const bool f64 = (pose_flags & NLR_POSE_F64) != 0;
  if (!poses || !state || misaligned(poses, f64 ? 8 : 4) || misaligned(state, 8)) return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, poses, (int)f64, B, (double*)state);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlr_pose_rays(const void* state, const float* K, const float* uv, int B, int Rp, float* pose32_out, float* rays_o, float* rays_d, float* centres, void* stream) {
  bool go;
  const int rc = batch_args(B, Rp, go);
  if (rc != NL_OK || !go) return rc;
  if (!state || !K || !uv || !rays_o || !rays_d || !centres) return NL_ERR_BAD_ARG;
  if (misaligned(state, 8) || misaligned(K, 4) || misaligned(uv, 4) || misaligned(pose32_out, 4) || misaligned(rays_o, 4) || misaligned(rays_d, 4) ||
      misaligned(centres, 4))
    return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(pose_rays_kernel, dim3((unsigned)nl_cdiv(Rp, TPB)), dim3(TPB), 0, (hipStream_t)stream, (const double*)state, K, uv, B, Rp, pose32_out, rays_o,
                     rays_d, centres);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlr_sample_target(const float* map, int layout, int C, int h, int w, int H, int W, const float* uv, int Rp, float* out, void* stream) {
  if (Rp < 0 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1 || (layout != NLR_LAYOUT_NCHW && layout != NLR_LAYOUT_NHWC)) return NL_ERR_BAD_ARG;
  if (Rp > NLR_MAX_RAYS || C > NLR_MAX_CHANNELS || h > NLR_MAX_IMAGE || w > NLR_MAX_IMAGE || H > NLR_MAX_IMAGE || W > NLR_MAX_IMAGE) return NL_ERR_UNSUPPORTED;
  if (Rp == 0) return NL_OK;
  if (!map || !uv || !out || misaligned(map, 4) || misaligned(uv, 4) || misaligned(out, 4)) return NL_ERR_BAD_ARG;
  const long long total = (long long)Rp * C;   // <= 2^30
  hipLaunchKernelGGL(sample_kernel, dim3((unsigned)nl_cdiv(total, TPB)), dim3(TPB), 0, (hipStream_t)stream, map, layout == NLR_LAYOUT_NHWC ? 1 : 0, C, h, w, H, W, uv,
                     total, out);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlr_loss(const float* out, const uint8_t* mask, const float* target, int B, int Rp, int C, float* g_out, double* row_loss, void* stream) {
  bool go;
  const int rc = batch_args(B, Rp, go);
  if (rc != NL_OK) return rc;
  if (C < 1) return NL_ERR_BAD_ARG;
  if (C > NLR_MAX_CHANNELS) return NL_ERR_UNSUPPORTED;
  if (!go) return NL_OK;
  if (!out || !mask || !target || !g_out || !row_loss) return NL_ERR_BAD_ARG;
  if (misaligned(out, 4) || misaligned(target, 4) || misaligned(g_out, 4) || misaligned(row_loss, 8)) return NL_ERR_BAD_ARG;
  const int R = B * Rp;   // <= 2^24
  const bool vec = C % 4 == 0 && !misaligned(out, 16) && !misaligned(target, 16) && !misaligned(g_out, 16);
  const dim3 grid((unsigned)nl_cdiv(R, TPB / 64));
  if (vec) hipLaunchKernelGGL(loss_kernel<4>, grid, dim3(TPB), 0, (hipStream_t)stream, out, (const unsigned char*)mask, target, R, Rp, C, g_out, row_loss);
  else hipLaunchKernelGGL(loss_kernel<1>, grid, dim3(TPB), 0, (hipStream_t)stream, out, (const unsigned char*)mask, target, R, Rp, C, g_out, row_loss);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlr_step(void* state, const double* row_loss, const float* g_rays_o, const float* g_rays_d, const float* g_centres, const float* K, const float* uv, int B, int Rp,
             int C, double lr, double beta1, double beta2, double eps, void* stream) {
  bool go;
  const int rc = batch_args(B, Rp, go);
  if (rc != NL_OK) return rc;
  if (C < 1) return NL_ERR_BAD_ARG;
  if (C > NLR_MAX_CHANNELS) return NL_ERR_UNSUPPORTED;
  if (!go) return NL_OK;
  if (!state || !row_loss || !g_rays_o || !g_rays_d || !g_centres || !K || !uv) return NL_ERR_BAD_ARG;
  if (misaligned(state, 8) || misaligned(row_loss, 8) || misaligned(g_rays_o, 4) || misaligned(g_rays_d, 4) || misaligned(g_centres, 4) || misaligned(K, 4) ||
      misaligned(uv, 4))
    return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(step_kernel, dim3(B), dim3(TPB), 0, (hipStream_t)stream, (double*)state, row_loss, g_rays_o, g_rays_d, g_centres, K, uv, Rp, C, lr, beta1, beta2,
                     eps);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlr_finish(const void* state, int B, double* T_c2w64, float* T_c2w32, double* info, void* stream) {
  if (B < 0) return NL_ERR_BAD_ARG;
  if (B > NLR_MAX_POSES) return NL_ERR_UNSUPPORTED;
  if (B == 0) return NL_OK;
  if (!state || !info || misaligned(state, 8) || misaligned(info, 8) || misaligned(T_c2w64, 8) || misaligned(T_c2w32, 4)) return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)state, B, T_c2w64, T_c2w32, info);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // extern "C"
