// libnerfloc_cnn_train.so — DepthFusionNet for training (include/nerfloc_cnn_train.h is the contract; this file is its only unit).
//
// The forward is the inference chain of cnn_kernels.h on a plan that overwrites nothing; its one own kernel, cnt_in_stats_keep_kernel, is cnn_in_stats_kernel
// writing act(IN(x)) next to the raw plane instead of over it (and 1 / sqrt(var + eps) into the norm's fourth word).  The backward's kernels:
//   cnt_in_bwd_kernel          one workgroup per (view, channel) plane: the activation's derivative from the kept output, the two plane sums by the forward's tree,
//                              the cotangent of the raw convolution sums, and (s1, s2) for the gamma / beta gradients.
//   cnt_wgrad_kernel           weight gradient as an implicit GEMM on v_mfma_f32_32x32x2_f32, the pixels as the reduction dimension: a workgroup owns 32 output
//                              channels x 128 k of one (view, pixel range) and writes a partial; cnt_wgrad_reduce_kernel adds the partials in ascending order
//                              into the parameter's own layout.  The gather is the forward's: reflecting, concatenating.
//   cnt_dgrad_kernel           data gradient on the padded input domain, an implicit GEMM too: rows = input channels, columns = padded pixels, k = (tap, out);
//                              g_y is gathered with a zero border and, at stride 2, only where the parity matches.
//   cnt_fold_kernel            folds the padded border back (reflect's transpose), adds the earlier consumers' sum and a ReLU-masked identity cotangent.
//   cnt_up2_bwd_kernel         the bilinear x 2's transpose in gather form.
//   cnt_head_bwd_kernel        one thread per pixel: recomputes the head's hidden values, writes them and the cotangents the 1 x 1 weight gradients read.
//   cnt_chan_sum_kernel        a bias gradient: per-plane tree sums added in ascending view order.
//   cnt_in_params_kernel       every InstanceNorm's g_gamma, g_beta from the planes' (s1, s2), views ascending, and the four exact-zero biases: one launch.
#include <algorithm>

#include "cnn_kernels.h"
#include "../../include/nerfloc_cnn_train.h"

namespace {

// cnn_in_stats_kernel with the activated plane written to y (act != NONE) and the raw plane kept: the same expressions in the same order
__global__ __launch_bounds__(CNN_THREADS) void cnt_in_stats_keep_kernel(const float* __restrict__ x, int n, const float* __restrict__ gamma,
                                                                        const float* __restrict__ beta, int act, float* __restrict__ nrm, float* __restrict__ y) {
  __shared__ float red[CNN_THREADS];
  const int c = blockIdx.x, C = gridDim.x, v = blockIdx.y, tid = threadIdx.x;
  const size_t plane = (size_t)v * C + c;
  const float* p = x + plane * n;
  float s = 0.f;
  for (int i = tid; i < n; i += CNN_THREADS) s += p[i];
  const float mean = cnn_block_sum(s, red) / (float)n;
  float q = 0.f;
  for (int i = tid; i < n; i += CNN_THREADS) {
    const float d = p[i] - mean;
    q += d * d;
  }
  q = cnn_block_sum(q, red);
  const float sd = sqrtf(q / (float)n + CNN_EPS);
  const float k = gamma[c] / sd, bt = beta[c];
  if (tid == 0) ((float4*)nrm)[plane] = make_float4(mean, k, bt, 1.f / sd);
  if (act == CNN_ACT_NONE) return;
  float* o = y + plane * n;
  for (int i = tid; i < n; i += CNN_THREADS) {
    const float t = (p[i] - mean) * k + bt;
    o[i] = act == CNN_ACT_RELU ? cnn_relu(t) : nl_elu(t);
  }
}

__device__ __forceinline__ float cnt_dact(float g, const float* y, size_t at, int act) {
  if (act == CNN_ACT_NONE) return g;
  const float t = y[at];
  if (act == CNN_ACT_RELU) return t > 0.f ? g : 0.f;
  return t > 0.f ? g : g * (t + 1.f);
}

// grid (C, V).  gx may be g (each thread rewrites only what it alone read, after the sums); pp[plane] = (s1, s2)
__global__ __launch_bounds__(CNN_THREADS) void cnt_in_bwd_kernel(const float* __restrict__ x, const float* __restrict__ nrm, const float* __restrict__ y, int act,
                                                                 const float* g, int n, float* gx, float* __restrict__ pp) {
  __shared__ float red[CNN_THREADS];
  const int c = blockIdx.x, C = gridDim.x, v = blockIdx.y, tid = threadIdx.x;
  const size_t plane = (size_t)v * C + c, base = plane * n;
  const float4 nm = ((const float4*)nrm)[plane];
  float s1 = 0.f, s2 = 0.f;
  for (int i = tid; i < n; i += CNN_THREADS) {
    const float gz = cnt_dact(g[base + i], y, base + i, act);
    s1 += gz;
    s2 += gz * ((x[base + i] - nm.x) * nm.w);
  }
  s1 = cnn_block_sum(s1, red);
  s2 = cnn_block_sum(s2, red);
  if (tid == 0) { pp[2 * plane] = s1; pp[2 * plane + 1] = s2; }
  if (!gx) return;
  const float m1 = s1 / (float)n, m2 = s2 / (float)n;
  for (int i = tid; i < n; i += CNN_THREADS) {
    const float gz = cnt_dact(g[base + i], y, base + i, act);
    const float xh = (x[base + i] - nm.x) * nm.w;
    gx[base + i] = nm.y * (gz - m1 - xh * m2);
  }
}

constexpr int CNT_MAX_SITES = 20;
struct CntInSite {
  const float* pp;   // (V, C, 2)
  float *gg, *gb;    // g_gamma, g_beta (C) or null
  int C;
};
struct CntInParamsArgs {
  CntInSite s[CNT_MAX_SITES];
  float* zero[4];
  int zn[4];
  int V;
};
// grid (sites): block j < 4 also writes the j-th zero vector
__global__ __launch_bounds__(CNN_THREADS) void cnt_in_params_kernel(const CntInParamsArgs a) {
  const CntInSite& s = a.s[blockIdx.x];
  for (int c = threadIdx.x; c < s.C; c += CNN_THREADS) {
    float s1 = 0.f, s2 = 0.f;
    for (int v = 0; v < a.V; ++v) {
      s1 += s.pp[2 * ((size_t)v * s.C + c)];
      s2 += s.pp[2 * ((size_t)v * s.C + c) + 1];
    }
    if (s.gb) s.gb[c] = s1;
    if (s.gg) s.gg[c] = s2;
  }
  if (blockIdx.x < 4 && a.zero[blockIdx.x])
    for (int c = threadIdx.x; c < a.zn[blockIdx.x]; c += CNN_THREADS) a.zero[blockIdx.x][c] = 0.f;
}

// grid (C): out[c] = sum over v ascending of the tree sum of plane (v, c) of g (V, C, n)
__global__ __launch_bounds__(CNN_THREADS) void cnt_chan_sum_kernel(const float* __restrict__ g, int V, int n, float* __restrict__ out) {
  __shared__ float red[CNN_THREADS];
  const int c = blockIdx.x, C = gridDim.x, tid = threadIdx.x;
  float tot = 0.f;
  for (int v = 0; v < V; ++v) {
    const float* p = g + ((size_t)v * C + c) * n;
    float s = 0.f;
    for (int i = tid; i < n; i += CNN_THREADS) s += p[i];
    tot += cnn_block_sum(s, red);
  }
  if (tid == 0) out[c] = tot;
}

// ------------------------------------------------------------------------------------------ weight gradient
struct CntSrc {
  const float* x;    // view v, channel c: x + v vstride + c hin win
  int C;
  size_t vstride;
};
struct CntWgradArgs {
  CntSrc s0, s1;
  const float* gy;   // (V, cout, ho, wo)
  float* part;       // [V chunks][cout][K]
  int cout, K, ks, tap_major, cin;
  int hin, win, ho, wo, stride, pad;
  int chunks, CH;
};
constexpr int CNT_WK = 128;   // k per workgroup: 32 per wave

// grid (cdiv(K, 128), cdiv(cout, 32), V chunks)
__global__ __launch_bounds__(CNN_THREADS) void cnt_wgrad_kernel(const CntWgradArgs a) {
  __shared__ float Gs[32][33];            // [pixel][out]
  __shared__ float Ps[32][CNT_WK + 1];    // [pixel][k]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kb = blockIdx.x * CNT_WK, ob = blockIdx.y * 32, split = blockIdx.z, v = split / a.chunks, ch = split - v * a.chunks;
  const int npix = a.ho * a.wo, npl = a.hin * a.win;
  const int pbeg = ch * a.CH, pend = min(npix, pbeg + a.CH);
  const int px = tid & 31, r = tid >> 5;

  // this thread stages k = kb + r + 8 j of every step: (channel of the concat) | ky << 12 | kx << 16 | valid << 20, worked out once
  int kc[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int k = kb + r + 8 * j;
    kc[j] = 0;
    if (k < a.K) {
      int in, t;
      if (a.tap_major) { t = k / a.cin; in = k - t * a.cin; } else { in = k / (a.ks * a.ks); t = k - in * a.ks * a.ks; }
      const int ky = t / a.ks, kx = t - ky * a.ks;
      kc[j] = in | ky << 12 | kx << 16 | 1 << 20;
    }
  }
  const float* gyv = a.gy + (size_t)v * a.cout * npix;
  const float* x0 = a.s0.x + (size_t)v * a.s0.vstride;
  const float* x1 = a.s1.C ? a.s1.x + (size_t)v * a.s1.vstride : nullptr;

  cnn_f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  for (int p0 = pbeg; p0 < pend; p0 += 32) {
    const int P = p0 + px;
    const bool ok = P < pend;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int o = ob + r + 8 * j;
      Gs[px][r + 8 * j] = ok && o < a.cout ? gyv[(size_t)o * npix + P] : 0.f;
    }
    const int oy = ok ? P / a.wo : 0, ox = ok ? P - oy * a.wo : 0;
    const int by = oy * a.stride - a.pad, bx = ox * a.stride - a.pad;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      float val = 0.f;
      if (ok && (kc[j] >> 20)) {
        const int in = kc[j] & 4095, ky = (kc[j] >> 12) & 15, kx = (kc[j] >> 16) & 15;
        const int iy = cnn_reflect(by + ky, a.hin), ix = cnn_reflect(bx + kx, a.win);
        const float* src = in < a.s0.C ? x0 + (size_t)in * npl : x1 + (size_t)(in - a.s0.C) * npl;
        val = src[iy * a.win + ix];
      }
      Ps[px][r + 8 * j] = val;
    }
    __syncthreads();
    if (kb + 32 * wave < a.K) {   // wave-uniform
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        const int kk = 2 * s + (lane >> 5);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Gs[kk][lane & 31], Ps[kk][32 * wave + (lane & 31)], acc, 0, 0, 0);
      }
    }
    __syncthreads();
  }
  // C/D layout: column (k) = lane & 31, row (out) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int k = kb + 32 * wave + (lane & 31);
  if (k < a.K) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int o = ob + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      if (o < a.cout) a.part[((size_t)split * a.cout + o) * a.K + k] = acc[i];
    }
  }
}

// grid (cdiv(cout K, 256)): gw (cout, cin, T) = the partials added in ascending order; tap-major k = t cin + in goes to in T + t
__global__ __launch_bounds__(CNN_THREADS) void cnt_wgrad_reduce_kernel(const float* __restrict__ part, int nsplit, int cout, int K, int cin, int tap_major,
                                                                       float* __restrict__ gw) {
  const int i = blockIdx.x * CNN_THREADS + threadIdx.x;
  if (i >= cout * K) return;
  float s = 0.f;
  for (int sp = 0; sp < nsplit; ++sp) s += part[(size_t)sp * cout * K + i];
  const int o = i / K, k = i - o * K, T = K / cin;
  gw[tap_major ? (size_t)o * K + (size_t)(k % cin) * T + k / cin : (size_t)i] = s;
}

// ------------------------------------------------------------------------------------------ data gradient
struct CntDgradArgs {
  const float* gy;   // (V, cout, ho, wo)
  const float* wt;   // [(ky ks + kx) cout + out][cin]
  float* gp;         // (V, cin, hp, wp): the padded domain
  int cin, cout, ks, stride;
  int ho, wo, hp, wp;
};

// grid (cdiv(hp wp, 128), V, cin / 32): wave w owns padded pixels 32 w .. of the tile, all 32 input channels of blockIdx.z
__global__ __launch_bounds__(CNN_THREADS) void cnt_dgrad_kernel(const CntDgradArgs a) {
  __shared__ float Gs[CNN_BK][CNN_XS];
  __shared__ __attribute__((aligned(16))) float Ws[CNN_BK][32];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v = blockIdx.y, c0 = blockIdx.z * 32;
  const int npp = a.hp * a.wp, npo = a.ho * a.wo, K = a.ks * a.ks * a.cout;
  const int p = tid & (CNN_TP - 1), kq = tid >> 7;
  const int P = blockIdx.x * CNN_TP + p;
  const bool pix_ok = P < npp;
  const int py = pix_ok ? P / a.wp : 0, pxx = pix_ok ? P - py * a.wp : 0;
  const float* gyv = a.gy + (size_t)v * a.cout * npo;

  cnn_f32x16 acc;
#pragma unroll
  for (int i = 0; i < 16; ++i) acc[i] = 0.f;

  for (int k0 = 0; k0 < K; k0 += CNN_BK) {   // one tap, 32 output channels (cout is a multiple of 32)
    const int tap = k0 / a.cout, o0 = k0 - tap * a.cout;
    const int ky = tap / a.ks, kx = tap - ky * a.ks;
    const int ty = py - ky, tx = pxx - kx;
    const int oy = ty / a.stride, ox = tx / a.stride;
    const bool valid = pix_ok && ty >= 0 && tx >= 0 && oy * a.stride == ty && ox * a.stride == tx && oy < a.ho && ox < a.wo;
    const float* src = gyv + (size_t)(o0 + kq) * npo + (valid ? oy * a.wo + ox : 0);
#pragma unroll
    for (int i = 0; i < CNN_BK / 2; ++i) Gs[kq + 2 * i][p] = valid ? src[(size_t)(2 * i) * npo] : 0.f;
    *(float4*)&Ws[tid >> 3][4 * (tid & 7)] = *(const float4*)(a.wt + (size_t)(k0 + (tid >> 3)) * a.cin + c0 + 4 * (tid & 7));
    __syncthreads();
#pragma unroll
    for (int s = 0; s < CNN_BK / 2; ++s) {
      const int kk = 2 * s + (lane >> 5);
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[kk][lane & 31], Gs[kk][32 * wave + (lane & 31)], acc, 0, 0, 0);
    }
    __syncthreads();
  }
  const int Po = blockIdx.x * CNN_TP + 32 * wave + (lane & 31);
  if (Po < npp) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      const int ci = c0 + (i & 3) + 8 * (i >> 2) + 4 * (lane >> 5);
      a.gp[((size_t)v * a.cin + ci) * npp + Po] = acc[i];
    }
  }
}

// grid (cdiv(h w, 256), V C): gx (V, C, h, w) = fold of channels coff .. coff + C of gp (V, Ctot, h + 2 pad, w + 2 pad) [+ gx] [+ add (mask > 0)]
__global__ __launch_bounds__(CNN_THREADS) void cnt_fold_kernel(const float* __restrict__ gp, int Ctot, int coff, int C, int h, int w, int pad, float* gx,
                                                               int accumulate, const float* __restrict__ add, const float* __restrict__ mask) {
  const int plane = blockIdx.y, v = plane / C, c = plane - v * C;
  const int i = blockIdx.x * CNN_THREADS + threadIdx.x;
  if (i >= h * w) return;
  const int iy = i / w, ix = i - iy * w, hp = h + 2 * pad, wp = w + 2 * pad;
  const float* src = gp + ((size_t)v * Ctot + coff + c) * hp * wp;
  int rows[3], cols[3], nr = 0, nc = 0;
  if (pad && iy == 1) rows[nr++] = 0;
  rows[nr++] = iy + pad;
  if (pad && iy == h - 2) rows[nr++] = h + 1;
  if (pad && ix == 1) cols[nc++] = 0;
  cols[nc++] = ix + pad;
  if (pad && ix == w - 2) cols[nc++] = w + 1;
  float s = 0.f;
  for (int r = 0; r < nr; ++r)
    for (int q = 0; q < nc; ++q) s += src[rows[r] * wp + cols[q]];
  const size_t at = (size_t)plane * h * w + i;
  if (accumulate) s = gx[at] + s;
  if (add) s = s + (mask ? (mask[at] > 0.f ? add[at] : 0.f) : add[at]);
  gx[at] = s;
}

// grid (cdiv(h w, 256), planes): g (planes, 2 h, 2 w) -> gx (planes, h, w)
__global__ __launch_bounds__(CNN_THREADS) void cnt_up2_bwd_kernel(const float* __restrict__ g, int h, int w, float ry, float rx, float* __restrict__ gx) {
  const size_t plane = blockIdx.y;
  const int i = blockIdx.x * CNN_THREADS + threadIdx.x;
  if (i >= h * w) return;
  const int sy = i / w, sx = i - sy * w, H2 = 2 * h, W2 = 2 * w;
  const float* src = g + plane * 4 * h * w;
  float s = 0.f;
  // a destination row oy reads source rows floor(ry oy) and the next: those with either equal to sy lie in 2 sy - 3 .. 2 sy + 4 (1 / ry = 2 + 1 / (h - 1) <= 3)
  for (int oy = max(0, 2 * sy - 3); oy <= min(H2 - 1, 2 * sy + 4); ++oy) {
    const float fy = ry * (float)oy;
    const int y0 = (int)fy, y1 = y0 + (y0 < h - 1 ? 1 : 0);
    const float ly = fy - (float)y0, hy = 1.f - ly;
    const float wy = (y0 == sy ? hy : 0.f) + (y1 == sy ? ly : 0.f);
    if (y0 != sy && y1 != sy) continue;
    for (int ox = max(0, 2 * sx - 3); ox <= min(W2 - 1, 2 * sx + 4); ++ox) {
      const float fx = rx * (float)ox;
      const int x0 = (int)fx, x1 = x0 + (x0 < w - 1 ? 1 : 0);
      const float lx = fx - (float)x0, hx = 1.f - lx;
      if (x0 != sx && x1 != sx) continue;
      const float wx = (x0 == sx ? hx : 0.f) + (x1 == sx ? lx : 0.f);
      s += src[oy * W2 + ox] * (wy * wx);
    }
  }
  gx[plane * h * w + i] = s;
}

// ------------------------------------------------------------------------------------------ the head
struct CntHeadBwdArgs {
  const float* i2;       // (V, 32, n): ELU(IN(iconv2)), kept
  const float* cnn_in;
  const float *ocw, *ocb, *d0w, *d0b, *d2w, *d2b, *cow, *cob;   // the inference image's [k][out] weights
  const float* g_out;    // (V, 32, n)
  float* g_i2;           // (V, 32, n)
  float* cat;            // (V, 48, n): [d, f]
  float* hid;            // (V, 32, n): the depth skip's ReLU'd hidden values, (c8, py, px)
  float* g_f;            // (V, 32, n)
  float* g_d;            // (V, 16, n)
  float* g_hid;          // (V, 8, H/2, W/2): the cotangent of depth_skip.0's output, before its bias
  int H, W, hq, wq;
};

// grid (cdiv(hq wq, 256), V)
__global__ __launch_bounds__(CNN_THREADS) void cnt_head_bwd_kernel(const CntHeadBwdArgs a) {
  __shared__ __attribute__((aligned(16))) float w[HEAD_N];
  const int tid = threadIdx.x, v = blockIdx.y;
  for (int i = tid; i < 1024; i += CNN_THREADS) w[HEAD_OCW + i] = a.ocw[i];
  for (int i = tid; i < 512; i += CNN_THREADS) w[HEAD_D2W + i] = a.d2w[i];
  for (int i = tid; i < 1536; i += CNN_THREADS) w[HEAD_COW + i] = a.cow[i];
  if (tid < 32) { w[HEAD_OCB + tid] = a.ocb[tid]; w[HEAD_D0W + tid] = a.d0w[tid]; w[HEAD_COB + tid] = a.cob[tid]; }
  if (tid < 8) w[HEAD_D0B + tid] = a.d0b[tid];
  if (tid < 16) w[HEAD_D2B + tid] = a.d2b[tid];
  __syncthreads();
  const int n = a.hq * a.wq, P = blockIdx.x * CNN_THREADS + tid;
  if (P >= n) return;
  const int y = P / a.wq, x = P % a.wq;

  // the forward's f, hidden values and d, in its order
  float t[32], f[32];
#pragma unroll
  for (int c = 0; c < 32; ++c) t[c] = a.i2[((size_t)v * 32 + c) * n + P];
#pragma unroll
  for (int co = 0; co < 32; ++co) f[co] = 0.f;
#pragma unroll
  for (int k = 0; k < 32; ++k)
#pragma unroll
    for (int co = 0; co < 32; ++co) f[co] = fmaf(t[k], w[HEAD_OCW + 32 * k + co], f[co]);
#pragma unroll
  for (int co = 0; co < 32; ++co) {
    f[co] += w[HEAD_OCB + co];
    a.cat[((size_t)v * 48 + 16 + co) * n + P] = f[co];
  }
  const float* dp = a.cnn_in + ((size_t)v * 12 + 3) * a.H * a.W + (size_t)(4 * y) * a.W + 4 * x;
  float patch[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float4 q = *(const float4*)(dp + (size_t)r * a.W);
    patch[r][0] = q.x; patch[r][1] = q.y; patch[r][2] = q.z; patch[r][3] = q.w;
  }
#pragma unroll
  for (int c8 = 0; c8 < 8; ++c8)
#pragma unroll
    for (int py = 0; py < 2; ++py)
#pragma unroll
      for (int px = 0; px < 2; ++px) {
        float s = 0.f;
#pragma unroll
        for (int ky = 0; ky < 2; ++ky)
#pragma unroll
          for (int kx = 0; kx < 2; ++kx) s = fmaf(patch[2 * py + ky][2 * px + kx], w[HEAD_D0W + 8 * (2 * ky + kx) + c8], s);
        t[(c8 * 2 + py) * 2 + px] = cnn_relu(s + w[HEAD_D0B + c8]);
      }
  float d[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) d[c] = 0.f;
#pragma unroll
  for (int k = 0; k < 32; ++k)
#pragma unroll
    for (int c = 0; c < 16; ++c) d[c] = fmaf(t[k], w[HEAD_D2W + 16 * k + c], d[c]);
#pragma unroll
  for (int c = 0; c < 16; ++c) a.cat[((size_t)v * 48 + c) * n + P] = d[c] + w[HEAD_D2B + c];
#pragma unroll
  for (int k = 0; k < 32; ++k) a.hid[((size_t)v * 32 + k) * n + P] = t[k];

  // the cotangents: out = conv_out(cat[d, f])
  float go[32];
#pragma unroll
  for (int co = 0; co < 32; ++co) go[co] = a.g_out[((size_t)v * 32 + co) * n + P];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    float s = 0.f;
#pragma unroll
    for (int co = 0; co < 32; ++co) s = fmaf(go[co], w[HEAD_COW + 32 * k + co], s);
    d[k] = s;
    a.g_d[((size_t)v * 16 + k) * n + P] = s;
  }
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    float s = 0.f;
#pragma unroll
    for (int co = 0; co < 32; ++co) s = fmaf(go[co], w[HEAD_COW + 32 * (16 + k) + co], s);
    f[k] = s;
    a.g_f[((size_t)v * 32 + k) * n + P] = s;
  }
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    float s = 0.f;
#pragma unroll
    for (int co = 0; co < 32; ++co) s = fmaf(f[co], w[HEAD_OCW + 32 * k + co], s);
    a.g_i2[((size_t)v * 32 + k) * n + P] = s;
  }
  const int H2 = a.H / 2, W2 = a.W / 2;
#pragma unroll
  for (int k = 0; k < 32; ++k) {
    float s = 0.f;
#pragma unroll
    for (int c = 0; c < 16; ++c) s = fmaf(d[c], w[HEAD_D2W + 16 * k + c], s);
    const int c8 = k >> 2, py = (k >> 1) & 1, px = k & 1;
    a.g_hid[(((size_t)v * 8 + c8) * H2 + 2 * y + py) * W2 + 2 * x + px] = t[k] > 0.f ? s : 0.f;
  }
}

// dst[(t O + o) Cin + in] = src[o][in][t]: the data gradient's operand
__global__ __launch_bounds__(CNN_THREADS) void cnt_pack_t_kernel(const float* __restrict__ src, float* __restrict__ dst, int O, int Cin, int T) {
  const int i = blockIdx.x * CNN_THREADS + threadIdx.x;
  if (i >= O * Cin * T) return;
  const int o = i / (Cin * T), r = i % (Cin * T), ci = r / T, t = r % T;
  dst[((size_t)t * O + o) * Cin + ci] = src[i];
}

// ------------------------------------------------------------------------------------------ host: the image
// the 19 convolutions with a data gradient, in table order, and the offsets (floats) of their transposed copies behind the inference image
struct CntTrans {
  int widx[19];
  size_t off[19];
  int n;
  size_t total;   // floats, the whole image
};
CntTrans make_trans() {
  const CnnTable& t = table();
  CntTrans r;
  r.n = 0;
  size_t at = nl_align_up(t.total, 64);
  auto add = [&](int i) {
    r.widx[r.n] = i;
    r.off[r.n++] = at;
    at += nl_align_up((size_t)t.w[i].O * t.w[i].K, 64);
  };
  for (int L = 1; L <= 3; ++L) {
    const int b0 = w_block(L, 0), b1 = w_block(L, 1);
    add(b0); add(b0 + 3); add(b0 + 6); add(b1); add(b1 + 3);
  }
  for (int j = 0; j < 4; ++j) add(W_DEC + 4 * j);
  r.total = at;
  return r;
}
const CntTrans& trans() {
  static const CntTrans t = make_trans();
  return t;
}
size_t trans_off(int widx) {
  const CntTrans& t = trans();
  for (int i = 0; i < t.n; ++i)
    if (t.widx[i] == widx) return t.off[i];
  return 0;
}

// ------------------------------------------------------------------------------------------ host: the state (offsets in floats; every buffer a multiple of 64)
struct CntBlockState {
  size_t a_raw, a, b_raw, out, na, nb;
};
struct CntState {
  size_t c0_raw, c0, nc0;
  CntBlockState blk[3][2];
  size_t d_raw[3], nd[3];
  size_t up3, u3_raw, u3, i3_raw, i3, up2, u2_raw, u2, i2_raw, i2, nu3, ni3, nu2, ni2;
  size_t total;
};
CntState make_state(int V, int H, int W) {
  CntState p;
  size_t at = 0;
  auto take = [&](size_t floats) { const size_t o = at; at += nl_align_up(floats, 64); return o; };
  const size_t n0 = (size_t)(H / 2 - 1) * (W / 2 - 1), n1 = (size_t)(H / 4) * (W / 4);
  p.c0_raw = take(V * 32 * n0); p.c0 = take(V * 32 * n0); p.nc0 = take((size_t)V * 32 * 4);
  for (int L = 0; L < 3; ++L) {
    const size_t C = 32u << L, m = (size_t)V * C * (n1 >> (2 * L));
    for (int b = 0; b < 2; ++b) {
      CntBlockState& s = p.blk[L][b];
      s.a_raw = take(m); s.a = take(m); s.b_raw = take(m); s.out = take(m); s.na = take(V * C * 4); s.nb = take(V * C * 4);
    }
    p.d_raw[L] = take(m); p.nd[L] = take(V * C * 4);
  }
  p.up3 = take(V * 128 * (n1 / 4)); p.u3_raw = take(V * 64 * (n1 / 4)); p.u3 = take(V * 64 * (n1 / 4)); p.i3_raw = take(V * 64 * (n1 / 4)); p.i3 = take(V * 64 * (n1 / 4));
  p.up2 = take(V * 64 * n1); p.u2_raw = take(V * 32 * n1); p.u2 = take(V * 32 * n1); p.i2_raw = take(V * 32 * n1); p.i2 = take(V * 32 * n1);
  p.nu3 = take((size_t)V * 64 * 4); p.ni3 = take((size_t)V * 64 * 4); p.nu2 = take((size_t)V * 32 * 4); p.ni2 = take((size_t)V * 32 * 4);
  p.total = at;
  return p;
}

// ------------------------------------------------------------------------------------------ host: one convolution's gradients
struct CntConvSpec {
  int V, C0, C1, cout, hin, win, ks, stride, pad, tap_major;
  int cin() const { return C0 + C1; }
  int K() const { return cin() * ks * ks; }
  int ho() const { return (hin + 2 * pad - ks) / stride + 1; }
  int wo() const { return (win + 2 * pad - ks) / stride + 1; }
  int hp() const { return hin + 2 * pad; }
  int wp() const { return win + 2 * pad; }
};
void wgrad_split(int V, int npix, int& chunks, int& CH) {
  const int64_t c = std::min<int64_t>(nl_cdiv(npix, 512), std::max(1, 256 / V));
  CH = (int)nl_align_up((size_t)nl_cdiv(npix, c), 32);
  chunks = (int)nl_cdiv(npix, CH);
}
size_t wgrad_part_floats(const CntConvSpec& c) {
  int chunks, CH;
  wgrad_split(c.V, c.ho() * c.wo(), chunks, CH);
  return (size_t)c.V * chunks * c.cout * c.K();
}
size_t dgrad_pad_floats(const CntConvSpec& c) { return (size_t)c.V * c.cin() * c.hp() * c.wp(); }

// g_w (the parameter's layout) of one convolution: two launches
int run_wgrad(const CntConvSpec& c, CntSrc s0, CntSrc s1, const float* gy, float* part, float* gw, hipStream_t s, int& launches) {
  CntWgradArgs a;
  a.s0 = s0; a.s1 = s1; a.gy = gy; a.part = part;
  a.cout = c.cout; a.K = c.K(); a.ks = c.ks; a.tap_major = c.tap_major; a.cin = c.cin();
  a.hin = c.hin; a.win = c.win; a.ho = c.ho(); a.wo = c.wo(); a.stride = c.stride; a.pad = c.pad;
  wgrad_split(c.V, a.ho * a.wo, a.chunks, a.CH);
  const int nsplit = c.V * a.chunks;
  hipLaunchKernelGGL(cnt_wgrad_kernel, dim3((unsigned)nl_cdiv(a.K, CNT_WK), (unsigned)nl_cdiv(a.cout, 32), (unsigned)nsplit), dim3(CNN_THREADS), 0, s, a);
  ++launches;
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(cnt_wgrad_reduce_kernel, dim3((unsigned)nl_cdiv((int64_t)a.cout * a.K, CNN_THREADS)), dim3(CNN_THREADS), 0, s, (const float*)part, nsplit,
                     a.cout, a.K, a.cin, a.tap_major, gw);
  ++launches;
  NL_LAUNCH_CHECK();
  return NL_OK;
}
// the padded-domain gradient of cat[x0, x1]: one launch
int run_dgrad(const CntConvSpec& c, const float* gy, const float* wt, float* gp, hipStream_t s, int& launches) {
  CntDgradArgs a;
  a.gy = gy; a.wt = wt; a.gp = gp;
  a.cin = c.cin(); a.cout = c.cout; a.ks = c.ks; a.stride = c.stride;
  a.ho = c.ho(); a.wo = c.wo(); a.hp = c.hp(); a.wp = c.wp();
  hipLaunchKernelGGL(cnt_dgrad_kernel, dim3((unsigned)nl_cdiv((int64_t)a.hp * a.wp, CNN_TP), (unsigned)c.V, (unsigned)(a.cin / 32)), dim3(CNN_THREADS), 0, s, a);
  ++launches;
  NL_LAUNCH_CHECK();
  return NL_OK;
}
int run_fold(const CntConvSpec& c, const float* gp, int coff, int C, float* gx, int accumulate, const float* add, const float* mask, hipStream_t s, int& launches) {
  hipLaunchKernelGGL(cnt_fold_kernel, dim3((unsigned)nl_cdiv((int64_t)c.hin * c.win, CNN_THREADS), (unsigned)(c.V * C)), dim3(CNN_THREADS), 0, s, gp, c.cin(), coff,
                     C, c.hin, c.win, c.pad, gx, accumulate, add, mask);
  ++launches;
  NL_LAUNCH_CHECK();
  return NL_OK;
}
int run_up2_bwd(const float* g, int planes, int h, int w, float* gx, hipStream_t s, int& launches) {
  hipLaunchKernelGGL(cnt_up2_bwd_kernel, dim3((unsigned)nl_cdiv((int64_t)h * w, CNN_THREADS), (unsigned)planes), dim3(CNN_THREADS), 0, s, g, h, w,
                     (float)(h - 1) / (float)(2 * h - 1), (float)(w - 1) / (float)(2 * w - 1), gx);
  ++launches;
  NL_LAUNCH_CHECK();
  return NL_OK;
}

// ------------------------------------------------------------------------------------------ host: the backward's workspace
// the net's convolutions: index 0 conv1; 1 + 5 L + {0: b0.conv1, 1: b0.conv2, 2: downsample, 3: b1.conv1, 4: b1.conv2}; 16 .. 19 the decoder; 20 .. 23 the head
// (conv_out, out_conv, depth_skip.2, depth_skip.0)
constexpr int CNT_NCONV = 24;
void conv_list(int V, int H, int W, CntConvSpec* c) {
  auto set = [&](int i, int C0, int C1, int cout, int hin, int win, int ks, int stride, int pad, int tm) {
    c[i] = CntConvSpec{V, C0, C1, cout, hin, win, ks, stride, pad, tm};
  };
  set(0, 12, 0, 32, H, W, 8, 2, 2, 0);
  int h = H / 2 - 1, w = W / 2 - 1;
  for (int L = 0; L < 3; ++L) {
    const int C = 32 << L, Cp = L == 0 ? 32 : C / 2, ho = H >> (2 + L), wo = W >> (2 + L);
    set(1 + 5 * L, Cp, 0, C, h, w, 3, 2, 1, 1);
    set(2 + 5 * L, C, 0, C, ho, wo, 3, 1, 1, 1);
    set(3 + 5 * L, Cp, 0, C, h, w, 1, 2, 0, 0);
    set(4 + 5 * L, C, 0, C, ho, wo, 3, 1, 1, 1);
    set(5 + 5 * L, C, 0, C, ho, wo, 3, 1, 1, 1);
    h = ho; w = wo;
  }
  set(16, 128, 0, 64, H / 8, W / 8, 3, 1, 1, 1);
  set(17, 64, 64, 64, H / 8, W / 8, 3, 1, 1, 1);
  set(18, 64, 0, 32, H / 4, W / 4, 3, 1, 1, 1);
  set(19, 32, 32, 32, H / 4, W / 4, 3, 1, 1, 1);
  set(20, 48, 0, 32, H / 4, W / 4, 1, 1, 0, 0);
  set(21, 32, 0, 32, H / 4, W / 4, 1, 1, 0, 0);
  set(22, 32, 0, 16, H / 4, W / 4, 1, 1, 0, 0);
  set(23, 1, 0, 8, H, W, 2, 2, 0, 0);
}

struct CntBwdPlan {
  size_t g_c0, ga[3], gb[3], gd[3], gy[3], gx[3];   // cotangents: conv1's map; per layer a, b, downsample, block 0's output, the layer's output
  size_t g_up3, g_u3, g_i3, g_up2, g_u2, g_i2;
  size_t cat, hid, g_f, g_d, g_hid;
  size_t pp[CNT_MAX_SITES];
  size_t pad, part;
  size_t total;
};
CntBwdPlan make_bwd_plan(int V, int H, int W) {
  CntBwdPlan p;
  size_t at = 0;
  auto take = [&](size_t floats) { const size_t o = at; at += nl_align_up(floats, 64); return o; };
  const size_t n0 = (size_t)(H / 2 - 1) * (W / 2 - 1), n1 = (size_t)(H / 4) * (W / 4);
  p.g_c0 = take(V * 32 * n0);
  for (int L = 0; L < 3; ++L) {
    const size_t m = (size_t)V * (32u << L) * (n1 >> (2 * L));
    p.ga[L] = take(m); p.gb[L] = take(m); p.gd[L] = take(m); p.gy[L] = take(m); p.gx[L] = take(m);
  }
  p.g_up3 = take(V * 128 * (n1 / 4)); p.g_u3 = take(V * 64 * (n1 / 4)); p.g_i3 = take(V * 64 * (n1 / 4));
  p.g_up2 = take(V * 64 * n1); p.g_u2 = take(V * 32 * n1); p.g_i2 = take(V * 32 * n1);
  p.cat = take(V * 48 * n1); p.hid = take(V * 32 * n1); p.g_f = take(V * 32 * n1); p.g_d = take(V * 16 * n1); p.g_hid = take(V * 32 * n1);
  for (int i = 0; i < CNT_MAX_SITES; ++i) p.pp[i] = take((size_t)V * 128 * 2);
  CntConvSpec c[CNT_NCONV];
  conv_list(V, H, W, c);
  size_t pad = 0, part = 0;
  for (int i = 0; i < CNT_NCONV; ++i) {
    part = std::max(part, wgrad_part_floats(c[i]));
    if (i >= 1 && i < 20) pad = std::max(pad, dgrad_pad_floats(c[i]));
  }
  p.pad = take(pad); p.part = take(part);
  p.total = at;
  return p;
}

}  // namespace

extern "C" {

int nlct_abi_version(void) { return NLCT_ABI_VERSION; }

size_t nlct_dfnet_packed_bytes(void) { return nl_align_up(trans().total * sizeof(float), 256); }

int nlct_dfnet_pack_weights(const void* const* ptrs, int n, void* packed, size_t packed_bytes, void* stream) {
  const CnnTable& t = table();
  if (!ptrs || n != t.n) return NL_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i)
    if (!ptrs[i] || !aligned(ptrs[i], 4)) return NL_ERR_BAD_ARG;
  if (!packed || !aligned(packed, 256) || packed_bytes < nlct_dfnet_packed_bytes()) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n; ++i) {
    const CnnWeight& w = t.w[i];
    hipLaunchKernelGGL(cnn_pack_kernel, dim3((unsigned)nl_cdiv((int64_t)w.O * w.K, CNN_THREADS)), dim3(CNN_THREADS), 0, s, (const float*)ptrs[i],
                       (float*)packed + w.off, w.O, w.K / w.T, w.T, w.T > 1 ? 1 : 0);
    NL_LAUNCH_CHECK();
  }
  const CntTrans& tr = trans();
  for (int j = 0; j < tr.n; ++j) {
    const CnnWeight& w = t.w[tr.widx[j]];
    hipLaunchKernelGGL(cnt_pack_t_kernel, dim3((unsigned)nl_cdiv((int64_t)w.O * w.K, CNN_THREADS)), dim3(CNN_THREADS), 0, s, (const float*)ptrs[tr.widx[j]],
                       (float*)packed + tr.off[j], w.O, w.K / w.T, w.T);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

size_t nlct_dfnet_state_bytes(int V, int H, int W) {
  if (!shape_ok(V, H, W)) return 0;
  return nl_align_up(make_state(V, H, W).total * sizeof(float), 256);
}

int nlct_dfnet_forward_train(const void* packed, const float* cnn_in, int V, int H, int W, float* out, void* state, size_t state_bytes, void* stream) {
  if (!shape_ok(V, H, W)) return NL_ERR_UNSUPPORTED;
  if (!packed || !cnn_in || !out || !aligned(packed, 256) || !aligned(cnn_in, 16) || !aligned(out, 4)) return NL_ERR_BAD_ARG;
  if (!state || !aligned(state, 256) || state_bytes < nlct_dfnet_state_bytes(V, H, W)) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const CnnTable& t = table();
  const CntState p = make_state(V, H, W);
  const float* pk = (const float*)packed;
  float* w = (float*)state;
  auto wt = [&](int i) { return pk + t.w[i].off; };
  int launches = 0;

  auto run_conv = [&](CnnSrc s0, CnnSrc s1, int widx, int ks, int stride, int pad, int cout, int hin, int win, float* y, int& ho, int& wo) -> int {
    CnnConvArgs a;
    a.s0 = s0; a.s1 = s1; a.wt = wt(widx); a.y = y; a.cout = cout;
    a.hin = hin; a.win = win;
    a.stride = stride; a.pad = pad;
    a.ho = ho = (hin + 2 * pad - ks) / stride + 1;
    a.wo = wo = (win + 2 * pad - ks) / stride + 1;
    if (!conv(a, ks, V, s)) return NL_ERR_UNSUPPORTED;
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  auto run_stats = [&](const float* x, int C, int n, int gamma_idx, int act, float* nrm, float* y) -> int {
    hipLaunchKernelGGL(cnt_in_stats_keep_kernel, dim3((unsigned)C, (unsigned)V), dim3(CNN_THREADS), 0, s, x, n, wt(gamma_idx), wt(gamma_idx + 1), act, nrm, y);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  auto run_up2 = [&](const float* x, int C, int hh, int ww, float* y) -> int {
    hipLaunchKernelGGL(cnn_up2_kernel, dim3((unsigned)nl_cdiv(4 * hh * ww, CNN_THREADS), (unsigned)(V * C)), dim3(CNN_THREADS), 0, s, x, hh, ww,
                       (float)(hh - 1) / (float)(2 * hh - 1), (float)(ww - 1) / (float)(2 * ww - 1), y);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  auto run_tail = [&](const float* b, const float* nb, const float* idn, const float* nd, int C, int n, float* y) -> int {
    hipLaunchKernelGGL(cnn_block_tail_kernel, dim3((unsigned)nl_cdiv(n, CNN_THREADS), (unsigned)(V * C)), dim3(CNN_THREADS), 0, s, b, nb, idn, nd, n, y,
                       (float*)nullptr);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
#define CNT_TRY(expr) do { const int st_ = (expr); if (st_ != NL_OK) return st_; } while (0)
  const CnnSrc none = {nullptr, 0};
  int h, wd, ho, wo;

  CNT_TRY(run_conv(CnnSrc{cnn_in, 12}, none, W_CONV1, 8, 2, 2, 32, H, W, w + p.c0_raw, h, wd));
  CNT_TRY(run_stats(w + p.c0_raw, 32, h * wd, W_BN1, CNN_ACT_RELU, w + p.nc0, w + p.c0));
  CnnSrc x = {w + p.c0, 32};
  for (int L = 0; L < 3; ++L) {
    const int C = 32 << L, b0 = w_block(L + 1, 0), b1 = w_block(L + 1, 1);
    const CntBlockState &s0 = p.blk[L][0], &s1 = p.blk[L][1];
    CNT_TRY(run_conv(x, none, b0 + 0, 3, 2, 1, C, h, wd, w + s0.a_raw, ho, wo));
    CNT_TRY(run_stats(w + s0.a_raw, C, ho * wo, b0 + 1, CNN_ACT_RELU, w + s0.na, w + s0.a));
    CNT_TRY(run_conv(x, none, b0 + 6, 1, 2, 0, C, h, wd, w + p.d_raw[L], ho, wo));
    CNT_TRY(run_stats(w + p.d_raw[L], C, ho * wo, b0 + 7, CNN_ACT_NONE, w + p.nd[L], nullptr));
    h = ho; wd = wo;
    CNT_TRY(run_conv(CnnSrc{w + s0.a, C}, none, b0 + 3, 3, 1, 1, C, h, wd, w + s0.b_raw, ho, wo));
    CNT_TRY(run_stats(w + s0.b_raw, C, h * wd, b0 + 4, CNN_ACT_NONE, w + s0.nb, nullptr));
    CNT_TRY(run_tail(w + s0.b_raw, w + s0.nb, w + p.d_raw[L], w + p.nd[L], C, h * wd, w + s0.out));
    CNT_TRY(run_conv(CnnSrc{w + s0.out, C}, none, b1 + 0, 3, 1, 1, C, h, wd, w + s1.a_raw, ho, wo));
    CNT_TRY(run_stats(w + s1.a_raw, C, h * wd, b1 + 1, CNN_ACT_RELU, w + s1.na, w + s1.a));
    CNT_TRY(run_conv(CnnSrc{w + s1.a, C}, none, b1 + 3, 3, 1, 1, C, h, wd, w + s1.b_raw, ho, wo));
    CNT_TRY(run_stats(w + s1.b_raw, C, h * wd, b1 + 4, CNN_ACT_NONE, w + s1.nb, nullptr));
    CNT_TRY(run_tail(w + s1.b_raw, w + s1.nb, w + s0.out, nullptr, C, h * wd, w + s1.out));
    x = CnnSrc{w + s1.out, C};
  }
  CNT_TRY(run_up2(x.x, 128, h, wd, w + p.up3));
  h *= 2; wd *= 2;
  CNT_TRY(run_conv(CnnSrc{w + p.up3, 128}, none, W_DEC + 0, 3, 1, 1, 64, h, wd, w + p.u3_raw, ho, wo));
  CNT_TRY(run_stats(w + p.u3_raw, 64, h * wd, W_DEC + 2, CNN_ACT_ELU, w + p.nu3, w + p.u3));
  CNT_TRY(run_conv(CnnSrc{w + p.u3, 64}, CnnSrc{w + p.blk[1][1].out, 64}, W_DEC + 4, 3, 1, 1, 64, h, wd, w + p.i3_raw, ho, wo));
  CNT_TRY(run_stats(w + p.i3_raw, 64, h * wd, W_DEC + 6, CNN_ACT_ELU, w + p.ni3, w + p.i3));
  CNT_TRY(run_up2(w + p.i3, 64, h, wd, w + p.up2));
  h *= 2; wd *= 2;
  CNT_TRY(run_conv(CnnSrc{w + p.up2, 64}, none, W_DEC + 8, 3, 1, 1, 32, h, wd, w + p.u2_raw, ho, wo));
  CNT_TRY(run_stats(w + p.u2_raw, 32, h * wd, W_DEC + 10, CNN_ACT_ELU, w + p.nu2, w + p.u2));
  CNT_TRY(run_conv(CnnSrc{w + p.u2, 32}, CnnSrc{w + p.blk[0][1].out, 32}, W_DEC + 12, 3, 1, 1, 32, h, wd, w + p.i2_raw, ho, wo));
  CNT_TRY(run_stats(w + p.i2_raw, 32, h * wd, W_DEC + 14, CNN_ACT_ELU, w + p.ni2, w + p.i2));

  CnnHeadArgs ha;
  ha.i2 = w + p.i2; ha.cnn_in = cnn_in;
  ha.ocw = wt(W_OUTCONV); ha.ocb = wt(W_OUTCONV + 1); ha.d0w = wt(W_DS0); ha.d0b = wt(W_DS0 + 1); ha.d2w = wt(W_DS2); ha.d2b = wt(W_DS2 + 1);
  ha.cow = wt(W_CONVOUT); ha.cob = wt(W_CONVOUT + 1);
  ha.out = out; ha.H = H; ha.W = W; ha.hq = H / 4; ha.wq = W / 4;
  hipLaunchKernelGGL(cnn_head_kernel, dim3((unsigned)nl_cdiv((int64_t)ha.hq * ha.wq, CNN_THREADS), (unsigned)V), dim3(CNN_THREADS), 0, s, ha);
  ++launches;
  NL_LAUNCH_CHECK();
  return launches == NLCT_FORWARD_LAUNCHES ? NL_OK : NL_ERR_HIP;
}

size_t nlct_dfnet_backward_workspace_bytes(int V, int H, int W) {
  if (!shape_ok(V, H, W)) return 0;
  return nl_align_up(make_bwd_plan(V, H, W).total * sizeof(float), 256);
}

int nlct_dfnet_backward(const void* packed, const float* cnn_in, int V, int H, int W, const void* state, const float* g_out, void* const* grads, void* ws,
                        size_t ws_bytes, void* stream) {
  if (!shape_ok(V, H, W)) return NL_ERR_UNSUPPORTED;
  if (!packed || !cnn_in || !state || !g_out || !grads || !aligned(packed, 256) || !aligned(cnn_in, 16) || !aligned(state, 256) || !aligned(g_out, 4))
    return NL_ERR_BAD_ARG;
  for (int i = 0; i < NLC_DFNET_NUM_WEIGHTS; ++i)
    if (!aligned(grads[i], 4)) return NL_ERR_BAD_ARG;
  if (!ws || !aligned(ws, 256) || ws_bytes < nlct_dfnet_backward_workspace_bytes(V, H, W)) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const CnnTable& t = table();
  const CntState p = make_state(V, H, W);
  const CntBwdPlan q = make_bwd_plan(V, H, W);
  const float* pk = (const float*)packed;
  const float* st = (const float*)state;
  float* w = (float*)ws;
  CntConvSpec cv[CNT_NCONV];
  conv_list(V, H, W, cv);
  auto wt = [&](int i) { return pk + t.w[i].off; };
  auto grad = [&](int i) { return (float*)grads[i]; };
  int launches = 0, skipped = 0, nsite = 0;
  CntInParamsArgs ip;
  memset(&ip, 0, sizeof ip);
  ip.V = V;

  // a map (V, C, plane) as a gather source
  auto src = [&](const float* x, int C, int plane) { return CntSrc{x, C, (size_t)C * plane}; };
  const CntSrc none = {nullptr, 0, 0};
  // the weight gradient of convolution ci (parameter widx) if it is wanted
  auto wgrad = [&](int ci, int widx, CntSrc s0, CntSrc s1, const float* gy) -> int {
    if (!grad(widx)) { skipped += 2; return NL_OK; }
    return run_wgrad(cv[ci], s0, s1, gy, w + q.part, grad(widx), s, launches);
  };
  // InstanceNorm with parameters (gamma_idx, gamma_idx + 1): g (cotangent of act(IN(x)) or, for a tail, of the block's output y) -> gx
  auto in_bwd = [&](const float* x, const float* nrm, const float* y, int act, const float* g, int C, int n, float* gx, int gamma_idx) -> int {
    if (nsite >= CNT_MAX_SITES) return NL_ERR_HIP;
    const int site = nsite++;
    hipLaunchKernelGGL(cnt_in_bwd_kernel, dim3((unsigned)C, (unsigned)V), dim3(CNN_THREADS), 0, s, x, nrm, y, act, g, n, gx, w + q.pp[site]);
    ++launches;
    NL_LAUNCH_CHECK();
    ip.s[site] = CntInSite{w + q.pp[site], grad(gamma_idx), grad(gamma_idx + 1), C};
    return NL_OK;
  };
  auto chan_sum = [&](const float* g, int C, int n, int widx) -> int {
    if (!grad(widx)) { skipped += 1; return NL_OK; }
    hipLaunchKernelGGL(cnt_chan_sum_kernel, dim3((unsigned)C), dim3(CNN_THREADS), 0, s, g, V, n, grad(widx));
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  const int hq = H / 4, wq = W / 4, n1 = hq * wq;

  // ---- the head
  CntHeadBwdArgs ha;
  ha.i2 = st + p.i2; ha.cnn_in = cnn_in;
  ha.ocw = wt(W_OUTCONV); ha.ocb = wt(W_OUTCONV + 1); ha.d0w = wt(W_DS0); ha.d0b = wt(W_DS0 + 1); ha.d2w = wt(W_DS2); ha.d2b = wt(W_DS2 + 1);
  ha.cow = wt(W_CONVOUT); ha.cob = wt(W_CONVOUT + 1);
  ha.g_out = g_out; ha.g_i2 = w + q.g_i2; ha.cat = w + q.cat; ha.hid = w + q.hid; ha.g_f = w + q.g_f; ha.g_d = w + q.g_d; ha.g_hid = w + q.g_hid;
  ha.H = H; ha.W = W; ha.hq = hq; ha.wq = wq;
  hipLaunchKernelGGL(cnt_head_bwd_kernel, dim3((unsigned)nl_cdiv((int64_t)n1, CNN_THREADS), (unsigned)V), dim3(CNN_THREADS), 0, s, ha);
  ++launches;
  NL_LAUNCH_CHECK();
  CNT_TRY(wgrad(20, W_CONVOUT, src(w + q.cat, 48, n1), none, g_out));
  CNT_TRY(chan_sum(g_out, 32, n1, W_CONVOUT + 1));
  CNT_TRY(wgrad(21, W_OUTCONV, src(st + p.i2, 32, n1), none, w + q.g_f));
  CNT_TRY(chan_sum(w + q.g_f, 32, n1, W_OUTCONV + 1));
  CNT_TRY(wgrad(22, W_DS2, src(w + q.hid, 32, n1), none, w + q.g_d));
  CNT_TRY(chan_sum(w + q.g_d, 16, n1, W_DS2 + 1));
  CNT_TRY(wgrad(23, W_DS0, CntSrc{cnn_in + (size_t)3 * H * W, 1, (size_t)12 * H * W}, none, w + q.g_hid));
  CNT_TRY(chan_sum(w + q.g_hid, 8, 4 * n1, W_DS0 + 1));

  // ---- the decoder.  One ConvIN: g (cotangent of ELU(IN(raw)), rewritten in place as the raw sums' cotangent), the weight gradient, the padded data gradient
  auto conv_in_bwd = [&](int ci, int widx, const float* raw, const float* nrm, const float* y, int act, float* g, const float* gin, CntSrc s0, CntSrc s1,
                         bool dgrad) -> int {
    const CntConvSpec& c = cv[ci];
    const int gamma_idx = ci >= 16 ? widx + 2 : widx + 1;   // the decoder's convolutions have a bias in between
    CNT_TRY(in_bwd(raw, nrm, y, act, gin, c.cout, c.ho() * c.wo(), g, gamma_idx));
    CNT_TRY(wgrad(ci, widx, s0, s1, g));
    if (dgrad) CNT_TRY(run_dgrad(c, g, pk + trans_off(widx), w + q.pad, s, launches));
    return NL_OK;
  };
  const int n2 = n1 / 4;
  const float* x1 = st + p.blk[0][1].out;
  const float* x2 = st + p.blk[1][1].out;
  // iconv2
  CNT_TRY(conv_in_bwd(19, W_DEC + 12, st + p.i2_raw, st + p.ni2, st + p.i2, CNN_ACT_ELU, w + q.g_i2, w + q.g_i2, src(st + p.u2, 32, n1), src(x1, 32, n1), true));
  CNT_TRY(run_fold(cv[19], w + q.pad, 0, 32, w + q.g_u2, 0, nullptr, nullptr, s, launches));
  CNT_TRY(run_fold(cv[19], w + q.pad, 32, 32, w + q.gx[0], 0, nullptr, nullptr, s, launches));
  // upconv2
  CNT_TRY(conv_in_bwd(18, W_DEC + 8, st + p.u2_raw, st + p.nu2, st + p.u2, CNN_ACT_ELU, w + q.g_u2, w + q.g_u2, src(st + p.up2, 64, n1), none, true));
  CNT_TRY(run_fold(cv[18], w + q.pad, 0, 64, w + q.g_up2, 0, nullptr, nullptr, s, launches));
  CNT_TRY(run_up2_bwd(w + q.g_up2, V * 64, H / 8, W / 8, w + q.g_i3, s, launches));
  // iconv3
  CNT_TRY(conv_in_bwd(17, W_DEC + 4, st + p.i3_raw, st + p.ni3, st + p.i3, CNN_ACT_ELU, w + q.g_i3, w + q.g_i3, src(st + p.u3, 64, n2), src(x2, 64, n2), true));
  CNT_TRY(run_fold(cv[17], w + q.pad, 0, 64, w + q.g_u3, 0, nullptr, nullptr, s, launches));
  CNT_TRY(run_fold(cv[17], w + q.pad, 64, 64, w + q.gx[1], 0, nullptr, nullptr, s, launches));
  // upconv3
  CNT_TRY(conv_in_bwd(16, W_DEC + 0, st + p.u3_raw, st + p.nu3, st + p.u3, CNN_ACT_ELU, w + q.g_u3, w + q.g_u3, src(st + p.up3, 128, n2), none, true));
  CNT_TRY(run_fold(cv[16], w + q.pad, 0, 128, w + q.g_up3, 0, nullptr, nullptr, s, launches));
  CNT_TRY(run_up2_bwd(w + q.g_up3, V * 128, H / 16, W / 16, w + q.gx[2], s, launches));

  // ---- layer3 .. layer1
  for (int L = 2; L >= 0; --L) {
    const int C = 32 << L, Cp = L == 0 ? 32 : C / 2, b0 = w_block(L + 1, 0), b1 = w_block(L + 1, 1), base = 1 + 5 * L;
    const int n = n1 >> (2 * L);
    const int nprev = cv[base].hin * cv[base].win;
    const CntBlockState &s0 = p.blk[L][0], &s1 = p.blk[L][1];
    const float* prev = L == 0 ? st + p.c0 : st + p.blk[L - 1][1].out;
    float* g_prev = L == 0 ? w + q.g_c0 : w + q.gx[L - 1];
    // block 1: x = ReLU(IN(b) + y)
    CNT_TRY(conv_in_bwd(base + 4, b1 + 3, st + s1.b_raw, st + s1.nb, st + s1.out, CNN_ACT_RELU, w + q.gb[L], w + q.gx[L], src(st + s1.a, C, n), none, true));
    CNT_TRY(run_fold(cv[base + 4], w + q.pad, 0, C, w + q.ga[L], 0, nullptr, nullptr, s, launches));
    CNT_TRY(conv_in_bwd(base + 3, b1 + 0, st + s1.a_raw, st + s1.na, st + s1.a, CNN_ACT_RELU, w + q.ga[L], w + q.ga[L], src(st + s0.out, C, n), none, true));
    CNT_TRY(run_fold(cv[base + 3], w + q.pad, 0, C, w + q.gy[L], 0, w + q.gx[L], st + s1.out, s, launches));
    // block 0: y = ReLU(IN(b) + IN(downsample))
    CNT_TRY(conv_in_bwd(base + 1, b0 + 3, st + s0.b_raw, st + s0.nb, st + s0.out, CNN_ACT_RELU, w + q.gb[L], w + q.gy[L], src(st + s0.a, C, n), none, true));
    CNT_TRY(run_fold(cv[base + 1], w + q.pad, 0, C, w + q.ga[L], 0, nullptr, nullptr, s, launches));
    CNT_TRY(conv_in_bwd(base + 0, b0 + 0, st + s0.a_raw, st + s0.na, st + s0.a, CNN_ACT_RELU, w + q.ga[L], w + q.ga[L], src(prev, Cp, nprev), none, true));
    CNT_TRY(run_fold(cv[base + 0], w + q.pad, 0, Cp, g_prev, L > 0 ? 1 : 0, nullptr, nullptr, s, launches));
    CNT_TRY(conv_in_bwd(base + 2, b0 + 6, st + p.d_raw[L], st + p.nd[L], st + s0.out, CNN_ACT_RELU, w + q.gd[L], w + q.gy[L], src(prev, Cp, nprev), none, true));
    CNT_TRY(run_fold(cv[base + 2], w + q.pad, 0, Cp, g_prev, 1, nullptr, nullptr, s, launches));
  }
  // ---- conv1
  CNT_TRY(conv_in_bwd(0, W_CONV1, st + p.c0_raw, st + p.nc0, st + p.c0, CNN_ACT_RELU, w + q.g_c0, w + q.g_c0, CntSrc{cnn_in, 12, (size_t)12 * H * W}, none, false));
#undef CNT_TRY

  // ---- every gamma and beta, and the four zero biases
  for (int j = 0; j < 4; ++j) {
    ip.zero[j] = grad(W_DEC + 4 * j + 1);
    ip.zn[j] = t.w[W_DEC + 4 * j + 1].O;
  }
  if (nsite != CNT_MAX_SITES) return NL_ERR_HIP;
  hipLaunchKernelGGL(cnt_in_params_kernel, dim3((unsigned)nsite), dim3(CNN_THREADS), 0, s, ip);
  ++launches;
  NL_LAUNCH_CHECK();
  return launches + skipped == NLCT_BACKWARD_LAUNCHES ? NL_OK : NL_ERR_HIP;
}

// ------------------------------------------------------------------------------------------ the stages
static bool conv_spec_ok(int V, int C0, int C1, int cout, int hin, int win, int ks, int stride, CntConvSpec* out) {
  if (V < 1 || V > NLC_DFNET_MAX_VIEWS || C0 < 1 || C1 < 0 || C0 + C1 > 512 || cout < 1 || cout > 512 || (ks != 1 && ks != 3 && ks != 8) ||
      (stride != 1 && stride != 2) || hin < 2 || win < 2 || hin > 8192 || win > 8192)
    return false;
  const int pad = ks == 8 ? 2 : ks == 3 ? 1 : 0;
  if (hin <= pad || win <= pad || hin + 2 * pad < ks || win + 2 * pad < ks) return false;
  const CntConvSpec c = {V, C0, C1, cout, hin, win, ks, stride, pad, ks == 3 ? 1 : 0};
  const int64_t lim = (int64_t)1 << 31;
  if ((int64_t)V * c.cin() * c.hp() * c.wp() >= lim || (int64_t)V * cout * c.ho() * c.wo() >= lim || (int64_t)cout * c.K() >= lim) return false;
  if ((int64_t)wgrad_part_floats(c) >= ((int64_t)1 << 34)) return false;
  *out = c;
  return true;
}
// the stage workspace: the transposed weights, the padded gradient, the partials (floats, each a multiple of 64)
static void conv_ws(const CntConvSpec& c, size_t& wt, size_t& pad, size_t& part, size_t& total) {
  wt = 0;
  pad = wt + nl_align_up((size_t)c.cout * c.K(), 64);
  part = pad + nl_align_up(dgrad_pad_floats(c), 64);
  total = part + nl_align_up(wgrad_part_floats(c), 64);
}

size_t nlct_conv_backward_workspace_bytes(int V, int C0, int C1, int cout, int hin, int win, int ks, int stride) {
  CntConvSpec c;
  if (!conv_spec_ok(V, C0, C1, cout, hin, win, ks, stride, &c)) return 0;
  size_t a, b, d, total;
  conv_ws(c, a, b, d, total);
  return nl_align_up(total * sizeof(float), 256);
}

int nlct_conv_backward(const float* x0, int C0, const float* x1, int C1, const float* wgt, const float* g_y, int V, int cout, int hin, int win, int ks, int stride,
                       float* g_x0, float* g_x1, float* g_w, void* ws, size_t ws_bytes, void* stream) {
  CntConvSpec c;
  if (!conv_spec_ok(V, C0, C1, cout, hin, win, ks, stride, &c)) return NL_ERR_UNSUPPORTED;
  const bool dg = g_x0 || g_x1;
  if (dg && (ks == 8 || cout % 32 || c.cin() % 32)) return NL_ERR_UNSUPPORTED;
  if (g_x1 && !C1) return NL_ERR_BAD_ARG;
  if (!g_y || !aligned(g_y, 4) || !aligned(g_x0, 4) || !aligned(g_x1, 4) || !aligned(g_w, 4) || !aligned(x0, 4) || !aligned(x1, 4) || !aligned(wgt, 4))
    return NL_ERR_BAD_ARG;
  if (g_w && (!x0 || (C1 && !x1))) return NL_ERR_BAD_ARG;
  if (dg && !wgt) return NL_ERR_BAD_ARG;
  if (!ws || !aligned(ws, 256) || ws_bytes < nlct_conv_backward_workspace_bytes(V, C0, C1, cout, hin, win, ks, stride)) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  size_t owt, opad, opart, total;
  conv_ws(c, owt, opad, opart, total);
  float* w = (float*)ws;
  int launches = 0;
  const size_t npl = (size_t)hin * win;
  if (g_w) {
    const int st = run_wgrad(c, CntSrc{x0, C0, C0 * npl}, CntSrc{x1, C1, C1 * npl}, g_y, w + opart, g_w, s, launches);
    if (st != NL_OK) return st;
  }
  if (dg) {
    hipLaunchKernelGGL(cnt_pack_t_kernel, dim3((unsigned)nl_cdiv((int64_t)cout * c.K(), CNN_THREADS)), dim3(CNN_THREADS), 0, s, wgt, w + owt, cout, c.cin(), ks * ks);
    NL_LAUNCH_CHECK();
    int st = run_dgrad(c, g_y, w + owt, w + opad, s, launches);
    if (st == NL_OK && g_x0) st = run_fold(c, w + opad, 0, C0, g_x0, 0, nullptr, nullptr, s, launches);
    if (st == NL_OK && g_x1) st = run_fold(c, w + opad, C0, C1, g_x1, 0, nullptr, nullptr, s, launches);
    if (st != NL_OK) return st;
  }
  return NL_OK;
}

int nlct_instnorm_backward(const float* x, const float* nrm, const float* y, int act, const float* g_y, int V, int C, int n, float* g_x, float* g_gamma,
                           float* g_beta, void* ws, size_t ws_bytes, void* stream) {
  if (V < 1 || V > NLC_DFNET_MAX_VIEWS || C < 1 || C > 4096 || n < 1 || (int64_t)V * C * n >= ((int64_t)1 << 31)) return NL_ERR_UNSUPPORTED;
  if (act != CNN_ACT_NONE && act != CNN_ACT_RELU && act != CNN_ACT_ELU) return NL_ERR_BAD_ARG;
  if (!x || !nrm || !g_y || (act != CNN_ACT_NONE && !y) || !aligned(x, 4) || !aligned(nrm, 16) || !aligned(y, 4) || !aligned(g_y, 4) || !aligned(g_x, 4) ||
      !aligned(g_gamma, 4) || !aligned(g_beta, 4))
    return NL_ERR_BAD_ARG;
  if (!ws || !aligned(ws, 256) || ws_bytes < (size_t)8 * V * C) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(cnt_in_bwd_kernel, dim3((unsigned)C, (unsigned)V), dim3(CNN_THREADS), 0, s, x, nrm, y, act, g_y, n, g_x, (float*)ws);
  NL_LAUNCH_CHECK();
  CntInParamsArgs ip;
  memset(&ip, 0, sizeof ip);
  ip.V = V;
  ip.s[0] = CntInSite{(const float*)ws, g_gamma, g_beta, C};
  hipLaunchKernelGGL(cnt_in_params_kernel, dim3(1), dim3(CNN_THREADS), 0, s, ip);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nlct_up2_backward(const float* g_y, int planes, int h, int w, float* g_x, void* stream) {
  if (planes < 1 || planes > 65535 || h < 2 || w < 2 || (int64_t)4 * planes * h * w >= ((int64_t)1 << 31)) return NL_ERR_UNSUPPORTED;
  if (!g_y || !g_x || !aligned(g_y, 4) || !aligned(g_x, 4)) return NL_ERR_BAD_ARG;
  int launches = 0;
  return run_up2_bwd(g_y, planes, h, w, g_x, (hipStream_t)stream, launches);
}

}  // extern "C"
