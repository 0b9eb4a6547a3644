// The device code, weight table, plan and launch helpers of the per-frame encoder DepthFusionNet, shared by cnn.hip (libnerfloc_cnn.so, inference) and
// cnn_train.hip (libnerfloc_cnn_train.so, the kept forward and the backward).  Everything lies in an unnamed namespace: each unit gets its own copy.
#ifndef NERFLOC_CNN_KERNELS_H
#define NERFLOC_CNN_KERNELS_H
#include <stdio.h>
#include <string.h>

#include "common.h"
#include "../../include/nerfloc_cnn.h"

namespace {

constexpr int CNN_THREADS = 256;
constexpr int CNN_TP = 128;            // output pixels per workgroup
constexpr int CNN_BK = 32;             // k per step
constexpr int CNN_XS = CNN_TP + 32;    // LDS row stride of the pixel operand: the two half-waves (k, k + 1) then read different banks
constexpr float CNN_EPS = 1e-5f;
enum { CNN_ACT_NONE = 0, CNN_ACT_RELU = 1, CNN_ACT_ELU = 2 };

typedef float cnn_f32x16 __attribute__((ext_vector_type(16)));

struct CnnSrc {
  const float* x;     // (V, C, hin, win): a finished map
  int C;
};
struct CnnConvArgs {
  CnnSrc s0, s1;        // the input is cat[s0, s1] along the channels; s1.C == 0: one source
  const float* wt;      // [K][cout], K = (s0.C + s1.C) KS KS in the kernel's k order
  float* y;             // (V, cout, ho, wo)
  int cout;
  int hin, win;         // the sources' planes
  int ho, wo, stride, pad;
};

__device__ __forceinline__ float cnn_relu(float x) { return x < 0.f ? 0.f : x; }   // a NaN stays a NaN
// IN(x) by the plane's (mean, gamma / sqrt(var + eps), beta); nrm == null: x is a finished value
__device__ __forceinline__ float cnn_norm(float x, const float* nrm, size_t plane) {
  if (!nrm) return x;
  const float4 n = ((const float4*)nrm)[plane];
  return (x - n.x) * n.y + n.z;
}
__device__ __forceinline__ int cnn_reflect(int i, int n) { return i < 0 ? -i : i >= n ? 2 * (n - 1) - i : i; }

template <int KS, int NB>
__global__ __launch_bounds__(CNN_THREADS) void cnn_conv_kernel(const CnnConvArgs a) {
  constexpr int COUT = 32 * NB;                   // the output channels of this workgroup: blockIdx.z * COUT ..
  constexpr int WSR = NB == 1 ? 32 : COUT + 32;   // LDS row stride of the weight operand (half-waves on different banks)
  __shared__ float Xs[CNN_BK][CNN_XS];
  __shared__ __attribute__((aligned(16))) float Ws[CNN_BK][WSR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v = blockIdx.y, c0 = blockIdx.z * COUT;
  const int npix = a.ho * a.wo, npl = a.hin * a.win;
  const int cin = a.s0.C + a.s1.C, K = cin * KS * KS;

  // the gather: this thread stages pixel p of the tile for k = kq, kq + 2, ..., kq + 30 of every step.  A step of 32 k is ONE tap (ky, kx) and 32 consecutive
  // input channels (KS == 3, 1: k = (ky KS + kx) cin + in), so the border arithmetic is done once per step; conv1 (KS == 8, 12 channels: k = (in 8 + ky) 8 + kx)
  // takes four rows of eight taps of one channel, and its four column offsets are the same in every step.
  const int p = tid & (CNN_TP - 1), kq = tid >> 7;
  const int P = blockIdx.x * CNN_TP + p;
  const bool pix_ok = P < npix;
  const int oy = pix_ok ? P / a.wo : 0, ox = pix_ok ? P % a.wo : 0;
  const int by = oy * a.stride - a.pad, bx = ox * a.stride - a.pad;
  int ix8[4] = {0, 0, 0, 0};
  if constexpr (KS == 8) {
#pragma unroll
    for (int j = 0; j < 4; ++j) ix8[j] = cnn_reflect(bx + kq + 2 * j, a.win);
  }

  float xreg[CNN_BK / 2];
  float4 w0, w1, w2, w3;   // 32 x COUT floats per step over 256 threads: NB float4 each (named, not an array: they must stay in registers)
  w0 = w1 = w2 = w3 = make_float4(0.f, 0.f, 0.f, 0.f);
  int pf_tap = 0, pf_c = 0;   // the tap and first channel of the step the next prefetch fetches (KS != 8)

  auto prefetch = [&](int k0) {
    if (!pix_ok) {
#pragma unroll
      for (int i = 0; i < CNN_BK / 2; ++i) xreg[i] = 0.f;
    } else if constexpr (KS == 8) {
      const int ci = k0 >> 6, ky0 = (k0 & 63) >> 3;
      const float* src = a.s0.x + ((size_t)v * a.s0.C + ci) * npl;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = cnn_reflect(by + ky0 + r, a.hin) * a.win;
#pragma unroll
        for (int j = 0; j < 4; ++j) xreg[4 * r + j] = src[row + ix8[j]];
      }
    } else {
      const bool second = pf_c >= a.s0.C;   // uniform: the whole step lies in one source
      const CnnSrc& s = second ? a.s1 : a.s0;
      const int ky = pf_tap / KS, kx = pf_tap - ky * KS;
      const int iy = cnn_reflect(by + ky, a.hin), ix = cnn_reflect(bx + kx, a.win);
      const size_t plane0 = (size_t)v * s.C + (second ? pf_c - a.s0.C : pf_c) + kq;
      const int off = iy * a.win + ix;
#pragma unroll
      for (int i = 0; i < CNN_BK / 2; ++i) xreg[i] = s.x[(plane0 + 2 * i) * npl + off];
      pf_c += CNN_BK;
      if (pf_c == cin) { pf_c = 0; ++pf_tap; }
    }
    // row r of the step's weight tile: COUT floats at wt[(k0 + r) cout + c0]
    auto wload = [&](int idx) { return *(const float4*)(a.wt + (size_t)(k0 + idx / (COUT / 4)) * a.cout + c0 + 4 * (idx % (COUT / 4))); };
    w0 = wload(tid);
    if constexpr (NB >= 2) w1 = wload(tid + CNN_THREADS);
    if constexpr (NB == 4) { w2 = wload(tid + 2 * CNN_THREADS); w3 = wload(tid + 3 * CNN_THREADS); }
  };

  cnn_f32x16 acc[NB];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;

  prefetch(0);
  for (int k0 = 0; k0 < K; k0 += CNN_BK) {
#pragma unroll
    for (int i = 0; i < CNN_BK / 2; ++i) Xs[kq + 2 * i][p] = xreg[i];
    auto wstore = [&](int idx, const float4& val) { *(float4*)&Ws[idx / (COUT / 4)][4 * (idx % (COUT / 4))] = val; };
    wstore(tid, w0);
    if constexpr (NB >= 2) wstore(tid + CNN_THREADS, w1);
    if constexpr (NB == 4) { wstore(tid + 2 * CNN_THREADS, w2); wstore(tid + 3 * CNN_THREADS, w3); }
    __syncthreads();
    if (k0 + CNN_BK < K) prefetch(k0 + CNN_BK);
#pragma unroll
    for (int ks = 0; ks < CNN_BK / 2; ++ks) {
      const int kk = 2 * ks + (lane >> 5);
      const float bv = Xs[kk][32 * wave + (lane & 31)];
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[kk][32 * cb + (lane & 31)], bv, acc[cb], 0, 0, 0);
    }
    __syncthreads();
  }

  // C/D layout: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
  const int Po = blockIdx.x * CNN_TP + 32 * wave + (lane & 31);
  if (Po < npix) {
#pragma unroll
    for (int cb = 0; cb < NB; ++cb)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int ch = c0 + 32 * cb + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
        a.y[((size_t)v * a.cout + ch) * npix + Po] = acc[cb][r];
      }
  }
}

// the 256 threads' values added in a fixed tree; every thread gets the sum
__device__ __forceinline__ float cnn_block_sum(float s, float* red) {
  const int tid = threadIdx.x;
  red[tid] = s;
  __syncthreads();
  for (int st = CNN_THREADS / 2; st > 0; st >>= 1) {
    if (tid < st) red[tid] = red[tid] + red[tid + st];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// grid (C, V): plane (v, c) of x (V, C, n) -> nrm[v][c] = (mean, gamma[c] / sqrt(var + eps), beta[c], 0); with act != NONE the plane is then rewritten IN PLACE as
// act(IN(x)): every consumer of that map wants exactly this, so it is done once here, by the workgroup that has just read the plane twice, and not in each
// consumer's gather (a 3 x 3 convolution would redo it nine times per value and channel block)
__global__ __launch_bounds__(CNN_THREADS) void cnn_in_stats_kernel(float* __restrict__ x, int n, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                                   int act, float* __restrict__ nrm) {
  __shared__ float red[CNN_THREADS];
  const int c = blockIdx.x, C = gridDim.x, v = blockIdx.y, tid = threadIdx.x;
  const size_t plane = (size_t)v * C + c;
  float* p = x + plane * n;
  float s = 0.f;
  for (int i = tid; i < n; i += CNN_THREADS) s += p[i];
  const float mean = cnn_block_sum(s, red) / (float)n;
  float q = 0.f;
  for (int i = tid; i < n; i += CNN_THREADS) {
    const float d = p[i] - mean;
    q += d * d;
  }
  q = cnn_block_sum(q, red);
  const float k = gamma[c] / sqrtf(q / (float)n + CNN_EPS), bt = beta[c];
  if (tid == 0) ((float4*)nrm)[plane] = make_float4(mean, k, bt, 0.f);
  if (act == CNN_ACT_NONE) return;
  for (int i = tid; i < n; i += CNN_THREADS) {
    const float y = (p[i] - mean) * k + bt;
    p[i] = act == CNN_ACT_RELU ? cnn_relu(y) : nl_elu(y);
  }
}

// grid (cdiv(n, 256), V C): y = ReLU(IN(b) + i), i = idn (nd == null) or IN(idn) by nd; also written to tap if it is wanted
__global__ __launch_bounds__(CNN_THREADS) void cnn_block_tail_kernel(const float* __restrict__ b, const float* __restrict__ nb, const float* __restrict__ idn,
                                                                     const float* __restrict__ nd, int n, float* __restrict__ y, float* __restrict__ tap) {
  const size_t plane = blockIdx.y;
  const int i = blockIdx.x * CNN_THREADS + threadIdx.x;
  if (i >= n) return;
  const size_t at = plane * n + i;
  const float r = cnn_relu(cnn_norm(b[at], nb, plane) + cnn_norm(idn[at], nd, plane));
  y[at] = r;
  if (tap) tap[at] = r;
}

// grid (cdiv(4 h w, 256), V C): y (2 h x 2 w) = the bilinear x 2 of x (h x w) with align_corners, per plane
__global__ __launch_bounds__(CNN_THREADS) void cnn_up2_kernel(const float* __restrict__ x, int h, int w, float ry, float rx, float* __restrict__ y) {
  const size_t plane = blockIdx.y;
  const int i = blockIdx.x * CNN_THREADS + threadIdx.x, W2 = 2 * w;
  if (i >= 4 * h * w) return;
  const int oy = i / W2, ox = i - oy * W2;
  const float sy = ry * (float)oy, sx = rx * (float)ox;
  const int y0 = (int)sy, x0 = (int)sx;
  const int y1 = y0 + (y0 < h - 1 ? 1 : 0), x1 = x0 + (x0 < w - 1 ? 1 : 0);
  const float ly = sy - (float)y0, lx = sx - (float)x0, hy = 1.f - ly, hx = 1.f - lx;
  const float* src = x + plane * h * w;
  y[plane * 4 * h * w + i] = hy * (hx * src[y0 * w + x0] + lx * src[y0 * w + x1]) + ly * (hx * src[y1 * w + x0] + lx * src[y1 * w + x1]);
}

struct CnnHeadArgs {
  const float* i2;                     // (V, 32, hq, wq): ELU(IN(iconv2))
  const float* cnn_in;                 // (V, 12, H, W)
  const float *ocw, *ocb, *d0w, *d0b, *d2w, *d2b, *cow, *cob;   // [k][out] weights, biases
  float* out;                          // (V, 32, hq, wq)
  int H, W, hq, wq;
};
constexpr int HEAD_OCW = 0, HEAD_OCB = 1024, HEAD_D0W = 1056, HEAD_D0B = 1088, HEAD_D2W = 1096, HEAD_D2B = 1608, HEAD_COW = 1624, HEAD_COB = 3160, HEAD_N = 3192;

// grid (cdiv(hq wq, 256), V)
__global__ __launch_bounds__(CNN_THREADS) void cnn_head_kernel(const CnnHeadArgs a) {
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

  float t[32], g[32], o[32];
  // f = out_conv(i2)
#pragma unroll
  for (int c = 0; c < 32; ++c) t[c] = a.i2[((size_t)v * 32 + c) * n + P];
#pragma unroll
  for (int co = 0; co < 32; ++co) g[co] = 0.f;
#pragma unroll
  for (int k = 0; k < 32; ++k)
#pragma unroll
    for (int co = 0; co < 32; ++co) g[co] = fmaf(t[k], w[HEAD_OCW + 32 * k + co], g[co]);
#pragma unroll
  for (int co = 0; co < 32; ++co) g[co] += w[HEAD_OCB + co];

  // d = depth_skip(channel 3): the 4 x 4 patch -> (8, 2, 2) -> 16
  const float* dp = a.cnn_in + ((size_t)v * 12 + 3) * a.H * a.W + (size_t)(4 * y) * a.W + 4 * x;
  float patch[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float4 q = *(const float4*)(dp + (size_t)r * a.W);   // W is a multiple of 16 and cnn_in 16-byte aligned
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
  for (int c = 0; c < 16; ++c) d[c] += w[HEAD_D2B + c];

  // out = conv_out(cat[d, f])
#pragma unroll
  for (int co = 0; co < 32; ++co) o[co] = 0.f;
#pragma unroll
  for (int k = 0; k < 16; ++k)
#pragma unroll
    for (int co = 0; co < 32; ++co) o[co] = fmaf(d[k], w[HEAD_COW + 32 * k + co], o[co]);
#pragma unroll
  for (int k = 0; k < 32; ++k)
#pragma unroll
    for (int co = 0; co < 32; ++co) o[co] = fmaf(g[k], w[HEAD_COW + 32 * (16 + k) + co], o[co]);
#pragma unroll
  for (int co = 0; co < 32; ++co) a.out[((size_t)v * 32 + co) * n + P] = o[co] + w[HEAD_COB + co];
}

// dst[k][o] = src[o][in][t], k = t Cin + in if T > 1 (the 3 x 3 convolutions: tap-major) and k = in T + t = the source's own order otherwise
// (conv1, the 1 x 1 and 2 x 2 convolutions; a vector is O x 1 x 1: a plain copy)
__global__ __launch_bounds__(CNN_THREADS) void cnn_pack_kernel(const float* __restrict__ src, float* __restrict__ dst, int O, int Cin, int T, int tap_major) {
  const int i = blockIdx.x * CNN_THREADS + threadIdx.x;
  if (i >= O * Cin * T) return;
  const int o = i / (Cin * T), r = i % (Cin * T), ci = r / T, t = r % T;
  const int k = tap_major ? t * Cin + ci : r;
  dst[(size_t)k * O + o] = src[i];
}

// ------------------------------------------------------------------------------------------ the weight table
struct CnnWeight {
  char name[48];
  int O, K;        // a convolution (O, in, kh, kw): K = in kh kw; a vector of O values: K = 1
  int T;           // 9: a 3 x 3 convolution of the encoder, packed tap-major; 1: packed in its own k order
  size_t off;      // in floats, in the packed image
};
struct CnnTable {
  CnnWeight w[NLC_DFNET_NUM_WEIGHTS];
  int n;
  size_t total;    // floats
};
// indices into the table
constexpr int W_CONV1 = 0, W_BN1 = 1, W_DEC = 48, W_OUTCONV = 64, W_DS0 = 66, W_DS2 = 68, W_CONVOUT = 70;
constexpr int w_block(int layer, int blk) { return 3 + 15 * (layer - 1) + 9 * blk; }   // conv1, bn1.w, bn1.b, conv2, bn2.w, bn2.b [, down.0, down.1.w, down.1.b]

CnnTable make_table() {
  CnnTable t;
  t.n = 0;
  t.total = 0;
  auto add = [&](const char* name, int O, int K) {
    CnnWeight& w = t.w[t.n++];
    snprintf(w.name, sizeof w.name, "%s", name);
    w.O = O; w.K = K; w.T = 1; w.off = t.total;
    t.total += nl_align_up((size_t)O * K, 64);
  };
  char nm[64];
  auto addf = [&](const char* pre, const char* leaf, int O, int K, int T = 1) {
    snprintf(nm, sizeof nm, "%s%s", pre, leaf);
    add(nm, O, K);
    t.w[t.n - 1].T = T;
  };
  add("fuse_net.conv1.weight", 32, 12 * 64);
  add("fuse_net.bn1.weight", 32, 1);
  add("fuse_net.bn1.bias", 32, 1);
  for (int L = 1; L <= 3; ++L) {
    const int C = 32 << (L - 1), Cprev = L == 1 ? 32 : C / 2;
    for (int blk = 0; blk < 2; ++blk) {
      const int cin = blk == 0 ? Cprev : C;
      char pre[32];
      snprintf(pre, sizeof pre, "fuse_net.layer%d.%d.", L, blk);
      addf(pre, "conv1.weight", C, cin * 9, 9); addf(pre, "bn1.weight", C, 1); addf(pre, "bn1.bias", C, 1);
      addf(pre, "conv2.weight", C, C * 9, 9); addf(pre, "bn2.weight", C, 1); addf(pre, "bn2.bias", C, 1);
      if (blk == 0) { addf(pre, "downsample.0.weight", C, cin); addf(pre, "downsample.1.weight", C, 1); addf(pre, "downsample.1.bias", C, 1); }
    }
  }
  const struct { const char* pre; int cin, cout; } dec[4] = {{"fuse_net.upconv3.conv.", 128, 64}, {"fuse_net.iconv3.", 128, 64},
                                                             {"fuse_net.upconv2.conv.", 64, 32}, {"fuse_net.iconv2.", 64, 32}};
  for (int j = 0; j < 4; ++j) {
    addf(dec[j].pre, "conv.weight", dec[j].cout, dec[j].cin * 9, 9); addf(dec[j].pre, "conv.bias", dec[j].cout, 1);
    addf(dec[j].pre, "bn.weight", dec[j].cout, 1); addf(dec[j].pre, "bn.bias", dec[j].cout, 1);
  }
  add("fuse_net.out_conv.weight", 32, 32); add("fuse_net.out_conv.bias", 32, 1);
  add("depth_skip.0.weight", 8, 4); add("depth_skip.0.bias", 8, 1);
  add("depth_skip.2.weight", 16, 32); add("depth_skip.2.bias", 16, 1);
  add("conv_out.weight", 32, 48); add("conv_out.bias", 32, 1);
  return t;
}
const CnnTable& table() {
  static const CnnTable t = make_table();
  return t;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

bool shape_ok(int V, int H, int W) {
  return V >= 1 && V <= NLC_DFNET_MAX_VIEWS && H >= NLC_DFNET_MIN_SIDE && W >= NLC_DFNET_MIN_SIDE && H % 16 == 0 && W % 16 == 0 &&
         (int64_t)V * H * W <= NLC_DFNET_MAX_PIXELS;
}

// ------------------------------------------------------------------------------------------ the workspace (offsets in floats; every buffer 256-byte aligned)
struct CnnPlan {
  size_t c0, nc0;
  size_t a[3], b[3], d[3], y[3], x[3];          // per layer: the two raw maps of a block, the raw downsample map, block 0's output, the layer's output
  size_t na[3][2], nb[3][2], nd[3];             // their InstanceNorms (per block)
  size_t up3, u3, i3, up2, u2, i2, nu3, ni3, nu2, ni2;   // up3, up2: the bilinear x 2 of x3 and of i3
  size_t total;
};
CnnPlan make_plan(int V, int H, int W) {
  CnnPlan p;
  size_t at = 0;
  auto take = [&](size_t floats) { const size_t o = at; at += nl_align_up(floats, 64); return o; };
  const size_t n0 = (size_t)(H / 2 - 1) * (W / 2 - 1), n1 = (size_t)(H / 4) * (W / 4);
  p.c0 = take(V * 32 * n0); p.nc0 = take((size_t)V * 32 * 4);
  for (int L = 0; L < 3; ++L) {
    const size_t C = 32u << L, m = (size_t)V * C * (n1 >> (2 * L));
    p.a[L] = take(m); p.b[L] = take(m); p.d[L] = take(m); p.y[L] = take(m); p.x[L] = take(m);
    for (int blk = 0; blk < 2; ++blk) { p.na[L][blk] = take(V * C * 4); p.nb[L][blk] = take(V * C * 4); }
    p.nd[L] = take(V * C * 4);
  }
  p.up3 = take(V * 128 * (n1 / 4)); p.up2 = take(V * 64 * n1);
  p.u3 = take(V * 64 * (n1 / 4)); p.i3 = take(V * 64 * (n1 / 4)); p.u2 = take(V * 32 * n1); p.i2 = take(V * 32 * n1);
  p.nu3 = take((size_t)V * 64 * 4); p.ni3 = take((size_t)V * 64 * 4); p.nu2 = take((size_t)V * 32 * 4); p.ni2 = take((size_t)V * 32 * 4);
  p.total = at;
  return p;
}

template <int KS, int NB>
void launch_conv(const CnnConvArgs& a, int V, hipStream_t s) {
  hipLaunchKernelGGL((cnn_conv_kernel<KS, NB>), dim3((unsigned)nl_cdiv((int64_t)a.ho * a.wo, CNN_TP), (unsigned)V, (unsigned)(a.cout / (32 * NB))), dim3(CNN_THREADS),
                     0, s, a);
}
// Every output element is the same sum in the same order whichever way the output channels are dealt to workgroups, so the split may follow the size of the
// launch: all channels in one workgroup (the input is gathered once) where that still gives CNN_MIN_WGS workgroups, else 64 or 32 channels per workgroup.
constexpr int64_t CNN_MIN_WGS = 512;
// false: no kernel for this k
bool conv(const CnnConvArgs& a, int ks, int V, hipStream_t s) {
  const int64_t tiles = nl_cdiv((int64_t)a.ho * a.wo, CNN_TP) * V;
  int nb = a.cout / 32;
  while (nb > 1 && tiles * (a.cout / (32 * nb)) < CNN_MIN_WGS) nb /= 2;
#define CNN_CASE(KS, NB) if (ks == KS && nb == NB) { launch_conv<KS, NB>(a, V, s); return true; }
  CNN_CASE(8, 1) CNN_CASE(3, 1) CNN_CASE(3, 2) CNN_CASE(3, 4) CNN_CASE(1, 1) CNN_CASE(1, 2) CNN_CASE(1, 4)
#undef CNN_CASE
  return false;
}

}  // namespace

#endif
