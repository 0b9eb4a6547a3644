// libnerfloc_backbone.so — the 2-D backbone: ResNet-50 to layer2 with frozen BatchNorm + the two-level FPN (include/nerfloc_backbone.h is the contract; this file
// is its only unit).
//
// Six kernels make the whole chain:
//   bb_conv_kernel<KS, NB>        implicit-GEMM convolution on v_mfma_f32_32x32x2_f32, the tiling of cnn.hip's convolution: a workgroup (4 waves) owns 128
//                                 consecutive output pixels of ONE view and 32 NB output channels; wave w owns pixels 32 w .. 32 w + 31.  The weights are the A
//                                 operand (rows = output channels), the gathered input patches the B operand (columns = pixels): an accumulator register holds one
//                                 channel of 32 consecutive pixels across the lanes, and the NCHW store is 128 contiguous bytes per half-wave.  K is walked in
//                                 steps of 32: the next step's operands are fetched into registers under the current step's MFMAs, then go through LDS
//                                 ([k][pixel] and [k][channel]).  The gather pads with zeros; conv1 (KS == 7) normalises the image as it loads it.  The epilogue
//                                 is the rest of the layer: frozen BN as one multiply and one add, the residual add, ReLU, and a second store for a tap.
//   bb_conv3_kernel<KS, NB>       the same tile and epilogue for NLB_PRECISION_BF16X3: three v_mfma_f32_32x32x16_bf16 per 16 k on split-bf16 operands.
//   bb_pool_kernel                ReLU(BN(conv1)) and the 3 x 3 stride-2 max-pool in one pass over the raw conv1 map.
//   bb_in_kernel                  InstanceNorm of the FPN: one workgroup per (view, channel) plane, mean, then squared deviations from that mean, then the
//                                 normalised plane (in place or to the output), with the nearest-neighbour top-down term added where the level has one.
//   bb_nhwc_kernel                the channels-last write of an FPN output: 32 x 32 tiles through LDS, both sides coalesced.
//   bb_pack_conv_kernel, bb_pack_split_kernel, bb_fold_bn_kernel   the packed image.
#include <stdio.h>
#include <string.h>

#include "common.h"
#include "mfma.h"
#include "../../include/nerfloc_backbone.h"

namespace {

constexpr int BB_THREADS = 256;
constexpr int BB_TP = 128;           // output pixels per workgroup
constexpr int BB_BK = 32;            // k per step
constexpr int BB_XS = BB_TP + 32;    // LDS row stride of the pixel operand: the two half-waves (k, k + 1) then read different banks
constexpr float BB_EPS = 1e-5f;
constexpr int BB_CONV1_K = 147;      // 3 x 7 x 7; the packed image pads it to 160 rows

typedef float bb_f32x16 __attribute__((ext_vector_type(16)));

struct BbConvArgs {
  const float* x;       // (V, cin, hin, win)
  const float* wt;      // [K][cout], K a multiple of 32
  const unsigned short* w3;   // the split-bf16 planes of the same matrix: hi, then lo K cout values further, each [K / 8][cout][8] (bb_conv3_kernel)
  const float* sb;      // scale[cout], bias[cout] of the folded BN; null: raw sums
  const float* idn;     // (V, cout, ho, wo) added after the BN; null: none
  float* y;             // (V, cout, ho, wo)
  float* y2;            // a second copy of y (a tap); null: none
  int cin, cout, K;
  int hin, win, ho, wo, stride, pad;
  int relu;
};

__device__ __forceinline__ float bb_relu(float x) { return x < 0.f ? 0.f : x; }   // a NaN stays a NaN

// The rest of the layer on a workgroup's accumulators: frozen BN as one multiply and one add, the residual add, ReLU, the store(s).
// C/D layout of the 32 x 32 MFMAs: column (pixel) = lane & 31, row (channel) = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5)
template <int NB>
__device__ __forceinline__ void bb_epilogue(const BbConvArgs& a, const bb_f32x16 (&acc)[NB], int v, int c0, int npix) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int Po = blockIdx.x * BB_TP + 32 * wave + (lane & 31);
  if (Po >= npix) return;
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ch = c0 + 32 * cb + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
      const size_t at = ((size_t)v * a.cout + ch) * npix + Po;
      float val = acc[cb][r];
      if (a.sb) {
        val = val * a.sb[ch];
        val = val + a.sb[a.cout + ch];
      }
      if (a.idn) val = val + a.idn[at];
      if (a.relu) val = bb_relu(val);
      a.y[at] = val;
      if (a.y2) a.y2[at] = val;
    }
}

template <int KS, int NB>
__global__ __launch_bounds__(BB_THREADS) void bb_conv_kernel(const BbConvArgs a) {
  constexpr int COUT = 32 * NB;                   // the output channels of this workgroup: blockIdx.z * COUT ..
  constexpr int WSR = NB == 1 ? 32 : COUT + 32;   // LDS row stride of the weight operand (half-waves on different banks)
  __shared__ float Xs[BB_BK][BB_XS];
  __shared__ __attribute__((aligned(16))) float Ws[BB_BK][WSR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int v = blockIdx.y, c0 = blockIdx.z * COUT;
  const int npix = a.ho * a.wo, npl = a.hin * a.win;

  // the gather: this thread stages pixel p of the tile for k = kq, kq + 2, ..., kq + 30 of every step.  For KS == 1, 3 a step of 32 k is ONE tap (ky, kx) and 32
  // consecutive input channels, so the border test is done once per step; conv1 decodes (in, ky, kx) per value (five steps in all).
  const int p = tid & (BB_TP - 1), kq = tid >> 7;
  const int P = blockIdx.x * BB_TP + p;
  const bool pix_ok = P < npix;
  const int oy = pix_ok ? P / a.wo : 0, ox = pix_ok ? P % a.wo : 0;
  const int by = oy * a.stride - a.pad, bx = ox * a.stride - a.pad;

  float xreg[BB_BK / 2];
  float4 w0, w1, w2, w3;   // 32 x COUT floats per step over 256 threads: NB float4 each (named, not an array: they must stay in registers)
  w0 = w1 = w2 = w3 = make_float4(0.f, 0.f, 0.f, 0.f);
  int pf_tap = 0, pf_c = 0;   // the tap and first channel of the step the next prefetch fetches (KS != 7)

  auto prefetch = [&](int k0) {
    if constexpr (KS == 7) {
#pragma unroll
      for (int i = 0; i < BB_BK / 2; ++i) {
        const int k = k0 + kq + 2 * i;
        const int ci = k / 49, r = k - 49 * ci, ky = r / 7, kx = r - 7 * ky;
        const int iy = by + ky, ix = bx + kx;
        float val = 0.f;
        if (pix_ok && k < BB_CONV1_K && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) {
          const float mean = ci == 0 ? 0.485f : ci == 1 ? 0.456f : 0.406f, sd = ci == 0 ? 0.229f : ci == 1 ? 0.224f : 0.225f;
          val = (a.x[((size_t)v * 3 + ci) * npl + (size_t)iy * a.win + ix] - mean) / sd;
        }
        xreg[i] = val;
      }
    } else {
      const int ky = pf_tap / KS, kx = pf_tap - ky * KS;
      const int iy = by + ky, ix = bx + kx;
      if (pix_ok && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) {
        const size_t plane0 = (size_t)v * a.cin + pf_c + kq;
        const size_t off = (size_t)iy * a.win + ix;
#pragma unroll
        for (int i = 0; i < BB_BK / 2; ++i) xreg[i] = a.x[(plane0 + 2 * i) * npl + off];
      } else {
#pragma unroll
        for (int i = 0; i < BB_BK / 2; ++i) xreg[i] = 0.f;
      }
      pf_c += BB_BK;
      if (pf_c == a.cin) { pf_c = 0; ++pf_tap; }
    }
    // row r of the step's weight tile: COUT floats at wt[(k0 + r) cout + c0]
    auto wload = [&](int idx) { return *(const float4*)(a.wt + (size_t)(k0 + idx / (COUT / 4)) * a.cout + c0 + 4 * (idx % (COUT / 4))); };
    w0 = wload(tid);
    if constexpr (NB >= 2) w1 = wload(tid + BB_THREADS);
    if constexpr (NB == 4) { w2 = wload(tid + 2 * BB_THREADS); w3 = wload(tid + 3 * BB_THREADS); }
  };

  bb_f32x16 acc[NB];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;

  prefetch(0);
  for (int k0 = 0; k0 < a.K; k0 += BB_BK) {
#pragma unroll
    for (int i = 0; i < BB_BK / 2; ++i) Xs[kq + 2 * i][p] = xreg[i];
    auto wstore = [&](int idx, const float4& val) { *(float4*)&Ws[idx / (COUT / 4)][4 * (idx % (COUT / 4))] = val; };
    wstore(tid, w0);
    if constexpr (NB >= 2) wstore(tid + BB_THREADS, w1);
    if constexpr (NB == 4) { wstore(tid + 2 * BB_THREADS, w2); wstore(tid + 3 * BB_THREADS, w3); }
    __syncthreads();
    if (k0 + BB_BK < a.K) prefetch(k0 + BB_BK);
#pragma unroll
    for (int ks = 0; ks < BB_BK / 2; ++ks) {
      const int kk = 2 * ks + (lane >> 5);
      const float bv = Xs[kk][32 * wave + (lane & 31)];
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(Ws[kk][32 * cb + (lane & 31)], bv, acc[cb], 0, 0, 0);
    }
    __syncthreads();
  }

  bb_epilogue<NB>(a, acc, v, c0, npix);
}

// The same tile on v_mfma_f32_32x32x16_bf16 with three-term split-bf16 operands (KS == 1, 3): x = hi + lo with hi = bf16(x), lo = bf16(x - hi), and per 16 k
// acc += w_lo x_hi, then w_hi x_lo, then w_hi x_hi (the lo lo term, 2^-16 of the product, is dropped); accumulation, epilogue and output are fp32 as above.
// The weights come pre-split from the packed image, already in fragment order (a lane's 8 k of one channel are 16 contiguous bytes, a half-wave's 32 channels
// 512), so they go from global memory straight to registers; the activations are split as they are staged: a thread gathers 16 consecutive k of one pixel,
// splits them pairwise and writes the hi and the lo row of that pixel to LDS ([pixel][k], 80-byte rows: a half-wave's 16-byte reads fall on distinct banks).
template <int KS, int NB>
__global__ __launch_bounds__(BB_THREADS) void bb_conv3_kernel(const BbConvArgs a) {
  constexpr int COUT = 32 * NB;
  constexpr int XR = 40;   // 16-bit values per LDS row: 32 k + 8 of padding
  __shared__ __attribute__((aligned(16))) unsigned short Xh[BB_TP][XR];
  __shared__ __attribute__((aligned(16))) unsigned short Xl[BB_TP][XR];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, hh = lane >> 5;
  const int v = blockIdx.y, c0 = blockIdx.z * COUT;
  const int npix = a.ho * a.wo, npl = a.hin * a.win;

  // the gather: this thread stages k = 16 kh .. 16 kh + 15 of pixel p of every step; a step of 32 k is ONE tap and 32 consecutive input channels
  const int p = tid & (BB_TP - 1), kh = tid >> 7;
  const int P = blockIdx.x * BB_TP + p;
  const bool pix_ok = P < npix;
  const int oy = pix_ok ? P / a.wo : 0, ox = pix_ok ? P % a.wo : 0;
  const int by = oy * a.stride - a.pad, bx = ox * a.stride - a.pad;
  const unsigned short* wlo = a.w3 + (size_t)a.K * a.cout;

  float xreg[BB_BK / 2];
  int pf_tap = 0, pf_c = 0;
  auto prefetch = [&]() {
    const int ky = pf_tap / KS, kx = pf_tap - ky * KS;
    const int iy = by + ky, ix = bx + kx;
    if (pix_ok && iy >= 0 && iy < a.hin && ix >= 0 && ix < a.win) {
      const size_t plane0 = (size_t)v * a.cin + pf_c + 16 * kh;
      const size_t off = (size_t)iy * a.win + ix;
#pragma unroll
      for (int i = 0; i < BB_BK / 2; ++i) xreg[i] = a.x[(plane0 + i) * npl + off];
    } else {
#pragma unroll
      for (int i = 0; i < BB_BK / 2; ++i) xreg[i] = 0.f;
    }
    pf_c += BB_BK;
    if (pf_c == a.cin) { pf_c = 0; ++pf_tap; }
  };

  bb_f32x16 acc[NB];
#pragma unroll
  for (int cb = 0; cb < NB; ++cb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[cb][r] = 0.f;

  prefetch();
  for (int k0 = 0; k0 < a.K; k0 += BB_BK) {
    unsigned h[8], l[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) nl_split_pair<false>(xreg[2 * i], xreg[2 * i + 1], h[i], l[i]);
    *(uint4*)&Xh[p][16 * kh] = make_uint4(h[0], h[1], h[2], h[3]);
    *(uint4*)&Xh[p][16 * kh + 8] = make_uint4(h[4], h[5], h[6], h[7]);
    *(uint4*)&Xl[p][16 * kh] = make_uint4(l[0], l[1], l[2], l[3]);
    *(uint4*)&Xl[p][16 * kh + 8] = make_uint4(l[4], l[5], l[6], l[7]);
    // this lane's weight fragments of the step: k group (k0 / 8 + 2 s + hh), channel c0 + 32 cb + (lane & 31)
    uint4 wh[2][NB], wl[2][NB];
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        const size_t at = ((size_t)((k0 >> 3) + 2 * s + hh) * a.cout + c0 + 32 * cb + (lane & 31)) * 8;
        wh[s][cb] = *(const uint4*)(a.w3 + at);
        wl[s][cb] = *(const uint4*)(wlo + at);
      }
    __syncthreads();
    if (k0 + BB_BK < a.K) prefetch();
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      const nl_i16x8 xh = nl_frag(*(const uint4*)&Xh[32 * wave + (lane & 31)][16 * s + 8 * hh]);
      const nl_i16x8 xl = nl_frag(*(const uint4*)&Xl[32 * wave + (lane & 31)][16 * s + 8 * hh]);
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) {
        acc[cb] = nl_mfma<false>(nl_frag(wl[s][cb]), xh, acc[cb]);
        acc[cb] = nl_mfma<false>(nl_frag(wh[s][cb]), xl, acc[cb]);
        acc[cb] = nl_mfma<false>(nl_frag(wh[s][cb]), xh, acc[cb]);
      }
    }
    __syncthreads();
  }
  bb_epilogue<NB>(a, acc, v, c0, npix);
}

// grid (cdiv(h2 w2, 256), V 64): p0 = maxpool(3, 2, 1)(ReLU(x * scale + bias)) over the window's in-range pixels
__global__ __launch_bounds__(BB_THREADS) void bb_pool_kernel(const float* __restrict__ x, const float* __restrict__ sb, int h1, int w1, int h2, int w2,
                                                             float* __restrict__ y) {
  const size_t plane = blockIdx.y;
  const int c = (int)(plane & 63);
  const int i = blockIdx.x * BB_THREADS + threadIdx.x;
  if (i >= h2 * w2) return;
  const int oy = i / w2, ox = i - oy * w2;
  const float sc = sb[c], bi = sb[64 + c];
  const float* src = x + plane * h1 * w1;
  float m = 0.f;   // the window always holds its centre (2 oy, 2 ox), and a ReLU is never below 0
  bool nan = false;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = 2 * oy - 1 + ky, ix = 2 * ox - 1 + kx;
      if (iy < 0 || iy >= h1 || ix < 0 || ix >= w1) continue;
      float t = src[(size_t)iy * w1 + ix] * sc;
      t = bb_relu(t + bi);
      nan = nan || t != t;
      m = t > m ? t : m;
    }
  y[plane * h2 * w2 + i] = nan ? __builtin_nanf("") : m;
}

// the 256 threads' values added in a fixed tree; every thread gets the sum
__device__ __forceinline__ float bb_block_sum(float s, float* red) {
  const int tid = threadIdx.x;
  red[tid] = s;
  __syncthreads();
  for (int st = BB_THREADS / 2; st > 0; st >>= 1) {
    if (tid < st) red[tid] = red[tid] + red[tid + st];
    __syncthreads();
  }
  const float r = red[0];
  __syncthreads();
  return r;
}

// grid (C, V): plane (v, c) of x (V, C, h, w) -> dst = IN(x) [+ top[(y ht) / h][(x wt) / w] of top (V, C, ht, wt)]; dst may be x
__global__ __launch_bounds__(BB_THREADS) void bb_in_kernel(const float* x, int h, int w, const float* __restrict__ top, int ht, int wt, float* dst) {
  __shared__ float red[BB_THREADS];
  const int c = blockIdx.x, C = gridDim.x, v = blockIdx.y, tid = threadIdx.x, n = h * w;
  const size_t plane = (size_t)v * C + c;
  const float* p = x + plane * n;
  float* d = dst + plane * n;
  float s = 0.f;
  for (int i = tid; i < n; i += BB_THREADS) s += p[i];
  const float mean = bb_block_sum(s, red) / (float)n;
  float q = 0.f;
  for (int i = tid; i < n; i += BB_THREADS) {
    const float dv = p[i] - mean;
    q += dv * dv;
  }
  q = bb_block_sum(q, red);
  const float k = 1.f / sqrtf(q / (float)n + BB_EPS);
  const float* tp = top ? top + plane * ht * wt : nullptr;
  for (int i = tid; i < n; i += BB_THREADS) {
    float y = (p[i] - mean) * k;
    if (tp) {
      const int oy = i / w, ox = i - oy * w;
      y = y + tp[(oy * ht) / h * wt + (ox * wt) / w];
    }
    d[i] = y;
  }
}

// grid (cdiv(n, 32), C / 32, V): src (V, C, n) -> dst (V, n, C)
__global__ __launch_bounds__(BB_THREADS) void bb_nhwc_kernel(const float* __restrict__ src, int C, int n, float* __restrict__ dst) {
  __shared__ float t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int p0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  const size_t v = blockIdx.z;
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (p0 + tx < n) t[ty + 8 * j][tx] = src[(v * C + c0 + ty + 8 * j) * n + p0 + tx];
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (p0 + ty + 8 * j < n) dst[(v * n + p0 + ty + 8 * j) * C + c0 + tx] = t[tx][ty + 8 * j];
}

// dst[k][o] for k < Kpad: src[o][in][t] with k = t Cin + in (tap_major: the 3 x 3 convolutions) or k = in T + t (the source's own order), zero for k >= Cin T
__global__ __launch_bounds__(BB_THREADS) void bb_pack_conv_kernel(const float* __restrict__ src, float* __restrict__ dst, int O, int Cin, int T, int tap_major,
                                                                  int Kpad) {
  const int i = blockIdx.x * BB_THREADS + threadIdx.x;
  if (i >= Kpad * O) return;
  const int k = i / O, o = i - k * O;
  float val = 0.f;
  if (k < Cin * T) {
    const int r = tap_major ? (k % Cin) * T + k / Cin : k;
    val = src[(size_t)o * Cin * T + r];
  }
  dst[i] = val;
}

// the split-bf16 planes of a convolution: element (k, o) of the [k][out] matrix at ((k / 8) O + o) 8 + k % 8 of hi and of lo
__global__ __launch_bounds__(BB_THREADS) void bb_pack_split_kernel(const float* __restrict__ src, unsigned short* __restrict__ hi, unsigned short* __restrict__ lo,
                                                                   int O, int Cin, int T, int tap_major) {
  const int i = blockIdx.x * BB_THREADS + threadIdx.x;
  if (i >= Cin * T * O) return;
  const int k = i / O, o = i - k * O;
  const int r = tap_major ? (k % Cin) * T + k / Cin : k;
  nl_store_split(src[(size_t)o * Cin * T + r], ((size_t)(k >> 3) * O + o) * 8 + (k & 7), hi, lo, nullptr, nullptr);
}

// dst = scale[O], bias[O] of a frozen BatchNorm
__global__ __launch_bounds__(BB_THREADS) void bb_fold_bn_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ m,
                                                                const float* __restrict__ var, float* __restrict__ dst, int O) {
  const int o = blockIdx.x * BB_THREADS + threadIdx.x;
  if (o >= O) return;
  const float scale = w[o] * (1.f / sqrtf(var[o] + BB_EPS));
  dst[o] = scale;
  dst[O + o] = b[o] - m[o] * scale;
}

// ------------------------------------------------------------------------------------------ the weight table
enum { BB_CONV = 0, BB_BN = 1, BB_BN_REST = 2 };   // a convolution; a BN's `weight` (it owns the folded slot); its bias, running_mean, running_var
struct BbWeight {
  char name[48];
  int kind;
  int O, Cin, T, Kpad;   // a convolution (O, Cin, kh, kw): T = kh kw, Kpad rows in the packed image; a BN: O channels
  size_t off;            // in floats, in the packed image
  size_t off3;           // a 1 x 1 or 3 x 3 convolution: its split-bf16 planes (hi, lo: K O 16-bit values each = K O floats in all)
};
struct BbBlock { int c1, b1, c2, b2, c3, b3, dn, dbn; };   // indices into the table; dn = -1: no downsample
struct BbTable {
  BbWeight w[NLB_BACKBONE_NUM_WEIGHTS];
  int n;
  size_t total;    // floats
  int conv1, bn1;
  BbBlock l1[3], l2[4];
  int inner[2], layer[2];
};

bool fpn_ok(int F) { return F == 64 || F == 128 || F == 192 || F == 256; }

BbTable make_table(int F) {
  BbTable t;
  t.n = 0;
  t.total = 0;
  auto conv = [&](const char* pre, const char* leaf, int O, int Cin, int T) {
    BbWeight& w = t.w[t.n];
    snprintf(w.name, sizeof w.name, "%s%s", pre, leaf);
    w.kind = BB_CONV; w.O = O; w.Cin = Cin; w.T = T;
    w.Kpad = (int)nl_align_up((size_t)Cin * T, BB_BK);
    w.off = t.total;
    t.total += nl_align_up((size_t)w.Kpad * O, 64);
    w.off3 = t.total;
    if (T != 49) t.total += nl_align_up((size_t)w.Kpad * O, 64);
    return t.n++;
  };
  auto bn = [&](const char* pre, const char* leaf, int O) {
    static const char* const member[4] = {"weight", "bias", "running_mean", "running_var"};
    const int first = t.n;
    for (int j = 0; j < 4; ++j) {
      BbWeight& w = t.w[t.n++];
      snprintf(w.name, sizeof w.name, "%s%s.%s", pre, leaf, member[j]);
      w.kind = j == 0 ? BB_BN : BB_BN_REST; w.O = O; w.Cin = 1; w.T = 1; w.Kpad = 0;
      w.off = w.off3 = t.total;
    }
    t.total += nl_align_up((size_t)2 * O, 64);
    return first;
  };
  t.conv1 = conv("body.", "conv1.weight", 64, 3, 49);
  t.bn1 = bn("body.", "bn1", 64);
  int inplanes = 64;
  for (int L = 1; L <= 2; ++L) {
    const int planes = 64 * L, nblk = L == 1 ? 3 : 4;
    for (int b = 0; b < nblk; ++b) {
      char pre[32];
      snprintf(pre, sizeof pre, "body.layer%d.%d.", L, b);
      BbBlock& k = L == 1 ? t.l1[b] : t.l2[b];
      k.c1 = conv(pre, "conv1.weight", planes, inplanes, 1); k.b1 = bn(pre, "bn1", planes);
      k.c2 = conv(pre, "conv2.weight", planes, planes, 9); k.b2 = bn(pre, "bn2", planes);
      k.c3 = conv(pre, "conv3.weight", 4 * planes, planes, 1); k.b3 = bn(pre, "bn3", 4 * planes);
      k.dn = k.dbn = -1;
      if (b == 0) { k.dn = conv(pre, "downsample.0.weight", 4 * planes, inplanes, 1); k.dbn = bn(pre, "downsample.1", 4 * planes); }
      inplanes = 4 * planes;
    }
  }
  t.inner[0] = conv("fpn.", "inner_blocks.0.0.weight", F, 256, 1);
  t.inner[1] = conv("fpn.", "inner_blocks.1.0.weight", F, 512, 1);
  t.layer[0] = conv("fpn.", "layer_blocks.0.0.weight", F, F, 9);
  t.layer[1] = conv("fpn.", "layer_blocks.1.0.weight", F, F, 9);
  return t;
}
// one table per fpn_dim (F / 64 - 1); built once each
const BbTable& table(int F) {
  static const BbTable t[4] = {make_table(64), make_table(128), make_table(192), make_table(256)};
  return t[F / 64 - 1];
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

bool shape_ok(int V, int H, int W) {
  return V >= 1 && V <= NLB_BACKBONE_MAX_VIEWS && H >= NLB_BACKBONE_MIN_SIDE && W >= NLB_BACKBONE_MIN_SIDE && (int64_t)V * H * W <= NLB_BACKBONE_MAX_PIXELS;
}
int half_up(int n) { return (n - 1) / 2 + 1; }

// ------------------------------------------------------------------------------------------ the workspace (offsets in floats; every buffer 256-byte aligned)
struct BbPlan {
  size_t p0;                 // (V, 64, n2)
  size_t a1, b1;             // layer1: the two 64-channel maps of a block
  size_t d1, x1[2];          // layer1: block 0's identity, the blocks' outputs in turn (256 channels)
  size_t a2, b2;             // layer2: 128 channels at n2 (block 0's first map only), at n3
  size_t d2, x2[2];          // layer2: 512 channels at n3
  size_t i2, r2, i1, r1;     // FPN: the inner and the result maps of level layer2 (n3) and layer1 (n2)
  size_t total;
};
BbPlan make_plan(int V, int H, int W, int F) {
  BbPlan p;
  size_t at = 0;
  auto take = [&](size_t floats) { const size_t o = at; at += nl_align_up(floats, 64); return o; };
  const int h2 = half_up(half_up(H)), w2 = half_up(half_up(W)), h3 = half_up(h2), w3 = half_up(w2);
  const size_t n2 = (size_t)V * h2 * w2, n3 = (size_t)V * h3 * w3;
  p.p0 = take(64 * n2);
  p.a1 = take(64 * n2); p.b1 = take(64 * n2);
  p.d1 = take(256 * n2); p.x1[0] = take(256 * n2); p.x1[1] = take(256 * n2);
  p.a2 = take(128 * n2); p.b2 = take(128 * n3);
  p.d2 = take(512 * n3); p.x2[0] = take(512 * n3); p.x2[1] = take(512 * n3);
  p.i2 = take(F * n3); p.r2 = take(F * n3); p.i1 = take(F * n2); p.r1 = take(F * n2);
  p.total = at;
  return p;
}

template <int KS, int NB>
void launch_conv3(const BbConvArgs& a, int V, hipStream_t s) {
  hipLaunchKernelGGL((bb_conv3_kernel<KS, NB>), dim3((unsigned)nl_cdiv((int64_t)a.ho * a.wo, BB_TP), (unsigned)V, (unsigned)(a.cout / (32 * NB))), dim3(BB_THREADS), 0,
                     s, a);
}
template <int KS, int NB>
void launch_conv(const BbConvArgs& a, int V, hipStream_t s) {
  hipLaunchKernelGGL((bb_conv_kernel<KS, NB>), dim3((unsigned)nl_cdiv((int64_t)a.ho * a.wo, BB_TP), (unsigned)V, (unsigned)(a.cout / (32 * NB))), dim3(BB_THREADS), 0,
                     s, a);
}
// Every output element is the same sum in the same order whichever way the output channels are dealt to workgroups, so the split may follow the size of the
// launch: 128 channels per workgroup (the input is gathered once per 128) where that still gives BB_MIN_WGS workgroups, else 64 or 32.
constexpr int64_t BB_MIN_WGS = 512;
// false: no kernel for this k
bool conv(const BbConvArgs& a, int ks, bool split, int V, hipStream_t s) {
  const int64_t tiles = nl_cdiv((int64_t)a.ho * a.wo, BB_TP) * V;
  const int c32 = a.cout / 32;
  int nb = c32 % 4 == 0 ? 4 : c32 % 2 == 0 ? 2 : 1;
  if (ks == 7 && nb > 2) nb = 2;
  while (nb > 1 && tiles * (c32 / nb) < BB_MIN_WGS) nb /= 2;
#define BB_CASE3(KS, NB) if (split && ks == KS && nb == NB) { launch_conv3<KS, NB>(a, V, s); return true; }
  BB_CASE3(3, 1) BB_CASE3(3, 2) BB_CASE3(3, 4) BB_CASE3(1, 1) BB_CASE3(1, 2) BB_CASE3(1, 4)
#undef BB_CASE3
#define BB_CASE(KS, NB) if (ks == KS && nb == NB) { launch_conv<KS, NB>(a, V, s); return true; }
  BB_CASE(7, 1) BB_CASE(7, 2) BB_CASE(3, 1) BB_CASE(3, 2) BB_CASE(3, 4) BB_CASE(1, 1) BB_CASE(1, 2) BB_CASE(1, 4)
#undef BB_CASE
  return false;
}

}  // namespace

extern "C" {

int nlb_abi_version(void) { return NLB_ABI_VERSION; }

int nlb_backbone_num_weights(int fpn_dim) { return fpn_ok(fpn_dim) ? NLB_BACKBONE_NUM_WEIGHTS : 0; }

const char* nlb_backbone_weight_name(int i) { return i >= 0 && i < NLB_BACKBONE_NUM_WEIGHTS ? table(64).w[i].name : nullptr; }

size_t nlb_backbone_packed_bytes(int fpn_dim) { return fpn_ok(fpn_dim) ? nl_align_up(table(fpn_dim).total * sizeof(float), 256) : 0; }

int nlb_backbone_pack_weights(const void* const* ptrs, int n, int fpn_dim, void* packed, size_t packed_bytes, void* stream) {
  if (!fpn_ok(fpn_dim)) return NL_ERR_UNSUPPORTED;
  const BbTable& t = table(fpn_dim);
  if (!ptrs || n != t.n) return NL_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i)
    if (!ptrs[i] || !aligned(ptrs[i], 4)) return NL_ERR_BAD_ARG;
  if (!packed || !aligned(packed, 256) || packed_bytes < nlb_backbone_packed_bytes(fpn_dim)) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n; ++i) {
    const BbWeight& w = t.w[i];
    float* dst = (float*)packed + w.off;
    if (w.kind == BB_CONV) {
      hipLaunchKernelGGL(bb_pack_conv_kernel, dim3((unsigned)nl_cdiv((int64_t)w.Kpad * w.O, BB_THREADS)), dim3(BB_THREADS), 0, s, (const float*)ptrs[i], dst, w.O,
                         w.Cin, w.T, w.T == 9 ? 1 : 0, w.Kpad);
      NL_LAUNCH_CHECK();
      if (w.T != 49) {
        unsigned short* hi = (unsigned short*)((float*)packed + w.off3);
        hipLaunchKernelGGL(bb_pack_split_kernel, dim3((unsigned)nl_cdiv((int64_t)w.Kpad * w.O, BB_THREADS)), dim3(BB_THREADS), 0, s, (const float*)ptrs[i], hi,
                           hi + (size_t)w.Kpad * w.O, w.O, w.Cin, w.T, w.T == 9 ? 1 : 0);
        NL_LAUNCH_CHECK();
      }
    } else if (w.kind == BB_BN) {
      hipLaunchKernelGGL(bb_fold_bn_kernel, dim3((unsigned)nl_cdiv(w.O, BB_THREADS)), dim3(BB_THREADS), 0, s, (const float*)ptrs[i], (const float*)ptrs[i + 1],
                         (const float*)ptrs[i + 2], (const float*)ptrs[i + 3], dst, w.O);
      NL_LAUNCH_CHECK();
    }
  }
  return NL_OK;
}

size_t nlb_backbone_workspace_bytes(int V, int H, int W, int fpn_dim) {
  if (!shape_ok(V, H, W) || !fpn_ok(fpn_dim)) return 0;
  return nl_align_up(make_plan(V, H, W, fpn_dim).total * sizeof(float), 256);
}

int nlb_backbone_forward(const void* packed, const float* imgs, int V, int H, int W, int fpn_dim, int precision, int layout, float* conv1_out, float* p_layer1,
                         float* p_layer2, const nlb_backbone_taps* taps, void* ws, size_t ws_bytes, void* stream) {
  if (precision != NLB_PRECISION_FP32 && precision != NLB_PRECISION_BF16X3) return NL_ERR_BAD_ARG;
  if (layout != NLB_LAYOUT_NCHW && layout != NLB_LAYOUT_CHANNELS_LAST) return NL_ERR_BAD_ARG;
  if (!shape_ok(V, H, W) || !fpn_ok(fpn_dim)) return NL_ERR_UNSUPPORTED;
  if (!packed || !imgs || !conv1_out || !p_layer1 || !p_layer2 || !aligned(packed, 256) || !aligned(imgs, 4) || !aligned(conv1_out, 4) || !aligned(p_layer1, 4) ||
      !aligned(p_layer2, 4))
    return NL_ERR_BAD_ARG;
  if (taps && (!aligned(taps->layer1, 4) || !aligned(taps->layer2, 4))) return NL_ERR_BAD_ARG;
  if (!ws || !aligned(ws, 256) || ws_bytes < nlb_backbone_workspace_bytes(V, H, W, fpn_dim)) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int F = fpn_dim;
  const BbTable& t = table(F);
  const BbPlan p = make_plan(V, H, W, F);
  const float* pk = (const float*)packed;
  float* w = (float*)ws;
  auto wt = [&](int i) { return pk + t.w[i].off; };
  const int h1 = half_up(H), w1 = half_up(W), h2 = half_up(h1), w2 = half_up(w1), h3 = half_up(h2), w3 = half_up(w2);
  const bool nhwc = layout == NLB_LAYOUT_CHANNELS_LAST;
  int launches = 0;

  // one convolution with its epilogue: x (V, cin, hin, win) -> y (V, cout, ho, wo); bnidx < 0: raw sums
  auto run_conv = [&](const float* x, int hin, int win, int widx, int ks, int stride, int bnidx, const float* idn, int relu, float* y, float* y2) -> int {
    const BbWeight& cw = t.w[widx];
    BbConvArgs a;
    a.x = x; a.wt = wt(widx); a.w3 = (const unsigned short*)(pk + cw.off3); a.sb = bnidx < 0 ? nullptr : wt(bnidx); a.idn = idn; a.y = y; a.y2 = y2;
    a.cin = cw.Cin; a.cout = cw.O; a.K = cw.Kpad;
    a.hin = hin; a.win = win; a.stride = stride; a.pad = ks / 2;
    a.ho = (hin + 2 * a.pad - ks) / stride + 1;
    a.wo = (win + 2 * a.pad - ks) / stride + 1;
    a.relu = relu;
    if (!conv(a, ks, precision == NLB_PRECISION_BF16X3 && ks != 7, V, s)) return NL_ERR_UNSUPPORTED;
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  // x (V, F, h, w) -> dst = IN(x) [+ up(top)]
  auto run_in = [&](const float* x, int h, int wd, const float* top, int ht, int wtop, float* dst) -> int {
    hipLaunchKernelGGL(bb_in_kernel, dim3((unsigned)F, (unsigned)V), dim3(BB_THREADS), 0, s, x, h, wd, top, ht, wtop, dst);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  auto run_nhwc = [&](const float* src, int n, float* dst) -> int {
    hipLaunchKernelGGL(bb_nhwc_kernel, dim3((unsigned)nl_cdiv(n, 32), (unsigned)(F / 32), (unsigned)V), dim3(BB_THREADS), 0, s, src, F, n, dst);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
#define BB_TRY(expr) do { const int st_ = (expr); if (st_ != NL_OK) return st_; } while (0)

  // conv1 (raw), then BN + ReLU + max-pool
  BB_TRY(run_conv(imgs, H, W, t.conv1, 7, 2, -1, nullptr, 0, conv1_out, nullptr));
  hipLaunchKernelGGL(bb_pool_kernel, dim3((unsigned)nl_cdiv((int64_t)h2 * w2, BB_THREADS), (unsigned)(V * 64)), dim3(BB_THREADS), 0, s, conv1_out, wt(t.bn1), h1, w1,
                     h2, w2, w + p.p0);
  ++launches;
  NL_LAUNCH_CHECK();

  // layer1: three Bottlenecks at h2 x w2
  const float* x = w + p.p0;
  for (int b = 0; b < 3; ++b) {
    const BbBlock& k = t.l1[b];
    const float* idn = x;
    BB_TRY(run_conv(x, h2, w2, k.c1, 1, 1, k.b1, nullptr, 1, w + p.a1, nullptr));
    BB_TRY(run_conv(w + p.a1, h2, w2, k.c2, 3, 1, k.b2, nullptr, 1, w + p.b1, nullptr));
    if (k.dn >= 0) {
      BB_TRY(run_conv(x, h2, w2, k.dn, 1, 1, k.dbn, nullptr, 0, w + p.d1, nullptr));
      idn = w + p.d1;
    }
    float* y = w + p.x1[b & 1];
    BB_TRY(run_conv(w + p.b1, h2, w2, k.c3, 1, 1, k.b3, idn, 1, y, b == 2 && taps ? taps->layer1 : nullptr));
    x = y;
  }
  const float* x1 = x;

  // layer2: four Bottlenecks, the first to h3 x w3 (the stride sits on its 3 x 3 and on its downsample)
  for (int b = 0; b < 4; ++b) {
    const BbBlock& k = t.l2[b];
    const float* idn = x;
    const int hin = b == 0 ? h2 : h3, win = b == 0 ? w2 : w3, stride = b == 0 ? 2 : 1;
    BB_TRY(run_conv(x, hin, win, k.c1, 1, 1, k.b1, nullptr, 1, w + p.a2, nullptr));
    BB_TRY(run_conv(w + p.a2, hin, win, k.c2, 3, stride, k.b2, nullptr, 1, w + p.b2, nullptr));
    if (k.dn >= 0) {
      BB_TRY(run_conv(x, hin, win, k.dn, 1, stride, k.dbn, nullptr, 0, w + p.d2, nullptr));
      idn = w + p.d2;
    }
    float* y = w + p.x2[b & 1];
    BB_TRY(run_conv(w + p.b2, h3, w3, k.c3, 1, 1, k.b3, idn, 1, y, b == 3 && taps ? taps->layer2 : nullptr));
    x = y;
  }
  const float* x2 = x;

  // FPN, top level first
  BB_TRY(run_conv(x2, h3, w3, t.inner[1], 1, 1, -1, nullptr, 0, w + p.i2, nullptr));
  BB_TRY(run_in(w + p.i2, h3, w3, nullptr, 0, 0, w + p.i2));
  BB_TRY(run_conv(w + p.i2, h3, w3, t.layer[1], 3, 1, -1, nullptr, 0, w + p.r2, nullptr));
  BB_TRY(run_in(w + p.r2, h3, w3, nullptr, 0, 0, nhwc ? w + p.r2 : p_layer2));
  if (nhwc) BB_TRY(run_nhwc(w + p.r2, h3 * w3, p_layer2));
  BB_TRY(run_conv(x1, h2, w2, t.inner[0], 1, 1, -1, nullptr, 0, w + p.i1, nullptr));
  BB_TRY(run_in(w + p.i1, h2, w2, w + p.i2, h3, w3, w + p.i1));
  BB_TRY(run_conv(w + p.i1, h2, w2, t.layer[0], 3, 1, -1, nullptr, 0, w + p.r1, nullptr));
  BB_TRY(run_in(w + p.r1, h2, w2, nullptr, 0, 0, nhwc ? w + p.r1 : p_layer1));
  if (nhwc) BB_TRY(run_nhwc(w + p.r1, h2 * w2, p_layer1));
#undef BB_TRY
  return launches == NLB_BACKBONE_LAUNCHES - (nhwc ? 0 : 2) ? NL_OK : NL_ERR_HIP;
}

}  // extern "C"
