// libnerfloc_app.so (include/nerfloc_app.h states the contracts; tests/appearance_ref.py restates them in numpy): appearance adaptation.
//   nla_channel_stats   stats_nchw_kernel / stats_nhwc_kernel   one workgroup per plane segment: the segment's mean, then its sum of squared deviations from it
//                       stats_merge_kernel                      one wave per (image, channel): Chan's merge of the segments in a fixed order, mean and std out
//   nla_adapt_code      adapt_code_kernel                       one workgroup per view: the three layers, four threads per output value
//   nla_film            film_kernel                             y = a x + b (one multiply, one add), optionally clamped; a thread keeps ONE channel group, so a and b
//                                                               are loaded once per thread and no index is divided in the loop
//   nla_film_backward   film_bwd_kernel                         the same walk: g_x out, per-thread sums of m g x and m g, the workgroup's 2 C partial sums
//                       film_bwd_sum_kernel                     one thread per (view, channel): the partial sums added in ascending order
// All of it streams: the bound of every kernel is its bytes.  No atomics; every sum has a fixed order: two calls give the same bits.
#include "common.h"
#include "../../include/nerfloc_app.h"

namespace {

constexpr int APP_THREADS = 256;
constexpr int APP_MAX_C = 1024;
constexpr int APP_MAX_E = 512;
constexpr int64_t APP_MAX_HW_STATS = (int64_t)1 << 30;
constexpr int64_t APP_MAX_V = (int64_t)1 << 20;
constexpr int64_t APP_MAX_ELEMS = (int64_t)1 << 40;
constexpr int64_t APP_MAX_BLOCKS = ((int64_t)1 << 31) - 1;
constexpr int FILM_ITERS = 32;   // pixels per thread of the FiLM kernels' native mapping (nla_film_backward_block_pixels = rows per pass x this)

// sum over the workgroup's 256 threads, the same value in every thread: the wave tree, then the four waves in ascending order
__device__ __forceinline__ float block_sum(float v, float* sh4) {
  const float w = wave_sum(v);
  __syncthreads();   // sh4 may still be read from the previous call
  if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = w;
  __syncthreads();
  return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// ------------------------------------------------------------------------------------------------ channel statistics
// NCHW: workgroup blk = plane S + s owns the pixels [s SEG, s SEG + n) of plane (b, c), 16 values per thread in registers: ONE read of the data.
// VEC: HW % 4 == 0 and x 16-byte aligned, so every segment starts on a 16-byte boundary and n % 4 == 0.
template <bool VEC>
__global__ __launch_bounds__(APP_THREADS) void stats_nchw_kernel(const float* __restrict__ x, long long HW, int S, float* __restrict__ pmean, float* __restrict__ pm2) {
  __shared__ float sh4[4];
  constexpr int SEG = NLA_STATS_SEG_NCHW, PER = SEG / APP_THREADS;
  const long long blk = blockIdx.x, plane = blk / S, p0 = (blk % S) * SEG;
  const int n = (int)(HW - p0 < SEG ? HW - p0 : SEG), t = threadIdx.x;
  const float* src = x + plane * HW + p0;
  float v[PER];
  bool ok[PER];
  if (VEC) {
#pragma unroll
    for (int k = 0; k < PER / 4; ++k) {
      const int i = (k * APP_THREADS + t) * 4;
      const bool in = i < n;
      const float4 q = in ? *reinterpret_cast<const float4*>(src + i) : make_float4(0.f, 0.f, 0.f, 0.f);
      v[4 * k] = q.x; v[4 * k + 1] = q.y; v[4 * k + 2] = q.z; v[4 * k + 3] = q.w;
      ok[4 * k] = ok[4 * k + 1] = ok[4 * k + 2] = ok[4 * k + 3] = in;
    }
  } else {   // the same values in the same registers through 4-byte loads: the bits do not depend on which path a plane's alignment selects
#pragma unroll
    for (int k = 0; k < PER; ++k) {
      const int i = ((k / 4) * APP_THREADS + t) * 4 + (k & 3);
      ok[k] = i < n;
      v[k] = ok[k] ? src[i] : 0.f;
    }
  }
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) s += v[k];
  const float mean = block_sum(s, sh4) / (float)n;
  float m2 = 0.f;
#pragma unroll
  for (int k = 0; k < PER; ++k) {
    const float d = ok[k] ? v[k] - mean : 0.f;
    m2 += d * d;
  }
  m2 = block_sum(m2, sh4);
  if (t == 0) { pmean[blk] = mean; pm2[blk] = m2; }
}

struct F4 { float v[4]; };
template <bool VEC> struct StatsUnit;
template <> struct StatsUnit<true> {
  static constexpr int W = 4;
  static __device__ __forceinline__ F4 load(const float* p) { const float4 q = *reinterpret_cast<const float4*>(p); return F4{{q.x, q.y, q.z, q.w}}; }
};
template <> struct StatsUnit<false> {
  static constexpr int W = 1;
  static __device__ __forceinline__ F4 load(const float* p) { return F4{{*p, 0.f, 0.f, 0.f}}; }
};

// NHWC: workgroup blk = b S + s owns the pixels [s SEG, s SEG + n) of image b, all channels.  A thread keeps one channel unit (4 channels with VEC, else 1) and walks
// the pixels r, r + R, ...; the R threads of a unit are added through LDS in ascending r.  Two passes over the segment (at most SEG C 4 bytes = 1 MiB, from cache);
// KEEP (R >= 16, i.e. at most 16 channel units: 64 channels with VEC): the thread's at most SEG / 16 values stay in registers and the data is read ONCE.  The sums
// run in the same order either way.
constexpr int NHWC_KEEP = NLA_STATS_SEG_NHWC / 16;
template <bool VEC, bool KEEP>
__global__ __launch_bounds__(APP_THREADS) void stats_nhwc_kernel(const float* __restrict__ x, long long HW, int C, int S, float* __restrict__ pmean, float* __restrict__ pm2) {
  __shared__ float sh[APP_THREADS * 4];
  __shared__ float shm[APP_THREADS * 4];
  constexpr int SEG = NLA_STATS_SEG_NHWC, W = StatsUnit<VEC>::W;
  const long long blk = blockIdx.x, b = blk / S, s = blk % S, p0 = s * SEG;
  const int n = (int)(HW - p0 < SEG ? HW - p0 : SEG), t = threadIdx.x;
  const int CU = C / W, CW = CU < APP_THREADS ? CU : APP_THREADS, R = APP_THREADS / CW;
  const int cl = t % CW, r = t / CW;
  const float* img = x + (b * HW + p0) * C;
  for (int cb = 0; cb < CU; cb += CW) {   // uniform over the workgroup
    const int cu = cb + cl;
    const bool act = r < R && cu < CU;
    float acc[W];
#pragma unroll
    for (int j = 0; j < W; ++j) acc[j] = 0.f;
    F4 kept[KEEP ? NHWC_KEEP : 1];
    if constexpr (KEEP) {
#pragma unroll
      for (int k = 0; k < NHWC_KEEP; ++k) {
        const int p = r + k * R;
        if (act && p < n) kept[k] = StatsUnit<VEC>::load(img + (long long)p * C + cu * W);
      }
#pragma unroll
      for (int k = 0; k < NHWC_KEEP; ++k)
        if (act && r + k * R < n) {
#pragma unroll
          for (int j = 0; j < W; ++j) acc[j] += kept[k].v[j];
        }
    } else if (act) {
      for (int p = r; p < n; p += R) {
        const F4 q = StatsUnit<VEC>::load(img + (long long)p * C + cu * W);
#pragma unroll
        for (int j = 0; j < W; ++j) acc[j] += q.v[j];
      }
    }
    __syncthreads();   // the previous chunk's readers of sh / shm are done
#pragma unroll
    for (int j = 0; j < W; ++j) sh[t * 4 + j] = acc[j];
    __syncthreads();
    if (r == 0 && cu < CU) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        float tot = 0.f;
        for (int rr = 0; rr < R; ++rr) tot += sh[(rr * CW + cl) * 4 + j];
        shm[cl * 4 + j] = tot / (float)n;
      }
    }
    __syncthreads();
    float mean[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { mean[j] = shm[cl * 4 + j]; acc[j] = 0.f; }
    if constexpr (KEEP) {
#pragma unroll
      for (int k = 0; k < NHWC_KEEP; ++k)
        if (act && r + k * R < n) {
#pragma unroll
          for (int j = 0; j < W; ++j) { const float d = kept[k].v[j] - mean[j]; acc[j] += d * d; }
        }
    } else if (act) {
      for (int p = r; p < n; p += R) {
        const F4 q = StatsUnit<VEC>::load(img + (long long)p * C + cu * W);
#pragma unroll
        for (int j = 0; j < W; ++j) { const float d = q.v[j] - mean[j]; acc[j] += d * d; }
      }
    }
    __syncthreads();   // every thread has read its means and the totals' readers are done
#pragma unroll
    for (int j = 0; j < W; ++j) sh[t * 4 + j] = acc[j];
    __syncthreads();
    if (r == 0 && cu < CU) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        float tot = 0.f;
        for (int rr = 0; rr < R; ++rr) tot += sh[(rr * CW + cl) * 4 + j];
        const long long o = (b * C + cu * W + j) * S + s;
        pmean[o] = mean[j]; pm2[o] = tot;
      }
    }
  }
}

__device__ __forceinline__ void chan_merge(int& na, float& ma, float& qa, int nb, float mb, float qb) {
  if (nb == 0) return;
  if (na == 0) { na = nb; ma = mb; qa = qb; return; }
  const int n = na + nb;
  const float d = mb - ma, fn = (float)n;
  ma = ma + d * ((float)nb / fn);
  qa = (qa + qb) + (d * d) * ((float)na * (float)nb / fn);
  na = n;
}

// one wave per plane (b, c): lane l merges the segments l, l + 64, ... in ascending order, then the lanes merge l <- l + 32, 16, .., 1
__global__ __launch_bounds__(APP_THREADS) void stats_merge_kernel(const float* __restrict__ pmean, const float* __restrict__ pm2, long long planes, int C, long long HW, int S,
                                                                  int SEG, float* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const long long plane = (long long)blockIdx.x * (APP_THREADS / 64) + (threadIdx.x >> 6);
  if (plane >= planes) return;   // wave-uniform; no barrier below
  int n = 0;
  float mean = 0.f, m2 = 0.f;
  for (int s = lane; s < S; s += 64) {
    const long long left = HW - (long long)s * SEG;
    chan_merge(n, mean, m2, (int)(left < SEG ? left : SEG), pmean[plane * S + s], pm2[plane * S + s]);
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const int nb = __shfl_down(n, off);
    const float mb = __shfl_down(mean, off), qb = __shfl_down(m2, off);
    if (lane < off) chan_merge(n, mean, m2, nb, mb, qb);
  }
  if (lane == 0) {
    const long long b = plane / C, c = plane % C;
    out[b * 2 * C + c] = mean;
    out[b * 2 * C + C + c] = sqrtf(m2 / (float)(HW - 1));
  }
}

// ------------------------------------------------------------------------------------------------ the adaptation MLP
// out[o] = act(sum_k W[o][k] in[k] + bias[o]): a pass of the workgroup takes 64 outputs, four threads each; thread q of an output sums the products k = q, q + 4, ...
// in ascending order, the four partial sums are added as (s0 + s1) + (s2 + s3) (two quad permutes: every lane of the quad ends with the same bits), the bias last
template <bool ACT>
__device__ __forceinline__ void adapt_layer(const float* __restrict__ W, const float* __restrict__ bias, const float* in, int K, int N, float* out) {
  const int q = threadIdx.x & 3;
  for (int o0 = 0; o0 < N; o0 += APP_THREADS / 4) {   // uniform over the workgroup
    const int o = o0 + (threadIdx.x >> 2);
    float acc = 0.f;
    if (o < N) {
      const float* row = W + (long long)o * K;
#pragma unroll 8
      for (int k = q; k < K; k += 4) acc += row[k] * in[k];
    }
    acc += nl_dpp<0xB1>(acc);   // quad_perm [1, 0, 3, 2]
    acc += nl_dpp<0x4E>(acc);   // quad_perm [2, 3, 0, 1]
    if (o < N && q == 0) {
      const float s = acc + bias[o];
      out[o] = ACT ? nl_lrelu(s) : s;
    }
  }
}

__global__ __launch_bounds__(APP_THREADS) void adapt_code_kernel(const float* __restrict__ emb, const float* __restrict__ target, const float* __restrict__ W0,
                                                                 const float* __restrict__ b0, const float* __restrict__ W2, const float* __restrict__ b2,
                                                                 const float* __restrict__ W4, const float* __restrict__ b4, int E, int C, float* __restrict__ code) {
  __shared__ float d[APP_MAX_E];
  __shared__ float h1[NLA_ADAPT_HIDDEN], h2[NLA_ADAPT_HIDDEN];
  const long long v = blockIdx.x;
  for (int k = threadIdx.x; k < E; k += APP_THREADS) d[k] = target[k] - emb[v * E + k];
  __syncthreads();
  adapt_layer<true>(W0, b0, d, E, NLA_ADAPT_HIDDEN, h1);
  __syncthreads();
  adapt_layer<true>(W2, b2, h1, NLA_ADAPT_HIDDEN, NLA_ADAPT_HIDDEN, h2);
  __syncthreads();
  adapt_layer<false>(W4, b4, h2, NLA_ADAPT_HIDDEN, 2 * C, code + v * 2 * C);
}

// ------------------------------------------------------------------------------------------------ FiLM
// The walk both FiLM kernels share.  A workgroup owns `ppw` consecutive pixels of one view.  Channel units (4 channels with VEC, else 1) are taken CW = min(CU, 256)
// at a time; thread t keeps unit cb + t % CW and walks the pixels r, r + R, ... with r = t / CW, R = 256 / CW: consecutive lanes touch consecutive addresses, rows
// follow each other in memory, and a, b are loaded once per thread and chunk.
__host__ __device__ inline int film_rows(int C, bool vec) {
  const int CU = vec ? C / 4 : C;
  return APP_THREADS / (CU < APP_THREADS ? CU : APP_THREADS);
}

__device__ __forceinline__ float clip01(float y) { return y < 0.f ? 0.f : (y > 1.f ? 1.f : y); }   // a NaN passes through, as torch.clip

template <bool VEC, bool CLIP>
__global__ __launch_bounds__(APP_THREADS) void film_kernel(const float* x, const float* __restrict__ code, long long HW, int C, long long nblk, int ppw, float* y) {
  constexpr int W = VEC ? 4 : 1;
  const long long blk = blockIdx.x, v = blk / nblk, pbeg = (blk % nblk) * ppw;
  const long long pend = pbeg + ppw < HW ? pbeg + ppw : HW;
  const int t = threadIdx.x, CU = C / W, CW = CU < APP_THREADS ? CU : APP_THREADS, R = APP_THREADS / CW;
  const int cl = t % CW, r = t / CW;
  if (r >= R) return;   // no barrier in this kernel
  const float* cv = code + v * 2 * C;
  for (int cb = 0; cb < CU; cb += CW) {
    const int cu = cb + cl;
    if (cu >= CU) break;
    float a[W], b[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { a[j] = cv[cu * W + j]; b[j] = cv[C + cu * W + j]; }
    const long long base = v * HW * C + (long long)cu * W;
#pragma unroll 4
    for (long long p = pbeg + r; p < pend; p += R) {
      const long long i = base + p * C;
      if constexpr (VEC) {
        const float4 q = *reinterpret_cast<const float4*>(x + i);
        float4 o;
        o.x = a[0] * q.x + b[0]; o.y = a[1] * q.y + b[1]; o.z = a[2] * q.z + b[2]; o.w = a[3] * q.w + b[3];
        if (CLIP) { o.x = clip01(o.x); o.y = clip01(o.y); o.z = clip01(o.z); o.w = clip01(o.w); }
        *reinterpret_cast<float4*>(y + i) = o;
      } else {
        const float o = a[0] * x[i] + b[0];
        y[i] = CLIP ? clip01(o) : o;
      }
    }
  }
}

// part[(blk) 2 C + c] = sum of m g x, part[(blk) 2 C + C + c] = sum of m g over the workgroup's pixels; g_x and part may be NULL
template <bool VEC, bool CLIP>
__global__ __launch_bounds__(APP_THREADS) void film_bwd_kernel(const float* __restrict__ x, const float* __restrict__ code, const float* g_y, long long HW, int C,
                                                               long long nblk, int ppw, float* g_x, float* __restrict__ part) {
  __shared__ float sh[APP_THREADS * 8];
  constexpr int W = VEC ? 4 : 1;
  const long long blk = blockIdx.x, v = blk / nblk, pbeg = (blk % nblk) * ppw;
  const long long pend = pbeg + ppw < HW ? pbeg + ppw : HW;
  const int t = threadIdx.x, CU = C / W, CW = CU < APP_THREADS ? CU : APP_THREADS, R = APP_THREADS / CW;
  const int cl = t % CW, r = t / CW;
  const float* cv = code + v * 2 * C;
  for (int cb = 0; cb < CU; cb += CW) {   // uniform over the workgroup
    const int cu = cb + cl;
    const bool act = r < R && cu < CU;
    float sa[W], sb[W];
#pragma unroll
    for (int j = 0; j < W; ++j) sa[j] = sb[j] = 0.f;
    if (act) {
      float a[W], b[W];
#pragma unroll
      for (int j = 0; j < W; ++j) { a[j] = cv[cu * W + j]; b[j] = cv[C + cu * W + j]; }
      const long long base = v * HW * C + (long long)cu * W;
      // four pixels at a time, all loads before the first store: g_x may be g_y, so the compiler may not move a load of g_y above a store to g_x by itself —
      // but a thread only ever stores where it alone has loaded, so batching is safe and keeps eight 16-byte loads in flight per thread
      constexpr int U = 4;
      for (long long p = pbeg + r; p < pend; p += (long long)U * R) {
        float xv[U][W], gv[U][W];
#pragma unroll
        for (int u = 0; u < U; ++u) {
          const long long pu = p + (long long)u * R, i = base + pu * C;
          if (pu < pend) {
            if constexpr (VEC) {
              const float4 q = *reinterpret_cast<const float4*>(x + i), g = *reinterpret_cast<const float4*>(g_y + i);
              xv[u][0] = q.x; xv[u][1] = q.y; xv[u][2] = q.z; xv[u][3] = q.w;
              gv[u][0] = g.x; gv[u][1] = g.y; gv[u][2] = g.z; gv[u][3] = g.w;
            } else {
              xv[u][0] = x[i]; gv[u][0] = g_y[i];
            }
          } else {
#pragma unroll
            for (int j = 0; j < W; ++j) xv[u][j] = gv[u][j] = 0.f;
          }
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {   // ascending pixels
          const long long pu = p + (long long)u * R, i = base + pu * C;
          if (pu >= pend) break;
          float gx[W];
#pragma unroll
          for (int j = 0; j < W; ++j) {
            float g = gv[u][j];
            if (CLIP) {
              const float yv = a[j] * xv[u][j] + b[j];
              g = (yv >= 0.f && yv <= 1.f) ? g : 0.f;
            }
            sa[j] += g * xv[u][j];
            sb[j] += g;
            gx[j] = a[j] * g;
          }
          if (g_x) {
            if constexpr (VEC) *reinterpret_cast<float4*>(g_x + i) = make_float4(gx[0], gx[1], gx[2], gx[3]);
            else g_x[i] = gx[0];
          }
        }
      }
    }
    if (!part) continue;   // uniform
    __syncthreads();       // the previous chunk's readers are done
#pragma unroll
    for (int j = 0; j < W; ++j) { sh[t * 8 + j] = sa[j]; sh[t * 8 + 4 + j] = sb[j]; }
    __syncthreads();
    if (r == 0 && cu < CU) {
#pragma unroll
      for (int j = 0; j < W; ++j) {
        float ta = 0.f, tb = 0.f;
        for (int rr = 0; rr < R; ++rr) { ta += sh[(rr * CW + cl) * 8 + j]; tb += sh[(rr * CW + cl) * 8 + 4 + j]; }
        part[blk * 2 * C + cu * W + j] = ta;
        part[blk * 2 * C + C + cu * W + j] = tb;
      }
    }
  }
}

__global__ __launch_bounds__(APP_THREADS) void film_bwd_sum_kernel(const float* __restrict__ part, long long total, int C2, long long nblk, float* __restrict__ g_code) {
  const long long idx = (long long)blockIdx.x * APP_THREADS + threadIdx.x;
  if (idx >= total) return;
  const long long v = idx / C2;
  const int j = (int)(idx % C2);
  const float* p = part + v * nblk * C2 + j;
  float s = 0.f;
#pragma unroll 16
  for (long long w = 0; w < nblk; ++w) s += p[w * C2];   // the adds stay in ascending order; unrolling only puts the loads ahead of them
  g_code[idx] = s;
}

bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int64_t stats_segments(int64_t HW, int layout) { return nl_cdiv(HW, layout == NLA_LAYOUT_NCHW ? NLA_STATS_SEG_NCHW : NLA_STATS_SEG_NHWC); }

// NL_OK, or why the shape is refused
int stats_shape(int64_t B, int C, int64_t HW, int layout) {
  if (B < 0 || C < 1 || HW < 2 || (layout != NLA_LAYOUT_NCHW && layout != NLA_LAYOUT_NHWC)) return NL_ERR_BAD_ARG;
  if (C > APP_MAX_C || HW > APP_MAX_HW_STATS || B > APP_MAX_BLOCKS) return NL_ERR_UNSUPPORTED;
  const int64_t S = stats_segments(HW, layout);
  if (B * C > APP_MAX_BLOCKS / S) return NL_ERR_UNSUPPORTED;   // B C S, the partials' count and (NCHW) the grid, stays below 2^31
  return NL_OK;
}

int film_shape(int64_t V, int64_t HW, int C, unsigned flags) {
  if (V < 0 || HW < 1 || C < 1 || (flags & ~NLA_FILM_CLIP01)) return NL_ERR_BAD_ARG;
  if (C > APP_MAX_C || V > APP_MAX_V || HW >= APP_MAX_ELEMS) return NL_ERR_UNSUPPORTED;
  if (V > 0 && HW * C >= APP_MAX_ELEMS / V + (APP_MAX_ELEMS % V ? 1 : 0)) return NL_ERR_UNSUPPORTED;   // V HW C < 2^40
  if (V * nl_cdiv(HW, nla_film_backward_block_pixels(C)) > APP_MAX_BLOCKS) return NL_ERR_UNSUPPORTED;
  return NL_OK;
}

}  // namespace

extern "C" {

int nla_abi_version(void) { return NLA_ABI_VERSION; }

size_t nla_channel_stats_workspace_bytes(int64_t B, int C, int64_t HW, int layout) {
  if (stats_shape(B, C, HW, layout) != NL_OK || B == 0) return 0;
  return nl_align_up((size_t)(B * C * stats_segments(HW, layout)) * 2 * sizeof(float), 256);
}

int nla_channel_stats(const float* x, int64_t B, int C, int64_t HW, int layout, float* out, void* ws, size_t ws_bytes, void* stream) {
  const int st = stats_shape(B, C, HW, layout);
  if (st != NL_OK) return st;
  if (B == 0) return NL_OK;
  if (!x || !out || !aligned(x, 4) || !aligned(out, 4)) return NL_ERR_BAD_ARG;
  if (!ws || !aligned(ws, 256) || ws_bytes < nla_channel_stats_workspace_bytes(B, C, HW, layout)) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const int S = (int)stats_segments(HW, layout);
  const int64_t planes = B * C;
  float* pmean = (float*)ws;
  float* pm2 = pmean + planes * S;
  if (layout == NLA_LAYOUT_NCHW) {
    const dim3 grid((unsigned)(planes * S));
    if (HW % 4 == 0 && aligned(x, 16)) hipLaunchKernelGGL(stats_nchw_kernel<true>, grid, dim3(APP_THREADS), 0, s, x, (long long)HW, S, pmean, pm2);
    else hipLaunchKernelGGL(stats_nchw_kernel<false>, grid, dim3(APP_THREADS), 0, s, x, (long long)HW, S, pmean, pm2);
  } else {
    const dim3 grid((unsigned)(B * S));
    const bool vec = C % 4 == 0 && aligned(x, 16), keep = (vec ? C / 4 : C) <= APP_THREADS / 16;
#define NLA_NHWC_LAUNCH(VEC, KEEP) hipLaunchKernelGGL((stats_nhwc_kernel<VEC, KEEP>), grid, dim3(APP_THREADS), 0, s, x, (long long)HW, C, S, pmean, pm2)
    if (vec) { if (keep) NLA_NHWC_LAUNCH(true, true); else NLA_NHWC_LAUNCH(true, false); }
    else { if (keep) NLA_NHWC_LAUNCH(false, true); else NLA_NHWC_LAUNCH(false, false); }
#undef NLA_NHWC_LAUNCH
  }
  NL_LAUNCH_CHECK();
  hipLaunchKernelGGL(stats_merge_kernel, dim3((unsigned)nl_cdiv(planes, APP_THREADS / 64)), dim3(APP_THREADS), 0, s, (const float*)pmean, (const float*)pm2,
                     (long long)planes, C, (long long)HW, S, layout == NLA_LAYOUT_NCHW ? NLA_STATS_SEG_NCHW : NLA_STATS_SEG_NHWC, out);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nla_adapt_code(const float* emb, const float* target, const void* const* weights, int64_t V, int E, int C, float* code, void* stream) {
  if (V < 0 || E < 4 || E % 4 != 0 || C < 1) return NL_ERR_BAD_ARG;
  if (E > APP_MAX_E || C > APP_MAX_C || V > APP_MAX_V) return NL_ERR_UNSUPPORTED;
  if (V == 0) return NL_OK;
  if (!emb || !target || !weights || !code || !aligned(emb, 4) || !aligned(target, 4) || !aligned(code, 4)) return NL_ERR_BAD_ARG;
  for (int i = 0; i < 6; ++i)
    if (!weights[i] || !aligned(weights[i], 4)) return NL_ERR_BAD_ARG;
  hipLaunchKernelGGL(adapt_code_kernel, dim3((unsigned)V), dim3(APP_THREADS), 0, (hipStream_t)stream, emb, target, (const float*)weights[0], (const float*)weights[1],
                     (const float*)weights[2], (const float*)weights[3], (const float*)weights[4], (const float*)weights[5], E, C, code);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int64_t nla_film_backward_block_pixels(int C) {
  if (C < 1 || C > APP_MAX_C) return 0;
  return (int64_t)film_rows(C, C % 4 == 0) * FILM_ITERS;
}

int nla_film(const float* x, const float* code, int64_t V, int64_t HW, int C, unsigned flags, float* y, void* stream) {
  const int st = film_shape(V, HW, C, flags);
  if (st != NL_OK) return st;
  if (V == 0) return NL_OK;
  if (!x || !code || !y || !aligned(x, 4) || !aligned(code, 4) || !aligned(y, 4)) return NL_ERR_BAD_ARG;
  const int ppw = (int)nla_film_backward_block_pixels(C);
  const long long nblk = nl_cdiv(HW, ppw);
  const bool vec = C % 4 == 0 && aligned(x, 16) && aligned(y, 16) && aligned(code, 16), clip = flags & NLA_FILM_CLIP01;
  const dim3 grid((unsigned)(V * nblk)), block(APP_THREADS);
  hipStream_t s = (hipStream_t)stream;
#define NLA_FILM_LAUNCH(VEC, CLIP) hipLaunchKernelGGL((film_kernel<VEC, CLIP>), grid, block, 0, s, x, code, (long long)HW, C, nblk, ppw, y)
  if (vec) { if (clip) NLA_FILM_LAUNCH(true, true); else NLA_FILM_LAUNCH(true, false); }
  else { if (clip) NLA_FILM_LAUNCH(false, true); else NLA_FILM_LAUNCH(false, false); }
#undef NLA_FILM_LAUNCH
  NL_LAUNCH_CHECK();
  return NL_OK;
}

size_t nla_film_backward_workspace_bytes(int64_t V, int64_t HW, int C) {
  if (film_shape(V, HW, C, 0) != NL_OK || V == 0) return 0;
  return nl_align_up((size_t)(V * nl_cdiv(HW, nla_film_backward_block_pixels(C))) * 2 * C * sizeof(float), 256);
}

int nla_film_backward(const float* x, const float* code, const float* g_y, int64_t V, int64_t HW, int C, unsigned flags, float* g_x, float* g_code, void* ws,
                      size_t ws_bytes, void* stream) {
  const int st = film_shape(V, HW, C, flags);
  if (st != NL_OK) return st;
  if (V == 0) return NL_OK;
  if (!x || !code || !g_y || !aligned(x, 4) || !aligned(code, 4) || !aligned(g_y, 4) || !aligned(g_x, 4) || !aligned(g_code, 4)) return NL_ERR_BAD_ARG;
  if (g_code && (!ws || !aligned(ws, 256) || ws_bytes < nla_film_backward_workspace_bytes(V, HW, C))) return NL_ERR_WORKSPACE;
  if (!g_x && !g_code) return NL_OK;
  const int ppw = (int)nla_film_backward_block_pixels(C);
  const long long nblk = nl_cdiv(HW, ppw);
  const bool vec = C % 4 == 0 && aligned(x, 16) && aligned(g_y, 16) && aligned(g_x, 16) && aligned(code, 16), clip = flags & NLA_FILM_CLIP01;
  const dim3 grid((unsigned)(V * nblk)), block(APP_THREADS);
  hipStream_t s = (hipStream_t)stream;
  float* part = g_code ? (float*)ws : nullptr;
#define NLA_BWD_LAUNCH(VEC, CLIP) hipLaunchKernelGGL((film_bwd_kernel<VEC, CLIP>), grid, block, 0, s, x, code, g_y, (long long)HW, C, nblk, ppw, g_x, part)
  if (vec) { if (clip) NLA_BWD_LAUNCH(true, true); else NLA_BWD_LAUNCH(true, false); }
  else { if (clip) NLA_BWD_LAUNCH(false, true); else NLA_BWD_LAUNCH(false, false); }
#undef NLA_BWD_LAUNCH
  NL_LAUNCH_CHECK();
  if (g_code) {
    const long long total = V * 2 * C;
    hipLaunchKernelGGL(film_bwd_sum_kernel, dim3((unsigned)nl_cdiv(total, APP_THREADS)), block, 0, s, (const float*)part, total, 2 * C, nblk, g_code);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

}  // extern "C"
