// Generic "segment GEMM" for the GEMM-shaped stages that are not (yet) inside a fused kernel:
//   C[out_row(m), n] = act( sum_seg sum_k A_seg[in_row_seg(m), k] * B[koff_seg + k, n] + bias[n] )
// A is assembled on the fly from up to 6 sources (channel concat, conv taps along the ray, row
// broadcast), so Linear, Conv1d(k=3), ConvTranspose1d(k=3,s=2) and the concat-MLPs of the
// reference all run through one MFMA kernel without materialising im2col / concat tensors.
//
// Tiling (wave64, gfx950): 256 threads = 4 waves; block tile 128 (M) x BN (N) x 32 (K); wave w owns
// rows [32w,32w+32) x all BN columns as BN/32 accumulators of 32x32 (16 VGPR each).
//   NL_PREC_F32    : v_mfma_f32_32x32x2_f32, operands staged in LDS as f32 (A transposed [k][m] so
//                    both operand reads are conflict-free ds_read_b32)
//   NL_PREC_BF16X3 : v_mfma_f32_32x32x16_bf16 x3 (hi*hi + hi*lo + lo*hi), A split to bf16 hi/lo when
//   NL_PREC_BF16   : staged ([m][k] rows padded to 80 B -> conflict-free ds_read_b128), weights pre-split
// Global loads of tile t+1 are issued before the MFMAs of tile t (register prefetch).
#include "common.h"
#include "mfma.h"

namespace {

constexpr int BM = 128;
constexpr int BK = 32;

__device__ __forceinline__ float bf2f(unsigned short h) { return __uint_as_float(((unsigned int)h) << 16); }

struct RowMap {
  int base;   // r*Li  (or m for plain)
  int t;      // position along the ray (row-mapped) ; unused for plain
  int mdiv;   // m / rdiv for broadcast segments
  bool ok;
};

__device__ __forceinline__ RowMap map_row(const NlGemmArgs& a, int m, int rdiv) {
  RowMap r;
  r.ok = m < a.M;
  if (a.So > 0) {
    int q = m / a.So;
    r.t = m - q * a.So;
    r.base = q * a.Li;
    r.mdiv = 0;
  } else {
    r.t = 0;
    r.base = m;
    r.mdiv = rdiv > 1 ? m / rdiv : m;
  }
  return r;
}

// 4 consecutive k of one segment for one output row (zero beyond the segment / outside the ray)
__device__ __forceinline__ float4 load_a4(const NlGemmArgs& a, const RowMap& rm, int s, int kin) {
  const NlGemmSeg& sg = a.seg[s];
  int ioff = sg.ioff;
  if (sg.ntap > 1) {   // [32-channel block][tap][32]
    const int cc = kin >> 5, cb = cc / sg.ntap;
    ioff += cc - cb * sg.ntap - (sg.ntap >> 1);
    kin = (cb << 5) + (kin & 31);
  }
  int row;
  if (a.So > 0) {
    int i = rm.t + ioff;
    if (i < 0 || i >= a.Li) return make_float4(0.f, 0.f, 0.f, 0.f);
    row = rm.base + i;
  } else {
    row = sg.rdiv > 1 ? rm.mdiv : rm.base;
  }
  const float* p = sg.ptr + (size_t)row * sg.ld + kin;
  if (sg.vec && kin + 3 < sg.k) return *(const float4*)p;
  float4 v;
  v.x = kin + 0 < sg.k ? p[0] : 0.f;
  v.y = kin + 1 < sg.k ? p[1] : 0.f;
  v.z = kin + 2 < sg.k ? p[2] : 0.f;
  v.w = kin + 3 < sg.k ? p[3] : 0.f;
  return v;
}

// Every segment occupies round_up(k, 32) slots of K-space, so a 32-wide k-tile lies inside exactly ONE segment: the
// lookup depends on k0 only, is wave-uniform, and `a.seg[s]` becomes scalar loads (a per-lane index into the kernarg
// struct costs dependent vector loads / waterfall loops on every element).
__device__ __forceinline__ int find_seg(const NlGemmArgs& a, int k0, int& kbase) {
  int s = -1, acc = 0;
  for (int j = 0; j < a.nseg; ++j) {
    const int kp = ((a.seg[j].k + 31) & ~31) * a.seg[j].ntap;
    if (s < 0 && k0 < acc + kp) { s = j; kbase = k0 - acc; }
    acc += kp;
  }
  return __builtin_amdgcn_readfirstlane(s);
}

__device__ __forceinline__ int out_row(const NlGemmArgs& a, int m) {
  if (a.So > 0) {
    int q = m / a.So;
    int t = m - q * a.So;
    return q * a.Lo + t * a.ostride + a.ooff;
  }
  return m;
}

// ------------------------------------------------------------------------------------------ F32
template <int BN>
__global__ __launch_bounds__(256) void gemm_f32_kernel(const NlGemmArgs a) {
  __shared__ float As[BK][BM + 1];
  __shared__ float Bs[BK][BN];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int k4_a = (tid & 7) * 4, row_a = tid >> 3;  // this thread stages A[row_a + 32*i][k4_a .. k4_a+3]
  int rdiv = 1;
  for (int s = 0; s < a.nseg; ++s) rdiv = a.seg[s].rdiv > rdiv ? a.seg[s].rdiv : rdiv;

  RowMap rm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rm[i] = map_row(a, m0 + row_a + 32 * i, rdiv);

  constexpr int NB4 = BN / 32;  // float4 B loads per thread per tile
  const float* Bg = (const float*)a.B;
  float4 areg[4];
  float4 breg[NB4];

  auto prefetch = [&](int k0) {
    int kbase = 0;
    const int s = find_seg(a, k0, kbase);
    const int kin = __builtin_amdgcn_readfirstlane(kbase) + k4_a;
#pragma unroll
    for (int i = 0; i < 4; ++i) areg[i] = (s >= 0 && rm[i].ok) ? load_a4(a, rm[i], s, kin) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NB4; ++j) {
      int idx = tid + 256 * j;
      int kk = idx / (BN / 4), c4 = idx % (BN / 4);
      int col = n0 + c4 * 4;
      breg[j] = (col < a.Npad) ? *(const float4*)(Bg + (size_t)(k0 + kk) * a.Npad + col) : make_float4(0, 0, 0, 0);
    }
  };

  nl_f32x16 acc[BN / 32];
#pragma unroll
  for (int c = 0; c < BN / 32; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  prefetch(0);
  for (int k0 = 0; k0 < a.Kpad; k0 += BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      As[k4_a + 0][row_a + 32 * i] = areg[i].x; As[k4_a + 1][row_a + 32 * i] = areg[i].y;
      As[k4_a + 2][row_a + 32 * i] = areg[i].z; As[k4_a + 3][row_a + 32 * i] = areg[i].w;
    }
#pragma unroll
    for (int j = 0; j < NB4; ++j) {
      int idx = tid + 256 * j;
      int kk = idx / (BN / 4), c4 = idx % (BN / 4);
      *(float4*)&Bs[kk][c4 * 4] = breg[j];
    }
    __syncthreads();
    if (k0 + BK < a.Kpad) prefetch(k0 + BK);
#pragma unroll
    for (int ks = 0; ks < BK / 2; ++ks) {
      int kk = 2 * ks + (lane >> 5);
      float av = As[kk][32 * wave + (lane & 31)];
#pragma unroll
      for (int c = 0; c < BN / 32; ++c) {
        float bv = Bs[kk][32 * c + (lane & 31)];
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[c], 0, 0, 0);
      }
    }
    __syncthreads();
  }

  // epilogue: C/D layout col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m >= a.M) continue;
    size_t orow = (size_t)out_row(a, m) * a.ldc;
#pragma unroll
    for (int c = 0; c < BN / 32; ++c) {
      int col = n0 + 32 * c + (lane & 31);
      if (col < a.N) {
        float v = acc[c][r] + (a.bias ? a.bias[col] : 0.f);
        a.C[orow + col] = nl_act(v, a.act);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ BF16 / BF16X3
// 128 x BN x 32 tiles.  LDS rows are 32 bf16 (64 B) padded to 80 B: a 16-lane ds_read_b128 group then touches 16
// distinct 16-B slots of the 256-B bank row (conflict-free).  fp32 -> bf16 hi/lo split uses v_cvt_pk_bf16_f32.
constexpr int LDS_ROW = 40;  // in bf16 elements (80 B)

template <int BN, bool X3>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(const NlGemmArgs a) {
  __shared__ __attribute__((aligned(16))) unsigned short Ah[BM * LDS_ROW];
  __shared__ __attribute__((aligned(16))) unsigned short Al[X3 ? BM * LDS_ROW : 8];
  __shared__ __attribute__((aligned(16))) unsigned short Bh[BN * LDS_ROW];
  __shared__ __attribute__((aligned(16))) unsigned short Bl[X3 ? BN * LDS_ROW : 8];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int k4_a = (tid & 7) * 4, row_a = tid >> 3;   // this thread stages A[row_a + 32*i][k4_a .. k4_a+3], i < 4
  int rdiv = 1;
  for (int s = 0; s < a.nseg; ++s) rdiv = a.seg[s].rdiv > rdiv ? a.seg[s].rdiv : rdiv;
  RowMap rm[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) rm[i] = map_row(a, m0 + row_a + 32 * i, rdiv);

  // B: packed [Npad][Kpad] bf16 (k contiguous). Tile = BN rows x 32 k = BN*64 B -> BN*4 16-B chunks / 256 threads
  constexpr int NBC = BN / 64;  // 16-B chunks per thread per part
  const unsigned short* Bgh = (const unsigned short*)a.B;
  const unsigned short* Bgl = (const unsigned short*)a.Blo;
  float4 areg[4];
  uint4 bh[NBC], bl[NBC];

  auto prefetch = [&](int k0) {
    int kbase = 0;
    const int s = find_seg(a, k0, kbase);
    const int kin = __builtin_amdgcn_readfirstlane(kbase) + k4_a;
#pragma unroll
    for (int i = 0; i < 4; ++i) areg[i] = (s >= 0 && rm[i].ok) ? load_a4(a, rm[i], s, kin) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int j = 0; j < NBC; ++j) {
      const int idx = tid + 256 * j;        // chunk id: n = idx>>2, part = idx&3 (8 bf16 each)
      const int n = idx >> 2, part = idx & 3;
      const bool ok = (n0 + n < a.Npad);
      const size_t off = (size_t)(n0 + n) * a.Kpad + k0 + part * 8;
      bh[j] = ok ? *(const uint4*)(Bgh + off) : make_uint4(0, 0, 0, 0);
      if (X3) bl[j] = ok ? *(const uint4*)(Bgl + off) : make_uint4(0, 0, 0, 0);
    }
  };

  nl_f32x16 acc[BN / 32];
#pragma unroll
  for (int c = 0; c < BN / 32; ++c)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[c][r] = 0.f;

  prefetch(0);
  for (int k0 = 0; k0 < a.Kpad; k0 += BK) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float v[4] = {areg[i].x, areg[i].y, areg[i].z, areg[i].w};
      nl_bf16x4 h, l;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        h[j] = (__bf16)v[j];
        if (X3) l[j] = (__bf16)(v[j] - (float)h[j]);
      }
      *(uint2*)&Ah[(row_a + 32 * i) * LDS_ROW + k4_a] = __builtin_bit_cast(uint2, h);
      if (X3) *(uint2*)&Al[(row_a + 32 * i) * LDS_ROW + k4_a] = __builtin_bit_cast(uint2, l);
    }
#pragma unroll
    for (int j = 0; j < NBC; ++j) {
      const int idx = tid + 256 * j;
      const int n = idx >> 2, part = idx & 3;
      *(uint4*)&Bh[n * LDS_ROW + part * 8] = bh[j];
      if (X3) *(uint4*)&Bl[n * LDS_ROW + part * 8] = bl[j];
    }
    __syncthreads();
    if (k0 + BK < a.Kpad) prefetch(k0 + BK);
#pragma unroll
    for (int ks = 0; ks < BK / 16; ++ks) {  // two 16-deep MFMA k-steps per 32-wide tile
      const int ko = ks * 16 + 8 * (lane >> 5);
      const nl_i16x8 ah = *(const nl_i16x8*)&Ah[(32 * wave + (lane & 31)) * LDS_ROW + ko];
      nl_i16x8 al;
      if (X3) al = *(const nl_i16x8*)&Al[(32 * wave + (lane & 31)) * LDS_ROW + ko];
#pragma unroll
      for (int c = 0; c < BN / 32; ++c) {
        const nl_i16x8 bhv = *(const nl_i16x8*)&Bh[(32 * c + (lane & 31)) * LDS_ROW + ko];
        if (X3) {
          const nl_i16x8 blv = *(const nl_i16x8*)&Bl[(32 * c + (lane & 31)) * LDS_ROW + ko];
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al, bhv, acc[c], 0, 0, 0);
          acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, blv, acc[c], 0, 0, 0);
        }
        acc[c] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah, bhv, acc[c], 0, 0, 0);
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    int m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m >= a.M) continue;
    size_t orow = (size_t)out_row(a, m) * a.ldc;
#pragma unroll
    for (int c = 0; c < BN / 32; ++c) {
      int col = n0 + 32 * c + (lane & 31);
      if (col < a.N) {
        float v = acc[c][r] + (a.bias ? a.bias[col] : 0.f);
        a.C[orow + col] = nl_act(v, a.act);
      }
    }
  }
}

template <int BN>
int launch_bn(const NlGemmArgs& a, int precision, hipStream_t st) {
  dim3 grid((unsigned)nl_cdiv(a.M, BM), (unsigned)nl_cdiv(a.N, BN));
  if (precision == NL_PREC_F32) {
    hipLaunchKernelGGL(gemm_f32_kernel<BN>, grid, dim3(256), 0, st, a);
  } else if (precision == NL_PREC_BF16X3) {
    hipLaunchKernelGGL((gemm_bf16_kernel<BN, true>), grid, dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((gemm_bf16_kernel<BN, false>), grid, dim3(256), 0, st, a);
  }
  return hipPeekAtLastError() == hipSuccess ? NL_OK : NL_ERR_HIP;
}

}  // namespace

int nl_gemm_launch(const NlGemmArgs& a, int precision, hipStream_t st) {
  if (a.M <= 0) return NL_OK;
  if (nl_tgemm_supported(a, precision)) return nl_tgemm_launch(a, precision, st);
  for (int s = 0; s < a.nseg; ++s) if (a.seg[s].frag) return NL_ERR_UNSUPPORTED;   // a fragment-native source is the streaming kernel's alone
  if (a.epi != NL_EPI_NONE || a.act == NL_ACT_LRELU_MASK) return NL_ERR_UNSUPPORTED;   // callers check nl_tgemm_supported() before asking for a fused epilogue
  if (a.N <= 64) return launch_bn<64>(a, precision, st);
  // 128-wide column blocks also for N = 256, in every precision: 2 waves/SIMD instead of 1 hides the tile-load latency better than the
  // saved A re-read (A comes from L2 the second time); measured for exact fp32 too (fp32 render 59.4 -> 44.5 ms per config-2 batch)
  return launch_bn<128>(a, precision, st);
}
