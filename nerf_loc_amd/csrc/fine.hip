// Fine matcher (reference: models/matching/fine_matching.py): the two stages behind the coarse matches of matcher.py:101-124.
//
// nl_fine_windows (FinePreprocess.forward, fine_matching.py:35-76 with fine_concat_coarse_feat = False): out[m][ww] = proj(window cell ww of match m), the 7 x 7
//   window of F.unfold(kernel 7, stride s, padding 3) gathered straight from the NHWC fine map — the unfolded map is never formed.  A wave owns one match and TWO
//   32-channel output blocks: D[cell][channel] = X . W^T on the 32x32 MFMAs, A = the window's pixels (two 32-row tiles: 49 cells padded to 64; a lane reads the 8
//   (fp32 mode: 4) consecutive channels of its cell's pixel, zeros outside the map and for the 15 padding rows), B = the weight fragments.  Accumulator register r of
//   half-wave hh is cell 32 t + nl_acc_row(r, hh), the lane's column is the channel: a store instruction writes 128 contiguous bytes per cell.
// nl_fine_match (FineMatching.forward, fine_matching.py:94-143): one wave per match.  The 49 product rows feat_f0[m] * feat_f1[m, r] are the two 32-column tiles of
//   s2d.h's MLP (cell = 32 t + column); the logit of cell `lane` ends up in lane `lane`, and softmax (temperature 1 / sqrt C), expectation over linspace(-1, 1, 7)
//   and the standard deviation are DPP reductions of that one wave.  Neither the products nor the hidden activations nor the logits reach memory.
//   NL_PREC_BF16X3 multiplies as three-term split-FP16 here (mfma.h: nl_split_pair<true>; the image's fp16 planes): the softmax multiplies a logit's error by the logit's size, and
//   split-bf16's 2^-17 per product missed the 1e-4 bar on nearly one-hot heat-maps.  nl_fine_windows stays split-bf16.
// Weights come from L2 in both kernels, not from LDS as in the coarse matcher: a wave uses every fragment once per match (there the same fragments serve 32 rows x
// 4 iterations per work item), and with the grid sized by M <= a few thousand a workgroup would fill 100 - 256 KiB of LDS to score four matches.
// A match's outputs depend on its own rows, the weights and the mode only: one wave, fixed reduction order, no atomics.
#include "common.h"
#include "mfma.h"
#include "s2d.h"
#include "fine.h"
#include "host.h"

namespace {

__device__ __forceinline__ void fine_win_store(const FineWinArgs& a, const nl_f32x16 (&acc)[2][2], int m, int rb0, bool has1, int lane) {
  const int hh = lane >> 5, col = lane & 31;
  const float* bias = (const float*)(a.img + fine_proj_layout(a.Cf, a.Cout).bias);
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (j == 1 && !has1) break;
    const int ch = 32 * (rb0 + j) + col;
    const float bv = bias[ch];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int cell = 32 * t + nl_acc_row(r, hh);
        if (cell < FINE_WW) a.out[((size_t)m * FINE_WW + cell) * a.Cout + ch] = acc[t][j][r] + bv;
      }
  }
}

template <bool X3>
__global__ __launch_bounds__(256) void fine_win_bf16_kernel(const FineWinArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)a.M * a.Q) return;   // wave-uniform; the kernel has no barrier
  const int m = (int)(item / a.Q), rb0 = 2 * (int)(item - (long long)m * a.Q);
  const int nrb = a.Cout >> 5, nk = a.Cf >> 4;
  const bool has1 = rb0 + 1 < nrb;
  const FineProjLayout L = fine_proj_layout(a.Cf, a.Cout);
  const uint4* whi = (const uint4*)(a.img + L.hi);
  const uint4* wlo = (const uint4*)(a.img + L.lo);
  const float* row[2] = {fine_cell_row(a, m, col), fine_cell_row(a, m, 32 + col)};

  nl_f32x16 acc[2][2];
#pragma unroll
  for (int t = 0; t < 2; ++t)   // (written out: with nl_acc_zero this kernel compiles to other code)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[t][j][r] = 0.f;

  for (int s = 0; s < nk; ++s) {
    nl_i16x8 ah[2], al[2];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      float4 x0 = make_float4(0.f, 0.f, 0.f, 0.f), x1 = x0;
      if (row[t]) {
        x0 = *(const float4*)(row[t] + 16 * s + 8 * hh);
        x1 = *(const float4*)(row[t] + 16 * s + 8 * hh + 4);
      }
      unsigned ph[4], pl[4];
      nl_split_bf16_pair(x0.x, x0.y, ph[0], pl[0]);
      nl_split_bf16_pair(x0.z, x0.w, ph[1], pl[1]);
      nl_split_bf16_pair(x1.x, x1.y, ph[2], pl[2]);
      nl_split_bf16_pair(x1.z, x1.w, ph[3], pl[3]);
      ah[t] = nl_frag(ph[0], ph[1], ph[2], ph[3]);
      al[t] = nl_frag(pl[0], pl[1], pl[2], pl[3]);
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      if (j == 1 && !has1) break;
      const int f = (s * nrb + rb0 + j) * 64 + lane;
      const nl_i16x8 bh = nl_frag(whi[f]);
      if (X3) {
        const nl_i16x8 bl = nl_frag(wlo[f]);
#pragma unroll
        for (int t = 0; t < 2; ++t) {
          acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[t], bh, acc[t][j], 0, 0, 0);
          acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bl, acc[t][j], 0, 0, 0);
        }
      }
#pragma unroll
      for (int t = 0; t < 2; ++t) acc[t][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[t], bh, acc[t][j], 0, 0, 0);
    }
  }
  fine_win_store(a, acc, m, rb0, has1, lane);
}

// NL_PREC_F32: v_mfma_f32_32x32x2_f32, half-wave hh supplies k slot hh; step t of channel group g multiplies channel 8 g + 4 hh + t
__global__ __launch_bounds__(256) void fine_win_f32_kernel(const FineWinArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const long long item = (long long)blockIdx.x * 4 + wave;
  if (item >= (long long)a.M * a.Q) return;
  const int m = (int)(item / a.Q), rb0 = 2 * (int)(item - (long long)m * a.Q);
  const int nrb = a.Cout >> 5, ng = a.Cf >> 3;
  const bool has1 = rb0 + 1 < nrb;
  const float* wf = (const float*)(a.img + fine_proj_layout(a.Cf, a.Cout).f32);
  const float* row[2] = {fine_cell_row(a, m, col), fine_cell_row(a, m, 32 + col)};

  nl_f32x16 acc[2][2];
  nl_acc_zero(acc);

  for (int g = 0; g < ng; ++g) {
    float x[2][4];
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      const float4 v = row[t] ? *(const float4*)(row[t] + 8 * g + 4 * hh) : make_float4(0.f, 0.f, 0.f, 0.f);
      x[t][0] = v.x; x[t][1] = v.y; x[t][2] = v.z; x[t][3] = v.w;
    }
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        if (j == 1 && !has1) break;
        const float w = wf[((g * 4 + e) * nrb + rb0 + j) * 64 + lane];
        acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[0][e], w, acc[0][j], 0, 0, 0);
        acc[1][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(x[1][e], w, acc[1][j], 0, 0, 0);
      }
  }
  fine_win_store(a, acc, m, rb0, has1, lane);
}

// ------------------------------------------------------------------------------------------ match
struct FineMatchArgs {
  const unsigned char* img;
  const float* f0; const float* f1; const float* kc;
  float* expec; float* kf; float* heat;
  int M, C;
  float temp;
};

// the logit of cell `lane` is in logit[lane >> 5] of lane `lane`: softmax over the 49 cells, expectation and std of one match (fine_matching.py:124-136, 149)
__device__ __forceinline__ void fine_finish(const FineMatchArgs& a, const float (&logit)[2], int m, int lane) {
  const bool valid = lane < FINE_WW;
  const float z = (lane >> 5 ? logit[1] : logit[0]) * a.temp;
  const float zmax = wave_max(valid ? z : -3.4028235e38f);
  const float e = valid ? expf(z - zmax) : 0.f;
  const float h = e / wave_sum(e);
  const int wy = lane / FINE_W, wx = lane - wy * FINE_W;
  const float gx = (float)(wx - 3) / 3.f, gy = (float)(wy - 3) / 3.f;   // linspace(-1, 1, 7), x along the fast axis
  const float cx = wave_sum(h * gx), cy = wave_sum(h * gy);
  const float vx = wave_sum(gx * gx * h) - cx * cx, vy = wave_sum(gy * gy * h) - cy * cy;
  const float sd = sqrtf(fmaxf(vx, 1e-10f)) + sqrtf(fmaxf(vy, 1e-10f));
  if (a.heat && valid) a.heat[(size_t)m * FINE_WW + lane] = h;
  if (lane == 0) {
    a.expec[(size_t)m * 3 + 0] = cx; a.expec[(size_t)m * 3 + 1] = cy; a.expec[(size_t)m * 3 + 2] = sd;
    a.kf[(size_t)m * 2 + 0] = a.kc[(size_t)m * 2 + 0] + cx * (float)(FINE_W / 2);
    a.kf[(size_t)m * 2 + 1] = a.kc[(size_t)m * 2 + 1] + cy * (float)(FINE_W / 2);
  }
}

// F16: the parity mode multiplies as three-term split-FP16 (mfma.h), from the image's fp16 planes
template <bool X3, bool F16>
__global__ __launch_bounds__(256) void fine_match_bf16_kernel(const FineMatchArgs a) {
  if constexpr (F16) __builtin_amdgcn_s_setreg(1473, 1);   // MODE.FP16_OVFL: conversions to f16 saturate at 65504 instead of producing inf (as tgemm.hip's split-FP16 rows)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const int m = blockIdx.x * 4 + wave;
  if (m >= a.M) return;   // wave-uniform; the kernel has no barrier
  const int C = a.C, nk1 = C >> 4;
  const S2dLayout L = s2d_layout(C);
  const uint4* w1hi = (const uint4*)(a.img + (F16 ? L.h1hi : L.w1hi));
  const uint4* w1lo = (const uint4*)(a.img + (F16 ? L.h1lo : L.w1lo));
  const uint4* w2hi = (const uint4*)(a.img + (F16 ? L.h2hi : L.w2hi));
  const uint4* w2lo = (const uint4*)(a.img + (F16 ? L.h2lo : L.w2lo));
  const float* small = (const float*)(a.img + L.small);
  const float* xp = a.f0 + (size_t)m * C + 8 * hh;
  const float* ya = a.f1 + ((size_t)m * FINE_WW + col) * C + 8 * hh;
  const float* yb = a.f1 + ((size_t)m * FINE_WW + min(32 + col, FINE_WW - 1)) * C + 8 * hh;   // columns 49 .. 63 repeat cell 48; their logits are dropped

  nl_f32x16 acc[2][4];
  nl_acc_zero(acc);
  for (int s = 0; s < nk1; ++s) {
    const float4 x0 = *(const float4*)(xp + 16 * s), x1 = *(const float4*)(xp + 16 * s + 4);
    const float4 ya0 = *(const float4*)(ya + 16 * s), ya1 = *(const float4*)(ya + 16 * s + 4);
    const float4 yb0 = *(const float4*)(yb + 16 * s), yb1 = *(const float4*)(yb + 16 * s + 4);
    unsigned ph[2][4], pl[2][4];
    nl_split_pair<F16>(x0.x * ya0.x, x0.y * ya0.y, ph[0][0], pl[0][0]);
    nl_split_pair<F16>(x0.z * ya0.z, x0.w * ya0.w, ph[0][1], pl[0][1]);
    nl_split_pair<F16>(x1.x * ya1.x, x1.y * ya1.y, ph[0][2], pl[0][2]);
    nl_split_pair<F16>(x1.z * ya1.z, x1.w * ya1.w, ph[0][3], pl[0][3]);
    nl_split_pair<F16>(x0.x * yb0.x, x0.y * yb0.y, ph[1][0], pl[1][0]);
    nl_split_pair<F16>(x0.z * yb0.z, x0.w * yb0.w, ph[1][1], pl[1][1]);
    nl_split_pair<F16>(x1.x * yb1.x, x1.y * yb1.y, ph[1][2], pl[1][2]);
    nl_split_pair<F16>(x1.z * yb1.z, x1.w * yb1.w, ph[1][3], pl[1][3]);
    s2d_layer1_step<X3, F16>(acc, w1hi, w1lo, s, lane, ph, pl);
  }
  s2d_layer2<X3, F16>(acc, small + 64 * hh, w2hi, w2lo, lane);
  float logit[2];
  s2d_logits(acc, small, hh, logit);
  fine_finish(a, logit, m, lane);
}

__global__ __launch_bounds__(256) void fine_match_f32_kernel(const FineMatchArgs a) {
  extern __shared__ __attribute__((aligned(16))) float fine_hidden[];   // S2D_F32_LDS bytes
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, hh = lane >> 5, col = lane & 31;
  const int m = blockIdx.x * 4 + wave;
  if (m >= a.M) return;
  const int C = a.C, ng = C >> 3;
  const S2dLayout L = s2d_layout(C);
  const float* w1f = (const float*)(a.img + L.f32w1);
  const float* w2f = (const float*)(a.img + L.f32w2);
  const float* small = (const float*)(a.img + L.small);
  float* hbuf = fine_hidden + wave * (128 * 64) + lane;   // only this lane reads what it wrote
  const float* xp = a.f0 + (size_t)m * C + 4 * hh;
  const float* ya = a.f1 + ((size_t)m * FINE_WW + col) * C + 4 * hh;
  const float* yb = a.f1 + ((size_t)m * FINE_WW + min(32 + col, FINE_WW - 1)) * C + 4 * hh;

  nl_f32x16 acc[2][4];
  nl_acc_zero(acc);
  for (int g = 0; g < ng; ++g) {
    const float4 x = *(const float4*)(xp + 8 * g), va = *(const float4*)(ya + 8 * g), vb = *(const float4*)(yb + 8 * g);
    const float pa[4] = {x.x * va.x, x.y * va.y, x.z * va.z, x.w * va.w};
    const float pb[4] = {x.x * vb.x, x.y * vb.y, x.z * vb.z, x.w * vb.w};
    s2d_f32_layer1_group(acc, w1f, g, lane, pa, pb);
  }
  s2d_f32_layer2(acc, small + 64 * hh, hbuf, w2f, lane);
  float logit[2];
  s2d_logits(acc, small, hh, logit);
  fine_finish(a, logit, m, lane);
}

}  // namespace

// out (M * 49, Cout) = rows (M * 49, Cin) . W^T with `img` a proj image of W (Cout x Cin) — the window kernels on dense rows (the backward's g_out . proj.weight,
// with the training image of proj.weight^T, whose bias is zero); split-bf16, three terms with x3.  There is no exact-fp32 form on purpose: fine_win_f32_kernel
// must never run on a training image, whose fp32 plane holds the plain transpose (the packer's staging), not fragment order
int nl_launch_fine_rows(const void* img, int Cin, int Cout, bool x3, const float* rows, int64_t M, float* out, hipStream_t st) {
  FineWinArgs a;
  a.img = (const unsigned char*)img;
  a.feat = rows;
  a.b_ids = nullptr; a.j_ids = nullptr;
  a.out = out;
  a.B = 1; a.Hf = 1; a.Wf = 1; a.Cf = Cin; a.Cout = Cout; a.M = (int)M; a.stride = 1; a.Lx = 1; a.L = 1;
  a.Q = ((Cout >> 5) + 1) >> 1;
  a.dense = 1;
  const unsigned grid = (unsigned)nl_cdiv(M * a.Q, 4);
  if (x3) hipLaunchKernelGGL(fine_win_bf16_kernel<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(fine_win_bf16_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

extern "C" {

size_t nl_fine_proj_packed_bytes(int Cf, int Cout) { return fine_c_ok(Cf) && fine_c_ok(Cout) ? nl_align_up(fine_proj_layout(Cf, Cout).total, 16) : 0; }

int nl_fine_pack_proj(int Cf, int Cout, const float* w, const float* b, void* packed, size_t packed_bytes, void* stream) {
  if (!fine_c_ok(Cf) || !fine_c_ok(Cout)) return NL_ERR_BAD_ARG;
  if (!w || !b || !packed || ((uintptr_t)packed & 15) != 0) return NL_ERR_BAD_ARG;
  if (packed_bytes < nl_fine_proj_packed_bytes(Cf, Cout)) return NL_ERR_WORKSPACE;
  const FineProjLayout L = fine_proj_layout(Cf, Cout);
  unsigned char* img = (unsigned char*)packed;
  hipStream_t st = (hipStream_t)stream;
  if (const int e = nl_launch_frag_pack(w, Cout, Cf, (unsigned short*)(img + L.hi), (unsigned short*)(img + L.lo), nullptr, nullptr, (float*)(img + L.f32), false, st))
    return e;
  NL_CHECK_HIP(hipMemcpyAsync(img + L.bias, b, (size_t)Cout * 4, hipMemcpyDeviceToDevice, st));
  return NL_OK;
}

int nl_fine_windows(const void* packed, int Cf, int Cout, int precision, const float* feat_nhwc, int B, int Hf, int Wf, const int64_t* b_ids, const int64_t* j_ids,
                    int64_t M, int stride, float* out, void* stream) {
  if (M < 0 || stride < 1 || B < 1 || Hf < 1 || Wf < 1 || !fine_c_ok(Cf) || !fine_c_ok(Cout)) return NL_ERR_BAD_ARG;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (M > FINE_MAX_M || (int64_t)B * Hf * Wf > ((int64_t)1 << 40)) return NL_ERR_UNSUPPORTED;
  if (M == 0) return NL_OK;
  if (!packed || !feat_nhwc || !b_ids || !j_ids || !out) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)packed | (uintptr_t)feat_nhwc) & 15) != 0 || (((uintptr_t)b_ids | (uintptr_t)j_ids) & 7) != 0 || ((uintptr_t)out & 3) != 0) return NL_ERR_BAD_ARG;
  FineWinArgs a;
  a.img = (const unsigned char*)packed;
  a.feat = feat_nhwc;
  a.b_ids = (const long long*)b_ids; a.j_ids = (const long long*)j_ids;
  a.out = out;
  a.B = B; a.Hf = Hf; a.Wf = Wf; a.Cf = Cf; a.Cout = Cout; a.M = (int)M; a.stride = stride;
  a.Lx = (Wf - 1) / stride + 1;
  a.L = ((Hf - 1) / stride + 1) * a.Lx;
  a.Q = ((Cout >> 5) + 1) >> 1;
  a.dense = 0;
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)nl_cdiv(M * a.Q, 4);   // sized by M: a device-wide persistent grid would idle at a few thousand tiles
  if (precision == NL_PREC_F32) hipLaunchKernelGGL(fine_win_f32_kernel, dim3(grid), dim3(256), 0, st, a);
  else if (precision == NL_PREC_BF16X3) hipLaunchKernelGGL(fine_win_bf16_kernel<true>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(fine_win_bf16_kernel<false>, dim3(grid), dim3(256), 0, st, a);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

int nl_fine_match(const void* packed_mlp, int C, int precision, const float* feat_f0, const float* feat_f1, int64_t M, const float* mkps2d_c, float* expec_f,
                  float* mkps2d_f, float* heatmap, void* stream) {
  if (M < 0 || !fine_c_ok(C)) return NL_ERR_BAD_ARG;
  if (const int ps = nl_prec_status_no_mx(precision)) return ps;
  if (M > FINE_MAX_M) return NL_ERR_UNSUPPORTED;
  if (M == 0) return NL_OK;
  if (!packed_mlp || !feat_f0 || !feat_f1 || !mkps2d_c || !expec_f || !mkps2d_f) return NL_ERR_BAD_ARG;
  if ((((uintptr_t)packed_mlp | (uintptr_t)feat_f0 | (uintptr_t)feat_f1) & 15) != 0) return NL_ERR_BAD_ARG;   // read as 16-byte pieces
  if ((((uintptr_t)mkps2d_c | (uintptr_t)expec_f | (uintptr_t)mkps2d_f | (uintptr_t)heatmap) & 3) != 0) return NL_ERR_BAD_ARG;
  FineMatchArgs a;
  a.img = (const unsigned char*)packed_mlp;
  a.f0 = feat_f0; a.f1 = feat_f1; a.kc = mkps2d_c;
  a.expec = expec_f; a.kf = mkps2d_f; a.heat = heatmap;
  a.M = (int)M; a.C = C;
  a.temp = (float)(1.0 / sqrt((double)C));
  hipStream_t st = (hipStream_t)stream;
  const unsigned grid = (unsigned)nl_cdiv(M, 4);
  if (precision == NL_PREC_F32) {
    static std::atomic<unsigned long long> lds_set{0};
    if (const int e = nl_allow_dynamic_lds((const void*)fine_match_f32_kernel, S2D_F32_LDS, lds_set)) return e;
    hipLaunchKernelGGL(fine_match_f32_kernel, dim3(grid), dim3(256), S2D_F32_LDS, st, a);
  } else if (precision == NL_PREC_BF16X3) {
    hipLaunchKernelGGL((fine_match_bf16_kernel<true, true>), dim3(grid), dim3(256), 0, st, a);
  } else {
    hipLaunchKernelGGL((fine_match_bf16_kernel<false, false>), dim3(grid), dim3(256), 0, st, a);
  }
  NL_LAUNCH_CHECK();
  return NL_OK;
}

}  // extern "C"
