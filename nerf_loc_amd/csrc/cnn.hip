// libnerfloc_cnn.so — the per-frame visibility encoder DepthFusionNet (include/nerfloc_cnn.h is the contract; this file is its only unit).
//
// Five kernels make the whole chain:
//   cnn_conv_kernel<KS, NB>       implicit-GEMM convolution on v_mfma_f32_32x32x2_f32.  A workgroup (4 waves) owns 128 consecutive output pixels of ONE view and all
//                                 32 NB output channels; wave w owns pixels 32 w .. 32 w + 31.  The weights are the A operand (rows = output channels), the gathered
//                                 input patches the B operand (columns = pixels): an accumulator register then holds one channel of 32 consecutive pixels across
//                                 the lanes, and the NCHW store is 128 contiguous bytes per half-wave.  K = (in, ky, kx) is walked in steps of 16: the next step's
//                                 operands are fetched into registers under the current step's MFMAs, then go through LDS ([k][pixel] and [k][channel]).
//                                 The gather reflects at the border and reads two sources for a concat.  The output is the raw sum.  The output channels
//                                 are dealt to workgroups 32, 64 or 128 at a time (grid z).
//   cnn_in_stats_kernel           one workgroup per (view, channel) plane: mean, then the squared deviations from that mean, -> (mean, gamma / sqrt(var + eps), beta);
//                                 where the map's only readers want act(IN(x)), the same workgroup rewrites the plane in place.
//   cnn_up2_kernel                the bilinear x 2 in front of upconv3 and upconv2, materialised (inside the consumer's gather it cost four loads per value).
//   cnn_block_tail_kernel         ReLU(IN(b) + identity) of a BasicBlock, materialised (it is read by two consumers, and it is what `taps` hands out).
//   cnn_head_kernel               ELU(IN(iconv2)) -> out_conv, depth_skip on channel 3 of the input, conv_out: one thread per output pixel, weights in LDS.
// The kernels, the weight table, make_plan and the launch helpers live in cnn_kernels.h, which cnn_train.hip includes too.
#include "cnn_kernels.h"

extern "C" {

int nlc_abi_version(void) { return NLC_ABI_VERSION; }

int nlc_dfnet_num_weights(void) { return table().n; }

const char* nlc_dfnet_weight_name(int i) { return i >= 0 && i < table().n ? table().w[i].name : nullptr; }

size_t nlc_dfnet_packed_bytes(void) { return nl_align_up(table().total * sizeof(float), 256); }

int nlc_dfnet_pack_weights(const void* const* ptrs, int n, void* packed, size_t packed_bytes, void* stream) {
  const CnnTable& t = table();
  if (!ptrs || n != t.n) return NL_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i)
    if (!ptrs[i] || !aligned(ptrs[i], 4)) return NL_ERR_BAD_ARG;
  if (!packed || !aligned(packed, 256) || packed_bytes < nlc_dfnet_packed_bytes()) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < n; ++i) {
    const CnnWeight& w = t.w[i];
    hipLaunchKernelGGL(cnn_pack_kernel, dim3((unsigned)nl_cdiv((int64_t)w.O * w.K, CNN_THREADS)), dim3(CNN_THREADS), 0, s, (const float*)ptrs[i],
                       (float*)packed + w.off, w.O, w.K / w.T, w.T, w.T > 1 ? 1 : 0);
    NL_LAUNCH_CHECK();
  }
  return NL_OK;
}

size_t nlc_dfnet_workspace_bytes(int V, int H, int W) {
  if (!shape_ok(V, H, W)) return 0;
  return nl_align_up(make_plan(V, H, W).total * sizeof(float), 256);
}

int nlc_dfnet_forward(const void* packed, const float* cnn_in, int V, int H, int W, float* out, const nlc_dfnet_taps* taps, void* ws, size_t ws_bytes,
                      void* stream) {
  if (!shape_ok(V, H, W)) return NL_ERR_UNSUPPORTED;
  if (!packed || !cnn_in || !out || !aligned(packed, 256) || !aligned(cnn_in, 16) || !aligned(out, 4)) return NL_ERR_BAD_ARG;
  if (taps && (!aligned(taps->x1, 4) || !aligned(taps->x2, 4) || !aligned(taps->x3, 4))) return NL_ERR_BAD_ARG;
  if (!ws || !aligned(ws, 256) || ws_bytes < nlc_dfnet_workspace_bytes(V, H, W)) return NL_ERR_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const CnnTable& t = table();
  const CnnPlan p = make_plan(V, H, W);
  const float* pk = (const float*)packed;
  float* w = (float*)ws;
  auto wt = [&](int i) { return pk + t.w[i].off; };
  int launches = 0;

  // one convolution: sources s0 (+ s1), planes hin x win, -> y (V, cout, ho, wo)
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
  auto run_stats = [&](float* x, int C, int n, int gamma_idx, int act, float* nrm) -> int {
    hipLaunchKernelGGL(cnn_in_stats_kernel, dim3((unsigned)C, (unsigned)V), dim3(CNN_THREADS), 0, s, x, n, wt(gamma_idx), wt(gamma_idx + 1), act, nrm);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  auto run_up2 = [&](const float* x, int C, int hh, int ww, float* y) -> int {   // (V, C, hh, ww) -> (V, C, 2 hh, 2 ww)
    hipLaunchKernelGGL(cnn_up2_kernel, dim3((unsigned)nl_cdiv(4 * hh * ww, CNN_THREADS), (unsigned)(V * C)), dim3(CNN_THREADS), 0, s, x, hh, ww,
                       (float)(hh - 1) / (float)(2 * hh - 1), (float)(ww - 1) / (float)(2 * ww - 1), y);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
  auto run_tail = [&](const float* b, const float* nb, const float* idn, const float* nd, int C, int n, float* y, float* tap) -> int {
    hipLaunchKernelGGL(cnn_block_tail_kernel, dim3((unsigned)nl_cdiv(n, CNN_THREADS), (unsigned)(V * C)), dim3(CNN_THREADS), 0, s, b, nb, idn, nd, n, y, tap);
    ++launches;
    NL_LAUNCH_CHECK();
    return NL_OK;
  };
#define CNN_TRY(expr) do { const int st_ = (expr); if (st_ != NL_OK) return st_; } while (0)
  const CnnSrc none = {nullptr, 0};
  int h, wd, ho, wo;

  // conv1 + bn1 + ReLU
  CNN_TRY(run_conv(CnnSrc{cnn_in, 12}, none, W_CONV1, 8, 2, 2, 32, H, W, w + p.c0, h, wd));
  CNN_TRY(run_stats(w + p.c0, 32, h * wd, W_BN1, CNN_ACT_RELU, w + p.nc0));
  CnnSrc x = {w + p.c0, 32};

  // layer1 .. layer3
  float* tap[3] = {taps ? taps->x1 : nullptr, taps ? taps->x2 : nullptr, taps ? taps->x3 : nullptr};
  for (int L = 0; L < 3; ++L) {
    const int C = 32 << L, b0 = w_block(L + 1, 0), b1 = w_block(L + 1, 1);
    // block 0: stride 2, identity through downsample; b and d stay raw, the tail applies their InstanceNorms
    CNN_TRY(run_conv(x, none, b0 + 0, 3, 2, 1, C, h, wd, w + p.a[L], ho, wo));
    CNN_TRY(run_stats(w + p.a[L], C, ho * wo, b0 + 1, CNN_ACT_RELU, w + p.na[L][0]));
    CNN_TRY(run_conv(x, none, b0 + 6, 1, 2, 0, C, h, wd, w + p.d[L], ho, wo));
    CNN_TRY(run_stats(w + p.d[L], C, ho * wo, b0 + 7, CNN_ACT_NONE, w + p.nd[L]));
    h = ho; wd = wo;
    CNN_TRY(run_conv(CnnSrc{w + p.a[L], C}, none, b0 + 3, 3, 1, 1, C, h, wd, w + p.b[L], ho, wo));
    CNN_TRY(run_stats(w + p.b[L], C, h * wd, b0 + 4, CNN_ACT_NONE, w + p.nb[L][0]));
    CNN_TRY(run_tail(w + p.b[L], w + p.nb[L][0], w + p.d[L], w + p.nd[L], C, h * wd, w + p.y[L], nullptr));
    // block 1: stride 1, plain identity
    CNN_TRY(run_conv(CnnSrc{w + p.y[L], C}, none, b1 + 0, 3, 1, 1, C, h, wd, w + p.a[L], ho, wo));
    CNN_TRY(run_stats(w + p.a[L], C, h * wd, b1 + 1, CNN_ACT_RELU, w + p.na[L][1]));
    CNN_TRY(run_conv(CnnSrc{w + p.a[L], C}, none, b1 + 3, 3, 1, 1, C, h, wd, w + p.b[L], ho, wo));
    CNN_TRY(run_stats(w + p.b[L], C, h * wd, b1 + 4, CNN_ACT_NONE, w + p.nb[L][1]));
    CNN_TRY(run_tail(w + p.b[L], w + p.nb[L][1], w + p.y[L], nullptr, C, h * wd, w + p.x[L], tap[L]));
    x = CnnSrc{w + p.x[L], C};
  }
  // here h x wd = H/16 x W/16 and x = x3

  // decoder (conv biases in front of an InstanceNorm cancel: not read)
  CNN_TRY(run_up2(x.x, 128, h, wd, w + p.up3));
  h *= 2; wd *= 2;
  CNN_TRY(run_conv(CnnSrc{w + p.up3, 128}, none, W_DEC + 0, 3, 1, 1, 64, h, wd, w + p.u3, ho, wo));
  CNN_TRY(run_stats(w + p.u3, 64, h * wd, W_DEC + 2, CNN_ACT_ELU, w + p.nu3));
  CNN_TRY(run_conv(CnnSrc{w + p.u3, 64}, CnnSrc{w + p.x[1], 64}, W_DEC + 4, 3, 1, 1, 64, h, wd, w + p.i3, ho, wo));
  CNN_TRY(run_stats(w + p.i3, 64, h * wd, W_DEC + 6, CNN_ACT_ELU, w + p.ni3));
  CNN_TRY(run_up2(w + p.i3, 64, h, wd, w + p.up2));
  h *= 2; wd *= 2;
  CNN_TRY(run_conv(CnnSrc{w + p.up2, 64}, none, W_DEC + 8, 3, 1, 1, 32, h, wd, w + p.u2, ho, wo));
  CNN_TRY(run_stats(w + p.u2, 32, h * wd, W_DEC + 10, CNN_ACT_ELU, w + p.nu2));
  CNN_TRY(run_conv(CnnSrc{w + p.u2, 32}, CnnSrc{w + p.x[0], 32}, W_DEC + 12, 3, 1, 1, 32, h, wd, w + p.i2, ho, wo));
  CNN_TRY(run_stats(w + p.i2, 32, h * wd, W_DEC + 14, CNN_ACT_ELU, w + p.ni2));
#undef CNN_TRY

  // out_conv, depth_skip, conv_out
  CnnHeadArgs ha;
  ha.i2 = w + p.i2; ha.cnn_in = cnn_in;
  ha.ocw = wt(W_OUTCONV); ha.ocb = wt(W_OUTCONV + 1); ha.d0w = wt(W_DS0); ha.d0b = wt(W_DS0 + 1); ha.d2w = wt(W_DS2); ha.d2b = wt(W_DS2 + 1);
  ha.cow = wt(W_CONVOUT); ha.cob = wt(W_CONVOUT + 1);
  ha.out = out; ha.H = H; ha.W = W; ha.hq = H / 4; ha.wq = W / 4;
  hipLaunchKernelGGL(cnn_head_kernel, dim3((unsigned)nl_cdiv((int64_t)ha.hq * ha.wq, CNN_THREADS), (unsigned)V), dim3(CNN_THREADS), 0, s, ha);
  ++launches;
  NL_LAUNCH_CHECK();
  return launches == NLC_DFNET_LAUNCHES ? NL_OK : NL_ERR_HIP;
}

}  // extern "C"
