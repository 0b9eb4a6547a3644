// The packed weight blob of libnerfloc_render.so: the weight table, the blob's layout (make_layout), the kernels that write its images and nl_pack_weights —
// and the fragment packer of the localisation head's images (nl_launch_frag_pack: s2d.hip, fine.hip, sct.hip).
#include <stddef.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <unordered_map>
#include "common.h"
#include "mfma.h"
#include "host.h"
using namespace nlhost;

namespace nlhost {

// ------------------------------------------------------------------------------------------ weight table
const char* kWeightNames[] = {
    "ray_diff_fc.0.weight", "ray_diff_fc.0.bias", "ray_diff_fc.2.weight", "ray_diff_fc.2.bias",
#define NL_DEC(d)                                                                                                         \
  "multiview_aggregator.dist_decoder." d "_decoder.0.weight", "multiview_aggregator.dist_decoder." d "_decoder.0.bias",   \
  "multiview_aggregator.dist_decoder." d "_decoder.2.weight", "multiview_aggregator.dist_decoder." d "_decoder.2.bias",   \
  "multiview_aggregator.dist_decoder." d "_decoder.4.weight", "multiview_aggregator.dist_decoder." d "_decoder.4.bias"
    NL_DEC("mean"), NL_DEC("var"), NL_DEC("aw"), NL_DEC("vis"),
#undef NL_DEC
    "multiview_aggregator.out_fc.0.weight", "multiview_aggregator.out_fc.0.bias",
    "multiview_aggregator.out_fc.2.weight", "multiview_aggregator.out_fc.2.bias",
    "base_mlp.0.weight", "base_mlp.0.bias", "base_mlp.2.weight", "base_mlp.2.bias", "base_mlp.4.weight", "base_mlp.4.bias",
    "base_mlp_attn.w_qs.weight", "base_mlp_attn.w_ks.weight", "base_mlp_attn.w_vs.weight", "base_mlp_attn.fc.weight",
    "base_mlp_attn.layer_norm.weight", "base_mlp_attn.layer_norm.bias",
#define NL_UN(n) "ray_unet." n ".0.weight", "ray_unet." n ".0.bias", "ray_unet." n ".1.weight", "ray_unet." n ".1.bias"
    NL_UN("conv1"), NL_UN("conv2"), NL_UN("conv3"), NL_UN("trans_conv3"), NL_UN("trans_conv2"), NL_UN("trans_conv1"), NL_UN("conv_out"),
#undef NL_UN
    "sigma_mlp.0.weight", "sigma_mlp.0.bias",
    "feat_mlp.0.weight", "feat_mlp.0.bias", "feat_mlp.2.weight", "feat_mlp.2.bias",
    "rgb_blending_mlp.0.weight", "rgb_blending_mlp.0.bias", "rgb_blending_mlp.2.weight", "rgb_blending_mlp.2.bias",
    "rgb_blending_mlp.4.weight", "rgb_blending_mlp.4.bias",
};
static_assert(sizeof(kWeightNames) / sizeof(kWeightNames[0]) == kNumWeights, "weight table");

bool cfg_ok(const nl_config* c) {
  return c && c->W >= 32 && c->W <= 256 && c->W % 32 == 0 && c->C > 0 && c->C <= 192 && c->S >= 8 && c->S <= 256 && c->S % 8 == 0 &&
         c->precision >= 0 && c->precision <= 2;   // (NL_PREC_F16MX is normalised to BF16X3 + a flag at every entry point: NL_EFF_CFG)
}

Layout make_layout(const nl_config* c) {
  Layout L;
  memset(&L, 0, sizeof(L));
  const int W = c->W, C = c->C, F = C + 3, S = c->S;
  auto set = [&](int i, int K, int N, bool bias) { L.g[i] = {K, N, (int)nl_align_up(K, 32), (int)nl_align_up(N, 32), bias}; };
  set(G_OUTFC0, 2 * F + 3, 64, true);
  set(G_OUTFC2, 64, W, true);
  set(G_BASE0, F + 90, W, true);
  set(G_BASE2, W, W, true);
  set(G_BASE4, W, W, true);
  set(G_KV, W, 256, false);
  set(G_Q, W, 128, false);
  set(G_FC, 128, W, false);
  set(G_CONV1, 3 * W, 64, true);
  set(G_CONV2, 3 * 64, 128, true);
  set(G_CONV3, 3 * 128, 128, true);
  set(G_T3E, 128, 128, true);
  set(G_T3O, 256, 128, true);
  set(G_T2E, 256, 64, true);
  set(G_T2O, 512, 64, true);
  set(G_T1E, 128, 32, true);
  set(G_T1O, 256, 32, true);
  // both output phases of a stride-2 transposed convolution as ONE GEMM: K = [x[m] | x[m+1]], N = [even outputs | odd outputs]
  // (the even phase's second K half is zero: 33 % more MACs for half the launches and one pass over the activations)
  set(G_T3M, 256, 256, true);
  set(G_T2M, 512, 128, true);
  set(G_T1M, 256, 64, true);
  // feat_mlp.0 and the blend projection with K in ACCUMULATOR order, for the per-sample chain kernel (tgemm.hip: sample_chain_kernel)
  set(G_FEAT0P, W, W, true);
  set(G_BLENDAP, W, 32, false);
  set(G_QP, W, 128, false);
  set(G_CONVOUT, 3 * (W + 32), W, true);
  set(G_CONV1F, 3 * W, 64, true);
  set(G_CONVOUTF, 3 * (W + 32), W, true);
  set(G_FEAT0, W, W, true);
  // feat_mlp's last Linear is applied AFTER compositing (it is linear): K = [composited hidden (W) | sum of weights (1)],
  // the bias row multiplies the weight sum (model.py:594-597)
  set(G_FEAT2, W + 32, C, false);
  // colour-blend layer 1 split by linearity (model.py:532-535): per-sample part (feature_agg columns), and a per-frame
  // projection of the support feature maps through the feature columns (G_BLENDP, applied once per frame; the
  // per-(sample, view) value is then a bilinear tap of the projected map inside mv_stats)
  set(G_BLENDA, W, 32, false);
  set(G_BLENDP, C, 32, false);
  // per-frame neural-point table T = sp_feature . base_mlp.0.weight[:, :F]^T + bias, columns in accumulator order (point_fused.hip)
  set(G_PTT, F, W, true);
  // dX = dY . W for y = x W^T: K = the layer's outputs, N = its inputs; base_mlp.0 only towards its posenc + ray_diff_fc columns
  // (the feature columns multiply rows of the frozen support table)
  set(G_FC_T, W, 128, false);
  set(G_Q_T, 128, W, false);
  set(G_KV_T, 256, W, false);
  set(G_BASE4_T, W, W, false);
  set(G_BASE2_T, W, W, false);
  set(G_BASE0_T, W, 96, false);
  set(G_BASE0_TF, W, F, false);
  set(G_BASE0_S, 90, W, false);
  set(G_FEAT0_T, W, W, false);
  set(G_FEAT2_T, C, W, false);
  set(G_OUTFC2_T, W, 64, false);
  set(G_OUTFC0_T, 64, (int)nl_align_up(2 * F + 3, 32), false);   // = ldg_of(C): the statistics row incl. its zero padding (416 columns: generic kernels)
  set(G_BLENDA_T, 32, W, false);
  // convolution input gradients: K = the layer's output channels x 3 taps (transposed convolutions: [even | odd | odd of the previous position])
  set(G_UB_OUTA, 3 * W, W, false);   // conv_out -> its feature_agg input channels
  set(G_UB_OUTB, 3 * W, 32, false);  // conv_out -> its x2 input channels
  set(G_UB_T1, 96, 128, false);
  set(G_UB_T2, 192, 256, false);
  set(G_UB_T3, 384, 128, false);
  set(G_UB_C3, 384, 128, false);
  set(G_UB_C2, 384, 64, false);
  set(G_UB_C1, 192, W, false);
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += nl_align_up(bytes, 256); return o; };
  for (int i = 0; i < G_COUNT; ++i) {
    const size_t n = (size_t)L.g[i].Kpad * L.g[i].Npad;
    L.b32[i] = take(n * 4);
    L.bhi[i] = take(n * 2);
    L.blo[i] = take(n * 2);
    L.bst[i] = take(L.g[i].N <= 256 ? nl_tgemm_stream_bytes(L.g[i].Kpad, L.g[i].N) : 0);
    L.bsh[i] = take(L.g[i].N <= 256 ? nl_tgemm_stream_bytes(L.g[i].Kpad, L.g[i].N) : 0);
    L.bias[i] = take((size_t)L.g[i].Npad * 4);
  }
  L.rd_w = take(4 * (64 + 16 + 27 * 16 + 27));
  L.dec_w = take(4 * 4 * 2178);
  L.sig_w = take(4 * W); L.sig_b = take(4);
  L.bl2_w = take(4 * 512); L.bl2_b = take(4 * 16); L.bl4_w = take(4 * 16); L.bl4_b = take(4);
  L.ln_g = take(4 * W); L.ln_b = take(4 * W);
  const int uc[U_COUNT] = {64, 128, 128, 128, 64, 32, W};
  const int ul[U_COUNT] = {S, S / 2, S / 4, S / 4, S / 2, S, S};
  for (int u = 0; u < U_COUNT; ++u) {
    L.un_c[u] = uc[u]; L.un_l[u] = ul[u];
    L.un_g[u] = take(4 * (size_t)uc[u] * ul[u]);
    L.un_b[u] = take(4 * (size_t)uc[u] * ul[u]);
    // the fused GEMM's view of the slab: a transposed convolution's merged launch has rows = input positions, columns = both phases
    const bool tr = u == U_T3 || u == U_T2 || u == U_T1;
    L.un_n[u] = tr ? 2 * uc[u] : uc[u];
    L.un_so[u] = tr ? ul[u] / 2 : ul[u];
    const size_t lm = 4 * (size_t)(L.un_so[u] > 32 ? L.un_so[u] : 32) * nl_tgemm_nrt(L.un_n[u]) * 32;
    L.un_gl[u] = take(lm);
    L.un_bl[u] = take(lm);
  }
  L.blw = take(4 * (256 + 32));
  L.dec_mfma = take(nl_mv_decoder_pack_bytes());
  L.pt_bias = take(4 * 3 * (size_t)W);
  L.pt_stream = take((W == 64 || W == 128 || W == 256) ? nl_point_stream_bytes(W) : 256);
  L.pt_stream2 = take((W == 128 || W == 256) ? nl_point_stream2_bytes(W) : 256);
  L.pt_stream2_mx = take((W == 128 || W == 256) ? nl_point_stream2_bytes(W) : 256);   // NL_PREC_F16MX: f16 fragments + MX-FP6 images of every layer
  L.pt_stream2_f16 = take((W == 128 || W == 128 * 2) ? nl_point_stream2_bytes(W) : 256);  // split-FP16 stream: the gradient path's fused forward (pt_forward_keep_fused)
  L.pt_bwd_stream = take(nl_point_bwd_chain_supported(W) ? nl_point_bwd_stream_bytes(W) : 256);   // transposed weights of the branch's rows: the frozen-weight way back (point_bwd.hip)
  L.mvf_pack = take(nl_mv_front_pack_bytes());                                          // out_fc.0 as register-resident A fragments of mv_front_kernel (C = 192)
  L.zeros = take(4096);
  L.mx_convout = take(W == 256 ? nl_tgemm_mx_image_bytes(L.g[G_CONVOUTF].Kpad) : 0);
  L.mx_feat0 = take(W == 256 ? nl_tgemm_mx_image_bytes(L.g[G_FEAT0P].Kpad) : 0);
  L.total = off;
  return L;
}

}  // namespace nlhost

namespace {

// ------------------------------------------------------------------------------------------ pack kernels

// dst[k0+k][n] (f32 [Kpad][Npad]) and bf16 hi/lo [n][Kpad] <- src[off + n*ld_n + k*ld_k], k < kc, n < N
__global__ void pack_block_kernel(const float* __restrict__ src, int off, int ld_n, int ld_k, int kc, int N, int k0,
                                  float* __restrict__ b32, unsigned short* __restrict__ bhi, unsigned short* __restrict__ blo,
                                  int Kpad, int Npad, unsigned short* __restrict__ bst, int nrts, int n0, int perm = 0,
                                  unsigned short* __restrict__ bsh = nullptr) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= kc * N) return;
  int k = i / N, n = i - k * N;
  // perm (k0 == 0 only): K position k of the packed matrix holds source column 32 c + m(8 ks + t, hh) for k = 32 c + 16 ks + 8 hh + t,
  // m(r, hh) = (r & 3) + 8 (r >> 2) + 4 hh — the order in which a 32x32 accumulator tile hands its rows to the next MFMA as B operand
  int ksrc = k;
  if (perm) { const int r = 8 * ((k >> 4) & 1) + (k & 7), hh = (k >> 3) & 1; ksrc = (k & ~31) + (r & 3) + 8 * (r >> 2) + 4 * hh; }   // (nl_acc_row written out: as one parenthesised term the sum associates differently and the kernel compiles to other code)
  float v = src[off + (size_t)n * ld_n + (size_t)ksrc * ld_k];
  b32[(size_t)(k0 + k) * Npad + n] = v;
  unsigned short h = nl_f2bf(v);
  float hf = __uint_as_float(((unsigned int)h) << 16);
  bhi[(size_t)n * Kpad + k0 + k] = h;
  const unsigned short l = nl_f2bf(v - hf);
  blo[(size_t)n * Kpad + k0 + k] = l;
  // weight stream of tgemm.hip: chunk (32 k) = [part hi/lo][k-step][row tile][lane = (n&31) + 32*((k>>3)&1)][k&7]
  if (!bst) return;   // (matrices wider than 256 columns have no streaming layout: generic kernels only)
  const int kk = k0 + k, ng = n0 + n;
  const size_t e = (size_t)(kk >> 5) * (4 * nrts * 512) + ((size_t)(((kk >> 4) & 1) * nrts + (ng >> 5)) * 64 + (ng & 31) + 32 * ((kk >> 3) & 1)) * 8 + (kk & 7);
  bst[e] = h;
  bst[e + (size_t)2 * nrts * 512] = l;
  if (bsh) {   // the same stream in fp16: hi = round(v), lo = round(v - hi)
    const _Float16 g = (_Float16)v;
    bsh[e] = __builtin_bit_cast(unsigned short, g);
    bsh[e + (size_t)2 * nrts * 512] = __builtin_bit_cast(unsigned short, (_Float16)(v - (float)g));
  }
}

// MX-FP6 images of a 256-column layer for tgemm_mx_kernel (tgemm.hip): one thread = one MX block = (slab of 64 k, row tile, lane, image).  The 32 weights of output
// column 32 rt + (lane & 31) whose k-slots belong to half lane >> 5 of the slab, in the natural position order P = 8 s + t <-> k = 64 slab + 16 s + 8 hh + t (what the
// kernel's activation images have): image 0 = e2m3(f16(w)) (meets the activations' residual image), image 1 = e2m3(w - f16(w)) (meets their hi image).  Block scale
// 2^(floor(log2 max) - 2): the largest magnitude lands in [4, 8) (e2m3 saturates at 7.5).  Per slab: [rt][image][lane] dwords 0-3 (16 KB) | [rt][image][lane]
// {dword 4, dword 5, E8M0 scale, 0} (16 KB).  K rows past Kpad are zero.
__global__ void pack_tgemm_mx6_kernel(const float* __restrict__ b32, int Kpad, int Npad, int N, int nslab, unsigned char* __restrict__ out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= nslab * 8 * 64 * 2) return;
  const int im = e & 1, lane = (e >> 1) & 63, rt = (e >> 7) & 7, sl = e >> 10;
  const int hh = lane >> 5, n = 32 * rt + (lane & 31);
  float v[32], mx = 0.f;
  for (int P = 0; P < 32; ++P) {
    const int k = 64 * sl + 16 * (P >> 3) + 8 * hh + (P & 7);
    const float w = (k < Kpad && n < N) ? b32[(size_t)k * Npad + n] : 0.f;
    const float h = (float)(_Float16)w;
    v[P] = im == 0 ? h : w - h;
    mx = fmaxf(mx, fabsf(v[P]));
  }
  int E = -60;
  if (mx > 0.f) { int ex; (void)frexpf(mx, &ex); E = ex - 1; }   // mx = 1.xxx 2^E
  int sb = E - 2 + 127;
  sb = sb < 1 ? 1 : (sb > 254 ? 254 : sb);
  const float inv = ldexpf(1.f, 127 - sb);
  unsigned d[6] = {0u, 0u, 0u, 0u, 0u, 0u};
  for (int P = 0; P < 32; ++P) {
    const unsigned c = nl_e2m3(fabsf(v[P]) * inv) | (v[P] < 0.f ? 32u : 0u);
    const int b = 6 * P;
    d[b >> 5] |= c << (b & 31);
    if ((b & 31) > 26) d[(b >> 5) + 1] |= c >> (32 - (b & 31));
  }
  unsigned char* base = out + (size_t)sl * (16384 + 16384);
  unsigned* a = reinterpret_cast<unsigned*>(base + ((size_t)(rt * 2 + im) * 64 + lane) * 16);
  a[0] = d[0]; a[1] = d[1]; a[2] = d[2]; a[3] = d[3];
  unsigned* b2 = reinterpret_cast<unsigned*>(base + 16384 + ((size_t)(rt * 2 + im) * 64 + lane) * 16);
  b2[0] = d[4]; b2[1] = d[5]; b2[2] = (unsigned)sb; b2[3] = 0u;   // (the matrix instruction reads byte 0 of the scale register)
}

// [32][8] = rgb(3) | vis(1) | angle(4) columns of rgb_blending_mlp.0.weight (32, W+F+5), then its bias[32]
__global__ void pack_blw_kernel(const float* __restrict__ w, const float* __restrict__ b, float* __restrict__ dst, int W, int F) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 256) {
    const int j = i >> 3, c = i & 7;
    const int col = c < 3 ? W + c : W + F + (c - 3);
    dst[i] = w[(size_t)j * (W + F + 5) + col];
  } else if (i < 288) dst[i] = b[i - 256];
}

// dst[l][c] = src[c][l]: LayerNorm([C, L]) affine tables, stored position-major like the activations
__global__ void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int Cc, int L) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Cc * L) return;
  const int l = i / Cc, c = i - l * Cc;
  dst[i] = src[(size_t)c * L + l];
}

// LayerNorm affine table (So positions x N channels, position-major) -> the order in which tgemm_kernel's LNSLAB epilogue reads it:
// [wave of the ray][row tile][gq][lane][4]: lane (j, hh) of wave w holds position (32 w + j) % So, channels 32 rt + 8 gq + 4 hh + 0..3 — one
// contiguous KB per load instruction instead of 64 rows
__global__ void ln_lane_major_kernel(const float* __restrict__ src, float* __restrict__ dst, int N, int So, int NRT, int total) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int i = e & 3, lane = (e >> 2) & 63, gq = (e >> 8) & 3, rt = (e >> 10) % NRT, wq = e / (1024 * NRT);
  const int j = lane & 31, hh = lane >> 5, n = 32 * rt + 8 * gq + 4 * hh + i, t = (32 * wq + j) % So;
  dst[e] = n < N ? src[(size_t)t * N + n] : 0.f;
}

__global__ void copy_kernel(const float* __restrict__ src, float* __restrict__ dst, int n) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) dst[i] = src[i];
}

// An N x K row-major fp32 matrix into up to five planes of N * K elements each, in mfma.h's fragment maps: bf16 hi / lo and fp16 hi / lo (nl_frag16_src; acc_order:
// its permuted form) and fp32 (nl_frag32_src).  A null plane is not stored; both maps are walked whatever planes exist.
struct FragPackArgs {
  const float* w;
  unsigned short *bf_hi, *bf_lo, *f16_hi, *f16_lo;
  float* f32;
  int N, K, acc_order;
};
__global__ __launch_bounds__(256) void frag_pack_kernel(const FragPackArgs a) {
  const int nrb = a.N >> 5, n = a.N * a.K;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    nl_store_split(a.w[nl_frag16_src(i, nrb, a.K, a.acc_order != 0)], i, a.bf_hi, a.bf_lo, a.f16_hi, a.f16_lo);
    if (a.f32) a.f32[i] = a.w[nl_frag32_src(i, nrb, a.K)];
  }
}

struct Packer {
  const float* const* t;
  char* base;
  const Layout* L;
  hipStream_t st;
  int rc = NL_OK;
  uint64_t has_bst = 0, has_bsh = 0;   // layers whose streaming images this pass wrote
  void mark(int g, bool bsh) { if (L->g[g].N <= 256) { has_bst |= 1ull << g; if (bsh) has_bsh |= 1ull << g; } }
  void block(int g, int k0, const float* src, int off, int ld_n, int ld_k, int kc, int perm = 0) {
    const GemmDim& d = L->g[g];
    mark(g, true);
    int n = kc * d.N;
    hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(n, 256)), dim3(256), 0, st, src, off, ld_n, ld_k, kc, d.N, k0,
                       (float*)(base + L->b32[g]), (unsigned short*)(base + L->bhi[g]), (unsigned short*)(base + L->blo[g]), d.Kpad, d.Npad,
                       (unsigned short*)(base + L->bst[g]), nl_tgemm_nrt(d.N), 0, perm, d.N <= 256 ? (unsigned short*)(base + L->bsh[g]) : nullptr);
  }
  void copy(const float* src, size_t dst_off, int n) {
    hipLaunchKernelGGL(copy_kernel, dim3((unsigned)nl_cdiv(n, 256)), dim3(256), 0, st, src, (float*)(base + dst_off), n);
  }
  void transpose(const float* src, size_t dst_off, int Cc, int Lp) {
    hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)nl_cdiv(Cc * Lp, 256)), dim3(256), 0, st, src, (float*)(base + dst_off), Cc, Lp);
  }
  void lane_major(size_t src_off, size_t dst_off, int N, int So) {
    const int nrt = nl_tgemm_nrt(N), total = (So > 32 ? So : 32) * nrt * 32;
    hipLaunchKernelGGL(ln_lane_major_kernel, dim3((unsigned)nl_cdiv(total, 256)), dim3(256), 0, st, (const float*)(base + src_off), (float*)(base + dst_off),
                       N, So, nrt, total);
  }
  void linear(int g, const float* w, const float* b) {  // torch (out, in)
    block(g, 0, w, 0, L->g[g].K, 1, L->g[g].K);
    if (b) copy(b, L->bias[g], L->g[g].N);
  }
  // conv taps over concatenated sources: weight (co, ci, 3); K index = tap-major then source channels
  // K order = per source (channel range [c0, c0 + wd) of the ci input channels), per 32-channel block, per tap: see NlGemmSeg::ntap
  // perm_mask bit s: source s arrives as a fragment image (NlGemmSeg::frag): its 32-channel blocks in accumulator order (pack_block_kernel: perm)
  void conv3(int g, const float* w, const float* b, int ci, const int* widths, int nsrc, unsigned perm_mask = 0) {
    int k0 = 0, c0 = 0;
    for (int sidx = 0; sidx < nsrc; ++sidx) {
      for (int cb = 0; cb < widths[sidx] / 32; ++cb)
        for (int j = 0; j < 3; ++j) { block(g, k0, w, (c0 + 32 * cb) * 3 + j, ci * 3, 3, 32, (perm_mask >> sidx) & 1); k0 += 32; }
      c0 += widths[sidx];
    }
    copy(b, L->bias[g], L->g[g].N);
  }
  // transposed conv weight (ci, co, 3): even phase uses tap 1; odd phase taps 2 (ioff 0) then 0 (ioff +1)
  // merged phases (see G_T3M): columns [0, co) = even phase (tap 1 on x[m]), [co, 2 co) = odd phase (tap 2 on x[m], tap 0 on x[m+1])
  void convT_merged(int g, const float* w, const float* b, int ci, int co) {
    const GemmDim& d = L->g[g];
    mark(g, true);
    auto win = [&](int k0, int tap, int n0) {
      const int n = ci * co;
      hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(n, 256)), dim3(256), 0, st, w, tap, 3, co * 3, ci, co, k0,
                         (float*)(base + L->b32[g]) + n0, (unsigned short*)(base + L->bhi[g]) + (size_t)n0 * d.Kpad,
                         (unsigned short*)(base + L->blo[g]) + (size_t)n0 * d.Kpad, d.Kpad, d.Npad, (unsigned short*)(base + L->bst[g]),
                         nl_tgemm_nrt(d.N), n0, 0, (unsigned short*)(base + L->bsh[g]));
    };
    win(0, 1, 0);
    win(0, 2, co);
    win(ci, 0, co);
    copy(b, L->bias[g], co);
    copy(b, L->bias[g] + 4 * (size_t)co, co);
  }
  // input-gradient weights of Conv1d(k = 3, padding 1), weight (co, ci, 3), for the input channels [n0, n0 + nn): K order [32-co block][tap slot
  // tau][32] like conv3 (NlGemmSeg::ntap), slot tau reads the output-gradient row t + tau - 1 and therefore carries tap 2 - tau
  void conv3_dgrad(int g, const float* w, int co, int ci, int n0, int nn) {
    const GemmDim& d = L->g[g];
    mark(g, false);
    int k0 = 0;
    for (int cb = 0; cb < co / 32; ++cb)
      for (int tau = 0; tau < 3; ++tau) {
        hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(32 * nn, 256)), dim3(256), 0, st, w, 32 * cb * ci * 3 + n0 * 3 + (2 - tau), 3, ci * 3, 32, nn, k0,
                           (float*)(base + L->b32[g]), (unsigned short*)(base + L->bhi[g]), (unsigned short*)(base + L->blo[g]), d.Kpad, d.Npad,
                           (unsigned short*)(base + L->bst[g]), nl_tgemm_nrt(d.N), 0);
        k0 += 32;
      }
  }
  // input-gradient weights of ConvTranspose1d(k = 3, stride 2), weight (ci, co, 3), against the merged-phase gradient rows [even | odd]:
  // K = [even: tap 1 | odd: tap 2 | odd of the previous position: tap 0]
  void convT_dgrad(int g, const float* w, int ci, int co) {
    const GemmDim& d = L->g[g];
    mark(g, false);
    const int taps[3] = {1, 2, 0};
    for (int part = 0; part < 3; ++part)
      hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(co * ci, 256)), dim3(256), 0, st, w, taps[part], co * 3, 3, co, ci, part * co,
                         (float*)(base + L->b32[g]), (unsigned short*)(base + L->bhi[g]), (unsigned short*)(base + L->blo[g]), d.Kpad, d.Npad,
                         (unsigned short*)(base + L->bst[g]), nl_tgemm_nrt(d.N), 0);
  }
  void convT(int ge, int go, const float* w, const float* b, int ci, int co) {
    block(ge, 0, w, 1, 3, co * 3, ci);
    block(go, 0, w, 2, 3, co * 3, ci);
    block(go, ci, w, 0, 3, co * 3, ci);
    copy(b, L->bias[ge], co);
    copy(b, L->bias[go], co);
  }
};

// Every nl_pack_weights call stamps its destination with a fresh generation number (host-side registry keyed by the blob's
// address): the per-frame tables derived from the weights are rebuilt when a blob is RE-packed in place, not only when another
// blob is used.
// ... and the registry remembers WHICH layers of the blob have a streaming-kernel image (bit g: bf16 hi / lo stream, fp16 hi / lo stream): run_gemm keeps a
// product off the streaming kernel when its stream was never written (it would multiply by zeros: the transposed out_fc.0 did, for feature widths whose
// statistics row fits 256 columns, until tools/grad_fuzz.py) — the generic kernels read the plain images every layer has.
std::mutex g_gen_mu;
std::unordered_map<const void*, PackInfo> g_pack_gen;
uint64_t g_gen_next = 1;
void bump_generation(const void* pk) {
  std::lock_guard<std::mutex> lk(g_gen_mu);
  g_pack_gen[pk] = PackInfo{g_gen_next++, 0, 0};
}
void set_pack_streams(const void* pk, uint64_t bst, uint64_t bsh) {
  std::lock_guard<std::mutex> lk(g_gen_mu);
  auto it = g_pack_gen.find(pk);
  if (it != g_pack_gen.end()) { it->second.bst = bst; it->second.bsh = bsh; }
}

}  // namespace

namespace nlhost {

uint64_t pack_generation(const void* pk) {
  std::lock_guard<std::mutex> lk(g_gen_mu);
  auto it = g_pack_gen.find(pk);
  return it == g_pack_gen.end() ? 0 : it->second.gen;
}
PackInfo pack_info(const void* pk) {
  std::lock_guard<std::mutex> lk(g_gen_mu);
  auto it = g_pack_gen.find(pk);
  return it == g_pack_gen.end() ? PackInfo{0, ~0ull, ~0ull} : it->second;   // (a blob this process did not pack, e.g. copied: trusted as complete)
}

}  // namespace nlhost

int nl_launch_frag_pack(const float* w, int N, int K, unsigned short* bf_hi, unsigned short* bf_lo, unsigned short* f16_hi, unsigned short* f16_lo, float* f32,
                        bool acc_order, hipStream_t st) {
  if (!w || N < 32 || (N & 31) != 0 || K < 16 || (K & 15) != 0 || (int64_t)N * K > (1 << 30)) return NL_ERR_BAD_ARG;   // whole fragments; element indices are ints
  const FragPackArgs a{w, bf_hi, bf_lo, f16_hi, f16_lo, f32, N, K, acc_order ? 1 : 0};
  hipLaunchKernelGGL(frag_pack_kernel, dim3(128), dim3(256), 0, st, a);
  NL_LAUNCH_CHECK();
  return NL_OK;
}

extern "C" {

int nl_num_weights(void) { return kNumWeights; }
const char* nl_weight_name(int i) { return (i >= 0 && i < kNumWeights) ? kWeightNames[i] : nullptr; }

size_t nl_packed_weights_bytes(const nl_config* cfg) {
  NL_EFF_CFG(cfg); return cfg_ok(cfg) ? make_layout(cfg).total : 0; }

int nl_pack_weights(const nl_config* cfg, const float* const* t, int n, void* packed, size_t bytes, void* stream) {
  NL_EFF_CFG(cfg);
  if (!cfg_ok(cfg) || !t || n != kNumWeights || !packed) return NL_ERR_BAD_ARG;
  for (int i = 0; i < n; ++i) if (!t[i]) return NL_ERR_BAD_ARG;
  const Layout L = make_layout(cfg);
  if (bytes < L.total) return NL_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  bump_generation(packed);
  NL_CHECK_HIP(hipMemsetAsync(packed, 0, L.total, st));
  Packer P{t, (char*)packed, &L, st};
  const int W = cfg->W, C = cfg->C, F = C + 3;
  P.linear(G_OUTFC0, t[T_OUT0W], t[T_OUT0B]);
  P.linear(G_OUTFC2, t[T_OUT2W], t[T_OUT2B]);
  P.linear(G_BASE0, t[T_B0W], t[T_B0B]);
  P.linear(G_BASE2, t[T_B2W], t[T_B2B]);
  P.linear(G_BASE4, t[T_B4W], t[T_B4B]);
  // KV: columns 0..127 = w_ks rows, 128..255 = w_vs rows
  {
    const GemmDim& d = L.g[G_KV];
    P.mark(G_KV, true);
    for (int half = 0; half < 2; ++half) {
      const float* w = t[half ? T_WV : T_WK];
      int nel = W * 128;
      // reuse pack_block with N=128 into a column window: emulate by offsetting destination pointers
      hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(nel, 256)), dim3(256), 0, st, w, 0, W, 1, W, 128, 0,
                         (float*)((char*)packed + L.b32[G_KV]) + half * 128,
                         (unsigned short*)((char*)packed + L.bhi[G_KV]) + (size_t)half * 128 * d.Kpad,
                         (unsigned short*)((char*)packed + L.blo[G_KV]) + (size_t)half * 128 * d.Kpad, d.Kpad, d.Npad,
                         (unsigned short*)((char*)packed + L.bst[G_KV]), nl_tgemm_nrt(d.N), half * 128, 0, (unsigned short*)((char*)packed + L.bsh[G_KV]));
    }
  }
  P.linear(G_Q, t[T_WQ], nullptr);
  P.linear(G_FC, t[T_FC], nullptr);
  // transposed copies (element [k = output o][n = input i] = w[o][i]): source strides swapped
  P.block(G_FC_T, 0, t[T_FC], 0, 1, 128, W);
  P.block(G_Q_T, 0, t[T_WQ], 0, 1, W, 128);
  {
    const GemmDim& d = L.g[G_KV_T];   // K = [k-projection outputs 128 | v-projection outputs 128]
    P.mark(G_KV_T, false);
    for (int half = 0; half < 2; ++half)
      hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(128 * W, 256)), dim3(256), 0, st, t[half ? T_WV : T_WK], 0, 1, W, 128, W, half * 128,
                         (float*)((char*)packed + L.b32[G_KV_T]), (unsigned short*)((char*)packed + L.bhi[G_KV_T]),
                         (unsigned short*)((char*)packed + L.blo[G_KV_T]), d.Kpad, d.Npad, (unsigned short*)((char*)packed + L.bst[G_KV_T]), nl_tgemm_nrt(d.N), 0);
  }
  P.block(G_BASE4_T, 0, t[T_B4W], 0, 1, W, W);
  P.block(G_BASE2_T, 0, t[T_B2W], 0, 1, W, W);
  {
    const GemmDim& d = L.g[G_BASE0_T];   // columns F .. F+89 of base_mlp.0.weight (W, F + 90); the 6 pad columns stay zero
    P.mark(G_BASE0_T, false);
    hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(W * 90, 256)), dim3(256), 0, st, t[T_B0W], F, 1, F + 90, W, 90, 0,
                       (float*)((char*)packed + L.b32[G_BASE0_T]), (unsigned short*)((char*)packed + L.bhi[G_BASE0_T]),
                       (unsigned short*)((char*)packed + L.blo[G_BASE0_T]), d.Kpad, d.Npad, (unsigned short*)((char*)packed + L.bst[G_BASE0_T]), nl_tgemm_nrt(d.N), 0);
  }
  {
    const GemmDim& d = L.g[G_BASE0_TF];   // columns 0 .. F-1 of base_mlp.0.weight
    P.mark(G_BASE0_TF, false);
    hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(W * F, 256)), dim3(256), 0, st, t[T_B0W], 0, 1, F + 90, W, F, 0,
                       (float*)((char*)packed + L.b32[G_BASE0_TF]), (unsigned short*)((char*)packed + L.bhi[G_BASE0_TF]),
                       (unsigned short*)((char*)packed + L.blo[G_BASE0_TF]), d.Kpad, d.Npad, (unsigned short*)((char*)packed + L.bst[G_BASE0_TF]), nl_tgemm_nrt(d.N), 0);
  }
  P.block(G_BASE0_S, 0, t[T_B0W], F, F + 90, 1, 90);
  P.block(G_OUTFC2_T, 0, t[T_OUT2W], 0, 1, 64, W);
  P.block(G_FEAT0_T, 0, t[T_F0W], 0, 1, W, W);
  P.block(G_FEAT2_T, 0, t[T_F2W], 0, 1, W, C);
  {
    // out_fc.0.weight (64, 2F + 3): element [k = o][n = i].  416 columns at C = 192: generic kernels, no streaming layout; a narrower feature map (C <= 123) puts
    // the product on the streaming kernel, whose weight stream must then exist (it was left zero-filled until tools/grad_fuzz.py: every gradient through the
    // statistics rows vanished for such C in the non-fp32 modes)
    const GemmDim& d = L.g[G_OUTFC0_T];
    const bool stream = d.N <= 256;
    if (stream) P.mark(G_OUTFC0_T, true);
    hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(64 * (2 * F + 3), 256)), dim3(256), 0, st, t[T_OUT0W], 0, 1, 2 * F + 3, 64, 2 * F + 3, 0,
                       (float*)((char*)packed + L.b32[G_OUTFC0_T]), (unsigned short*)((char*)packed + L.bhi[G_OUTFC0_T]),
                       (unsigned short*)((char*)packed + L.blo[G_OUTFC0_T]), d.Kpad, d.Npad,
                       stream ? (unsigned short*)((char*)packed + L.bst[G_OUTFC0_T]) : (unsigned short*)nullptr, nl_tgemm_nrt(d.N), 0, 0,
                       stream ? (unsigned short*)((char*)packed + L.bsh[G_OUTFC0_T]) : (unsigned short*)nullptr);
  }
  {
    const GemmDim& d = L.g[G_BLENDA_T];   // the feature_agg columns of rgb_blending_mlp.0.weight (32, W + F + 5)
    P.mark(G_BLENDA_T, false);
    hipLaunchKernelGGL(pack_block_kernel, dim3((unsigned)nl_cdiv(32 * W, 256)), dim3(256), 0, st, t[T_BL0W], 0, 1, W + F + 5, 32, W, 0,
                       (float*)((char*)packed + L.b32[G_BLENDA_T]), (unsigned short*)((char*)packed + L.bhi[G_BLENDA_T]),
                       (unsigned short*)((char*)packed + L.blo[G_BLENDA_T]), d.Kpad, d.Npad, (unsigned short*)((char*)packed + L.bst[G_BLENDA_T]), nl_tgemm_nrt(d.N), 0);
  }
  const float* const* un = t + T_UNET;
  { const int w1[1] = {W}, w2[1] = {64}, w3[1] = {128};
    P.conv3(G_CONV1, un[0], un[1], W, w1, 1);
    P.conv3(G_CONV1F, un[0], un[1], W, w1, 1, 1u);
    P.conv3(G_CONV2, un[4], un[5], 64, w2, 1);
    P.conv3(G_CONV3, un[8], un[9], 128, w3, 1); }
  P.convT(G_T3E, G_T3O, un[12], un[13], 128, 128);
  P.convT(G_T2E, G_T2O, un[16], un[17], 256, 64);
  P.convT(G_T1E, G_T1O, un[20], un[21], 128, 32);
  P.convT_merged(G_T3M, un[12], un[13], 128, 128);
  P.convT_merged(G_T2M, un[16], un[17], 256, 64);
  P.convT_merged(G_T1M, un[20], un[21], 128, 32);
  { const int wo[2] = {W, 32}; P.conv3(G_CONVOUT, un[24], un[25], W + 32, wo, 2); P.conv3(G_CONVOUTF, un[24], un[25], W + 32, wo, 2, 1u); }
  if (W == 256) {   // NL_PREC_F16MX: conv_out's fp6 images for tgemm_mx_kernel, from the layer's packed fp32 matrix (same K order as its streams)
    const GemmDim& d = L.g[G_CONVOUTF];
    const int nslab = (d.Kpad / 32 + 1) / 2;
    hipLaunchKernelGGL(pack_tgemm_mx6_kernel, dim3((unsigned)nl_cdiv((int64_t)nslab * 1024, 256)), dim3(256), 0, st, (const float*)((char*)packed + L.b32[G_CONVOUTF]), d.Kpad, d.Npad,
                       d.N, nslab, (unsigned char*)packed + L.mx_convout);
  }
  P.conv3_dgrad(G_UB_OUTA, un[24], W, W + 32, 0, W);
  P.conv3_dgrad(G_UB_OUTB, un[24], W, W + 32, W, 32);
  P.convT_dgrad(G_UB_T1, un[20], 128, 32);
  P.convT_dgrad(G_UB_T2, un[16], 256, 64);
  P.convT_dgrad(G_UB_T3, un[12], 128, 128);
  P.conv3_dgrad(G_UB_C3, un[8], 128, 128, 0, 128);
  P.conv3_dgrad(G_UB_C2, un[4], 128, 64, 0, 64);
  P.conv3_dgrad(G_UB_C1, un[0], 64, W, 0, W);
  for (int u = 0; u < U_COUNT; ++u) {
    P.transpose(un[4 * u + 2], L.un_g[u], L.un_c[u], L.un_l[u]);   // (C, L) -> (L, C)
    P.transpose(un[4 * u + 3], L.un_b[u], L.un_c[u], L.un_l[u]);
    P.lane_major(L.un_g[u], L.un_gl[u], L.un_n[u], L.un_so[u]);
    P.lane_major(L.un_b[u], L.un_bl[u], L.un_n[u], L.un_so[u]);
  }
  P.linear(G_FEAT0, t[T_F0W], t[T_F0B]);
  P.block(G_FEAT2, 0, t[T_F2W], 0, W, 1, W);
  P.block(G_FEAT2, W, t[T_F2B], 0, 1, 0, 1);   // bias as the K-row that meets the weight-sum column
  P.block(G_BLENDA, 0, t[T_BL0W], 0, W + F + 5, 1, W);
  if (W % 32 == 0) {   // accumulator-order copies for the chain kernel
    P.block(G_FEAT0P, 0, t[T_F0W], 0, W, 1, W, 1);
    P.copy(t[T_F0B], L.bias[G_FEAT0P], W);
    if (W == 256) {   // NL_PREC_F16MX: feat_mlp.0's fp6 images for feat_comp_mx_kernel (K in accumulator order = the order of feature_agg's fragment image)
      const GemmDim& d = L.g[G_FEAT0P];
      const int nslab = (d.Kpad / 32 + 1) / 2;
      hipLaunchKernelGGL(pack_tgemm_mx6_kernel, dim3((unsigned)nl_cdiv((int64_t)nslab * 1024, 256)), dim3(256), 0, st, (const float*)((char*)packed + L.b32[G_FEAT0P]), d.Kpad, d.Npad,
                         d.N, nslab, (unsigned char*)packed + L.mx_feat0);
    }
    P.block(G_BLENDAP, 0, t[T_BL0W], 0, W + F + 5, 1, W, 1);
    P.block(G_QP, 0, t[T_WQ], 0, W, 1, W, 1);
  }
  P.block(G_BLENDP, 0, t[T_BL0W], W + 3, W + F + 5, 1, C);
  if (nl_pack_ptt(t[T_B0W], t[T_B0B], W, F, L.g[G_PTT].Kpad, L.g[G_PTT].Npad, (float*)((char*)packed + L.b32[G_PTT]),
                  (float*)((char*)packed + L.bias[G_PTT]), st) != NL_OK) return NL_ERR_HIP;
  hipLaunchKernelGGL(pack_blw_kernel, dim3(2), dim3(256), 0, st, t[T_BL0W], t[T_BL0B], (float*)((char*)packed + L.blw), W, F);
  // small VALU-side weights
  P.copy(t[T_RD0W], L.rd_w, 64); P.copy(t[T_RD0B], L.rd_w + 4 * 64, 16);
  P.copy(t[T_RD2W], L.rd_w + 4 * 80, 27 * 16); P.copy(t[T_RD2B], L.rd_w + 4 * (80 + 432), 27);
  for (int d = 0; d < 4; ++d) {
    const float* const* q = t + T_DEC + 6 * d;
    const size_t o = L.dec_w + 4 * (size_t)d * 2178;
    const int nout = d < 2 ? 2 : 1;
    P.copy(q[0], o, 1024); P.copy(q[1], o + 4 * 1024, 32);
    P.copy(q[2], o + 4 * 1056, 1024); P.copy(q[3], o + 4 * 2080, 32);
    P.copy(q[4], o + 4 * 2112, 32 * nout); P.copy(q[5], o + 4 * 2176, nout);
  }
  if (nl_pack_mv_decoder((const float*)((char*)packed + L.dec_w), (char*)packed + L.dec_mfma, st) != NL_OK) return NL_ERR_HIP;
  P.copy(t[T_SIGW], L.sig_w, W); P.copy(t[T_SIGB], L.sig_b, 1);
  P.copy(t[T_BL2W], L.bl2_w, 512); P.copy(t[T_BL2B], L.bl2_b, 16);
  P.copy(t[T_BL4W], L.bl4_w, 16); P.copy(t[T_BL4B], L.bl4_b, 1);
  P.copy(t[T_LNW], L.ln_g, W); P.copy(t[T_LNB], L.ln_b, W);
  P.copy(t[T_B0B], L.pt_bias, W); P.copy(t[T_B2B], L.pt_bias + 4 * (size_t)W, W); P.copy(t[T_B4B], L.pt_bias + 8 * (size_t)W, W);
  if (cfg->C == 192) {
    int rc = nl_pack_mv_front(t[T_OUT0W], t[T_OUT0B], (char*)packed + L.mvf_pack, st);
    if (rc != NL_OK) return rc;
  }
  if (W == 64 || W == 128 || W == 256) {
    int rc = nl_pack_point_stream(t[T_B0W], t[T_B2W], t[T_B4W], t[T_WK], t[T_WV], (char*)packed + L.pt_stream, W, F, st);
    if (rc != NL_OK) return rc;
  }
  if (W == 128 || W == 256) {   // rd_w was filled by the copies above (same stream)
    int rc = nl_pack_point_stream2(t[T_B0W], t[T_B2W], t[T_B4W], t[T_WK], t[T_WV], t[T_B2B], t[T_B4B], (const float*)((char*)packed + L.rd_w),
                                   (char*)packed + L.pt_stream2, W, F, st);
    if (rc != NL_OK) return rc;
    rc = nl_pack_point_stream2(t[T_B0W], t[T_B2W], t[T_B4W], t[T_WK], t[T_WV], t[T_B2B], t[T_B4B], (const float*)((char*)packed + L.rd_w),
                               (char*)packed + L.pt_stream2_mx, W, F, st, 1);
    if (rc != NL_OK) return rc;
    rc = nl_pack_point_stream2(t[T_B0W], t[T_B2W], t[T_B4W], t[T_WK], t[T_WV], t[T_B2B], t[T_B4B], (const float*)((char*)packed + L.rd_w),
                               (char*)packed + L.pt_stream2_f16, W, F, st, 2);
    if (rc != NL_OK) return rc;
    rc = nl_pack_point_bwd_stream(t[T_B0W], t[T_B2W], t[T_B4W], t[T_WK], t[T_WV], (char*)packed + L.pt_bwd_stream, W, F, st);
    if (rc != NL_OK) return rc;
  }
  NL_LAUNCH_CHECK();
  static_assert(G_COUNT <= 64, "one bit per layer");
  set_pack_streams(packed, P.has_bst, P.has_bsh);
  return NL_OK;
}

}  // extern "C"
