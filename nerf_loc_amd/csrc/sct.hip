// SelfCrossTransformer (reference: models/COTR/transformer.py:17-64, 171-250): four post-norm layers (self v0, self v1, cross v0 <- v1, cross v1 <- new v0), each
// three kernels on rows flattened over the batch ([B * N][C] fp32, batch first).  The kernels serve three uses.  Inference (eval mode) is this file's entry points.
// The training forward (sct_bwd.hip) launches the same projections and attention from here, into rows it keeps (nl_launch_sct_qkv_attn), and the row chain itself,
// with the stores of what the backward needs.  The training forward with dropout takes the attention's and the chain's instantiations with a trailing SctDrop
// argument (sct_drop.h); a kernel without that argument is the kernel as it was.
//
// sct_proj_kernel   q / k / v = (x [+ pos]) . W^T + b.  A workgroup owns 32 rows: x and x + pos are formed once while the tile is loaded into LDS (no x + pos tensor),
//   the four waves share the 32-column output blocks of in_proj_weight; [q; k] blocks multiply the x + pos tile, v blocks the x tile.  Cross layers launch it twice
//   (q from the target side, k and v once from the memory side).
// sct_attn_kernel   flash-style attention: a wave owns (batch item, head, 32-query tile, key range).  S^T = K . Q^T on the 32x32 MFMAs puts a query in a lane's
//   COLUMN, so a row's running maximum and sum are in-lane reductions over the 16 accumulator registers plus one exchange between the half-waves, and the probabilities
//   are already the B operand of O^T = V^T . P^T (k slot (hh, j) of step s = accumulator register 8 s + j; the V fragment is gathered in that key order).  Keys beyond Nk
//   get -inf before the maximum; their loads are clamped to the last key.  The next key tile's K / V values are fetched before the current tile's arithmetic.  A long
//   key sequence is cut into 2 or 4 ranges (>= 4 / >= 16 tiles) held by neighbouring waves of the workgroup, whose (maximum, sum, accumulator) meet in 18 KB of LDS and
//   are added in range order by the first of them: with one range per item the 4800 x 4800 layer is 1200 waves for 1024 SIMDs, each waiting on its own loads.
//   No Nq x Nk value ever reaches memory.  The head dimension (8 / 16 / 24 / 32) is padded with zero k slots to 16 / 32; fp32 mode needs no padding (k step 2).
//   The same kernel serves every Nq, also Nq == 1 (the fine shape: B x 8 waves with one live column each, four (batch item, head) pairs to a workgroup): a row's bits
//   must not depend on how many rows or batch items the call holds (tests/test_gpu_sct.py), which rules out a second kernel chosen by Nq or B; the number of key
//   ranges depends on Nk alone.
// sct_chain_kernel  (sct.h) out_proj, + residual, LayerNorm, linear1, ReLU, linear2, + residual, LayerNorm for 32 rows that stay in LDS from the attention output to the
//   layer output; the F-wide hidden rows live in LDS only.  The four waves split the output blocks of each product, so every weight fragment is read by exactly ONE wave
//   of the workgroup, straight from L2 in 1-KB coalesced pieces (fragment order): a copy through LDS would add a barrier pair per chunk and no reuse.
//   Measured: the kernel takes ~90 us per launch whatever the row count — it waits on these loads, which are not requested ahead of use; not yet changed.
//
// Precision: NL_PREC_F32 = v_mfma_f32_32x32x2_f32 on fp32 operands; NL_PREC_BF16X3 = three-term split-FP16 (mfma.h: hi = f16(v), lo = f16(v - hi)) for every product —
//   the logits feed a softmax (as in fine.hip) and one format keeps one code path; NL_PREC_BF16 = one bf16 product.  LayerNorm, softmax and residuals are fp32 everywhere.
// Every output row depends on its own row, the memory side, the weights and the mode only: fixed reduction orders, no atomics.
#include "sct_kernels.h"

int nl_launch_sct_qkv_attn(const void* img, int C, int F, int layer, int precision, const float* x, const float* xpos, int64_t Nq, const float* mem, const float* mpos,
                           int64_t Nk, int64_t B, float* q, float* k, float* v, float* attn, float drop_p, unsigned long long drop_seed, hipStream_t st) {
  float* const keep[4] = {q, k, v, attn};
  const SctDrop d = sct_drop_make(drop_p, drop_seed, layer);
  const SctRun r{(const unsigned char*)img, C, F, layer, x, xpos, Nq, mem, mpos, Nk, B, nullptr, nullptr, 0, keep, d.thr ? &d : nullptr};
  return sct_run(r, precision, st);
}

extern "C" {

size_t nl_sct_packed_bytes(int C, int nhead, int F) { return sct_cfg_ok(C, nhead, F) ? nl_align_up(sct_layout(C, F).total, 256) : 0; }

int nl_sct_pack_weights(int C, int nhead, int F, const float* const* tensors, int n_tensors, void* packed, size_t packed_bytes, void* stream) {
  if (!sct_cfg_ok(C, nhead, F)) return NL_ERR_UNSUPPORTED;
  if (!tensors || n_tensors != SCT_TENSORS || !packed || ((uintptr_t)packed & 15) != 0) return NL_ERR_BAD_ARG;
  for (int i = 0; i < SCT_TENSORS; ++i)
    if (!tensors[i]) return NL_ERR_BAD_ARG;
  if (packed_bytes < nl_sct_packed_bytes(C, nhead, F)) return NL_ERR_WORKSPACE;
  const SctLayout L = sct_layout(C, F);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* img = (unsigned char*)packed;
  for (int l = 0; l < SCT_LAYERS; ++l) {
    const float* const* t = tensors + sct_param_first(l);
    const int ln = sct_param_norm(l);
    const int N[4] = {3 * C, C, F, C}, K[4] = {C, C, C, F};
    for (int k = 0; k < 4; ++k) {
      const SctMatOff& m = L.l[l].m[k];
      if (const int e = nl_launch_frag_pack(t[2 * k], N[k], K[k], (unsigned short*)(img + m.bf), nullptr, (unsigned short*)(img + m.hi), (unsigned short*)(img + m.lo),
                                            (float*)(img + m.f32), false, st))
        return e;
    }
    float* vec = (float*)(img + L.l[l].vec);
    const float* src[8] = {t[1], t[3], t[5], t[7], t[ln], t[ln + 1], t[ln + 2], t[ln + 3]};
    const int cnt[8] = {3 * C, C, F, C, C, C, C, C};
    for (int k = 0; k < 8; ++k) {
      NL_CHECK_HIP(hipMemcpyAsync(vec, src[k], (size_t)cnt[k] * 4, hipMemcpyDeviceToDevice, st));
      vec += cnt[k];
    }
  }
  NL_LAUNCH_CHECK();
  return NL_OK;
}

size_t nl_sct_workspace_bytes(int64_t B, int64_t N0, int64_t N1, int C, int F) {
  (void)F;   // the hidden rows never leave LDS
  if (!sct_counts_ok(B, N0, N1) || C < 1 || !sct_counts_fit(B, N0, N1, N0 > N1 ? N0 : N1)) return 0;
  return 4 * sct_ws_part(B ? B : 1, N0, N1, C);
}

int nl_sct_layer(const void* packed, int C, int nhead, int F, int layer, int precision, const float* x, const float* x_pos, int64_t Nq, const float* mem,
                 const float* mem_pos, int64_t Nk, int64_t B, float* out, void* ws, size_t ws_bytes, void* stream) {
  if (layer < 0 || layer >= SCT_LAYERS) return NL_ERR_BAD_ARG;
  if (layer < 2) {   // self layers: the memory side is the target side
    if ((mem && mem != x) || (mem_pos && mem_pos != x_pos) || Nk != Nq) return NL_ERR_BAD_ARG;
    mem = x; mem_pos = x_pos;
  }
  const void* ptrs[5] = {x, x_pos, mem, mem_pos, out};
  bool empty;
  if (const int s = sct_check(packed, C, nhead, F, precision, B, Nq, Nk, ptrs, 5, ws, ws_bytes, &empty)) return s;
  if (empty) return NL_OK;
  const SctRun r{(const unsigned char*)packed, C, F, layer, x, x_pos, Nq, mem, mem_pos, Nk, B, out, (unsigned char*)ws, sct_ws_part(B, Nq, Nk, C)};
  return sct_run(r, precision, (hipStream_t)stream);
}

int nl_sct_forward(const void* packed, int C, int nhead, int F, int precision, const float* v0, const float* pos0, int64_t N0, const float* v1, const float* pos1,
                   int64_t N1, int64_t B, float* out0, float* out1, void* ws, size_t ws_bytes, void* stream) {
  const void* ptrs[6] = {v0, pos0, v1, pos1, out0, out1};
  bool empty;
  if (const int s = sct_check(packed, C, nhead, F, precision, B, N0, N1, ptrs, 6, ws, ws_bytes, &empty)) return s;
  if (empty) return NL_OK;
  if (out0 == out1) return NL_ERR_BAD_ARG;
  const unsigned char* img = (const unsigned char*)packed;
  unsigned char* w = (unsigned char*)ws;
  const size_t part = sct_ws_part(B, N0, N1, C);
  hipStream_t st = (hipStream_t)stream;
  // out0 / out1 carry the self layers' results; the cross layers then work in place (transformer.py:57-61: layer 3 reads the OUTPUT of layer 2)
  const SctRun r[SCT_LAYERS] = {{img, C, F, 0, v0, pos0, N0, v0, pos0, N0, B, out0, w, part},
                                {img, C, F, 1, v1, pos1, N1, v1, pos1, N1, B, out1, w, part},
                                {img, C, F, 2, out0, pos0, N0, out1, pos1, N1, B, out0, w, part},
                                {img, C, F, 3, out1, pos1, N1, out0, pos0, N0, B, out1, w, part}};
  for (int l = 0; l < SCT_LAYERS; ++l)
    if (const int s = sct_run(r[l], precision, st)) return s;
  return NL_OK;
}

}  // extern "C"
