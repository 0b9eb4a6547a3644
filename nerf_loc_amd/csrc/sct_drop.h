// The dropout masks of the SelfCrossTransformer training step (sct.hip's dropping attention, sct_bwd.hip): ONE definition, used by every kernel that drops and by
// nl_sct_dropout_mask; tests/sct_dropout_ref.py restates it in numpy bit for bit.  Needs common.h alone; sct.h includes it.
//
// Generator: Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11) with its published constants; key = the 64-bit seed
// (low word, high word).  One call gives four 32-bit words = eight 16-bit fields = a block of 4 x 2 elements:
//   counter = (major >> 2, minor >> 1, group, 4 layer + site);  element (major, minor) is bits [16 (minor & 1), + 16) of word major & 3
//   site 0 (attention probabilities): major = key, minor = query, group = 8 batch item + head
//   site 1 (out_proj's output), 2 (the ReLU'd hidden rows), 3 (linear2's output): major = row flattened over the batch (batch first), minor = column, group = 0
// An element is KEPT when its field >= thr, thr = round(65536 p) (half to even, at most 65535): the keep probability is exactly 1 - thr / 65536 — within 2^-17 of
// 1 - p — and kept values are multiplied by 65536 / (65536 - thr), ITS inverse, so that the expectation is exact.  The mask is a pure function of (seed, p, layer,
// site, element): no tile size, key range, wave or call shape enters.
// Why 4 x 2: the accumulator registers of the 32 x 32 products come in runs of four consecutive rows (mfma.h: nl_acc_row).  Where the registers run along `major`
// (keys in the forward and the dQ pass, rows in the row chain) one call serves four registers of two neighbouring lanes; where they run along `minor` (queries in
// the dK / dV pass) one call serves two registers of four neighbouring lanes.  The lanes share their calls (below), so every field of every call is used: 128 calls
// per 32 x 32 tile and wave in both orientations = two per lane.
#pragma once
#include <cmath>
#include <type_traits>
#include "common.h"

namespace {

struct SctDrop {
  unsigned k0, k1;   // the seed's low and high word
  unsigned thr;      // 16-bit threshold; 0: nothing is dropped
  unsigned tag;      // 4 * layer
  float scale;       // 65536 / (65536 - thr)
};

inline bool sct_drop_p_ok(float p) { return p >= 0.f && p < 1.f; }   // false for NaN
inline SctDrop sct_drop_make(float p, unsigned long long seed, int layer) {
  SctDrop d;
  long t = lrint((double)p * 65536.0);
  if (t > 65535) t = 65535;
  d.k0 = (unsigned)seed; d.k1 = (unsigned)(seed >> 32);
  d.thr = (unsigned)t; d.tag = 4u * (unsigned)layer;
  d.scale = (float)(65536.0 / (double)(65536 - t));
  return d;
}

__device__ __forceinline__ uint4 sct_philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0, p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1; c3 = (unsigned)p0; c0 = n0; c2 = n2;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return make_uint4(c0, c1, c2, c3);
}

// the four words of the block that holds elements (4 major4 .. + 3, 2 minor2 .. + 1) of a site
__device__ __forceinline__ uint4 sct_drop_words(const SctDrop& d, int site, unsigned group, unsigned major4, unsigned minor2) {
  return sct_philox4x32_10(major4, minor2, group, d.tag + (unsigned)site, d.k0, d.k1);
}
__device__ __forceinline__ unsigned sct_drop_word(const uint4& w, unsigned i) { return i == 0 ? w.x : i == 1 ? w.y : i == 2 ? w.z : w.w; }
__device__ __forceinline__ bool sct_drop_keep(const SctDrop& d, unsigned word, unsigned half) { return ((word >> (16 * half)) & 0xffffu) >= d.thr; }
// one element
__device__ __forceinline__ bool sct_drop_keep_at(const SctDrop& d, int site, unsigned group, unsigned major, unsigned minor) {
  return sct_drop_keep(d, sct_drop_word(sct_drop_words(d, site, group, major >> 2, minor >> 1), major & 3), minor & 1);
}

// Neighbouring lanes need the same generator calls, so they share them: each makes its part and the KEEP BITS (not the words) travel between the lanes by DPP
// inside a quad.  Every lane of the wave must be active where these two are called (the kernels call them in wave-uniform control flow only).
template <int CTRL>
__device__ __forceinline__ unsigned sct_drop_quad(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, false); }
// bit k = element (word k, half) of one call
__device__ __forceinline__ unsigned sct_drop_call_bits(const SctDrop& d, const uint4& w, unsigned half) {
  return (unsigned)sct_drop_keep(d, w.x, half) | (unsigned)sct_drop_keep(d, w.y, half) << 1 | (unsigned)sct_drop_keep(d, w.z, half) << 2 |
         (unsigned)sct_drop_keep(d, w.w, half) << 3;
}

// keep bits of a lane's 16 accumulator registers (bit r = register r) where the registers run along `major`: register r is element (major0 + nl_acc_row(r, hh),
// minor), major0 a multiple of 8 and `minor` = an even base + (lane & 1).  The lanes minor and minor ^ 1 need the same four calls (one per run of four registers):
// the even lane makes runs 0 and 1, the odd lane runs 2 and 3, each evaluates both halves, and they swap one register.  Two calls per lane.
__device__ __forceinline__ unsigned sct_drop_bits_major(const SctDrop& d, int site, unsigned group, unsigned major0, int hh, unsigned minor) {
  const unsigned odd = minor & 1;
  const uint4 wa = sct_drop_words(d, site, group, (major0 >> 2) + 4 * odd + hh, minor >> 1);       // run 2 odd
  const uint4 wb = sct_drop_words(d, site, group, (major0 >> 2) + 4 * odd + 2 + hh, minor >> 1);   // run 2 odd + 1
  const unsigned mine = sct_drop_call_bits(d, wa, odd) | sct_drop_call_bits(d, wb, odd) << 4;
  const unsigned theirs = sct_drop_quad<0xB1>(sct_drop_call_bits(d, wa, odd ^ 1) | sct_drop_call_bits(d, wb, odd ^ 1) << 4);   // quad_perm [1, 0, 3, 2]
  return odd ? (theirs | mine << 8) : (mine | theirs << 8);
}
// ... where the registers run along `minor`: register r is element (major, minor0 + nl_acc_row(r, hh)), minor0 a multiple of 8 and `major` = a base that is a
// multiple of 4 + (lane & 3).  The four lanes of a quad need the same eight calls (one per pair of registers) and each its own word of them: lane q makes calls 2 q
// and 2 q + 1, evaluates all eight fields of both, and every lane reads the four lanes' 16 bits.  Two calls per lane.
__device__ __forceinline__ unsigned sct_drop_bits_minor(const SctDrop& d, int site, unsigned group, unsigned major, unsigned minor0, int hh) {
  const unsigned q = major & 3;
  unsigned mine = 0;   // bit 8 i + 2 k + h: call 2 q + i, word k, half h
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const unsigned minor = minor0 + 8 * q + 2 * i + 4 * hh;   // = minor0 + nl_acc_row(2 (2 q + i), hh): even
    const uint4 w = sct_drop_words(d, site, group, major >> 2, minor >> 1);
    const unsigned lo = sct_drop_call_bits(d, w, 0), hi = sct_drop_call_bits(d, w, 1);
#pragma unroll
    for (int k = 0; k < 4; ++k) mine |= (((lo >> k) & 1u) | ((hi >> k) & 1u) << 1) << (8 * i + 2 * k);
  }
  const unsigned s0 = sct_drop_quad<0x00>(mine), s1 = sct_drop_quad<0x55>(mine), s2 = sct_drop_quad<0xAA>(mine), s3 = sct_drop_quad<0xFF>(mine);
  // lane s's calls 2 s, 2 s + 1 are registers 4 s .. 4 s + 3; this lane's word is q
  auto take = [q](unsigned v) { return ((v >> (2 * q)) & 3u) | ((v >> (8 + 2 * q)) & 3u) << 2; };
  return take(s0) | take(s1) << 4 | take(s2) << 8 | take(s3) << 12;
}
// A kernel that has variants takes a trailing parameter pack: empty (the kernel as it was, with the same signature and device code), or the variants' argument
// structs — one SctDrop where it drops.  sct_arg<T>(pack...) is the pack's T, or an SctNone where it holds none.
struct SctNone {};
template <class T>
__device__ __forceinline__ SctNone sct_arg() { return SctNone{}; }
template <class T, class A, class... R>
__device__ __forceinline__ auto sct_arg(const A& a, const R&... r) {
  if constexpr (std::is_same_v<T, A>) return a;
  else return sct_arg<T>(r...);
}
__device__ __forceinline__ float sct_drop_apply(const SctDrop& d, unsigned bits, int r, float v) { return (bits >> r) & 1u ? v * d.scale : 0.f; }

}  // namespace
