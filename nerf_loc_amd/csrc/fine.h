// What the fine matcher's forward (fine.hip) and backward (fine_bwd.hip) share: the window geometry, the layout of the packed proj image and the argument block of
// the window kernels.  Include after common.h.
#pragma once
#include "common.h"
#include "s2d.h"

namespace {

constexpr int FINE_W = 7, FINE_WW = 49;
constexpr int64_t FINE_MAX_M = 1 << 24;
inline bool fine_c_ok(int C) { return s2d_c_ok(C); }

// ------------------------------------------------------------------------------------------ proj: layout
// bf16 hi / lo and fp32 planes of proj.weight (Cout x Cf) in mfma.h's fragment maps (written by pack.hip's nl_launch_frag_pack), then the bias.
// The training image (nl_fine_pack_proj_train) is the same layout of proj.weight^T (Cf x Cout) with two differences: its fp32 plane holds the PLAIN transpose
// (row-major, the packer's staging; not fragment order, so only the bf16 window kernels may read this image: nl_launch_fine_rows) and its bias is zero.
struct FineProjLayout { size_t hi, lo, f32, bias, total; };
__host__ __device__ inline FineProjLayout fine_proj_layout(int Cf, int Cout) {
  FineProjLayout l;
  const size_t n = (size_t)Cf * Cout;
  l.hi = 0;
  l.lo = n * 2;
  l.f32 = n * 4;
  l.bias = n * 8;
  l.total = l.bias + (size_t)Cout * 4;
  return l;
}

// ------------------------------------------------------------------------------------------ windows
struct FineWinArgs {
  const unsigned char* img;
  const float* feat;
  const long long* b_ids; const long long* j_ids;
  float* out;
  int B, Hf, Wf, Cf, Cout, M, stride, Lx, L, Q;   // L = Ly * Lx windows per image, Q = work items per match (pairs of 32-channel blocks)
  int dense;   // the backward's g_out . W: feat is (M, 49, Cf) rows, cell r of match m is row m * 49 + r (no ids, no map)
};

// the lane's pixel row for tile t (cell 32 t + column), or null: outside the map, a padding row, or ids the host check should have refused
__device__ __forceinline__ const float* fine_cell_row(const FineWinArgs& a, int m, int cell) {
  if (a.dense) return cell < FINE_WW ? a.feat + ((size_t)m * FINE_WW + cell) * a.Cf : nullptr;
  const long long b = a.b_ids[m], l = a.j_ids[m];
  if (cell >= FINE_WW || b < 0 || b >= a.B || l < 0 || l >= a.L) return nullptr;
  const int ly = (int)(l / a.Lx), lx = (int)(l - (long long)ly * a.Lx);
  const int py = ly * a.stride + cell / FINE_W - FINE_W / 2, px = lx * a.stride + cell % FINE_W - FINE_W / 2;
  if (py < 0 || py >= a.Hf || px < 0 || px >= a.Wf) return nullptr;
  return a.feat + (((size_t)b * a.Hf + py) * a.Wf + px) * a.Cf;
}

}  // namespace
