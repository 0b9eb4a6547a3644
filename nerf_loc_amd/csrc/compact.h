// Ordered compaction — "keep the flagged rows, in order, with a device-side count" — as every unit of the four libraries does it (head.hip, geom.hip, setup.hip,
// fine_bwd.hip).  Device functions only, and nothing of any library's ABI.
//   rank of a flagged row = flagged lanes below it in its wave (ballot + mbcnt) + the totals of the waves below it in its workgroup (LDS, added in wave order)
//                           + the exclusive offset of its workgroup's chunk (nl_scan_exclusive over the chunk counts, one workgroup)
// Integers only, no atomics, no kernel that waits on another workgroup: the order is the rows' own and two calls give the same bits.  What is written behind the
// count (zero padding) never meets a live row, because every rank is below the total.
// These are the only functions of the tree in which the place of one __syncthreads() decides the order of an output: each says which barrier is its own and which
// is the caller's.
#pragma once
#include <hip/hip_runtime.h>

// set bits of `ballot` below this lane
__device__ __forceinline__ int nl_lane_rank(unsigned long long ballot) {
  return __builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// flagged lanes below this one; lane 0 of every wave leaves the wave's count in wtot[wave] (blockDim.x / 64 ints of LDS per counted set).  The CALLER's
// __syncthreads() publishes wtot to nl_group_rank / nl_group_total; every thread of the workgroup calls this (a lane that has left is a lane not counted)
__device__ __forceinline__ int nl_wave_rank(bool f, int* __restrict__ wtot) {
  const unsigned long long bal = __ballot(f);
  if ((threadIdx.x & 63) == 0) wtot[threadIdx.x >> 6] = __popcll(bal);
  return nl_lane_rank(bal);
}

// behind that barrier: the rank inside the workgroup from the rank inside the wave
__device__ __forceinline__ int nl_group_rank(int rank, const int* __restrict__ wtot) {
  for (int w = 0; w < (int)(threadIdx.x >> 6); ++w) rank += wtot[w];
  return rank;
}

// behind that barrier: the workgroup's count; WAVES = blockDim.x / 64
template <int WAVES>
__device__ __forceinline__ int nl_group_total(const int* __restrict__ wtot) {
  int total = 0;
#pragma unroll
  for (int w = 0; w < WAVES; ++w) total += wtot[w];
  return total;
}

// a[0 .. n) becomes its exclusive scan in place; the total comes back in every thread.  One workgroup of exactly THREADS threads, all of them calling; part:
// THREADS ints of LDS.  Thread t owns [t per, (t + 1) per), per = ceil(n / THREADS): its sum, an inclusive Hillis-Steele scan of the THREADS sums in `part`,
// then its elements' offsets in ascending order.  a[] must be visible to the workgroup on entry (a barrier of the caller's if this kernel wrote it); the
// function ends on a barrier, so `part` may be reused at once.
template <int THREADS>
__device__ __forceinline__ int nl_scan_exclusive(int* a, int n, int* part) {
  const int tid = threadIdx.x;
  const int per = (n + THREADS - 1) / THREADS, lo = min(n, tid * per), hi = min(n, lo + per);
  int own = 0;
  for (int i = lo; i < hi; ++i) own += a[i];
  part[tid] = own;
  __syncthreads();
  for (int d = 1; d < THREADS; d <<= 1) {
    const int v = tid >= d ? part[tid - d] : 0;
    __syncthreads();   // every read of this step before any write of it
    part[tid] += v;
    __syncthreads();
  }
  int run = part[tid] - own;
  for (int i = lo; i < hi; ++i) { const int v = a[i]; a[i] = run; run += v; }
  const int total = part[THREADS - 1];
  __syncthreads();
  return total;
}
