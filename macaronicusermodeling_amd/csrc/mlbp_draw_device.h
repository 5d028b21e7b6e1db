// The draw rule of include/mlbp_exactsample.h on a vector of weights, shared by the libraries that draw a state on the device
// (libmlbp_exactsample.so, libmlbp_cutdraw.so; gfx950 only): by one wave with lane = state (wave_scan, wave_draw) and by the
// whole workgroup over a vector in LDS (block_min_max, block_draw).  Helpers only, no kernel: each library keeps its own.
// Not part of the ABI.  Include after mlbp_graph_device.h.
#ifndef MLBP_DRAW_DEVICE_H
#define MLBP_DRAW_DEVICE_H

#include "mlbp_graph_device.h"

namespace mlbp_graph {

// ---- X = 64: a wave per draw ---------------------------------------------------------------------------------
// WAVE prefix sums, as the header states them: lane i returns A_i.
__device__ __forceinline__ double wave_scan(double v, int lane) {
  v += dpp_mov<0x111>(v);                                      // row_shr:1, 2, 4, 8: a lane without a partner reads zero
  v += dpp_mov<0x112>(v);
  v += dpp_mov<0x114>(v);
  v += dpp_mov<0x118>(v);
  const double r0 = read_lane(v, 15), r1 = read_lane(v, 31), r2 = read_lane(v, 47);
  const int row = lane >> 4;
  const double before = row == 1 ? r0 : row == 2 ? r0 + r1 : (r0 + r1) + r2;
  return row == 0 ? v : v + before;
}

// The draw rule on the wave's vector b (lane = state) with uniform u: the state, and the probability's two terms.
__device__ __forceinline__ int wave_draw(double b, double u, int lane, double& num, double& total) {
  const double A = wave_scan(b, lane);
  total = read_lane(A, 63);
  const double thr = u * total;
  const unsigned long long live = __ballot(b > 0.0), cross = __ballot(A > thr && b > 0.0);
  const int x = cross ? __ffsll(cross) - 1 : live ? 63 - __clzll(live) : 0;
  num = read_lane(b, x);
  return x;
}

// ---- any X: a workgroup per draw -----------------------------------------------------------------------------
// The lowest of the workgroup's `lo` and the highest of its `hi`, the same in every thread; two barriers.
__device__ __forceinline__ void block_min_max(unsigned& lo, unsigned& hi, double* scratch) {
  unsigned* s = reinterpret_cast<unsigned*>(scratch);
  const unsigned a = wave_max_u32(~lo), b = wave_max_u32(hi);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    s[threadIdx.x >> 6] = a;
    s[4 + (threadIdx.x >> 6)] = b;
  }
  __syncthreads();
  lo = ~max(max(s[0], s[1]), max(s[2], s[3]));
  hi = max(max(s[4], s[5]), max(s[6], s[7]));
}

// The draw rule on a[0 .. n) (visible on entry) with uniform u, SEGMENTED prefix sums: thread t owns [t L, (t + 1) L).
// seg: [number of segments <= n].  Reached by every thread; ends behind a barrier.
__device__ __forceinline__ int block_draw(const double* a, int n, double u, double* seg, double* scratch, double& num, double& total) {
  const int t = threadIdx.x;
  const int L = (n + WG - 1) / WG, n_seg = (n + L - 1) / L, lo = min(n, t * L), hi = min(n, lo + L);
  double tot = 0.0;
  for (int j = lo; j < hi; ++j) tot += a[j];
  if (t < n_seg) seg[t] = tot;
  __syncthreads();
  double off = 0.0, all = 0.0;
  for (int s = 0; s < n_seg; ++s) {
    if (s == t) off = all;
    all += seg[s];
  }
  const double thr = u * all;
  unsigned first = 0xffffffffu, last = 0;                      // the crossing index; 1 + the highest index of positive weight
  double local = 0.0;
  for (int j = lo; j < hi; ++j) {
    local += a[j];
    if (!(a[j] > 0.0)) continue;
    last = (unsigned)j + 1;
    if (first == 0xffffffffu && off + local > thr) first = (unsigned)j;
  }
  block_min_max(first, last, scratch);
  const int x = first != 0xffffffffu ? (int)first : last ? (int)last - 1 : 0;
  num = a[x];
  total = all;
  __syncthreads();                                             // seg and a are written again by the caller
  return x;
}

}  // namespace mlbp_graph

#endif
