// dsx_reduce.h — the block reduction of the evaluation kernels, stated once (device only).  A workgroup is 256
// threads = 4 wave64s: every wave folds its 64 lanes with a shuffle butterfly, lane 0 parks the wave's result in LDS,
// and after one barrier the four results are combined.  Nothing here uses atomics, so the order of the additions is
// fixed by the code alone and equal inputs give equal bits.  tests/golden/reduce_bits.npz records the outputs of every
// kernel below; where an output is a double (the loss, the PSNR sums, SSIM / SSD) a changed order shows there, where it
// is rounded to fp32 first (k_lpips_dist, k_masked_mean) a one-ulp change of the double sum mostly does not.
//
// For doubles and floats the ORDER is part of each kernel's result.  Two choices exist, and every kernel keeps its own:
//   butterfly  kDown  offsets 32, 16, .. 1   every kernel but k_lpips_dist
//              kUp    offsets 1, 2, .. 32    k_lpips_dist (its two fp32 norms and its double accumulator)
//   combine    Pairwise  (r0 + r1) + (r2 + r3)   k_loss_partial, k_image_metrics, k_mix_range, k_lpips_minmax,
//                                                k_msssim_scale, k_msssim_finish, every RedRow, k_calib_partial
//              Serial    ((r0 + r1) + r2) + r3   k_masked_mean, k_lpips_dist, val_block_reduce
// (min, max and integer sums do not depend on either; k_mix_range, k_lpips_minmax and val_block_reduce are listed for
// completeness.)  The rows, RedRow<sums, (min, max) pairs>, all kDown and Pairwise:
//   RedRow<5, 1>  PsnrSums: k_stitch_psnr and k_blend<.., true>, once per channel (psnr_sums_write)
//   RedRow<5, 2>  PsnrSums + min / max of p: k_msssim_stats per chunk, k_msssim_coef over a plane's chunk rows
//   RedRow<4, 1>  k_tile_disagreement (dsx_tiles.hip), once per channel: two pixel counts, two sums of var, min / max of var
//   RedRow<9, 1>  k_comoments_partial (dsx_refine.hip): nine sums of shifted data, min / max of g
//   RedRow<8, 1>  k_consistency_partial (dsx_consistency.hip): two pixel counts, sums of r, r^2, x, x^2 over the
//                 unsaturated pixels, the count and the sum of r^2 / den where den > 0, min / max of r;
//                 k_consistency_finish folds a frame's workgroup rows as k_comoments_finish does
// k_comoments_finish then folds a plane's workgroup rows with ONE wave: lane l adds the rows l, l + 64, .. in ascending
// order, wave_reduce (kDown) folds the lanes.
// k_calib_partial (dsx_calib.hip) reduces no lanes with a butterfly: a bin's terms meet in the wave's row of LDS in
// ascending lane order, batch after batch; its four wave rows then combine Pairwise (block_combine per slot), and
// k_calib_finish folds the workgroup rows of a slot as k_comoments_finish does (rows l, l + 64, .. per lane, then kDown).
//
// Use.  One value:      r = block_reduce<RedSum, Pairwise>(v, red)          red: 4 elements of LDS, r in every thread
//       several values: block_park<Op>(v_j, red, n, j) for each slot j < n    red: 4 * n elements, [wave][slot]
//                       __syncthreads()
//                       block_combine<Op, Pairwise>(red, n, j)              in whichever thread writes slot j
//       a row:          Row::park(v, red)  __syncthreads()  Row::combine(red, j)    the same, Op chosen by j
// so that n values cost one barrier and the combines spread over n threads.  A kernel that reduces twice through the
// same array puts a barrier in front of the second parking (val_block_reduce: wave_reduce, barrier, wave_park, so
// that the shuffles of the early waves overlap the wait for the late ones).
#pragma once
#include <hip/hip_runtime.h>

#include "dsx_kernels.h"   // kPsnrMaxC

namespace dsx {

struct RedSum {
  template <class T> static __device__ __forceinline__ T op(T a, T b) { return a + b; }
};
struct RedMin {
  static __device__ __forceinline__ double op(double a, double b) { return fmin(a, b); }
  static __device__ __forceinline__ float op(float a, float b) { return fminf(a, b); }
  static __device__ __forceinline__ unsigned op(unsigned a, unsigned b) { return min(a, b); }
};
struct RedMax {
  static __device__ __forceinline__ double op(double a, double b) { return fmax(a, b); }
  static __device__ __forceinline__ float op(float a, float b) { return fmaxf(a, b); }
  static __device__ __forceinline__ unsigned op(unsigned a, unsigned b) { return max(a, b); }
};

enum WaveOrder { kDown, kUp };
// all 64 lanes of the wave -> the same value in every lane
template <class Op, WaveOrder kOrder = kDown, class T>
__device__ __forceinline__ T wave_reduce(T v) {
  if (kOrder == kDown) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = Op::op(v, __shfl_xor(v, o, 64));
  } else {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) v = Op::op(v, __shfl_xor(v, o, 64));
  }
  return v;
}

// the four wave results r[w] = red[w * n + slot]
struct Pairwise {
  template <class Op, class T> static __device__ __forceinline__ T of(T r0, T r1, T r2, T r3) {
    return Op::op(Op::op(r0, r1), Op::op(r2, r3));
  }
};
struct Serial {
  template <class Op, class T> static __device__ __forceinline__ T of(T r0, T r1, T r2, T r3) {
    return Op::op(Op::op(Op::op(r0, r1), r2), r3);
  }
};

// lane 0 of every wave parks the wave's (already reduced) value
template <class T>
__device__ __forceinline__ void wave_park(T v, T* red, int n = 1, int slot = 0) {
  if ((threadIdx.x & 63) == 0) red[(threadIdx.x >> 6) * n + slot] = v;
}
template <class Op, WaveOrder kOrder = kDown, class T>
__device__ __forceinline__ void block_park(T v, T* red, int n = 1, int slot = 0) {
  wave_park(wave_reduce<Op, kOrder>(v), red, n, slot);
}
template <class Op, class Combine, class T>
__device__ __forceinline__ T block_combine(const T* red, int n = 1, int slot = 0) {
  return Combine::template of<Op>(red[slot], red[n + slot], red[2 * n + slot], red[3 * n + slot]);
}
template <class Op, class Combine, WaveOrder kOrder = kDown, class T>
__device__ __forceinline__ T block_reduce(T v, T* red) {
  block_park<Op, kOrder>(v, red);
  __syncthreads();
  return block_combine<Op, Combine>(red);
}

// A ROW of doubles: NS sums, then NP (min, max) pairs; slot j alone names its operator.  kDown, Pairwise.
template <int NS, int NP>
struct RedRow {
  static constexpr int kSlots = NS + 2 * NP;
  static __device__ __forceinline__ bool is_sum(int j) { return j < NS; }
  static __device__ __forceinline__ bool is_min(int j) { return ((j - NS) & 1) == 0; }
  // the row that changes nothing, and row r folded into row v
  static __device__ __forceinline__ void init(double (&v)[kSlots]) {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) v[j] = is_sum(j) ? 0.0 : (is_min(j) ? INFINITY : -INFINITY);
  }
  static __device__ __forceinline__ void fold(double (&v)[kSlots], const double* r) {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) v[j] = is_sum(j) ? v[j] + r[j] : (is_min(j) ? fmin(v[j], r[j]) : fmax(v[j], r[j]));
  }
  // every thread: its row to the slots base .. base + kSlots - 1 of red[wave][n]
  static __device__ __forceinline__ void park(const double (&v)[kSlots], double* red, int n = kSlots, int base = 0) {
#pragma unroll
    for (int j = 0; j < kSlots; ++j) {
      if (is_sum(j)) block_park<RedSum>(v[j], red, n, base + j);
      else if (is_min(j)) block_park<RedMin>(v[j], red, n, base + j);
      else block_park<RedMax>(v[j], red, n, base + j);
    }
  }
  // after the barrier, in whichever thread writes slot j of the row
  static __device__ __forceinline__ double combine(const double* red, int j, int n = kSlots, int base = 0) {
    if (is_sum(j)) return block_combine<RedSum, Pairwise>(red, n, base + j);
    return is_min(j) ? block_combine<RedMin, Pairwise>(red, n, base + j) : block_combine<RedMax, Pairwise>(red, n, base + j);
  }
};

// The plane statistics of RangeInvariantPsnr (core/psnr.py) of a prediction p against its ground truth g, as a row:
// {sum p, sum p^2, sum g, sum g^2, sum g p, min g, max g}.  The closed form that consumes them:
// range_invariant_psnr_from_sums (core/psnr.py); on the device: k_msssim_coef.
struct PsnrSums {
  using Row = RedRow<5, 1>;
  double sp = 0, spp = 0, sg = 0, sgg = 0, sgp = 0, mn = INFINITY, mx = -INFINITY;
  __device__ __forceinline__ void add(float p, float g) {
    sp += p; spp += (double)p * p; sg += g; sgg += (double)g * g; sgp += (double)g * p;
    mn = fmin(mn, (double)g); mx = fmax(mx, (double)g);
  }
  __device__ __forceinline__ void park(double* red, int n, int base) const {
    const double v[Row::kSlots] = {sp, spp, sg, sgg, sgp, mn, mx};
    Row::park(v, red, n, base);
  }
};
// every thread of the workgroup: the sums of its channels -> row[C][8] of the workgroup, slot 7 = 0 (C <= kPsnrMaxC)
constexpr int kPsnrRed = 4 * kPsnrMaxC * PsnrSums::Row::kSlots;   // doubles of LDS, [wave][channel][slot]
__device__ __forceinline__ void psnr_sums_write(const PsnrSums (&acc)[kPsnrMaxC], int C, double* red, double* row) {
  constexpr int kS = PsnrSums::Row::kSlots;
#pragma unroll
  for (int c = 0; c < kPsnrMaxC; ++c) acc[c].park(red, kPsnrMaxC * kS, c * kS);
  __syncthreads();
  if (threadIdx.x < C * 8) {
    const int c = threadIdx.x >> 3, j = threadIdx.x & 7;
    row[c * 8 + j] = j < kS ? PsnrSums::Row::combine(red, j, kPsnrMaxC * kS, c * kS) : 0.0;
  }
}

}  // namespace dsx
