// dsx_validate.hip — the validation report of the training loop (split.py:174-241) on gfx950: un-normalise the
// visuals to uint16 counts, exact integer statistics for the per-channel PSNR, and the numerators of the [0, 1] images
// the loop writes.  Two launches: k_val_quantise, then k_val_finish, which reads the first launch's partial statistics.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

// ---------------------------------------------------------------------------
// The partition.  Plane p < B*C is channel p % C of the target / prediction, plane B*C + q is input plane q (b-major
// both).  Workgroup (x, p) of k_val_quantise owns pixels [x * kValChunk, (x + 1) * kValChunk) of plane p -- a function
// of the shape alone -- and leaves one row part[(p * nblk + x) * 4 + {0, 1, 2, 3}] = {sum (t - p)^2, min, max,
// undefined pixels}.  Every statistic is an integer, so its value does not depend on the order of the reduction.
// A thread takes the groups x * 1024 + k * 256 + tid (k = 0..3) of four consecutive pixels (dsx_kernels.h: one 16-byte
// load and one 8-byte store per tensor under VEC).
// ---------------------------------------------------------------------------
struct ValStat { unsigned long long ssd; unsigned lo, hi, undef; };
struct ValRed { unsigned long long ssd[4]; unsigned lo[4], hi[4], undef[4]; };   // LDS: the four waves' results
__device__ __forceinline__ ValStat val_block_reduce(ValStat s, ValRed& red) {
  s.ssd = wave_reduce<RedSum>(s.ssd);
  s.lo = wave_reduce<RedMin>(s.lo);
  s.hi = wave_reduce<RedMax>(s.hi);
  s.undef = wave_reduce<RedSum>(s.undef);
  __syncthreads();                         // `red` may still be read from the previous reduction
  wave_park(s.ssd, red.ssd);
  wave_park(s.lo, red.lo);
  wave_park(s.hi, red.hi);
  wave_park(s.undef, red.undef);
  __syncthreads();
  return {block_combine<RedSum, Serial>(red.ssd), block_combine<RedMin, Serial>(red.lo),
          block_combine<RedMax, Serial>(red.hi), block_combine<RedSum, Serial>(red.undef)};   // in every thread
}

// x * std + mean in double, the product and the sum rounded separately (numpy: float32 array * float64 -> float64)
__device__ __forceinline__ double val_unnormalise(float x, double sd, double mean) { return add_d(mul_d((double)x, sd), mean); }
// astype(uint16) of a target / input value: truncation.  The cast is undefined for NaN and outside [0, 65536): such a
// pixel is counted and stored as 0.
__device__ __forceinline__ unsigned val_cast(double v, unsigned& undef) {
  if (!(v >= 0.0 && v < 65536.0)) { ++undef; return 0u; }
  return (unsigned)v;
}
// the prediction: v[v < 0] = 0, v[v > 65535] = 65535, astype(uint16); only NaN is left undefined
__device__ __forceinline__ unsigned val_cast_clamped(double v, unsigned& undef) {
  if (v != v) { ++undef; return 0u; }
  v = v < 0.0 ? 0.0 : v;
  v = v > 65535.0 ? 65535.0 : v;
  return (unsigned)v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_val_quantise(const ValArgs a) {
  __shared__ ValRed red;
  const long long HW = a.HW;
  const int plane = blockIdx.y, nT = a.B * a.C;
  const long long g0 = (long long)blockIdx.x * (kValChunk / 4) + threadIdx.x;
  ValStat s = {0ull, 65535u, 0u, 0u};
  long long at[4][4];
  int cnt[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long i4 = g0 + k * 256;
    cnt[k] = i4 * 4 < HW ? group4<VEC>(i4, HW, at[k]) : 0;
  }
  if (plane < nT) {
    const int c = plane % a.C;
    const double mean = a.mean_t[c], sd = a.std_t[c];
    const float* tp = a.target + (long long)plane * HW;
    const float* pp = a.pred + (long long)plane * HW;
    float t[4][4], p[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)          // every load of the thread is issued before the first is used
      if (cnt[k] > 0) { load4<VEC>(tp, at[k], cnt[k], t[k]); load4<VEC>(pp, at[k], cnt[k], p[k]); }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (cnt[k] <= 0) continue;
      unsigned tq[4], pq[4];
      DSX_EACH4(j, cnt[k]) {
        tq[j] = val_cast(val_unnormalise(t[k][j], sd, mean), s.undef);
        pq[j] = val_cast_clamped(val_unnormalise(p[k][j], sd, mean), s.undef);
        const unsigned d = tq[j] > pq[j] ? tq[j] - pq[j] : pq[j] - tq[j];
        s.ssd += (unsigned long long)(d * d);                    // 65535^2 < 2^32
        s.lo = min(s.lo, tq[j]); s.hi = max(s.hi, tq[j]);
      }
      store4<VEC>(a.target_q + (long long)plane * HW, at[k], cnt[k], tq);
      store4<VEC>(a.pred_q + (long long)plane * HW, at[k], cnt[k], pq);
    }
  } else {
    const long long q = plane - nT;
    const float* ip = a.input + q * HW;
    float x[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k)
      if (cnt[k] > 0) load4<VEC>(ip, at[k], cnt[k], x[k]);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (cnt[k] <= 0) continue;
      unsigned iq[4];
      DSX_EACH4(j, cnt[k]) {
        iq[j] = val_cast(val_unnormalise(x[k][j], a.std_in, a.mean_in) / 2.0, s.undef);   // the halving is exact
        s.lo = min(s.lo, iq[j]); s.hi = max(s.hi, iq[j]);
      }
      store4<VEC>(a.input_q + q * HW, at[k], cnt[k], iq);
    }
  }
  s = val_block_reduce(s, red);
  if (threadIdx.x == 0) {
    unsigned long long* row = a.part + ((size_t)plane * a.nblk + blockIdx.x) * 4;
    row[0] = s.ssd; row[1] = s.lo; row[2] = s.hi; row[3] = s.undef;
  }
}

// ---------------------------------------------------------------------------
// k_val_finish: the statistics from the partial rows, and the numerators of the [0, 1] images (only with a.target_n).
//   stats[0]                          undefined pixels of all planes
//   stats[1 + 3 p + {0, 1, 2}]        target plane p: sum (target_q - pred_q)^2, min, max of target_q
//   stats[1 + 3 B C + 2 q + {0, 1}]   input plane q: min, max of input_q
//   target_n = target_q - tmin;  pred_n = min((pred_q - tmin) mod 2^16, tmax - tmin);  input_n = input_q - (min over
//   the item's input planes)
// Workgroup (x, p) reduces the rows it needs itself (a plane's nblk rows, an item's Cin * nblk rows: 32 bytes each, in
// L2), workgroup (0, p) writes plane p's statistics and workgroup (0, 0) also the counter; then the workgroups of a
// plane share its chunks x, x + gridDim.x, ...
// ---------------------------------------------------------------------------
__device__ __forceinline__ ValStat val_reduce_rows(const unsigned long long* part, long long r0, long long r1,
                                                   ValRed& red) {
  ValStat s = {0ull, 65535u, 0u, 0u};
  for (long long r = r0 + threadIdx.x; r < r1; r += 256) {
    const unsigned long long* row = part + r * 4;
    s.ssd += row[0]; s.lo = min(s.lo, (unsigned)row[1]); s.hi = max(s.hi, (unsigned)row[2]); s.undef += (unsigned)row[3];
  }
  return val_block_reduce(s, red);
}
// the undefined pixels alone, over many rows: the counter is 64 bits wide
__device__ __forceinline__ unsigned long long val_sum_undefined(const unsigned long long* part, long long rows,
                                                                ValRed& red) {
  ValStat s = {0ull, 65535u, 0u, 0u};
  for (long long r = threadIdx.x; r < rows; r += 256) s.ssd += part[r * 4 + 3];
  return val_block_reduce(s, red).ssd;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_val_finish(const ValArgs a) {
  __shared__ ValRed red;
  const long long HW = a.HW;
  const int plane = blockIdx.y, nT = a.B * a.C, nblk = a.nblk;
  const bool is_t = plane < nT;
  const ValStat own = val_reduce_rows(a.part, (long long)plane * nblk, (long long)(plane + 1) * nblk, red);
  unsigned lo = own.lo;
  if (!is_t) {                             // input_img.min(): over every input channel of the item
    const long long item0 = nT + (long long)((plane - nT) / a.Cin) * a.Cin;
    lo = val_reduce_rows(a.part, item0 * nblk, (item0 + a.Cin) * nblk, red).lo;
  }
  if (blockIdx.x == 0) {
    if (plane == 0) {
      const unsigned long long u = val_sum_undefined(a.part, (long long)(nT + a.B * a.Cin) * nblk, red);
      if (threadIdx.x == 0) a.stats[0] = u;
    }
    if (threadIdx.x == 0) {
      if (is_t) {
        unsigned long long* st = a.stats + 1 + (size_t)plane * 3;
        st[0] = own.ssd; st[1] = own.lo; st[2] = own.hi;
      } else {
        unsigned long long* st = a.stats + 1 + (size_t)nT * 3 + (size_t)(plane - nT) * 2;
        st[0] = own.lo; st[1] = own.hi;
      }
    }
  }
  if (a.target_n == nullptr) return;
  const unsigned span = own.hi - own.lo;   // target planes: tmax - tmin
  for (int x = blockIdx.x; x < nblk; x += gridDim.x) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const long long i4 = (long long)x * (kValChunk / 4) + k * 256 + threadIdx.x;
      if (i4 * 4 >= HW) continue;
      long long at[4];
      const int cnt = group4<VEC>(i4, HW, at);
      if (is_t) {
        unsigned tq[4], pq[4], tn[4], pn[4];
        load4<VEC>(a.target_q + (long long)plane * HW, at, cnt, tq);
        load4<VEC>(a.pred_q + (long long)plane * HW, at, cnt, pq);
        DSX_EACH4(j, cnt) {
          tn[j] = tq[j] - lo;
          pn[j] = min((pq[j] - lo) & 0xFFFFu, span);             // the uint16 subtraction wraps below the target's minimum
        }
        store4<VEC>(a.target_n + (long long)plane * HW, at, cnt, tn);
        store4<VEC>(a.pred_n + (long long)plane * HW, at, cnt, pn);
      } else {
        const long long q = plane - nT;
        unsigned iq[4], in[4];
        load4<VEC>(a.input_q + q * HW, at, cnt, iq);
        DSX_EACH4(j, cnt) in[j] = iq[j] - lo;
        store4<VEC>(a.input_n + q * HW, at, cnt, in);
      }
    }
  }
}

int val_blocks(long long HW) { return (int)((HW + kValChunk - 1) / kValChunk); }
hipError_t launch_val_report(const ValArgs& a, hipStream_t st) {
  // 16-byte loads of the fp32 tensors and 8-byte accesses of the uint16 ones: planes of 4 k pixels from aligned bases
  const bool vec = a.HW % 4 == 0 && aligned16(a.input, a.target, a.pred) &&
                   ((((uintptr_t)a.input_q | (uintptr_t)a.target_q | (uintptr_t)a.pred_q | (uintptr_t)a.input_n |
                      (uintptr_t)a.target_n | (uintptr_t)a.pred_n) & 7u) == 0);
  const unsigned planes = (unsigned)(a.B * (a.C + a.Cin));
  hipLaunchKernelGGL(vec ? k_val_quantise<true> : k_val_quantise<false>, dim3((unsigned)a.nblk, planes), dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const unsigned gx = a.target_n == nullptr ? 1u : (unsigned)(a.nblk < kValFinishBlocks ? a.nblk : kValFinishBlocks);
  hipLaunchKernelGGL(vec ? k_val_finish<true> : k_val_finish<false>, dim3(gx, planes), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dsx
