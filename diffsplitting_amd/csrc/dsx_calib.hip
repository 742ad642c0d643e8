// dsx_calib.hip — the calibration sums of a predicted spread (gfx950): per channel the pixels binned by their predicted
// standard deviation, {count, sum std^2, sum (target - mean)^2} per bin and the coverage counts |e| <= z std
// (include/dsx.h, dsx_calibration), in ONE pass over the three channel-last canvases.  Host side: dsx_calib.cpp.
//
// Partition, a function of n alone: calibration_blocks(n) workgroups, each owns calibration_span(n) consecutive pixels
// (a multiple of 4), that is span * C consecutive VALUES of the interleaved canvases; inside it thread t takes the
// groups of four values t, t + 256, .. in ascending order, whether the four arrive as one 16-byte load (kVec) or as
// four 4-byte loads.  A wave works through a group as four BATCHES of 64 values: batch j holds value j of every lane's
// group.  For C = 1, 2, 4 a batch is of one channel (j % C); for C = 3 the channel differs from lane to lane.
//
// A batch's sums, without floating-point atomics and in an order the code alone fixes: every value has a key
// (channel, bin).  A scalar loop walks the keys PRESENT in the batch (the key of the first pending lane, a ballot of the
// lanes that hold it).  A key of up to kCalSerial lanes gives each of them its rank among them and the key's count;
// then round r = 0, 1, .. lets the lanes of rank r add their s^2 and e^2 to the wave's row in LDS: in one round no two
// lanes share an address, LDS serves a wave's instructions in order, so a slot receives its terms in ascending lane
// order.  The rank-0 lane adds the key's count.  A CROWDED key (more lanes: a spatially smooth spread puts a whole batch
// into one or two bins, and 64 rounds would serialise the wave) is folded at once inside the key loop: the kDown
// butterfly over s^2 and e^2 with +0.0 in the other lanes, and its first lane adds the results to the slot.  Which way a
// key goes depends on the batch's values alone.  Cost: the key loop, about 8 instructions per key present, one LDS
// read-add-write per round (at most kCalSerial rounds) and two butterflies per crowded key (at most 7 in a batch); 64
// values over 30 equally filled bins take ~27 keys and ~6 rounds.  Coverage: one ballot per z, counted in scalar
// registers.  The four waves' rows meet after one barrier (Pairwise) in part[block][row];
// k_calib_finish folds the rows of a slot with one wave: row r on lane r % 64, ascending, then the kDown butterfly.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

constexpr int kCalChunk = 4096;      // pixels per workgroup up to kCalMaxBlocks workgroups
constexpr int kCalMaxBlocks = 2048;  // 8 per CU: the LDS round trips of a wave hide behind the other waves
constexpr int kCalSerial = 8;        // lanes of one key in a batch up to which they add one after the other

int calibration_blocks(long long n) {
  const long long b = (n + kCalChunk - 1) / kCalChunk;
  return (int)(b > kCalMaxBlocks ? kCalMaxBlocks : (b < 1 ? 1 : b));
}
long long calibration_span(long long n) {
  const long long b = calibration_blocks(n);
  return ((n + b - 1) / b + 3) / 4 * 4;
}

struct CalGroup { float m[4], s[4], t[4]; };

// the group of four values at f (a multiple of 4), values at or past e1 read as 0; kVec: e1 - f is 0 or at least 4
template <bool kVec>
__device__ __forceinline__ CalGroup cal_load(const CalArgs& a, long long f, long long e1) {
  CalGroup g;
#pragma unroll
  for (int j = 0; j < 4; ++j) g.m[j] = g.s[j] = g.t[j] = 0.f;
  if (kVec) {
    if (f < e1) {
      const float4 vm = *(const float4*)(a.mean + f), vs = *(const float4*)(a.sd + f), vt = *(const float4*)(a.target + f);
      g.m[0] = vm.x; g.m[1] = vm.y; g.m[2] = vm.z; g.m[3] = vm.w;
      g.s[0] = vs.x; g.s[1] = vs.y; g.s[2] = vs.z; g.s[3] = vs.w;
      g.t[0] = vt.x; g.t[1] = vt.y; g.t[2] = vt.z; g.t[3] = vt.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (f + j < e1) { g.m[j] = a.mean[f + j]; g.s[j] = a.sd[f + j]; g.t[j] = a.target[f + j]; }
  }
  return g;
}

template <bool kVec, int C>
__global__ __launch_bounds__(256) void k_calib_partial(CalArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cal_smem[];
  const int nbins = a.nbins, nz = a.nz, m = nbins - 1;
  const int stride = 3 * nbins + nz, R = C * stride;       // a channel's slots, a row
  double* red = (double*)cal_smem;                          // [wave][R]
  double* edg = red + 4 * R;                                // [C][m]
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  for (int j = tid; j < 4 * R; j += 256) red[j] = 0.0;
  for (int j = tid; j < C * m; j += 256) edg[j] = a.edges[j];
  __syncthreads();
  volatile double* row = red + wave * R;

  const long long e0 = (long long)blockIdx.x * a.span, e1 = min(a.elems, e0 + a.span);
  const int nit = e1 > e0 ? (int)((e1 - e0 + 1023) / 1024) : 0;
  int step0 = 0;                                            // the largest power of two <= m
  if (m > 0) step0 = 1 << (31 - __clz(m));
  int cb = (int)((e0 + 4 * tid) % C);                       // the channel of the group's first value
  unsigned cov[C][kCalMaxZ];
#pragma unroll
  for (int c = 0; c < C; ++c)
#pragma unroll
    for (int k = 0; k < kCalMaxZ; ++k) cov[c][k] = 0;

  long long f = e0 + 4 * tid;
  CalGroup nxt = cal_load<kVec>(a, f, e1);
  for (int it = 0; it < nit; ++it, f += 1024) {
    const CalGroup g = nxt;
    nxt = cal_load<kVec>(a, f + 1024, e1);                 // past e1: zeros, nothing is read
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const bool valid = f + j < e1;
      const int ch = C == 3 ? (cb + j) % 3 : j % C;
      const double s = (double)g.s[j];
      const double e = (double)g.t[j] - (double)g.m[j];
      const double s2 = __dmul_rn(s, s), e2 = __dmul_rn(e, e);
      // bin = #{ i : edges[ch][i] <= s }: the edges ascend, so the largest prefix whose last edge is <= s
      int bin = 0;
      const double* ed = edg + ch * m;
      for (int st = step0; st > 0; st >>= 1) {
        const int idx = bin + st;
        if (idx <= m && ed[idx - 1] <= s) bin = idx;
      }
      // coverage: a batch of one channel needs one ballot per z
      const double ae = fabs(e);
#pragma unroll
      for (int k = 0; k < kCalMaxZ; ++k) {
        if (k < nz) {
          const bool in = valid && s >= 0.0 && ae <= __dmul_rn(a.z[k], s);
          if (C == 3) {
#pragma unroll
            for (int c = 0; c < C; ++c) cov[c][k] += (unsigned)__popcll(__ballot(in && ch == c));
          } else {
            cov[j % C][k] += (unsigned)__popcll(__ballot(in));
          }
        }
      }
      // the keys present in the batch: every lane's rank among the lanes of its key, and the key's count
      const int key = ch * nbins + bin;
      volatile double* p = row + ch * stride + 3 * bin;
      unsigned long long pend = __ballot(valid);
      int rank = -1, cnt = 0, rounds = 0;
      while (pend) {
        const int leader = __ffsll((long long)pend) - 1;
        const int k = __builtin_amdgcn_readlane(key, leader);
        const bool mine = valid && key == k;
        const unsigned long long same = __ballot(mine);
        const int c = __popcll(same);
        if (c > kCalSerial) {                                 // a crowded key: fold its lanes at once, absent lanes add +0.0
          const double v = wave_reduce<RedSum>(mine ? s2 : 0.0), w = wave_reduce<RedSum>(mine ? e2 : 0.0);
          if (lane == leader) { p[0] += (double)c; p[1] += v; p[2] += w; }
        } else {
          if (mine) {
            rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(same >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)same, 0u));
            cnt = c;
          }
          rounds = max(rounds, c);
        }
        pend &= ~same;
      }
      for (int r = 0; r < rounds; ++r) {
        if (rank == r) {
          if (r == 0) p[0] += (double)cnt;
          p[1] += s2;
          p[2] += e2;
        }
        __builtin_amdgcn_wave_barrier();
      }
    }
    if (C == 3) cb = (cb + 1024 % 3) % 3;
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < C; ++c)
#pragma unroll
      for (int k = 0; k < kCalMaxZ; ++k)
        if (k < nz) row[c * stride + 3 * nbins + k] = (double)cov[c][k];
  }
  __syncthreads();
  for (int j = tid; j < R; j += 256) a.part[(size_t)blockIdx.x * R + j] = block_combine<RedSum, Pairwise>(red, R, j);
}

// one wave per slot of the row: lane l adds the workgroup rows l, l + 64, .. in ascending order, the kDown butterfly
// folds the lanes (counts are integers below 2^53: exact in any order)
__global__ __launch_bounds__(64) void k_calib_finish(const double* __restrict__ part, int nblk, int R, double* __restrict__ out) {
  const int j = blockIdx.x;
  double tot = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 64) tot += part[(size_t)k * R + j];
  tot = wave_reduce<RedSum>(tot);
  if (threadIdx.x == 0) out[j] = tot;
}

template <bool kVec>
static void launch_partial(const CalArgs& a, int nblk, size_t lds, hipStream_t st) {
  const dim3 grid((unsigned)nblk), block(256);
  switch (a.C) {
    case 1: hipLaunchKernelGGL((k_calib_partial<kVec, 1>), grid, block, lds, st, a); break;
    case 2: hipLaunchKernelGGL((k_calib_partial<kVec, 2>), grid, block, lds, st, a); break;
    case 3: hipLaunchKernelGGL((k_calib_partial<kVec, 3>), grid, block, lds, st, a); break;
    default: hipLaunchKernelGGL((k_calib_partial<kVec, 4>), grid, block, lds, st, a); break;
  }
}

hipError_t launch_calibration(const CalArgs& a, bool vec, hipStream_t st) {
  const int R = calibration_row(a.C, a.nbins, a.nz);
  const int nblk = calibration_blocks(a.elems / a.C);       // a workgroup whose span begins past the end writes a row of zeros
  const size_t lds = sizeof(double) * (size_t)(4 * R + a.C * (a.nbins - 1));
  if (vec) launch_partial<true>(a, nblk, lds, st);
  else launch_partial<false>(a, nblk, lds, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_calib_finish, dim3((unsigned)R), dim3(64), 0, st, (const double*)a.part, nblk, R, a.out);
  return hipGetLastError();
}

}  // namespace dsx
