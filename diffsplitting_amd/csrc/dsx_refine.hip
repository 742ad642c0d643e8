// dsx_refine.hip — the centred second moments of plane triples (g, p1, p2) (gfx950): everything the refinement of the
// mixing time needs of three planes (include/dsx.h, dsx_comoments), in ONE pass over them.  Host side: dsx_refine.cpp.
//
// Centring: one pass on SHIFTED data.  Every operand is shifted by the first element of its plane,
//   x' = (double)x[i] - (double)x[0]
// (the same IEEE subtraction for every reader, so a restatement holds the same x'), and the partials are plain sums of
// x', y', z' and of their six products, in double with one fma per product.  k_comoments_finish undoes the shift:
//   mean x = (double)x[0] + Sx / n,      Cxy = Sxy - Sx * Sy / n.
// What is left of the cancellation is that of data centred on one of its own values: Sxy exceeds Cxy by
// n (x0 - mean x)(y0 - mean y), a few variances, not by n mean x mean y as for raw moments (1e5 times the variance for
// raw counts of mean 1e4 and spread 30).  min / max of g are taken on the raw values: exact.
//
// Partition, a function of n alone: comoments_blocks(n) workgroups per plane, each owns comoments_span(n) consecutive
// pixels (a multiple of 4); inside it thread t takes the groups of four pixels t, t + 256, .. in ascending order, one
// pixel after the other, whether the four arrive as one 16-byte load (kVec) or as four strided 4-byte loads.  So a
// plane's numbers do not depend on the load path, on its position in the call or on the number of planes.  Reduction:
// dsx_reduce.h (kDown butterfly, Pairwise combine) into part[plane][block][kComSlots]; k_comoments_finish folds the rows
// of a plane with one wave: row r on lane r % 64, ascending, then the kDown butterfly.  No atomics.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

constexpr int kComChunk = 8192;      // pixels per workgroup up to kComMaxBlocks workgroups: 8 groups of four per thread
constexpr int kComMaxBlocks = 1024;

int comoments_blocks(long long n) {
  const long long b = (n + kComChunk - 1) / kComChunk;
  return (int)(b > kComMaxBlocks ? kComMaxBlocks : (b < 1 ? 1 : b));
}
long long comoments_span(long long n) {
  const long long b = comoments_blocks(n);
  return ((n + b - 1) / b + 3) / 4 * 4;
}

struct ComAcc {
  double sg = 0, s1 = 0, s2 = 0, gg = 0, c11 = 0, c22 = 0, g1 = 0, g2 = 0, c12 = 0;
  float mn = INFINITY, mx = -INFINITY;
  __device__ __forceinline__ void add(float gf, float af, float bf, double g0, double a0, double b0) {
    const double g = (double)gf - g0, a = (double)af - a0, b = (double)bf - b0;
    sg += g; s1 += a; s2 += b;
    gg = fma(g, g, gg); c11 = fma(a, a, c11); c22 = fma(b, b, c22);
    g1 = fma(g, a, g1); g2 = fma(g, b, g2); c12 = fma(a, b, c12);
    mn = fminf(mn, gf); mx = fmaxf(mx, gf);
  }
};

template <bool kVec>
__global__ __launch_bounds__(256) void k_comoments_partial(ComArgs a) {
  __shared__ double red[4 * kComSlots];
  const long long plane = blockIdx.y;
  const float* __restrict__ g = a.g + plane * a.stride[0];
  const float* __restrict__ p1 = a.p1 + plane * a.stride[2];
  const float* __restrict__ p2 = a.p2 + plane * a.stride[4];
  const long long sg = a.stride[1], s1 = a.stride[3], s2 = a.stride[5];
  const double g0 = (double)g[0], a0 = (double)p1[0], b0 = (double)p2[0];
  const long long i0 = (long long)blockIdx.x * a.span, i1 = min(a.n, i0 + a.span);
  ComAcc acc;
#pragma unroll 2
  for (long long i = i0 + 4 * (long long)threadIdx.x; i < i1; i += 4 * 256) {
    if (kVec) {                                  // n % 4 == 0 and span % 4 == 0: the group is whole
      const float4 vg = *(const float4*)(g + i), v1 = *(const float4*)(p1 + i), v2 = *(const float4*)(p2 + i);
      acc.add(vg.x, v1.x, v2.x, g0, a0, b0);
      acc.add(vg.y, v1.y, v2.y, g0, a0, b0);
      acc.add(vg.z, v1.z, v2.z, g0, a0, b0);
      acc.add(vg.w, v1.w, v2.w, g0, a0, b0);
    } else {
      const int m = (int)min((long long)4, i1 - i);
      float vg[4], v1[4], v2[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < m) { vg[j] = g[(i + j) * sg]; v1[j] = p1[(i + j) * s1]; v2[j] = p2[(i + j) * s2]; }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (j < m) acc.add(vg[j], v1[j], v2[j], g0, a0, b0);
    }
  }
  using Row = RedRow<9, 1>;                      // slot 11 of a part row: unused, 0
  const double v[Row::kSlots] = {acc.sg, acc.s1, acc.s2, acc.gg, acc.c11, acc.c22, acc.g1, acc.g2, acc.c12,
                                 (double)acc.mn, (double)acc.mx};
  Row::park(v, red, kComSlots);
  __syncthreads();
  if (threadIdx.x < kComSlots) {
    const int j = threadIdx.x;
    a.part[((size_t)plane * gridDim.x + blockIdx.x) * kComSlots + j] = j < Row::kSlots ? Row::combine(red, j, kComSlots) : 0.0;
  }
}

// one wave per plane: lane l adds the rows l, l + 64, .. of every slot in ascending order (independent loads: a serial
// walk over up to 1024 rows by one thread cost a memory latency per row), the kDown butterfly folds the 64 lanes, lane 0
// undoes the shift and writes {n, min g, max g, mean g, mean p1, mean p2, Cgg, C11, C22, Cg1, Cg2, C12}
__global__ __launch_bounds__(64) void k_comoments_finish(ComArgs a, int nblk) {
  const long long plane = blockIdx.x;
  const double* p = a.part + (size_t)plane * nblk * kComSlots;
  double tot[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, mn = INFINITY, mx = -INFINITY;
  for (int k = threadIdx.x; k < nblk; k += 64) {
    const double* row = p + (size_t)k * kComSlots;
#pragma unroll
    for (int j = 0; j < 9; ++j) tot[j] += row[j];
    mn = fmin(mn, row[9]); mx = fmax(mx, row[10]);
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) tot[j] = wave_reduce<RedSum>(tot[j]);
  mn = wave_reduce<RedMin>(mn); mx = wave_reduce<RedMax>(mx);
  if (threadIdx.x == 0) {
    const double n = (double)a.n;
    const double g0 = (double)a.g[plane * a.stride[0]], a0 = (double)a.p1[plane * a.stride[2]],
                 b0 = (double)a.p2[plane * a.stride[4]];
    const double sg = tot[0], s1 = tot[1], s2 = tot[2];
    double* o = a.out + plane * 12;
    o[0] = n; o[1] = mn; o[2] = mx;
    o[3] = g0 + sg / n; o[4] = a0 + s1 / n; o[5] = b0 + s2 / n;
    o[6] = tot[3] - sg * sg / n; o[7] = tot[4] - s1 * s1 / n; o[8] = tot[5] - s2 * s2 / n;
    o[9] = tot[6] - sg * s1 / n; o[10] = tot[7] - sg * s2 / n; o[11] = tot[8] - s1 * s2 / n;
  }
}

hipError_t launch_comoments(const ComArgs& a, int planes, bool vec, hipStream_t st) {
  const int nblk = comoments_blocks(a.n);
  const dim3 grid((unsigned)nblk, (unsigned)planes);
  if (vec) hipLaunchKernelGGL(k_comoments_partial<true>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_comoments_partial<false>, grid, dim3(256), 0, st, a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_comoments_finish, dim3((unsigned)planes), dim3(64), 0, st, a, nblk);
  return hipGetLastError();
}

}  // namespace dsx
