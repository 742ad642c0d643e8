// dsx_quantiles.hip — per-element quantiles and ranks across a stack of n <= 64 samples (gfx950): every element's n
// samples are sorted IN REGISTERS by a fully unrolled compare-exchange network, the requested order statistics are
// picked under the wave-uniform positions and interpolated in double (include/dsx.h, dsx_sample_quantiles), in ONE
// pass over the stack.  Host side: dsx_quantiles.cpp.
//
// A thread owns kE neighbouring elements: sample r of them is one load of 4 kE bytes, coalesced across the wave
// (kE = 1: the 4-byte path, taken whenever a base, the stride or the count is no multiple of kE; the arithmetic of an
// element is the same code on either path, so the bits are).  The samples become their order-preserving integer image
// (negative floats: the magnitude bits flipped), so a compare-exchange is one v_min_i32 / v_max_i32 pair, -0 sorts before
// +0 and no NaN rule of a floating-point minimum takes part.  The network is Batcher's odd-even merge sort over
// kP = n padded to 2, 4, .. 64 wires, the pads +inf: 1, 5, 19, 63, 191, 543 comparators for 2, 4, .. 64 wires
// (a bitonic sorter of 64 has 672), every one ascending, every index a compile-time constant after unrolling: nothing
// here is indexed at run time (such arrays go to scratch).  v[lo] and v[hi] are picked by an unrolled chain of selects
// under the scalar comparison j == lo.
// The rank #{ r : x_r < target } is counted on the fp32 values as they are loaded (a pad, +inf, never counts).
//
// Elements per thread on the wide path, from the register counts: 4 up to 32 wires, 2 at 64 wires
// (4 would need 256 registers for the samples alone).  The launch is capped (grid_for: 4096 workgroups), a thread
// walks its groups of kE elements with the grid's stride.
#include "dsx_kernels.h"

namespace dsx {

namespace {

template <int kE> struct QVec;
template <> struct QVec<1> { typedef float type; };
template <> struct QVec<2> { typedef float2 type; };
template <> struct QVec<4> { typedef float4 type; };

// the order-preserving integer image of an fp32 value, and back (the map is its own inverse)
__device__ __forceinline__ int q_image(float f) {
  const int b = __float_as_int(f);
  return b ^ ((b >> 31) & 0x7fffffff);
}
__device__ __forceinline__ float q_value(int i) { return __int_as_float(i ^ ((i >> 31) & 0x7fffffff)); }

template <int kE>
__device__ __forceinline__ void q_load(const float* p, float (&f)[kE]) {
  const typename QVec<kE>::type v = *(const typename QVec<kE>::type*)p;
  __builtin_memcpy(f, &v, sizeof v);
}
template <int kE>
__device__ __forceinline__ void q_store(float* p, const float (&f)[kE]) {
  typename QVec<kE>::type v;
  __builtin_memcpy(&v, f, sizeof v);
  *(typename QVec<kE>::type*)p = v;
}

// Batcher's odd-even merge sort of kP wires (a power of two), ascending; all indices fold to constants
template <int kP, int kE>
__device__ __forceinline__ void q_sort(int (&v)[kP][kE]) {
#pragma unroll
  for (int p = 1; p < kP; p <<= 1)
#pragma unroll
    for (int k = p; k >= 1; k >>= 1)
#pragma unroll
      for (int j = k % p; j + k < kP; j += 2 * k)
#pragma unroll
        for (int i = 0; i < k; ++i)
          if (i + j + k < kP && (i + j) / (2 * p) == (i + j + k) / (2 * p)) {
#pragma unroll
            for (int e = 0; e < kE; ++e) {
              const int lo = min(v[i + j][e], v[i + j + k][e]), hi = max(v[i + j][e], v[i + j + k][e]);
              v[i + j][e] = lo;
              v[i + j + k][e] = hi;
            }
          }
}

template <int kP, int kE>
__global__ __launch_bounds__(256) void k_quantiles(QuantArgs a) {
  const long long groups = a.count / kE;
  const long long step = (long long)gridDim.x * 256;
  const float inf = __builtin_huge_valf();
  for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < groups; g += step) {
    const long long i0 = g * kE;
    // the call's scalars, opaque to the optimiser once per trip: the comparisons against them below (r < n, k < nq,
    // j == lo) and the sample offsets r * stride would otherwise all be hoisted out of this loop and held in scalar
    // registers, several hundred of them
    int n = a.n, nq = a.nq;
    long long stride = a.stride;
    asm volatile("" : "+s"(n), "+s"(nq), "+s"(stride));
    const float* px = a.x + i0;
    float x[kP][kE];
#pragma unroll
    for (int r = 0; r < kP; ++r) {
#pragma unroll
      for (int e = 0; e < kE; ++e) x[r][e] = inf;
      if (r < n) q_load<kE>(px, x[r]);
      px += stride;
    }
    if (a.rank) {
      float t[kE], c[kE];
      q_load<kE>(a.target + i0, t);
#pragma unroll
      for (int e = 0; e < kE; ++e) {
        int cnt = 0;
#pragma unroll
        for (int r = 0; r < kP; ++r) cnt += x[r][e] < t[e] ? 1 : 0;
        c[e] = (float)cnt;
      }
      q_store<kE>(a.rank + i0, c);
    }
    if (nq == 0) continue;
    int v[kP][kE];
#pragma unroll
    for (int r = 0; r < kP; ++r)
#pragma unroll
      for (int e = 0; e < kE; ++e) v[r][e] = q_image(x[r][e]);
    q_sort<kP, kE>(v);
#pragma unroll
    for (int k = 0; k < kQuantMaxQ; ++k) {
      if (k < nq) {
        int lo = a.lo[k];
        asm volatile("" : "+s"(lo));
        const bool same = a.hi[k] == lo;
        const double t = a.t[k], u = sub_d(1.0, t);
        int va[kE], vb[kE];
#pragma unroll
        for (int e = 0; e < kE; ++e) va[e] = vb[e] = v[0][e];
#pragma unroll
        for (int j = 0; j < kP; ++j) {
          if (j == lo) {
#pragma unroll
            for (int e = 0; e < kE; ++e) { va[e] = v[j][e]; vb[e] = v[j + 1 < kP ? j + 1 : j][e]; }
          }
        }
        float o[kE];
#pragma unroll
        for (int e = 0; e < kE; ++e) {
          const double fa = (double)q_value(va[e]), fb = same ? fa : (double)q_value(vb[e]);
          const double d = sub_d(fb, fa);
          o[e] = (float)(t < 0.5 ? add_d(fa, mul_d(d, t)) : sub_d(fb, mul_d(d, u)));
        }
        q_store<kE>(a.out + (long long)k * a.count + i0, o);
      }
    }
  }
}

template <int kP>
hipError_t launch_p(const QuantArgs& a, bool wide, hipStream_t st) {
  constexpr int kE = quantiles_per_thread(kP);
  if (wide) hipLaunchKernelGGL((k_quantiles<kP, kE>), dim3(grid_for(a.count / kE)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_quantiles<kP, 1>), dim3(grid_for(a.count)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace

hipError_t launch_quantiles(const QuantArgs& a, bool wide, hipStream_t st) {
  switch (quantiles_wires(a.n)) {
    case 2: return launch_p<2>(a, wide, st);
    case 4: return launch_p<4>(a, wide, st);
    case 8: return launch_p<8>(a, wide, st);
    case 16: return launch_p<16>(a, wide, st);
    case 32: return launch_p<32>(a, wide, st);
    default: return launch_p<64>(a, wide, st);
  }
}

}  // namespace dsx
