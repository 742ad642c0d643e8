// dsx_objective.hip — the loss half of the training objective (gfx950): the per-sample L1 / L2 reduction the loss is
// formed from.  The noising step in front of the UNet forward is k_q_sample (dsx_steps.hip).
#include "dsx_kernels.h"

namespace dsx {

// ---------------------------------------------------------------------------
// Per-sample sum |a - b| (L1Loss) or sum (a - b)^2 (MSELoss) over (C, H, W): difference, square and accumulation in
// double.  Workgroup (x, b) owns elements [x * kLossChunk, (x + 1) * kLossChunk) of sample b -- loss_blocks(n) of them,
// a function of the shape alone -- and reduces thread -> wave shuffles -> 4 waves in a fixed order; k_loss_finish adds a
// sample's partials front to back.  No atomics: equal inputs give bitwise-equal outputs.
// ---------------------------------------------------------------------------
constexpr int kLossChunk = 4096;   // 16 elements per thread
__device__ __forceinline__ double loss_wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__global__ __launch_bounds__(256) void k_loss_partial(const float* __restrict__ a, const float* __restrict__ b,
                                                      long long n, int squared, double* __restrict__ part) {
  __shared__ double red[4];
  const long long base = (long long)blockIdx.y * n;
  const long long i0 = (long long)blockIdx.x * kLossChunk, i1 = min(n, i0 + kLossChunk);
  double s = 0;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    const double d = (double)a[base + i] - (double)b[base + i];   // exact: both are fp32 values
    s = add_d(s, squared ? mul_d(d, d) : fabs(d));                 // the square rounded on its own, never an fma
  }
  s = loss_wave_sum(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(64) void k_loss_finish(const double* __restrict__ part, int B, int nblk,
                                                    double* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0;
  for (int k = 0; k < nblk; ++k) s += part[(size_t)b * nblk + k];
  out[b] = s;
}
int loss_blocks(long long n) { return (int)((n + kLossChunk - 1) / kLossChunk); }
hipError_t launch_loss(const float* a, const float* b, int B, long long n, int squared, double* part, double* out,
                       hipStream_t st) {
  const int nblk = loss_blocks(n);
  hipLaunchKernelGGL(k_loss_partial, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, st, a, b, n, squared, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_loss_finish, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, part, B, nblk, out);
  return hipGetLastError();
}

}  // namespace dsx
