// dsx_objective.hip — the forward half of the training objective (gfx950): the noising step q_sample of the SR3 / DDPM /
// InDI samplers in one launch, and the per-sample L1 / L2 reduction the loss is formed from.  The UNet forward between
// them is the engine's own (dsx_unet_forward).
#include "dsx_kernels.h"

namespace dsx {

// ---------------------------------------------------------------------------
// q_sample (sr3 diffusion.py:215-222, ddpm diffusion.py:266-274, indi.py:116-124), NCHW fp32:
//   two terms   : dst = c0[b] * x0 + c2[b] * z
//   three terms : dst = (c0[b] * x0 + c1[b] * xe) + c2[b] * z
// every product and sum rounded on its own: mul_f / add_f (contraction off) -- hipcc fuses the plain product behind
// __fmul_rn into the sum that follows, and the result then differs from torch's in the last bit.  xe has Ce channels and
// is read at channel c % Ce; dst has Cdst channels and is written at channel coff + c.  z is read from `z`, or drawn: element i of
// the (B, C, H, W) tensor is element i of the stream (seed, subseq), i.e. what k_randn writes there.
// A thread owns one group of four consecutive elements (= one Philox block).  VEC: H * W is a multiple of 4 and every
// base pointer is 16-byte aligned, so a group lies inside one (b, c) row and is 16-byte aligned in every tensor.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float q_term(float c0, float x0, bool three, float c1, float xe, float c2, float z) {
  float v = mul_f(c0, x0);
  if (three) v = add_f(v, mul_f(c1, xe));
  return add_f(v, mul_f(c2, z));
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_q_sample(const QSampleArgs a) {
  const long long HW = a.HW, CHW = (long long)a.C * HW;
  const long long n = (long long)a.B * CHW, n4 = (n + 3) / 4;
  const bool three = a.xe != nullptr;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < n4;
       i4 += (long long)gridDim.x * blockDim.x) {
    const long long i0 = i4 * 4;
    float z[4];
    if (a.z == nullptr) normal4(a.seed, a.subseq, (unsigned long long)i4, z);
    if (VEC) {
      const long long row = i0 / HW, hw = i0 - row * HW;       // row = b * C + c
      const int b = (int)(row / a.C), c = (int)(row - (long long)b * a.C);
      const float c0 = a.c0[b], c2 = a.c2[b], c1 = three ? a.c1[b] : 0.f;
      const float4 x = *(const float4*)(a.x0 + i0);
      float4 e = make_float4(0.f, 0.f, 0.f, 0.f);
      if (three) e = *(const float4*)(a.xe + ((long long)b * a.Ce + c % a.Ce) * HW + hw);
      if (a.z != nullptr) {
        const float4 zz = *(const float4*)(a.z + i0);
        z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w;
      } else if (a.z_out != nullptr) {
        *(float4*)(a.z_out + i0) = make_float4(z[0], z[1], z[2], z[3]);
      }
      float4 o;
      o.x = q_term(c0, x.x, three, c1, e.x, c2, z[0]);
      o.y = q_term(c0, x.y, three, c1, e.y, c2, z[1]);
      o.z = q_term(c0, x.z, three, c1, e.z, c2, z[2]);
      o.w = q_term(c0, x.w, three, c1, e.w, c2, z[3]);
      *(float4*)(a.dst + ((long long)b * a.Cdst + a.coff + c) * HW + hw) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = i0 + j;
        if (i >= n) break;
        const long long row = i / HW, hw = i - row * HW;
        const int b = (int)(row / a.C), c = (int)(row - (long long)b * a.C);
        float zz = z[j];
        if (a.z != nullptr) zz = a.z[i];
        else if (a.z_out != nullptr) a.z_out[i] = zz;
        const float e = three ? a.xe[((long long)b * a.Ce + c % a.Ce) * HW + hw] : 0.f;
        a.dst[((long long)b * a.Cdst + a.coff + c) * HW + hw] =
            q_term(a.c0[b], a.x0[i], three, three ? a.c1[b] : 0.f, e, a.c2[b], zz);
      }
    }
  }
}

hipError_t launch_q_sample(const QSampleArgs& a, hipStream_t st) {
  const long long n4 = ((long long)a.B * a.C * a.HW + 3) / 4;
  long long g = (n4 + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  auto misaligned = [](const void* p) { return ((uintptr_t)p & 15u) != 0; };
  const bool vec = a.HW % 4 == 0 && !misaligned(a.x0) && !misaligned(a.xe) && !misaligned(a.z) && !misaligned(a.z_out) &&
                   !misaligned(a.dst);
  if (vec) hipLaunchKernelGGL(k_q_sample<true>, dim3((unsigned)g), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_q_sample<false>, dim3((unsigned)g), dim3(256), 0, st, a);
  return hipGetLastError();
}

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
