// dsx_steps.hip — caller-driven reverse sampling (gfx950): one reverse update with its intermediate quantities
// (p_mean_variance / p_sample of the Gaussian samplers, inference_one_step of InDI) and the start of interpolate.
// The UNet forward in front of a step is the engine's own (dsx_unet_forward); the loops keep k_update (dsx_ops.hip).
#include "dsx_kernels.h"

namespace dsx {

__device__ __forceinline__ float sub_f(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}

// element `zi` of the normal stream (seed, subseq): component zi % 4 of Philox block zi / 4
__device__ __forceinline__ float normal1(unsigned long long seed, unsigned long long subseq, long long zi) {
  float z[4];
  normal4(seed, subseq, (unsigned long long)(zi >> 2), z);
  return z[zi & 3];
}

// ---------------------------------------------------------------------------
// One reverse update (sr3 diffusion.py:141-175, ddpm diffusion.py:163-203, indi.py:62-69), NCHW fp32, k_update's
// arithmetic with per-sample coefficients, every product and sum rounded on its own:
//   x0   = predict_eps ? clamp(a[b]*x - b[b]*net) : net          (the clamp to +-1 only with clip)
//   mean = c1[b]*x0 + c2[b]*x
//   out  = sigma[b] != 0 ? mean + z*sigma[b] : mean               (no draw and no sum for such a sample)
// z: element i of `z` (element i % CHW with `repeat`: one draw shared by the batch), or the same element of the normal
// stream (seed, subseq).  A thread owns four consecutive elements (= one Philox block without `repeat`).  VEC: H * W is a
// multiple of 4 and every base pointer is 16-byte aligned, so a group lies inside one (b, c) row -- and, C*H*W being a
// multiple of 4 too, maps onto one whole Philox block under `repeat` as well.  x_out may be x: a thread reads its four
// elements before it writes them.
// ---------------------------------------------------------------------------
struct StepVals { float x0, mean, out; };
__device__ __forceinline__ StepVals step_term(const PosteriorStepArgs& a, int b, float x, float net, float z,
                                              bool use_z) {
  StepVals v;
  v.x0 = net;
  if (a.predict_eps) {
    v.x0 = sub_f(mul_f(a.a[b], x), mul_f(a.b[b], net));
    if (a.clip) v.x0 = fminf(fmaxf(v.x0, -1.0f), 1.0f);
  }
  v.mean = add_f(mul_f(a.c1[b], v.x0), mul_f(a.c2[b], x));
  v.out = use_z ? add_f(v.mean, mul_f(z, a.sigma[b])) : v.mean;
  return v;
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_posterior_step(const PosteriorStepArgs a) {
  const long long CHW = a.CHW, n = (long long)a.B * CHW, n4 = (n + 3) / 4;
  const bool philox = a.x_out != nullptr && a.z == nullptr;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < n4;
       i4 += (long long)gridDim.x * blockDim.x) {
    const long long i0 = i4 * 4;
    if (VEC) {
      const int b = (int)(i0 / CHW);
      const long long z0 = a.repeat ? i0 - (long long)b * CHW : i0;
      const bool use_z = a.x_out != nullptr && a.sigma[b] != 0.f;
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (use_z) {
        if (philox) {
          normal4(a.seed, a.subseq, (unsigned long long)(z0 >> 2), z);
        } else {
          const float4 zz = *(const float4*)(a.z + z0);
          z[0] = zz.x; z[1] = zz.y; z[2] = zz.z; z[3] = zz.w;
        }
      }
      const float4 x = *(const float4*)(a.x + i0), e = *(const float4*)(a.net + i0);
      const StepVals v0 = step_term(a, b, x.x, e.x, z[0], use_z), v1 = step_term(a, b, x.y, e.y, z[1], use_z);
      const StepVals v2 = step_term(a, b, x.z, e.z, z[2], use_z), v3 = step_term(a, b, x.w, e.w, z[3], use_z);
      if (a.x_recon_out) *(float4*)(a.x_recon_out + i0) = make_float4(v0.x0, v1.x0, v2.x0, v3.x0);
      if (a.mean_out) *(float4*)(a.mean_out + i0) = make_float4(v0.mean, v1.mean, v2.mean, v3.mean);
      if (a.x_out) *(float4*)(a.x_out + i0) = make_float4(v0.out, v1.out, v2.out, v3.out);
    } else {
      const int cnt = (int)min(4LL, n - i0);
      bool use_z[4] = {false, false, false, false}, any = false;
      for (int j = 0; j < cnt; ++j) {
        use_z[j] = a.x_out != nullptr && a.sigma[(i0 + j) / CHW] != 0.f;
        any = any || use_z[j];
      }
      float z[4] = {0.f, 0.f, 0.f, 0.f};
      if (any && philox && !a.repeat) normal4(a.seed, a.subseq, (unsigned long long)i4, z);
      float xs[4], es[4];
      for (int j = 0; j < cnt; ++j) { xs[j] = a.x[i0 + j]; es[j] = a.net[i0 + j]; }
      for (int j = 0; j < cnt; ++j) {
        const long long i = i0 + j;
        const int b = (int)(i / CHW);
        float zz = z[j];
        if (use_z[j]) {
          const long long zi = a.repeat ? i - (long long)b * CHW : i;
          if (!philox) zz = a.z[zi];
          else if (a.repeat) zz = normal1(a.seed, a.subseq, zi);
        }
        const StepVals v = step_term(a, b, xs[j], es[j], zz, use_z[j]);
        if (a.x_recon_out) a.x_recon_out[i] = v.x0;
        if (a.mean_out) a.mean_out[i] = v.mean;
        if (a.x_out) a.x_out[i] = v.out;
      }
    }
  }
}

static unsigned steps_grid(long long n4) {
  long long g = (n4 + 255) / 256;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (unsigned)g;
}
static bool misaligned(const void* p) { return ((uintptr_t)p & 15u) != 0; }   // nullptr counts as aligned

hipError_t launch_posterior_step(const PosteriorStepArgs& a, long long HW, hipStream_t st) {
  const long long n4 = ((long long)a.B * a.CHW + 3) / 4;
  const bool vec = HW % 4 == 0 && !misaligned(a.x) && !misaligned(a.net) && !misaligned(a.z) &&
                   !misaligned(a.x_recon_out) && !misaligned(a.mean_out) && !misaligned(a.x_out);
  if (vec) hipLaunchKernelGGL(k_posterior_step<true>, dim3(steps_grid(n4)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_posterior_step<false>, dim3(steps_grid(n4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The start of interpolate (ddpm diffusion.py:249-259), NCHW fp32:
//   out = c * (a0[b]*x1 + s0[b]*z1) + d * (a0[b]*x2 + s0[b]*z2)
// the two inner expressions being q_sample's two-term form (k_q_sample), c = fp32(1 - lam) and d = fp32(lam) the
// scalars torch multiplies an fp32 tensor with.  z1 / z2: injected, or the normal streams (seed, subseq) and
// (seed, subseq + 1) at the flat index.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float interp_term(float c, float d, float a0, float s0, float x1, float z1, float x2,
                                             float z2) {
  const float t1 = add_f(mul_f(a0, x1), mul_f(s0, z1));
  const float t2 = add_f(mul_f(a0, x2), mul_f(s0, z2));
  return add_f(mul_f(c, t1), mul_f(d, t2));
}

template <bool VEC>
__global__ __launch_bounds__(256) void k_interp_start(const InterpStartArgs a) {
  const long long CHW = a.CHW, n = (long long)a.B * CHW, n4 = (n + 3) / 4;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < n4;
       i4 += (long long)gridDim.x * blockDim.x) {
    const long long i0 = i4 * 4;
    float z1[4], z2[4];
    if (a.z1 == nullptr) {
      normal4(a.seed, a.subseq, (unsigned long long)i4, z1);
      normal4(a.seed, a.subseq + 1, (unsigned long long)i4, z2);
    }
    if (VEC) {
      const int b = (int)(i0 / CHW);
      const float a0 = a.a0[b], s0 = a.s0[b];
      if (a.z1 != nullptr) {
        const float4 p = *(const float4*)(a.z1 + i0), q = *(const float4*)(a.z2 + i0);
        z1[0] = p.x; z1[1] = p.y; z1[2] = p.z; z1[3] = p.w;
        z2[0] = q.x; z2[1] = q.y; z2[2] = q.z; z2[3] = q.w;
      }
      const float4 x1 = *(const float4*)(a.x1 + i0), x2 = *(const float4*)(a.x2 + i0);
      float4 o;
      o.x = interp_term(a.c, a.d, a0, s0, x1.x, z1[0], x2.x, z2[0]);
      o.y = interp_term(a.c, a.d, a0, s0, x1.y, z1[1], x2.y, z2[1]);
      o.z = interp_term(a.c, a.d, a0, s0, x1.z, z1[2], x2.z, z2[2]);
      o.w = interp_term(a.c, a.d, a0, s0, x1.w, z1[3], x2.w, z2[3]);
      *(float4*)(a.out + i0) = o;
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const long long i = i0 + j;
        if (i >= n) break;
        const int b = (int)(i / CHW);
        const float p = a.z1 != nullptr ? a.z1[i] : z1[j], q = a.z1 != nullptr ? a.z2[i] : z2[j];
        a.out[i] = interp_term(a.c, a.d, a.a0[b], a.s0[b], a.x1[i], p, a.x2[i], q);
      }
    }
  }
}

hipError_t launch_interp_start(const InterpStartArgs& a, long long HW, hipStream_t st) {
  const long long n4 = ((long long)a.B * a.CHW + 3) / 4;
  const bool vec = HW % 4 == 0 && !misaligned(a.x1) && !misaligned(a.x2) && !misaligned(a.z1) && !misaligned(a.z2) &&
                   !misaligned(a.out);
  if (vec) hipLaunchKernelGGL(k_interp_start<true>, dim3(steps_grid(n4)), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_interp_start<false>, dim3(steps_grid(n4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dsx
