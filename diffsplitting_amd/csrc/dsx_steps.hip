// dsx_steps.hip — the NCHW fp32 pointwise kernels of the samplers (gfx950): the noising step q_sample, one reverse
// update with its intermediate quantities (p_mean_variance / p_sample of the Gaussian samplers, inference_one_step of
// InDI) and the start of interpolate.  The UNet forward around them is the engine's own (dsx_unet_forward); the loops
// keep k_update (dsx_ops.hip), which shares step_update (dsx_kernels.h) with the single step.
#include "dsx_kernels.h"

namespace dsx {

// The skeleton the three kernels share (DSX_EACH4, group4, rows4, load4, store4, aligned16) is in dsx_kernels.h.
// The normals of a group: elements zi[j] of `z`, or of the stream (seed, subseq) when z is nullptr (element i of a
// stream is component i % 4 of Philox block i / 4).  block: zi is one whole Philox block -- always under VEC;
// otherwise (`repeat` on the scalar path) each element looks up its own.
template <bool VEC>
__device__ __forceinline__ void normals4(const float* z, unsigned long long seed, unsigned long long subseq,
                                         const long long zi[4], bool block, int cnt, float out[4]) {
  if (z != nullptr) {
    load4<VEC>(z, zi, cnt, out);
  } else if (VEC || block) {
    normal4(seed, subseq, (unsigned long long)(zi[0] >> 2), out);
  } else {
    DSX_EACH4(j, cnt) {
      float t[4];
      normal4(seed, subseq, (unsigned long long)(zi[j] >> 2), t);
      out[j] = t[zi[j] & 3];
    }
  }
}

// one group per thread: k is the VEC or the scalar instantiation
template <class Args>
static hipError_t launch_groups4(void (*k)(Args), const Args& a, long long n, hipStream_t st) {
  hipLaunchKernelGGL(k, dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// q_sample (sr3 diffusion.py:215-222, ddpm diffusion.py:266-274, indi.py:116-124):
//   two terms   : dst = c0[b] * x0 + c2[b] * z
//   three terms : dst = (c0[b] * x0 + c1[b] * xe) + c2[b] * z
// every product and sum rounded on its own: mul_f / add_f (contraction off) -- hipcc fuses the plain product behind
// __fmul_rn into the sum that follows, and the result then differs from torch's in the last bit.  xe has Ce channels and
// is read at channel c % Ce; dst has Cdst channels and is written at channel coff + c.  z is read from `z`, or drawn:
// element i of the (B, C, H, W) tensor is element i of the stream (seed, subseq), i.e. what k_randn writes there.
// ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void k_q_sample(const QSampleArgs a) {
  const long long HW = a.HW, n = (long long)a.B * a.C * HW;
  const bool three = a.xe != nullptr;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < (n + 3) / 4;
       i4 += (long long)gridDim.x * blockDim.x) {
    long long at[4], row[4], ex[4], dx[4];                     // row = b * C + c
    const int cnt = group4<VEC>(i4, n, at);
    rows4<VEC>(at, cnt, HW, row);
    float c0[4], c1[4], c2[4];
    DSX_EACH4(j, cnt) {
      const long long hw = at[j] - row[j] * HW;
      const int b = (int)(row[j] / a.C), c = (int)(row[j] - (long long)b * a.C);
      ex[j] = ((long long)b * a.Ce + c % a.Ce) * HW + hw;
      dx[j] = ((long long)b * a.Cdst + a.coff + c) * HW + hw;
      c0[j] = a.c0[b]; c2[j] = a.c2[b]; c1[j] = three ? a.c1[b] : 0.f;
    }
    float z[4], x[4], e[4] = {0.f, 0.f, 0.f, 0.f}, o[4];
    normals4<VEC>(a.z, a.seed, a.subseq, at, true, cnt, z);
    if (a.z_out) store4<VEC>(a.z_out, at, cnt, z);             // only with drawn normals (dsx_q_sample)
    load4<VEC>(a.x0, at, cnt, x);
    if (three) load4<VEC>(a.xe, ex, cnt, e);
    DSX_EACH4(j, cnt) {
      float v = mul_f(c0[j], x[j]);
      if (three) v = add_f(v, mul_f(c1[j], e[j]));
      o[j] = add_f(v, mul_f(c2[j], z[j]));
    }
    store4<VEC>(a.dst, dx, cnt, o);
  }
}
hipError_t launch_q_sample(const QSampleArgs& a, hipStream_t st) {
  const bool vec = a.HW % 4 == 0 && aligned16(a.x0, a.xe, a.z, a.z_out, a.dst);
  return launch_groups4(vec ? k_q_sample<true> : k_q_sample<false>, a, (long long)a.B * a.C * a.HW, st);
}

// ---------------------------------------------------------------------------
// One reverse update, step_update (dsx_kernels.h) with per-sample coefficients:
//   out = sigma[b] != 0 ? mean + z*sigma[b] : mean               (no draw and no sum for such a sample)
// z: element i of `z` (element i % CHW with `repeat`: one draw shared by the batch), or the same element of the normal
// stream (seed, subseq); C*H*W being a multiple of 4 under VEC, a group is one whole Philox block under `repeat` too.
// x_out may be x: a thread reads its four elements before it writes them.
// ---------------------------------------------------------------------------
// STREAMS (ids != nullptr): per-sample noise streams (include/dsx.h): element j of sample b takes element j of the stream
// (seed, ids[b]); under VEC a group is one whole Philox block of its sample's stream.
template <bool VEC, bool STREAMS>
__device__ __forceinline__ void posterior_step_body(const PosteriorStepArgs& a, const unsigned long long* ids) {
  const long long CHW = a.CHW, n = (long long)a.B * CHW;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < (n + 3) / 4;
       i4 += (long long)gridDim.x * blockDim.x) {
    long long at[4], b[4], zi[4];
    const int cnt = group4<VEC>(i4, n, at);
    rows4<VEC>(at, cnt, CHW, b);
    bool use_z[4] = {false, false, false, false}, any = false;
    DSX_EACH4(j, cnt) {
      zi[j] = (STREAMS || a.repeat) ? at[j] - b[j] * CHW : at[j];
      use_z[j] = a.x_out != nullptr && a.sigma[b[j]] != 0.f;
      any = any || use_z[j];
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f}, x[4], net[4], x0[4], mean[4], out[4];
    if (STREAMS) {
      if (VEC) {
        if (any) normal4(a.seed, ids[b[0]], (unsigned long long)(zi[0] >> 2), z);
      } else {
        DSX_EACH4(j, cnt) if (use_z[j]) z[j] = normal1(a.seed, ids[b[j]], (unsigned long long)(zi[j] >> 2), (int)(zi[j] & 3));
      }
    } else if (any) {
      normals4<VEC>(a.z, a.seed, a.subseq, zi, !a.repeat, cnt, z);
    }
    load4<VEC>(a.x, at, cnt, x);
    load4<VEC>(a.net, at, cnt, net);
    DSX_EACH4(j, cnt) {
      const long long s = b[j];
      const StepVals v = step_update(a.predict_eps ? a.a[s] : 0.f, a.predict_eps ? a.b[s] : 0.f, a.c1[s], a.c2[s],
                                     a.sigma[s], a.predict_eps, a.clip, x[j], net[j], z[j], use_z[j]);
      x0[j] = v.x0; mean[j] = v.mean; out[j] = v.out;
    }
    if (a.x_recon_out) store4<VEC>(a.x_recon_out, at, cnt, x0);
    if (a.mean_out) store4<VEC>(a.mean_out, at, cnt, mean);
    if (a.x_out) store4<VEC>(a.x_out, at, cnt, out);
  }
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_posterior_step(const PosteriorStepArgs a) {
  posterior_step_body<VEC, false>(a, nullptr);
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_posterior_step_streams(const PosteriorStepArgs a, const StreamIds s) {
  posterior_step_body<VEC, true>(a, s.subseq);
}
hipError_t launch_posterior_step(const PosteriorStepArgs& a, long long HW, hipStream_t st) {
  const bool vec = HW % 4 == 0 && aligned16(a.x, a.net, a.z, a.x_recon_out, a.mean_out, a.x_out);
  return launch_groups4(vec ? k_posterior_step<true> : k_posterior_step<false>, a, (long long)a.B * a.CHW, st);
}
hipError_t launch_posterior_step_streams(const PosteriorStepArgs& a, const StreamIds& s, long long HW, hipStream_t st) {
  if (a.B < 1 || a.B > kStreamRows) return hipErrorInvalidValue;
  const bool vec = HW % 4 == 0 && aligned16(a.x, a.net, a.x_recon_out, a.mean_out, a.x_out);
  hipLaunchKernelGGL(vec ? k_posterior_step_streams<true> : k_posterior_step_streams<false>,
                     dim3(grid_for(((long long)a.B * a.CHW + 3) / 4)), dim3(256), 0, st, a, s);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// The start of interpolate (ddpm diffusion.py:249-259):
//   out = c * (a0[b]*x1 + s0[b]*z1) + d * (a0[b]*x2 + s0[b]*z2)
// the two inner expressions being q_sample's two-term form, c = fp32(1 - lam) and d = fp32(lam) the scalars torch
// multiplies an fp32 tensor with.  z1 / z2: injected, or the normal streams (seed, subseq) and (seed, subseq + 1) at
// the flat index.
// ---------------------------------------------------------------------------
template <bool VEC>
__global__ __launch_bounds__(256) void k_interp_start(const InterpStartArgs a) {
  const long long n = (long long)a.B * a.CHW;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < (n + 3) / 4;
       i4 += (long long)gridDim.x * blockDim.x) {
    long long at[4], b[4];
    const int cnt = group4<VEC>(i4, n, at);
    rows4<VEC>(at, cnt, a.CHW, b);
    float z1[4], z2[4], x1[4], x2[4], o[4];
    normals4<VEC>(a.z1, a.seed, a.subseq, at, true, cnt, z1);
    normals4<VEC>(a.z2, a.seed, a.subseq + 1, at, true, cnt, z2);
    load4<VEC>(a.x1, at, cnt, x1);
    load4<VEC>(a.x2, at, cnt, x2);
    DSX_EACH4(j, cnt) {
      const float a0 = a.a0[b[j]], s0 = a.s0[b[j]];
      const float t1 = add_f(mul_f(a0, x1[j]), mul_f(s0, z1[j]));
      const float t2 = add_f(mul_f(a0, x2[j]), mul_f(s0, z2[j]));
      o[j] = add_f(mul_f(a.c, t1), mul_f(a.d, t2));
    }
    store4<VEC>(a.out, at, cnt, o);
  }
}
hipError_t launch_interp_start(const InterpStartArgs& a, long long HW, hipStream_t st) {
  const bool vec = HW % 4 == 0 && aligned16(a.x1, a.x2, a.z1, a.z2, a.out);
  return launch_groups4(vec ? k_interp_start<true> : k_interp_start<false>, a, (long long)a.B * a.CHW, st);
}

}  // namespace dsx
