// dsx_steps.hip — the pointwise kernels of the samplers (gfx950).  NCHW fp32, on caller tensors: the noising step
// q_sample, one reverse update with its intermediate quantities (p_mean_variance / p_sample of the Gaussian samplers,
// inference_one_step of InDI, one step of DDIM / DPM-Solver++(2M)) and the start of interpolate.  NHWC, inside the
// executor's loops: that same update on the state (k_update) and the step counter (k_advance).  Both updates evaluate
// step_update (dsx_kernels.h), so a chain of single steps reproduces a loop bit for bit.  The UNet forward around them
// is the engine's own (dsx_unet_forward).
#include "dsx_kernels.h"

namespace dsx {

// The skeleton the kernels share (DSX_EACH4, group4, rows4, load4, store4, aligned16) is in dsx_kernels.h.
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
// x0_prev is read for the samples whose cp != 0 only (under VEC a group lies inside one sample: one 16-byte load or
// none); with x0_prev == nullptr every cp counts as 0.  x_out may be x and x_recon_out may be x0_prev: a thread reads
// its four elements of each before it writes them.
// ---------------------------------------------------------------------------
// STREAMS (ids != nullptr): per-sample noise streams (include/dsx.h): element j of sample b takes element j of the stream
// (seed, ids[b]); under VEC a group is one whole Philox block of its sample's stream.
template <bool VEC, bool STREAMS>
__device__ __forceinline__ void step_body(const StepArgs& a, const unsigned long long* ids) {
  const long long CHW = a.CHW, n = (long long)a.B * CHW;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < (n + 3) / 4;
       i4 += (long long)gridDim.x * blockDim.x) {
    long long at[4], b[4], zi[4];
    const int cnt = group4<VEC>(i4, n, at);
    rows4<VEC>(at, cnt, CHW, b);
    bool use_z[4] = {false, false, false, false}, any = false;
    float cp[4] = {0.f, 0.f, 0.f, 0.f};
    DSX_EACH4(j, cnt) {
      zi[j] = (STREAMS || a.repeat) ? at[j] - b[j] * CHW : at[j];
      use_z[j] = a.x_out != nullptr && a.sigma[b[j]] != 0.f;
      any = any || use_z[j];
      cp[j] = a.x0_prev != nullptr ? a.cp[b[j]] : 0.f;
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f}, x[4], net[4], prev[4] = {0.f, 0.f, 0.f, 0.f}, x0[4], mean[4], out[4];
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
    if (VEC) {
      if (cp[0] != 0.f) load4<true>(a.x0_prev, at, cnt, prev);
    } else {
      DSX_EACH4(j, cnt) if (cp[j] != 0.f) prev[j] = a.x0_prev[at[j]];
    }
    DSX_EACH4(j, cnt) {
      const long long s = b[j];
      const StepVals v = step_update(a.predict_eps ? a.a[s] : 0.f, a.predict_eps ? a.b[s] : 0.f, a.c1[s], a.c2[s], cp[j],
                                     a.sigma[s], a.predict_eps, a.clip, x[j], net[j], prev[j], z[j], use_z[j]);
      x0[j] = v.x0; mean[j] = v.mean; out[j] = v.out;
    }
    if (a.x_recon_out) store4<VEC>(a.x_recon_out, at, cnt, x0);
    if (a.mean_out) store4<VEC>(a.mean_out, at, cnt, mean);
    if (a.x_out) store4<VEC>(a.x_out, at, cnt, out);
  }
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_step(const StepArgs a) {
  step_body<VEC, false>(a, nullptr);
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_step_streams(const StepArgs a, const StreamIds s) {
  step_body<VEC, true>(a, s.subseq);
}
hipError_t launch_step(const StepArgs& a, long long HW, const uint64_t* ids, uint64_t draw, hipStream_t st) {
  const bool vec = HW % 4 == 0 && aligned16(a.x, a.net, a.x0_prev, a.z, a.x_recon_out, a.mean_out, a.x_out);
  if (ids == nullptr) return launch_groups4(vec ? k_step<true> : k_step<false>, a, (long long)a.B * a.CHW, st);
  // (a chunk starts kStreamRows * CHW elements on: under `vec` 16-byte aligned like the bases)
  return each_stream_chunk(a.B, ids, draw, [&](int b0, int rows, const StreamIds& s) {
    const size_t off = (size_t)b0 * a.CHW;
    auto el = [&](auto* p) { return p ? p + off : nullptr; };
    auto co = [&](const float* p) { return p ? p + b0 : nullptr; };
    StepArgs c = a;
    c.x = el(a.x); c.net = el(a.net); c.x0_prev = el(a.x0_prev);
    c.a = co(a.a); c.b = co(a.b); c.c1 = co(a.c1); c.c2 = co(a.c2); c.cp = co(a.cp); c.sigma = co(a.sigma);
    c.z = nullptr; c.subseq = 0; c.repeat = 0;
    c.x_recon_out = el(a.x_recon_out); c.mean_out = el(a.mean_out); c.x_out = el(a.x_out);
    c.B = rows;
    hipLaunchKernelGGL(vec ? k_step_streams<true> : k_step_streams<false>, dim3(grid_for(((long long)rows * a.CHW + 3) / 4)),
                       dim3(256), 0, st, c, s);
    return hipGetLastError();
  });
}

// ---------------------------------------------------------------------------
// The loop update: step_update inside the captured step of dsx_sample_loop, dsx_sample_loop_streams and
// dsx_solver_loop.  The step index lives in device memory so one captured graph replays T times.  The state, the UNet
// output and the solvers' x0 history are NHWC fp32 of one shape, so the update is flat: a thread owns group i4 (four
// consecutive elements = one Philox block of the default noise) and, under VEC (H*W*C a multiple of 4, every base
// 16-byte aligned: a group lies inside one sample), moves each tensor with one 16-byte access, plus the 8-byte store
// of the first conv's 16-bit copy.  Coefficients: row `step` of the table, or with per_sample row step*B + b, looked up
// once per group under VEC and once per element otherwise.
// Noise: Philox (seed, step + 1) at the flat index, drawn when per_sample or sigma != 0; injected draws in NCHW order;
// STREAMS: per-sample noise streams (include/dsx.h) -- the four elements of a group may lie in different pixels and
// channels (C = 3), so each looks up its own (b, c, hw), the stream of its sample (a.sample_ids[b] << 24 | step + 1)
// and component (c*HW + hw) % 4 of Philox block (c*HW + hw) / 4, the element the NCHW tensor of dsx_randn_samples
// holds there.  The stream form neither draws nor adds where sigma == 0, as the single step does; the other two
// always take the sum.
// History (a.x0_hist, never with per_sample): the row is uniform over the launch, so whether it is read is one
// decision per launch -- at a row with cp == 0 (the first) it is not read, whatever it holds.
// ---------------------------------------------------------------------------
struct UpdateRow { float a, b, c1, c2, cp, sg; };
__device__ __forceinline__ UpdateRow update_row(const UpdateArgs& a, size_t k) {
  const size_t T = (size_t)a.n_steps;
  return {a.tab[1 * T + k], a.tab[2 * T + k], a.tab[3 * T + k], a.tab[4 * T + k], a.tab[5 * T + k], a.tab[6 * T + k]};
}
// the 16-bit image of v in the activation storage kind (1 bf16, 2 fp16), rounded to nearest even
__device__ __forceinline__ unsigned act16(float v, int kind) {
  if (kind == 1) return __builtin_bit_cast(unsigned short, (__bf16)v);
  return __builtin_bit_cast(unsigned short, (_Float16)v);
}
template <bool VEC, bool STREAMS>
__global__ __launch_bounds__(256) void k_update(const UpdateArgs a) {
  const int step = *a.step_ctr;
  const UpdateRow r0 = update_row(a, a.per_sample ? 0 : (size_t)step);   // the launch's row (per_sample: a placeholder, replaced below)
  const long long HW = (long long)a.H * a.W, per = HW * a.C, n = (long long)a.B * per;
  const unsigned long long seed = a.loop_params[0];
  const float* __restrict__ noise = (const float*)(uintptr_t)a.loop_params[1];
  const bool hist = a.x0_hist != nullptr && r0.cp != 0.f;
  const bool by_sample = STREAMS || a.use_noise || a.per_sample;      // someone needs the element's sample
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < (n + 3) / 4;
       i4 += (long long)gridDim.x * blockDim.x) {
    long long at[4], b[4] = {0, 0, 0, 0};
    const int cnt = group4<VEC>(i4, n, at);
    if (by_sample) rows4<VEC>(at, cnt, per, b);
    UpdateRow r[4] = {r0, r0, r0, r0};
    if (a.per_sample) {
      if (VEC) r[0] = r[1] = r[2] = r[3] = update_row(a, (size_t)step * a.B + (size_t)b[0]);
      else DSX_EACH4(j, cnt) r[j] = update_row(a, (size_t)step * a.B + (size_t)b[j]);
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!STREAMS && !a.use_noise && (a.per_sample || r0.sg != 0.f)) normal4(seed, (unsigned long long)step + 1, (unsigned long long)i4, z);
    DSX_EACH4(j, cnt) if (a.use_noise || (STREAMS && r[j].sg != 0.f)) {
      const long long p = at[j] / a.C;
      const long long e = (at[j] - p * a.C) * HW + (p - b[j] * HW);     // the element's NCHW index inside its sample
      if (STREAMS) z[j] = normal1(seed, (a.sample_ids[b[j]] << 24) | (unsigned long long)(step + 1), (unsigned long long)(e >> 2), (int)(e & 3));
      else z[j] = noise[(size_t)step * n + b[j] * per + e];
    }
    float x[4], net[4], prev[4] = {0.f, 0.f, 0.f, 0.f}, x0[4], out[4];
    load4<VEC>(a.x, at, cnt, x);
    load4<VEC>(a.net, at, cnt, net);
    if (hist) load4<VEC>(a.x0_hist, at, cnt, prev);
    DSX_EACH4(j, cnt) {
      const StepVals v = step_update(r[j].a, r[j].b, r[j].c1, r[j].c2, hist ? r[j].cp : 0.f, r[j].sg, a.predict_eps, a.clip,
                                     x[j], net[j], prev[j], z[j], !STREAMS || r[j].sg != 0.f);
      x0[j] = v.x0; out[j] = v.out;
    }
    if (a.x0_hist) store4<VEC>(a.x0_hist, at, cnt, x0);
    store4<VEC>(a.x, at, cnt, out);
    if (a.x_act) {
      unsigned h[4] = {0u, 0u, 0u, 0u};
      DSX_EACH4(j, cnt) h[j] = act16(out[j], a.x_act_kind);
      store4<VEC>((unsigned short*)a.x_act, at, cnt, h);
    }
  }
}
hipError_t launch_update(const UpdateArgs& a, hipStream_t st) {
  if (a.x0_hist && a.per_sample) return hipErrorInvalidValue;
  const long long per = (long long)a.H * a.W * a.C;
  const bool vec = per % 4 == 0 && aligned16(a.x, a.net, a.x0_hist, (const char*)a.x_act);
  auto k = a.sample_ids ? (vec ? k_update<true, true> : k_update<false, true>)
                        : (vec ? k_update<true, false> : k_update<false, false>);
  return launch_groups4(k, a, (long long)a.B * per, st);
}
__global__ void k_advance(int* ctr) { if (threadIdx.x == 0) *ctr += 1; }
hipError_t launch_advance(int* step_ctr, hipStream_t st) {
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, st, step_ctr);
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
