// dsx_solver.hip — the update of the few-step solvers (DDIM, DPM-Solver++(2M); rows: model/solvers.py) on gfx950:
// the loop form inside the captured step (k_solver_update, NHWC state, the previous predicted x0 kept on the device)
// and the caller-driven single step (k_solver_step, NCHW).  Both evaluate solver_update (dsx_kernels.h), so a chain of
// single steps reproduces the loop bit for bit; with cp == 0 both are the ancestral kernels' arithmetic.
#include "dsx_kernels.h"

namespace dsx {

// the 16-bit image of v in the activation storage kind (1 bf16, 2 fp16), rounded to nearest even
__device__ __forceinline__ unsigned act16(float v, int kind) {
  if (kind == 1) return __builtin_bit_cast(unsigned short, (__bf16)v);
  return __builtin_bit_cast(unsigned short, (_Float16)v);
}

// ---------------------------------------------------------------------------
// Loop update.  k_update (dsx_ops.hip) with the x0 history: the state, the UNet output and the history are NHWC fp32
// of one shape, so the update is flat -- a thread owns group i4 (four consecutive elements = one Philox block of the
// default noise) and, under VEC (the element count a multiple of 4, every base 16-byte aligned), moves each tensor with
// one 16-byte access: three loads (two where cp == 0) and two stores per group, plus the 8-byte store of the first
// conv's 16-bit copy.  The noise forms are k_update's: Philox (seed, step + 1) at the flat index, injected draws in
// NCHW order, per-sample streams (sample_ids[b] << 24 | step + 1) at the element's NCHW index inside its sample; the
// stream form adds nothing where sigma == 0.  The row's coefficients are uniform over the launch, so whether the
// history is read is one decision per launch: at the first row (cp == 0) it is not read, whatever it holds.
// ---------------------------------------------------------------------------
template <bool VEC, bool STREAMS>
__global__ __launch_bounds__(256) void k_solver_update(const SolverUpdateArgs a) {
  const int step = *a.step_ctr;
  const size_t T = (size_t)a.n_steps;
  const float ca = a.tab[1 * T + step], cb = a.tab[2 * T + step], cx = a.tab[3 * T + step], c0 = a.tab[4 * T + step],
              cp = a.tab[5 * T + step], sg = a.tab[6 * T + step];
  const long long HW = (long long)a.H * a.W;
  const long long n = (long long)a.B * HW * a.C;
  const unsigned long long seed = a.loop_params[0];
  const float* __restrict__ noise = (const float*)(uintptr_t)a.loop_params[1];
  const bool use_z = !STREAMS || sg != 0.f;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < (n + 3) / 4;
       i4 += (long long)gridDim.x * blockDim.x) {
    long long at[4];
    const int cnt = group4<VEC>(i4, n, at);
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!STREAMS && !a.use_noise && sg != 0.f) normal4(seed, (unsigned long long)step + 1, (unsigned long long)i4, z);
    if (a.use_noise || (STREAMS && sg != 0.f)) {
      DSX_EACH4(j, cnt) {
        const int c = (int)(at[j] % a.C);
        const long long p = at[j] / a.C;
        const long long b = p / HW, e = c * HW + p % HW;            // e: the element's NCHW index inside its sample
        if (STREAMS) z[j] = normal1(seed, (a.sample_ids[b] << 24) | (unsigned long long)(step + 1), (unsigned long long)(e >> 2), (int)(e & 3));
        else z[j] = noise[(size_t)step * n + b * a.C * HW + e];
      }
    }
    float x[4], net[4], prev[4] = {0.f, 0.f, 0.f, 0.f}, x0[4], out[4];
    load4<VEC>(a.x, at, cnt, x);
    load4<VEC>(a.net, at, cnt, net);
    if (cp != 0.f) load4<VEC>(a.x0_hist, at, cnt, prev);
    DSX_EACH4(j, cnt) {
      const SolverVals v = solver_update(ca, cb, cx, c0, cp, sg, a.clip, x[j], net[j], prev[j], z[j], use_z);
      x0[j] = v.x0; out[j] = v.out;
    }
    store4<VEC>(a.x0_hist, at, cnt, x0);
    store4<VEC>(a.x, at, cnt, out);
    if (a.x_act) {
      unsigned h[4] = {0u, 0u, 0u, 0u};
      DSX_EACH4(j, cnt) h[j] = act16(out[j], a.x_act_kind);
      store4<VEC>((unsigned short*)a.x_act, at, cnt, h);
    }
  }
}
hipError_t launch_solver_update(const SolverUpdateArgs& a, hipStream_t st) {
  const long long n = (long long)a.B * a.H * a.W * a.C;
  const bool vec = n % 4 == 0 && aligned16(a.x, a.net, a.x0_hist, (const char*)a.x_act);
  auto k = a.sample_ids ? (vec ? k_solver_update<true, true> : k_solver_update<false, true>)
                        : (vec ? k_solver_update<true, false> : k_solver_update<false, false>);
  hipLaunchKernelGGL(k, dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Single step: solver_update with per-sample coefficients on the NCHW skeleton of dsx_steps.hip.
//   out = sigma[b] != 0 ? m + z*sigma[b] : m                     (no draw and no sum for such a sample)
// x0_prev is read for the samples whose cp != 0 only (under VEC a group lies inside one sample: one 16-byte load or
// none); with x0_prev == nullptr every cp counts as 0.  x_out may be x and x_recon_out may be x0_prev: a thread reads
// its four elements of each before it writes them.
// STREAMS: element j of sample b takes element j of the stream (seed, ids[b]).
// ---------------------------------------------------------------------------
template <bool VEC, bool STREAMS>
__device__ __forceinline__ void solver_step_body(const SolverStepArgs& a, const unsigned long long* ids) {
  const long long CHW = a.CHW, n = (long long)a.B * CHW;
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < (n + 3) / 4;
       i4 += (long long)gridDim.x * blockDim.x) {
    long long at[4], b[4], zi[4];
    const int cnt = group4<VEC>(i4, n, at);
    rows4<VEC>(at, cnt, CHW, b);
    bool use_z[4] = {false, false, false, false}, any_z = false;
    float cp[4] = {0.f, 0.f, 0.f, 0.f};
    DSX_EACH4(j, cnt) {
      zi[j] = STREAMS ? at[j] - b[j] * CHW : at[j];
      use_z[j] = a.sigma[b[j]] != 0.f;
      any_z = any_z || use_z[j];
      cp[j] = a.x0_prev != nullptr ? a.cp[b[j]] : 0.f;
    }
    float z[4] = {0.f, 0.f, 0.f, 0.f}, x[4], net[4], prev[4] = {0.f, 0.f, 0.f, 0.f}, x0[4], out[4];
    if (STREAMS) {
      if (VEC) {
        if (any_z) normal4(a.seed, ids[b[0]], (unsigned long long)(zi[0] >> 2), z);
      } else {
        DSX_EACH4(j, cnt) if (use_z[j]) z[j] = normal1(a.seed, ids[b[j]], (unsigned long long)(zi[j] >> 2), (int)(zi[j] & 3));
      }
    } else if (any_z) {
      if (a.z != nullptr) load4<VEC>(a.z, at, cnt, z);
      else normal4(a.seed, a.subseq, (unsigned long long)i4, z);        // the group is Philox block i4 of the flat stream
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
      const SolverVals v = solver_update(a.a[s], a.b[s], a.cx[s], a.c0[s], cp[j], a.sigma[s], a.clip, x[j], net[j], prev[j],
                                         z[j], use_z[j]);
      x0[j] = v.x0; out[j] = v.out;
    }
    store4<VEC>(a.x_recon_out, at, cnt, x0);
    store4<VEC>(a.x_out, at, cnt, out);
  }
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_solver_step(const SolverStepArgs a) {
  solver_step_body<VEC, false>(a, nullptr);
}
template <bool VEC>
__global__ __launch_bounds__(256) void k_solver_step_streams(const SolverStepArgs a, const StreamIds s) {
  solver_step_body<VEC, true>(a, s.subseq);
}
static bool solver_step_vec(const SolverStepArgs& a, long long HW) {
  return HW % 4 == 0 && aligned16(a.x, a.net, a.x0_prev, a.z, a.x_recon_out, a.x_out);
}
hipError_t launch_solver_step(const SolverStepArgs& a, long long HW, hipStream_t st) {
  hipLaunchKernelGGL(solver_step_vec(a, HW) ? k_solver_step<true> : k_solver_step<false>,
                     dim3(grid_for(((long long)a.B * a.CHW + 3) / 4)), dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_solver_step_streams(const SolverStepArgs& a, const StreamIds& s, long long HW, hipStream_t st) {
  if (a.B < 1 || a.B > kStreamRows) return hipErrorInvalidValue;
  hipLaunchKernelGGL(solver_step_vec(a, HW) ? k_solver_step_streams<true> : k_solver_step_streams<false>,
                     dim3(grid_for(((long long)a.B * a.CHW + 3) / 4)), dim3(256), 0, st, a, s);
  return hipGetLastError();
}

}  // namespace dsx
