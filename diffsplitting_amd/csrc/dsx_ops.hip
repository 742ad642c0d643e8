// dsx_ops.hip — the non-conv kernels of the sampling path (gfx950):
// GroupNorm statistics (wavefront-shuffle reductions), time embedding + FiLM,
// the sampler update with Philox noise, layout conversion, tile gather / stitch.
// (Attention: dsx_attn.hip.)
#include "dsx_kernels.h"
#include <algorithm>

namespace dsx {

typedef __attribute__((ext_vector_type(16))) float f32x16;

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// ---------------------------------------------------------------------------
// Per-channel partial sums for GroupNorm (nn.GroupNorm inside Block /
// SelfAttention, unet.py:84,120).  x: [B][HW][C] fp32 NHWC.  One workgroup
// reduces one pixel chunk of one image; lanes run along C (coalesced float4),
// partial sums are kept in double so the later E[x^2]-E[x]^2 is safe.
// part[((b*nchunk + ch)*C + c)*2 + {0:sum, 1:sumsq}]
// ---------------------------------------------------------------------------
// activation storage kind `st`: 0 fp32, 1 bf16, 2 fp16
__device__ __forceinline__ float cvt16(unsigned short h, int st) {
  return st == 1 ? __builtin_bit_cast(float, (unsigned)h << 16) : (float)__builtin_bit_cast(_Float16, h);
}
__device__ __forceinline__ float4 load4_act(const void* base, size_t i, int st) {   // 4 consecutive elements
  if (st) {
    const uint2 r = *(const uint2*)((const unsigned short*)base + i);
    return make_float4(cvt16((unsigned short)(r.x & 0xffffu), st), cvt16((unsigned short)(r.x >> 16), st),
                       cvt16((unsigned short)(r.y & 0xffffu), st), cvt16((unsigned short)(r.y >> 16), st));
  }
  return *(const float4*)((const float*)base + i);
}
__device__ __forceinline__ float load1_act(const void* base, size_t i, int st) {
  return st ? cvt16(((const unsigned short*)base)[i], st) : ((const float*)base)[i];
}
__device__ __forceinline__ void store1_act(void* base, size_t i, float v, int st) {
  if (st == 1) {
    const __bf16 h = (__bf16)v;   // RNE
    ((unsigned short*)base)[i] = __builtin_bit_cast(unsigned short, h);
  } else if (st == 2) {
    ((_Float16*)base)[i] = (_Float16)v;   // RNE
  } else {
    ((float*)base)[i] = v;
  }
}

__global__ __launch_bounds__(256) void k_chan_stats(const void* __restrict__ x, int bf16, int HW, int C,
                                                    int nchunk, double* __restrict__ part) {
  __shared__ double red[256 * 8];
  const int b = blockIdx.x / nchunk, ch = blockIdx.x % nchunk;
  const int CV = C >> 2;  // float4 columns
  const int p0 = (int)((long long)HW * ch / nchunk), p1 = (int)((long long)HW * (ch + 1) / nchunk);
  const size_t xb = (size_t)b * HW * C;
  for (int cv0 = 0; cv0 < CV; cv0 += 256) {
    const int cols = min(256, CV - cv0);   // columns in this pass
    const int rows = 256 / cols;           // pixel lanes per column (>=1)
    const int col = threadIdx.x % cols, rl = threadIdx.x / cols;
    double s[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
    if (rl < rows) {
      for (int p = p0 + rl; p < p1; p += rows) {
        const float4 v = load4_act(x, xb + (size_t)p * C + (cv0 + col) * 4, bf16);
        s[0] += v.x; q[0] += (double)v.x * v.x;
        s[1] += v.y; q[1] += (double)v.y * v.y;
        s[2] += v.z; q[2] += (double)v.z * v.z;
        s[3] += v.w; q[3] += (double)v.w * v.w;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) { red[threadIdx.x * 8 + j] = s[j]; red[threadIdx.x * 8 + 4 + j] = q[j]; }
    __syncthreads();
    if (threadIdx.x < cols) {
      double ts[4] = {0, 0, 0, 0}, tq[4] = {0, 0, 0, 0};
      for (int r = 0; r < rows; ++r) {
        const int t = r * cols + threadIdx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) { ts[j] += red[t * 8 + j]; tq[j] += red[t * 8 + 4 + j]; }
      }
      double* o = part + (((size_t)b * nchunk + ch) * C + (cv0 + threadIdx.x) * 4) * 2;
#pragma unroll
      for (int j = 0; j < 4; ++j) { o[2 * j] = ts[j]; o[2 * j + 1] = tq[j]; }
    }
    __syncthreads();
  }
}

hipError_t launch_chan_stats(const void* x, int bf16, int B, int HW, int C, int nchunk, double* part,
                             hipStream_t st) {
  hipLaunchKernelGGL(k_chan_stats, dim3((unsigned)(B * nchunk)), dim3(256), 0, st, x, bf16, HW, C, nchunk, part);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// GroupNorm finalize over a (possibly concatenated) input: groups may straddle
// the two sources (e.g. 128+64 channels / 32 groups).  One workgroup per image.
//   y = (x-mean)*rstd*gamma + beta  ==  x*scale + shift
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_gn_finalize(const GnFinArgs a) {
  // one wave per (image, group)
  const int lane = threadIdx.x;
  // first, so that they fly together with this launch's own loads: the consumer conv's weight slices -> this XCD's L2
  const PfAcc pf_acc = l2_prefetch(a.pf, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, lane, 64);
  gn_finalize_item<1>(a, blockIdx.x, blockIdx.y, lane, nullptr);
  l2_prefetch_retire(a.pf, pf_acc);
}
// four waves per (image, group): the launches with hundreds of partial rows per group (128^2 and 64^2 maps) were five
// dependent load round trips long with one wave
__global__ __launch_bounds__(256) void k_gn_finalize_wide(const GnFinArgs a) {
  __shared__ double red[8];
  const int tid = threadIdx.x;
  const PfAcc pf_acc = l2_prefetch(a.pf, blockIdx.y * gridDim.x + blockIdx.x, gridDim.x * gridDim.y, tid, 256);
  gn_finalize_item<4>(a, blockIdx.x, blockIdx.y, tid, red);
  l2_prefetch_retire(a.pf, pf_acc);
}

hipError_t launch_gn_finalize(const GnFinArgs& a, hipStream_t st) {
  const int cpg = (a.C0 + a.C1) / a.groups;
  const long long items = (long long)cpg * std::max(a.nchunk0, a.nchunk1);   // partial rows x channels per group (upper bound)
  if (items > 512)
    hipLaunchKernelGGL(k_gn_finalize_wide, dim3((unsigned)a.B, (unsigned)a.groups), dim3(256), 0, st, a);
  else
    hipLaunchKernelGGL(k_gn_finalize, dim3((unsigned)a.B, (unsigned)a.groups), dim3(64), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Time embedding MLP + every ResnetBlock's FiLM / time vector in ONE launch
// (29 addmm launches per forward in the reference).
//   sr3 : PositionalEncoding -> Linear -> Swish -> Linear ; film_k = Linear_k(t)
//         (unet.py:18-50,177-187)
//   ddpm: TimeEmbedding -> Linear -> Swish -> Linear ; film_k = Linear_k(Swish(t))
//         (ddpm unet.py:19-34,78-96,163-173)
// grid = (distinct time values, splits): every workgroup recomputes the tiny MLP (all 256 threads: four per output of
// the second layer) and then produces its slice of the F stacked FiLM outputs, one or two per thread.  When the whole
// batch shares ONE time value (InDI: one scalar t, indi.py:65; the SR3 / DDPM loops: the same step for every image,
// diffusion.py:153-154) the work is done once and the result written to all B rows of `film`.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_temb(const TembArgs a) {
  extern __shared__ float shf[];
  const int inner = a.inner, hid = 4 * inner;
  float* enc = shf;            // [inner]
  float* h1 = shf + inner;     // [hid]
  float* te = h1 + hid;        // [inner]
  const bool shared_t = gridDim.x == 1 && a.B > 1;     // one time value for every image
  const int b = blockIdx.x;
  float tv;
  if (a.time) tv = a.time[a.n_time == 1 ? 0 : b];
  else tv = a.per_sample ? a.table[(size_t)*a.step_ctr * a.B + b] : a.table[*a.step_ctr];
  const int half = inner / 2;
  for (int i = threadIdx.x; i < inner; i += 256) {
    const int k = i < half ? i : i - half;
    // sr3: gamma * exp(-ln(1e4) * k/half); ddpm: t * inv_freq[k] — both via the freq table
    const float arg = tv * a.freq[k];
    enc[i] = i < half ? sinf(arg) : cosf(arg);
  }
  __syncthreads();
  for (int o = threadIdx.x; o < hid; o += 256) {
    const float* w = a.w1 + (size_t)o * inner;
    float acc = 0.f;
    for (int k = 0; k < inner; k += 4) {                 // inner is a multiple of 4 (dsx_model_create)
      const float4 w4 = *(const float4*)(w + k);
      acc = fmaf(enc[k], w4.x, acc); acc = fmaf(enc[k + 1], w4.y, acc);
      acc = fmaf(enc[k + 2], w4.z, acc); acc = fmaf(enc[k + 3], w4.w, acc);
    }
    acc += a.b1[o];
    h1[o] = acc / (1.0f + expf(-acc));
  }
  __syncthreads();
  {
    // second layer: output o = four adjacent lanes, each over a quarter of the hidden units; fixed order
    const int part = threadIdx.x & 3, q = hid >> 2;      // hid = 4 * inner: whole quarters of whole float4s
    for (int o = threadIdx.x >> 2; o < inner; o += 64) {
      const float* w = a.w2 + (size_t)o * hid + part * q;
      const float* h = h1 + part * q;
      float acc = 0.f;
      for (int k = 0; k < q; k += 4) {
        const float4 w4 = *(const float4*)(w + k);
        acc = fmaf(h[k], w4.x, acc); acc = fmaf(h[k + 1], w4.y, acc);
        acc = fmaf(h[k + 2], w4.z, acc); acc = fmaf(h[k + 3], w4.w, acc);
      }
      acc += __shfl_xor(acc, 1, 64);
      acc += __shfl_xor(acc, 2, 64);
      if (part == 0) {
        acc += a.b2[o];
        te[o] = a.flavour == 1 ? acc / (1.0f + expf(-acc)) : acc;  // ddpm feeds Swish(t) to each block
      }
    }
  }
  __syncthreads();
  const int per = (a.F + gridDim.y - 1) / gridDim.y;
  const int f0 = blockIdx.y * per, f1 = min(a.F, f0 + per);
  for (int f = f0 + threadIdx.x; f < f1; f += 256) {
    const float* w = a.wf + (size_t)f * inner;
    float acc = 0.f;
    for (int k = 0; k < inner; k += 4) {
      const float4 w4 = *(const float4*)(w + k);
      acc = fmaf(te[k], w4.x, acc); acc = fmaf(te[k + 1], w4.y, acc);
      acc = fmaf(te[k + 2], w4.z, acc); acc = fmaf(te[k + 3], w4.w, acc);
    }
    acc += a.bf[f];
    if (shared_t) { for (int bb = 0; bb < a.B; ++bb) a.film[(size_t)bb * a.F + f] = acc; }
    else a.film[(size_t)b * a.F + f] = acc;
  }
}

hipError_t launch_temb(const TembArgs& a, hipStream_t st) {
  const size_t lds = (size_t)(6 * a.inner) * sizeof(float);
  // one time value for the whole batch: computed once (explicit times: n_time == 1; table mode: not per sample)
  const bool shared_t = a.time ? a.n_time == 1 : a.per_sample == 0;
  const int rows = shared_t ? 1 : a.B;
  int splits = (a.F + 255) / 256;                        // about one FiLM output per thread ...
  const int cap = rows >= 8 ? 8 : 64;                    // ... unless the batch already fills the chip
  if (splits > cap) splits = cap;
  if (splits < 1) splits = 1;
  hipLaunchKernelGGL(k_temb, dim3((unsigned)rows, (unsigned)splits), dim3(256), lds, st, a);
  return hipGetLastError();
}

hipError_t ops_init() { return hipSuccess; }   // one-time function attributes (none needed at present)

// split-K epilogue: sum the slices' slabs, then bias + FiLM + residual (deterministic order)
__global__ void k_splitk_reduce(const SplitKReduceArgs a) {
  const long long total = a.M * a.N;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long m = i / a.N;
    const int n = (int)(i - m * a.N);
    float v = 0.f;
    for (int s = 0; s < a.nsplit; ++s) v += a.slab[(size_t)s * a.slab_stride + i];
    if (a.bias) v += a.bias[n];
    if (a.film) v += a.film[(size_t)(m / a.HW) * a.film_bs + n];
    if (a.resid) v += load1_act(a.resid, (size_t)m * a.resid_ld + n, a.act_bf16);
    store1_act(a.out, (size_t)i, v, a.act_bf16);
  }
}
// same, plus the GroupNorm statistics of the tensor it writes: one workgroup per (image, 16-pixel chunk,
// 64 channels), 4 pixel lanes x 4 pixels per channel, fixed reduction order.
// stat_part[b][chunk][n][{sum, sumsq}] with HW/16 chunks per image.
__global__ __launch_bounds__(256) void k_splitk_reduce_stats(const SplitKReduceArgs a) {
  __shared__ float red[2][4][64];
  const int b = blockIdx.x, ch = blockIdx.z, n = blockIdx.y * 64 + (threadIdx.x & 63), pl = threadIdx.x >> 6;
  const float* __restrict__ slab = a.slab;
  const float bi = a.bias ? a.bias[n] : 0.f;
  const float fl = a.film ? a.film[(size_t)b * a.film_bs + n] : 0.f;
  float v[4] = {0.f, 0.f, 0.f, 0.f}, rs[4] = {0.f, 0.f, 0.f, 0.f};
  size_t idx[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const long long m = (long long)b * a.HW + ch * 16 + pl * 4 + k;
    idx[k] = (size_t)m * a.N + n;
    if (a.resid) rs[k] = load1_act(a.resid, (size_t)m * a.resid_ld + n, a.act_bf16);
  }
  for (int s = 0; s < a.nsplit; ++s) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] += slab[(size_t)s * a.slab_stride + idx[k]];
  }
  float s1 = 0.f, s2 = 0.f;
  const float pv = stat_pivot(StatPivot{a.bias, a.film, a.film_bs}, b, n);   // the statistics are shifted by it
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    float x = v[k];
    if (a.bias) x += bi;
    if (a.film) x += fl;
    if (a.resid) x += rs[k];
    store1_act(a.out, idx[k], x, a.act_bf16);
    const float d = x - pv;
    s1 += d; s2 += d * d;
  }
  red[0][pl][threadIdx.x & 63] = s1;
  red[1][pl][threadIdx.x & 63] = s2;
  __syncthreads();
  if (threadIdx.x < 64) {
    const int c = threadIdx.x;
    const float t1 = (red[0][0][c] + red[0][1][c]) + (red[0][2][c] + red[0][3][c]);
    const float t2 = (red[1][0][c] + red[1][1][c]) + (red[1][2][c] + red[1][3][c]);
    float* pp = a.stat_part + (((size_t)b * gridDim.z + ch) * a.N + n) * 2;
    pp[0] = t1; pp[1] = t2;
  }
}
hipError_t launch_splitk_reduce(const SplitKReduceArgs& a, hipStream_t st) {
  if (a.stat_part) {
    if (a.N % 64 != 0 || a.M % a.HW != 0 || a.HW % 16 != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_splitk_reduce_stats, dim3((unsigned)(a.M / a.HW), (unsigned)(a.N / 64), (unsigned)(a.HW / 16)),
                       dim3(256), 0, st, a);
    return hipGetLastError();
  }
  long long g = (a.M * a.N + 255) / 256;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(k_splitk_reduce, dim3((unsigned)g), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// layout conversion at the boundary (the reference passes NCHW)
// ---------------------------------------------------------------------------
__global__ void k_nchw_to_nhwc(const float* __restrict__ src, void* __restrict__ dst, int dst_bf16, int C, int ctot,
                               int coff, int HW, long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const long long p = i / C;
    const long long b = p / HW, hw = p % HW;
    store1_act(dst, (size_t)i, src[(b * ctot + coff + c) * HW + hw], dst_bf16);
  }
}
__global__ void k_nhwc_to_nchw(const float* __restrict__ src, float* __restrict__ dst, int C, int HW,
                               long long total) {
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const long long hw = i % HW;
    const long long p = i / HW;
    const int c = (int)(p % C);
    const long long b = p / C;
    dst[i] = src[(b * HW + hw) * C + c];
  }
}
hipError_t launch_nchw_slice_to_nhwc(const float* src, void* dst, int dst_bf16, int B, int C, int ctot, int coff,
                                     int HW, hipStream_t st) {
  const long long total = (long long)B * C * HW;
  hipLaunchKernelGGL(k_nchw_to_nhwc, dim3(grid_for(total)), dim3(256), 0, st, src, dst, dst_bf16, C, ctot, coff, HW, total);
  return hipGetLastError();
}
hipError_t launch_nhwc_to_nchw(const float* src, float* dst, int B, int C, int H, int W, hipStream_t st) {
  const long long total = (long long)B * C * H * W;
  hipLaunchKernelGGL(k_nhwc_to_nchw, dim3(grid_for(total)), dim3(256), 0, st, src, dst, C, H * W, total);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Philox4x32-10 + Box-Muller (device noise for the perf path; the parity path
// injects host-drawn noise instead, SURVEY §7 "Parity over 2000 steps")
// ---------------------------------------------------------------------------
// (philox4x32_10 and normal4 live in dsx_kernels.h: dsx_steps.hip draws from the same stream)
__global__ void k_randn(float* __restrict__ out, long long n, unsigned long long seed,
                        unsigned long long subseq) {
  const long long n4 = (n + 3) / 4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4;
       i += (long long)gridDim.x * blockDim.x) {
    float z[4];
    normal4(seed, subseq, (unsigned long long)i, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) if (i * 4 + j < n) out[i * 4 + j] = z[j];
  }
}
hipError_t launch_randn(float* out, long long n, unsigned long long seed, unsigned long long subseq,
                        hipStream_t st) {
  hipLaunchKernelGGL(k_randn, dim3(grid_for((n + 3) / 4)), dim3(256), 0, st, out, n, seed, subseq);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Sampler update (sr3 diffusion.py:141-175 / ddpm diffusion.py:194-203 /
// indi.py:62-69): step_update (dsx_kernels.h), the arithmetic k_posterior_step
// shares, so the loop and the single steps round alike.
// The step index lives in device memory so one captured graph replays T times.
// ---------------------------------------------------------------------------
__global__ void k_update(const UpdateArgs a) {
  const int step = *a.step_ctr;
  const int T = a.n_steps;
  float ca = 0.f, cb = 0.f, c1 = 0.f, c2 = 0.f, sg = 0.f;
  if (!a.per_sample) {
    ca = a.tab[1 * T + step]; cb = a.tab[2 * T + step];
    c1 = a.tab[3 * T + step]; c2 = a.tab[4 * T + step]; sg = a.tab[5 * T + step];
  }
  const long long HW = (long long)a.H * a.W;
  const long long n = (long long)a.B * HW * a.C;
  const long long n4 = (n + 3) / 4;
  const unsigned long long seed = a.loop_params[0];
  const float* __restrict__ noise = (const float*)(uintptr_t)a.loop_params[1];
  for (long long i4 = blockIdx.x * (long long)blockDim.x + threadIdx.x; i4 < n4;
       i4 += (long long)gridDim.x * blockDim.x) {
    float z[4] = {0.f, 0.f, 0.f, 0.f};
    if (!a.use_noise && (a.per_sample || sg != 0.f)) normal4(seed, (unsigned long long)step + 1, (unsigned long long)i4, z);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const long long i = i4 * 4 + j;  // NHWC linear index
      if (i >= n) break;
      float zz = z[j];
      if (a.use_noise) {
        const int c = (int)(i % a.C);
        const long long p = i / a.C;
        const long long b = p / HW, hw = p % HW;
        zz = noise[(size_t)step * n + (b * a.C + c) * HW + hw];
      }
      if (a.per_sample) {   // per-sample schedule: the row of this element's image
        const size_t k = (size_t)step * a.B + (size_t)(i / (HW * a.C));
        ca = a.tab[1 * (size_t)T + k]; cb = a.tab[2 * (size_t)T + k];
        c1 = a.tab[3 * (size_t)T + k]; c2 = a.tab[4 * (size_t)T + k]; sg = a.tab[5 * (size_t)T + k];
      }
      const float xn = step_update(ca, cb, c1, c2, sg, a.predict_eps, a.clip, a.x[i], a.net[i], zz, true).out;
      a.x[i] = xn;
      if (a.x_act) store1_act(a.x_act, (size_t)i, xn, a.x_act_kind);
    }
  }
}
hipError_t launch_update(const UpdateArgs& a, hipStream_t st) {
  const long long n4 = ((long long)a.B * a.H * a.W * a.C + 3) / 4;
  hipLaunchKernelGGL(k_update, dim3(grid_for(n4)), dim3(256), 0, st, a);
  return hipGetLastError();
}
__global__ void k_advance(int* ctr) { if (threadIdx.x == 0) *ctr += 1; }
hipError_t launch_advance(int* step_ctr, hipStream_t st) {
  hipLaunchKernelGGL(k_advance, dim3(1), dim3(64), 0, st, step_ctr);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// tiles: gather (N,H,W) frames -> (count, ph, pw); stitch valid regions of
// (count, C, ph, pw) predictions into the (N,H,W,C) canvas (tile_stitcher.py:26-80).
// The tiles of a launch are the arithmetic sequence  id = first + k * stride  (k = blockIdx.y): a rank's
// shard of a plan (or a batch of it) indexes the plan's device tables directly, nothing is uploaded per call.
// ---------------------------------------------------------------------------
__global__ void k_tiles_gather(const float* __restrict__ frames, int H, int W, int ph, int pw,
                               const int* __restrict__ starts, TileSeq seq, float* __restrict__ tiles) {
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int n = starts[t * 3], y0 = starts[t * 3 + 1], x0 = starts[t * 3 + 2];
  const int total = ph * pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / pw, x = i % pw;
    tiles[k * total + i] = frames[((size_t)n * H + (y0 + y)) * W + (x0 + x)];
  }
}
hipError_t launch_tiles_gather(const float* frames, int H, int W, int ph, int pw, const int* starts, TileSeq seq,
                               float* tiles, hipStream_t st) {
  int gx = (ph * pw + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, frames, H, W,
                     ph, pw, starts, seq, tiles);
  return hipGetLastError();
}

// tile crop + the dataset's normalisation in one pass (SplitDataset.__getitem__, data/split_dataset.py:237-278):
//   target_c = (frame_c - mean_target_c) / std_target_c                       (normalize_target, :199-201)
//   input    = w0 * target_0 + w1 * target_1                                   (input_from_normalized_target)
//            | ((w0 * frame_0 + w1 * frame_1) - mean_input) / std_input        (normalize_inp, :195-197)
// in double, rounded to fp32 once, exactly as numpy does with its float64 statistics.
struct GatherNormArgs {
  const float* f0; const float* f1;
  int H, W, ph, pw;
  const int* starts;       // dev [..][3], indexed by tile id
  TileSeq seq;
  float w0, w1;
  double mean_inp, std_inp, mt0, st0, mt1, st1;
  int from_norm_target;
  float* tin;              // (count, 1, ph, pw)
  float* ttar;             // (count, 2, ph, pw)
};
__global__ void k_tiles_gather_norm(const GatherNormArgs a) {
  const long long k = blockIdx.y, t = a.seq.first + k * a.seq.stride;
  const int n = a.starts[t * 3], y0 = a.starts[t * 3 + 1], x0 = a.starts[t * 3 + 2];
  const int total = a.ph * a.pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / a.pw, x = i % a.pw;
    const size_t src = ((size_t)n * a.H + (y0 + y)) * a.W + (x0 + x);
    const float p0 = a.f0[src], p1 = a.f1[src];
    const float t0 = (float)(((double)p0 - a.mt0) / a.st0), t1 = (float)(((double)p1 - a.mt1) / a.st1);
    float in;
    if (a.from_norm_target) in = __fadd_rn(__fmul_rn(a.w0, t0), __fmul_rn(a.w1, t1));
    else in = (float)(((double)__fadd_rn(__fmul_rn(a.w0, p0), __fmul_rn(a.w1, p1)) - a.mean_inp) / a.std_inp);
    a.tin[k * total + i] = in;
    a.ttar[(k * 2) * total + i] = t0;
    a.ttar[(k * 2 + 1) * total + i] = t1;
  }
}
hipError_t launch_tiles_gather_norm(const float* f0, const float* f1, int H, int W, int ph, int pw, const int* starts,
                                    TileSeq seq, float w0, float w1, const double norm[6], int from_norm_target,
                                    float* tin, float* ttar, hipStream_t st) {
  GatherNormArgs a{f0, f1, H, W, ph, pw, starts, seq, w0, w1, norm[0], norm[1], norm[2], norm[3], norm[4], norm[5],
                   from_norm_target, tin, ttar};
  int gx = (ph * pw + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather_norm, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, a);
  return hipGetLastError();
}

// (mul_f / add_f / mul_d / add_d, one IEEE operation each, live in dsx_kernels.h)
// The mixed inputs of the TimePredictor evaluation (notebooks/EvaluateJointIndiIterative.ipynb cells 40/43,
// time_prediction_evaluation.ipynb cell 4) cut, normalised, mixed and min-max-normalised in one pass; the op list is
// in include/dsx.h (dsx_tiles_gather_mix).  Channel 0 is indi1's input, channel 1 indi2's.
struct GatherMixArgs {
  const float* f0; const float* f1;
  int H, W, ph, pw;
  const int* starts;       // dev [..][3], indexed by tile id
  TileSeq seq;
  double mt0, st0, mt1, st1;
  MixWeights mw;
  float* ttar; float* tmix; float* tcls;   // (count, 2, ph, pw) each, or nullptr
};
__global__ void k_tiles_gather_mix(const GatherMixArgs a) {
  const long long k = blockIdx.y, t = a.seq.first + k * a.seq.stride;
  const int n = a.starts[t * 3], y0 = a.starts[t * 3 + 1], x0 = a.starts[t * 3 + 2];
  const int total = a.ph * a.pw;
  const MixWeights w = a.mw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / a.pw, x = i % a.pw;
    const size_t src = ((size_t)n * a.H + (y0 + y)) * a.W + (x0 + x);
    const float t0 = (float)(((double)a.f0[src] - a.mt0) / a.st0), t1 = (float)(((double)a.f1[src] - a.mt1) / a.st1);
    const size_t d0 = (size_t)(k * 2) * total + i, d1 = d0 + total;
    if (a.ttar) { a.ttar[d0] = t0; a.ttar[d1] = t1; }
    if (a.tmix || a.tcls) {
      const float m0 = add_f(mul_f(t0, w.w0), mul_f(t1, w.w1));
      const float m1 = add_f(mul_f(t1, w.w0), mul_f(t0, w.w1));
      if (a.tmix) { a.tmix[d0] = m0; a.tmix[d1] = m1; }
      if (a.tcls) {
        a.tcls[d0] = add_f(mul_f(2.0f, add_f(m0, -w.lo0)) / w.rng0, -1.0f);
        a.tcls[d1] = add_f(mul_f(2.0f, add_f(m1, -w.lo1)) / w.rng1, -1.0f);
      }
    }
  }
}
hipError_t launch_tiles_gather_mix(const float* f0, const float* f1, int H, int W, int ph, int pw, const int* starts,
                                   TileSeq seq, const double norm[4], const MixWeights& mw, float* ttar, float* tmix,
                                   float* tcls, hipStream_t st) {
  GatherMixArgs a{f0, f1, H, W, ph, pw, starts, seq, norm[0], norm[1], norm[2], norm[3], mw, ttar, tmix, tcls};
  int gx = (ph * pw + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather_mix, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, a);
  return hipGetLastError();
}

// The TimePredictor's input range table (compute_input_normalization_dict, data/time_predictor_dataset.py:6-21): for
// every t_int in 0..n the min and max over all pixels of  t * a + (1 - t) * b,  t = t_int / n,  a, b = the normalised
// channels -- n + 1 numpy passes over the frame set in the reference, one launch here.  All of it in fp64 with every
// operation rounded on its own (numpy has no fma), so the table is bitwise numpy's; min / max are exact, the result
// does not depend on the reduction tree.  fp64-VALU-bound, not HBM-bound: a thread keeps the running min / max of
// kMixTB values of t in registers (and their weights) while it strides over its workgroup's pixel chunk; the t blocks
// are blockIdx.x, so the workgroups that re-read a chunk are dispatched together and find it in L2 / MALL.  Wave
// reduction by shuffles, the four waves through LDS, one partial row per workgroup: part[chunk][t_int][{min, max}].
constexpr int kMixTB = 8;
constexpr int kMixMaxChunks = 512;
__global__ __launch_bounds__(256) void k_mix_range(const float* __restrict__ f0, const float* __restrict__ f1,
                                                   long long pixels, long long chunk, double m0, double s0, double m1,
                                                   double s1, int n, double* __restrict__ part) {
  __shared__ double red[4][kMixTB][2];
  const int tb = blockIdx.x * kMixTB;
  double tw[kMixTB], uw[kMixTB], mn[kMixTB], mx[kMixTB];
#pragma unroll
  for (int j = 0; j < kMixTB; ++j) {
    const int ti = min(tb + j, n);             // the rows past n of the last block repeat row n and are not written
    tw[j] = (double)ti / (double)n;            // IEEE division, as numpy's t_int / n_timesteps
    uw[j] = 1.0 - tw[j];
    mn[j] = INFINITY; mx[j] = -INFINITY;
  }
  const long long p0 = blockIdx.y * chunk, p1 = min(pixels, p0 + chunk);
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
    const double a = ((double)f0[p] - m0) / s0, b = ((double)f1[p] - m1) / s1;
#pragma unroll
    for (int j = 0; j < kMixTB; ++j) {
      const double v = add_d(mul_d(tw[j], a), mul_d(uw[j], b));
      mn[j] = fmin(mn[j], v); mx[j] = fmax(mx[j], v);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int j = 0; j < kMixTB; ++j) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn[j] = fmin(mn[j], __shfl_xor(mn[j], o, 64)); mx[j] = fmax(mx[j], __shfl_xor(mx[j], o, 64)); }
    if (lane == 0) { red[wave][j][0] = mn[j]; red[wave][j][1] = mx[j]; }
  }
  __syncthreads();
  if (threadIdx.x < kMixTB * 2) {
    const int j = threadIdx.x >> 1, kk = threadIdx.x & 1;
    if (tb + j <= n) {
      const double r0 = red[0][j][kk], r1 = red[1][j][kk], r2 = red[2][j][kk], r3 = red[3][j][kk];
      part[((size_t)blockIdx.y * (n + 1) + (tb + j)) * 2 + kk] =
          kk ? fmax(fmax(r0, r1), fmax(r2, r3)) : fmin(fmin(r0, r1), fmin(r2, r3));
    }
  }
}
// pixel workgroups (= rows of partials) of a call: about a thousand pixels per workgroup at least, 512 chunks at most
int mix_range_blocks(long long pixels) {
  const long long g = (pixels + 1023) / 1024;
  return (int)(g > kMixMaxChunks ? kMixMaxChunks : (g < 1 ? 1 : g));
}
hipError_t launch_mix_range(const float* f0, const float* f1, long long pixels, const double norm[4], int n, double* part,
                            hipStream_t st) {
  const int gy = mix_range_blocks(pixels);
  const long long chunk = (pixels + gy - 1) / gy;
  hipLaunchKernelGGL(k_mix_range, dim3((unsigned)((n + kMixTB) / kMixTB), (unsigned)gy), dim3(256), 0, st, f0, f1, pixels,
                     chunk, norm[0], norm[1], norm[2], norm[3], n, part);
  return hipGetLastError();
}

// Where the pixels of tile `t` (the k-th of the launch) come from: whole predicted tiles (count, C, ph, pw), or the
// packed exchange buffer of tiled multi-GPU prediction -- per rank one flat run of valid regions [C][h][w], tile after
// tile in id order (rank q owns the ids q, q + world, ...); `off` = pixel offset of every tile inside its rank's run.
struct TileSrc {
  const float* base;       // tiles, or the gathered flat buffer [world][rank_stride]
  int packed;              // 0: whole tiles, 1: packed valid regions
  int ph, pw;              // whole tiles
  const long long* off;    // packed: dev [total] pixel offsets
  long long rank_stride;   // packed: elements between two ranks' runs
  int world;
};
struct TileView { const float* p; int pitch; long long plane; };
__device__ __forceinline__ TileView tile_view(const TileSrc& s, long long k, long long t, int C, const int* r) {
  TileView v;
  if (s.packed) {
    v.p = s.base + (t % s.world) * s.rank_stride + s.off[t] * C;
    v.pitch = r[4]; v.plane = (long long)r[3] * r[4];
  } else {
    v.p = s.base + (size_t)k * C * s.ph * s.pw + (size_t)r[5] * s.pw + r[6];
    v.pitch = s.pw; v.plane = (long long)s.ph * s.pw;
  }
  return v;
}

__global__ void k_stitch(const TileSrc src, int C, const int* __restrict__ regions, TileSeq seq,
                         float* __restrict__ canvas, int H, int W) {
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int* r = regions + t * 8;
  const int n = r[0], y0 = r[1], x0 = r[2], h = r[3], w = r[4];
  const int total = h * w * C;
  const TileView v = tile_view(src, k, t, C, r);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i % C;
    const int p = i / C;
    const int x = p % w, y = p / w;
    canvas[(((size_t)n * H + (y0 + y)) * W + (x0 + x)) * C + c] = v.p[c * v.plane + (size_t)y * v.pitch + x];
  }
}

// The valid region of every tile of the sequence, [C][h][w], to its place in this rank's flat run: the crop of
// tile_stitcher.py:38-56 applied BEFORE the collective (a 512^2 tile of a 256 grid ships 256^2 .. 384^2 pixels).
__global__ void k_tiles_pack(const float* __restrict__ tiles, int C, int ph, int pw, const int* __restrict__ regions,
                             const long long* __restrict__ off, TileSeq seq, float* __restrict__ flat) {
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int* r = regions + t * 8;
  const int h = r[3], w = r[4], ry = r[5], rx = r[6];
  const int total = C * h * w;
  const float* tile = tiles + (size_t)k * C * ph * pw;
  float* dst = flat + off[t] * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int x = i % w, q = i / w, y = q % h, c = q / h;
    dst[i] = tile[((size_t)c * ph + (ry + y)) * pw + (rx + x)];
  }
}
hipError_t launch_tiles_pack(const float* tiles, int C, int ph, int pw, const int* regions, const long long* off,
                             TileSeq seq, float* flat, hipStream_t st) {
  int gx = (ph * pw * C + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_pack, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, tiles, C, ph, pw, regions,
                     off, seq, flat);
  return hipGetLastError();
}

// Stitch + the sums RangeInvariantPsnr needs (core/psnr.py:70-82), in the same pass: while a tile's valid region
// is pasted, every (tile, workgroup) also reduces, per channel, sum(p), sum(p^2), sum(g), sum(g^2), sum(g p),
// min(g), max(g) of prediction p against the ground truth g at the same canvas pixels (every canvas pixel is pasted
// exactly once).  Fixed reduction order (thread -> wave shuffles -> 4 waves): bitwise reproducible.
// part[k][blockIdx.x][c][8] doubles; the per-frame combination (a few hundred values) is the caller's.
constexpr int kPsnrMaxC = 4;
__global__ __launch_bounds__(256) void k_stitch_psnr(const TileSrc src, int C, const int* __restrict__ regions, TileSeq seq,
                                                      float* __restrict__ canvas, const float* __restrict__ gt, int H, int W,
                                                      double* __restrict__ part) {
  __shared__ double red[4][kPsnrMaxC][7];
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int* r = regions + t * 8;
  const int n = r[0], y0 = r[1], x0 = r[2], h = r[3], w = r[4];
  const TileView v = tile_view(src, k, t, C, r);
  double sp[kPsnrMaxC], spp[kPsnrMaxC], sg[kPsnrMaxC], sgg[kPsnrMaxC], sgp[kPsnrMaxC], mn[kPsnrMaxC], mx[kPsnrMaxC];
#pragma unroll
  for (int c = 0; c < kPsnrMaxC; ++c) { sp[c] = spp[c] = sg[c] = sgg[c] = sgp[c] = 0; mn[c] = INFINITY; mx[c] = -INFINITY; }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < h * w; i += gridDim.x * blockDim.x) {
    const int x = i % w, y = i / w;
    const size_t cpix = (((size_t)n * H + (y0 + y)) * W + (x0 + x)) * C;
#pragma unroll
    for (int c = 0; c < kPsnrMaxC; ++c) {
      if (c < C) {
        const float p = v.p[c * v.plane + (size_t)y * v.pitch + x];
        const float g = gt[cpix + c];
        canvas[cpix + c] = p;
        sp[c] += p; spp[c] += (double)p * p; sg[c] += g; sgg[c] += (double)g * g; sgp[c] += (double)g * p;
        mn[c] = fmin(mn[c], (double)g); mx[c] = fmax(mx[c], (double)g);
      }
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int c = 0; c < kPsnrMaxC; ++c) {
    sp[c] = wave_sum(sp[c]); spp[c] = wave_sum(spp[c]); sg[c] = wave_sum(sg[c]); sgg[c] = wave_sum(sgg[c]);
    sgp[c] = wave_sum(sgp[c]);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { mn[c] = fmin(mn[c], __shfl_xor(mn[c], o, 64)); mx[c] = fmax(mx[c], __shfl_xor(mx[c], o, 64)); }
    if (lane == 0) {
      red[wave][c][0] = sp[c]; red[wave][c][1] = spp[c]; red[wave][c][2] = sg[c]; red[wave][c][3] = sgg[c];
      red[wave][c][4] = sgp[c]; red[wave][c][5] = mn[c]; red[wave][c][6] = mx[c];
    }
  }
  __syncthreads();
  if (threadIdx.x < C * 8) {
    const int c = threadIdx.x >> 3, kk = threadIdx.x & 7;
    double o = 0;
    if (kk < 5) o = (red[0][c][kk] + red[1][c][kk]) + (red[2][c][kk] + red[3][c][kk]);
    else if (kk == 5) o = fmin(fmin(red[0][c][5], red[1][c][5]), fmin(red[2][c][5], red[3][c][5]));
    else if (kk == 6) o = fmax(fmax(red[0][c][6], red[1][c][6]), fmax(red[2][c][6], red[3][c][6]));
    part[(((size_t)k * gridDim.x + blockIdx.x) * C + c) * 8 + kk] = o;
  }
}
// gt == nullptr: plain paste; else also the RangeInvariantPsnr partial sums (C <= 4, gx workgroups per tile)
hipError_t launch_stitch(const StitchSrc& s, int C, const int* regions, TileSeq seq, float* canvas, int H, int W,
                         const float* gt, double* part, int gx, hipStream_t st) {
  const TileSrc src{s.base, s.packed, s.ph, s.pw, s.off, s.rank_stride, s.world < 1 ? 1 : s.world};
  if (gt != nullptr) {
    if (C < 1 || C > kPsnrMaxC || gx < 1 || part == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stitch_psnr, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, src, C, regions, seq,
                       canvas, gt, H, W, part);
  } else {
    int g = (s.ph * s.pw * C + 255) / 256;
    if (g > 64) g = 64;
    hipLaunchKernelGGL(k_stitch, dim3((unsigned)g, (unsigned)seq.count), dim3(256), 0, st, src, C, regions, seq, canvas,
                       H, W);
  }
  return hipGetLastError();
}

// SSIM (core/metrics.py:72-92) + sum of squared differences (calculate_psnr, :62-69) of image pairs in one pass.
// One workgroup per (32 x 32 tile of the valid region [5:-5, 5:-5], image plane): the 42 x 42 input tile (10-pixel
// halo, re-read by the neighbours through L2) is staged in LDS, quantised on the load when asked (tensor2img,
// :14-34: clamp, (x - lo) / (hi - lo) with IEEE division, * 255, round half to even); then the 11-tap Gaussian is
// applied horizontally to the five moments x, y, x^2, y^2, x y of all 42 rows (fp64, to LDS) and vertically to the
// 32 output rows.  Each plane's pixels are partitioned among its tiles (edge tiles also own the 5-pixel border) for
// the SSD: exact uint64 of integers when quantised, fp64 otherwise.  Fixed reduction order (thread -> wave shuffles
// -> 4 waves), no atomics: part[plane][tile] = {sum of the SSIM map over the tile, SSD}, bitwise reproducible.
constexpr int kSsimT = 32, kSsimIn = kSsimT + 10;
__device__ __forceinline__ float metrics_load(const float* p, bool quantize, float lo, float hi, float rng) {
  float x = *p;
  if (quantize) x = rintf((fminf(fmaxf(x, lo), hi) - lo) / rng * 255.0f);
  return x;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__global__ __launch_bounds__(256) void k_image_metrics(const float* __restrict__ a, const float* __restrict__ b, int H,
                                                       int W, int quantize, float lo, float hi, float rng, double c1,
                                                       double c2, SsimWindow win, int tiles_x, double* __restrict__ part) {
  __shared__ float sa[kSsimIn][kSsimIn], sb[kSsimIn][kSsimIn];
  __shared__ double hm[5][kSsimIn][kSsimT];
  __shared__ double red[4];
  __shared__ unsigned long long redq[4];
  const int tile = blockIdx.x, plane = blockIdx.y;
  const int y0 = (tile / tiles_x) * kSsimT, x0 = (tile % tiles_x) * kSsimT;    // output tile = input rows/cols + 5
  const int ty_last = (H - 10 + kSsimT - 1) / kSsimT - 1, tx_last = tiles_x - 1;
  // pixels of this tile's SSD share: its output rows/cols, widened to the image edge on the edge tiles
  const int oy0 = y0 == 0 ? 0 : y0 + 5, oy1 = y0 / kSsimT == ty_last ? H : y0 + 5 + kSsimT;
  const int ox0 = x0 == 0 ? 0 : x0 + 5, ox1 = x0 / kSsimT == tx_last ? W : x0 + 5 + kSsimT;
  const size_t pl = (size_t)plane * H * W;
  const bool q = quantize != 0;
  double ssd = 0;
  unsigned long long ssdq = 0;
  for (int i = threadIdx.x; i < kSsimIn * kSsimIn; i += 256) {
    const int r = i / kSsimIn, c = i % kSsimIn, y = y0 + r, x = x0 + c;
    float va = 0.f, vb = 0.f;
    if (y < H && x < W) {
      va = metrics_load(a + pl + (size_t)y * W + x, q, lo, hi, rng);
      vb = metrics_load(b + pl + (size_t)y * W + x, q, lo, hi, rng);
      if (y >= oy0 && y < oy1 && x >= ox0 && x < ox1) {
        if (q) { const int d = (int)va - (int)vb; ssdq += (unsigned long long)(d * d); }
        else { const double d = (double)va - (double)vb; ssd += d * d; }
      }
    }
    sa[r][c] = va; sb[r][c] = vb;
  }
  __syncthreads();
  const int col = threadIdx.x & (kSsimT - 1), r8 = threadIdx.x / kSsimT;
  for (int r = r8; r < kSsimIn; r += 256 / kSsimT) {
    double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double u = sa[r][col + k], v = sb[r][col + k], w = win.w[k];
      m0 += w * u; m1 += w * v; m2 += w * (u * u); m3 += w * (v * v); m4 += w * (u * v);
    }
    hm[0][r][col] = m0; hm[1][r][col] = m1; hm[2][r][col] = m2; hm[3][r][col] = m3; hm[4][r][col] = m4;
  }
  __syncthreads();
  // vertical: 4 consecutive output rows per thread share their 14 rows of horizontal sums (taps in ascending order)
  constexpr int kRows = kSsimT / (256 / kSsimT);
  const int rv = r8 * kRows;
  double acc = 0;
  if (x0 + col < W - 10) {
    double mu1[kRows] = {}, mu2[kRows] = {}, e11[kRows] = {}, e22[kRows] = {}, e12[kRows] = {};
#pragma unroll
    for (int k = 0; k < kRows + 10; ++k) {
      const double h0 = hm[0][rv + k][col], h1 = hm[1][rv + k][col], h2 = hm[2][rv + k][col],
                   h3 = hm[3][rv + k][col], h4 = hm[4][rv + k][col];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (k - j >= 0 && k - j < 11) {
          const double w = win.w[k - j];
          mu1[j] += w * h0; mu2[j] += w * h1; e11[j] += w * h2; e22[j] += w * h3; e12[j] += w * h4;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (y0 + rv + j < H - 10) {
        const double mu11 = mu1[j] * mu1[j], mu22 = mu2[j] * mu2[j], mu12 = mu1[j] * mu2[j];
        const double s11 = e11[j] - mu11, s22 = e22[j] - mu22, s12 = e12[j] - mu12;
        acc += ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu11 + mu22 + c1) * (s11 + s22 + c2));
      }
    }
  }
  acc = wave_sum(acc); ssd = wave_sum(ssd); ssdq = wave_sum_u64(ssdq);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[wave] = acc; redq[wave] = q ? ssdq : (unsigned long long)__double_as_longlong(ssd); }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)plane * gridDim.x + tile) * 2;
    o[0] = (red[0] + red[1]) + (red[2] + red[3]);
    if (q) {
      o[1] = __longlong_as_double((long long)((redq[0] + redq[1]) + (redq[2] + redq[3])));
    } else {
      double s[4];
      for (int w = 0; w < 4; ++w) s[w] = __longlong_as_double((long long)redq[w]);
      o[1] = (s[0] + s[1]) + (s[2] + s[3]);
    }
  }
}
int image_metrics_tiles(int H, int W) {
  return ((H - 10 + kSsimT - 1) / kSsimT) * ((W - 10 + kSsimT - 1) / kSsimT);
}
hipError_t launch_image_metrics(const float* a, const float* b, int planes, int H, int W, int quantize, float lo,
                                float hi, float rng, double c1, double c2, const SsimWindow& win, double* part,
                                hipStream_t st) {
  if (H < 11 || W < 11 || planes < 1 || planes > 65535) return hipErrorInvalidValue;
  const int tiles_x = (W - 10 + kSsimT - 1) / kSsimT;
  hipLaunchKernelGGL(k_image_metrics, dim3((unsigned)image_metrics_tiles(H, W), (unsigned)planes), dim3(256), 0, st,
                     a, b, H, W, quantize, lo, hi, rng, c1, c2, win, tiles_x, part);
  return hipGetLastError();
}

// TimePredictor head (time_predictor.py:38-44): sum(relu(u)*mask) / sum(mask) per image
__global__ __launch_bounds__(256) void k_masked_mean(const float* __restrict__ u,
                                                     const float* __restrict__ mask, long long n,
                                                     float* __restrict__ out) {
  __shared__ double red[8];
  const int b = blockIdx.x;
  double num = 0, den = 0;
  for (long long i = threadIdx.x; i < n; i += 256) {
    const float m = mask[(size_t)b * n + i];
    num += (double)(fmaxf(u[(size_t)b * n + i], 0.f) * m);
    den += (double)m;
  }
  num = wave_sum(num); den = wave_sum(den);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave * 2] = num; red[wave * 2 + 1] = den; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0, d = 0;
    for (int w = 0; w < 4; ++w) { a += red[w * 2]; d += red[w * 2 + 1]; }
    out[b] = (float)(a / d);
  }
}
hipError_t launch_masked_mean(const float* u, const float* mask, int B, long long n, float* out,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_masked_mean, dim3((unsigned)B), dim3(256), 0, st, u, mask, n, out);
  return hipGetLastError();
}

}  // namespace dsx
