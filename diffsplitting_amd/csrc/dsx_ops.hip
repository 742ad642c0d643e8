// dsx_ops.hip — the non-conv kernels of the sampling path (gfx950):
// GroupNorm statistics (wavefront-shuffle reductions), time embedding + FiLM,
// Philox noise, layout conversion, the TimePredictor head.  (The sampler update: dsx_steps.hip.)
// (Attention: dsx_attn.hip.  Tiles, stitch and the metrics: dsx_eval.hip.)
#include "dsx_kernels.h"
#include "dsx_reduce.h"
#include <algorithm>

namespace dsx {

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
  if (gn_finalize_is_wide(a))
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
// Per-sample noise streams (include/dsx.h): row blockIdx.y of out (rows, chw) = the first chw elements of the stream
// (seed, s.subseq[row]), i.e. what k_randn writes for that subsequence.  VEC: chw is a multiple of 4 and out is 16-byte
// aligned, so every Philox block of every row is one 16-byte store; otherwise scalar stores, the last block cut at chw.
template <bool VEC>
__global__ __launch_bounds__(256) void k_randn_samples(float* __restrict__ out, long long chw, unsigned long long seed,
                                                       const StreamIds s) {
  const unsigned long long subseq = s.subseq[blockIdx.y];
  float* __restrict__ row = out + (size_t)blockIdx.y * chw;
  const long long n4 = (chw + 3) / 4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n4;
       i += (long long)gridDim.x * blockDim.x) {
    float z[4];
    normal4(seed, subseq, (unsigned long long)i, z);
    if (VEC) {
      *(float4*)(row + i * 4) = make_float4(z[0], z[1], z[2], z[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) if (i * 4 + j < chw) row[i * 4 + j] = z[j];
    }
  }
}
hipError_t launch_randn_samples(float* out, int rows, long long chw, unsigned long long seed, const StreamIds& s,
                                hipStream_t st) {
  if (rows < 1 || rows > kStreamRows) return hipErrorInvalidValue;
  const bool vec = chw % 4 == 0 && aligned16(out);
  hipLaunchKernelGGL(vec ? k_randn_samples<true> : k_randn_samples<false>, dim3(grid_for((chw + 3) / 4), (unsigned)rows),
                     dim3(256), 0, st, out, chw, seed, s);
  return hipGetLastError();
}

// TimePredictor head (time_predictor.py:38-44): sum(relu(u)*mask) / sum(mask) per image
__global__ __launch_bounds__(256) void k_masked_mean(const float* __restrict__ u,
                                                     const float* __restrict__ mask, long long n,
                                                     float* __restrict__ out) {
  __shared__ double red[4 * 2];
  const int b = blockIdx.x;
  double num = 0, den = 0;
  for (long long i = threadIdx.x; i < n; i += 256) {
    const float m = mask[(size_t)b * n + i];
    num += (double)(fmaxf(u[(size_t)b * n + i], 0.f) * m);
    den += (double)m;
  }
  block_park<RedSum>(num, red, 2, 0);
  block_park<RedSum>(den, red, 2, 1);
  __syncthreads();
  if (threadIdx.x == 0) out[b] = (float)(block_combine<RedSum, Serial>(red, 2, 0) / block_combine<RedSum, Serial>(red, 2, 1));
}
hipError_t launch_masked_mean(const float* u, const float* mask, int B, long long n, float* out,
                              hipStream_t st) {
  hipLaunchKernelGGL(k_masked_mean, dim3((unsigned)B), dim3(256), 0, st, u, mask, n, out);
  return hipGetLastError();
}

}  // namespace dsx
