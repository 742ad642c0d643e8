// dsx_lpips.hip — LPIPS (AlexNet trunk, v0.1 linear heads, spatial off) on gfx950, fp32 end to end.
//
// The metric of notebooks/EvaluateJointIndi.ipynb cell 31 / EvaluateJointIndiIterative.ipynb cell 28.  A metric must
// not depend on a bf16 rounding choice, so every contraction runs on the exact-fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: a k-ordered fmaf chain); activations are NHWC fp32 and both images of a pair travel as one
// batch of 2 B images (image b and image B + b), so the weights are streamed once.
//
//   k_lpips_input_*   NCHW pair, or one channel of two channel-last frame stacks (cell 28's min-max map, replicated
//                     to three channels) -> scaling layer -> (2B, H, W, 3)
//   k_lpips_conv1     3 -> 64, 11 x 11, stride 4, pad 2: the receptive field is ONE K dimension (363, padded to 368)
//                     gathered from the LDS patch through a per-lane offset table, as k_conv_first does
//   k_lpips_conv<KS>  conv2 .. conv5: implicit GEMM, 16 x 16 output pixels x 64 channels per workgroup, the halo patch
//                     of 32 input channels in LDS per K chunk, weights in MFMA fragment order straight from L2
//   k_lpips_pool      3 x 3 / stride 2 max-pool, floor mode (a kernel of its own: see DESIGN.md)
//   k_lpips_dist      per tap: unit-normalise, lin-weighted squared difference, fixed-order partial sums in double
//   k_lpips_finish    adds the partial rows in order: bitwise repeatable, no atomics
//
// MFMA operands: A = weights (row = output channel, rows permuted so that a lane ends up with 16 consecutive
// channels), B = pixels (column = pixel); D: column = lane & 31 (pixel), row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// A lane reads 4 consecutive channels (16 B) of its pixel and uses component s in k step s, so the k order inside a
// group of 8 channels is {0, 4}, {1, 5}, {2, 6}, {3, 7}; the host packs the weights to match (dsx_lpips.cpp).
// Output sizes are odd (511, 255, 127 for a 2048 input): every tile masks its loads and stores, nothing is padded.
#include <hip/hip_runtime.h>

#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

typedef float f32x16_l __attribute__((ext_vector_type(16)));

namespace {

__device__ __forceinline__ void zero_acc(f32x16_l (&acc)[2][2]) {
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;
}

// one group of 8 k values: 4 MFMA steps for the 2 x 2 blocks of a wave
__device__ __forceinline__ void mfma_group(f32x16_l (&acc)[2][2], const float4& w0, const float4& w1, const float4& p0,
                                           const float4& p1) {
#define DSX_LP_STEP(c)                                                                      \
  acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0.c, p0.c, acc[0][0], 0, 0, 0);         \
  acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1.c, p0.c, acc[0][1], 0, 0, 0);         \
  acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0.c, p1.c, acc[1][0], 0, 0, 0);         \
  acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1.c, p1.c, acc[1][1], 0, 0, 0);
  DSX_LP_STEP(x) DSX_LP_STEP(y) DSX_LP_STEP(z) DSX_LP_STEP(w)
#undef DSX_LP_STEP
}

// + bias, ReLU, 16 consecutive channels of one pixel per lane
__device__ __forceinline__ void store_relu(const f32x16_l& acc, const float* __restrict__ bias, float* __restrict__ dst) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 bv = *(const float4*)(bias + 4 * j);
    float4 o;
    o.x = fmaxf(acc[4 * j] + bv.x, 0.f);
    o.y = fmaxf(acc[4 * j + 1] + bv.y, 0.f);
    o.z = fmaxf(acc[4 * j + 2] + bv.z, 0.f);
    o.w = fmaxf(acc[4 * j + 3] + bv.w, 0.f);
    *(float4*)(dst + 4 * j) = o;
  }
}

// ------------------------------------------------------------------ input
// ScalingLayer: (x - shift) / scale, IEEE division (not folded into conv1: conv1 zero-pads AFTER the scaling)
__device__ __forceinline__ float lp_shift(int c) { return c == 0 ? -.030f : (c == 1 ? -.088f : -.188f); }
__device__ __forceinline__ float lp_scale(int c) { return c == 0 ? .458f : (c == 1 ? .448f : .450f); }

__global__ __launch_bounds__(256) void k_lpips_input_nchw(const float* __restrict__ in0, const float* __restrict__ in1,
                                                          int B, long long HW, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2ll * B * HW) return;
  const int img = (int)(idx / HW);
  const long long p = idx - (long long)img * HW;
  const float* src = img < B ? in0 + (size_t)img * 3 * HW : in1 + (size_t)(img - B) * 3 * HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(size_t)idx * 3 + c] = __fdiv_rn(__fsub_rn(src[(size_t)c * HW + p], lp_shift(c)), lp_scale(c));
}

// cell 28: channel `ch` of frames f0 .. f0 + n of target and prediction (N, H, W, C), 2 (x - min) / (max - min) - 1 with
// the target channel's range (mm = {min, max}), every fp32 operation rounded on its own, three equal channels
__global__ __launch_bounds__(256) void k_lpips_input_frames(const float* __restrict__ tgt, const float* __restrict__ prd,
                                                            int n, long long HW, int C, int ch,
                                                            const float* __restrict__ mm, float* __restrict__ out) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= 2ll * n * HW) return;
  const int img = (int)(idx / HW);
  const long long p = idx - (long long)img * HW;
  const float* src = img < n ? tgt + ((size_t)img * HW + p) * C + ch : prd + ((size_t)(img - n) * HW + p) * C + ch;
  const float lo = mm[0], rng = __fsub_rn(mm[1], mm[0]);
  const float v = __fsub_rn(__fdiv_rn(__fmul_rn(2.f, __fsub_rn(*src, lo)), rng), 1.f);
#pragma unroll
  for (int c = 0; c < 3; ++c) out[(size_t)idx * 3 + c] = __fdiv_rn(__fsub_rn(v, lp_shift(c)), lp_scale(c));
}

// min / max of one channel of a channel-last stack (order-independent, so repeatable); part[blocks][2]
__global__ __launch_bounds__(256) void k_lpips_minmax(const float* __restrict__ x, long long pixels, int C, int ch,
                                                      float* __restrict__ part) {
  __shared__ float red[4 * 2];
  float lo = INFINITY, hi = -INFINITY;
  for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < pixels; p += (long long)gridDim.x * 256) {
    const float v = x[(size_t)p * C + ch];
    lo = fminf(lo, v);
    hi = fmaxf(hi, v);
  }
  block_park<RedMin>(lo, red, 2, 0);
  block_park<RedMax>(hi, red, 2, 1);
  __syncthreads();
  if (threadIdx.x < 2)
    part[2 * blockIdx.x + threadIdx.x] = threadIdx.x ? block_combine<RedMax, Pairwise>(red, 2, 1)
                                                     : block_combine<RedMin, Pairwise>(red, 2, 0);
}
__global__ __launch_bounds__(64) void k_lpips_minmax_fin(const float* __restrict__ part, int blocks, float* __restrict__ mm) {
  if (threadIdx.x != 0) return;
  float lo = INFINITY, hi = -INFINITY;
  for (int i = 0; i < blocks; ++i) { lo = fminf(lo, part[2 * i]); hi = fmaxf(hi, part[2 * i + 1]); }
  mm[0] = lo; mm[1] = hi;
}

// ------------------------------------------------------------------ conv1
constexpr int C1_PS = 71;                  // input rows / columns under 16 outputs: 15 * 4 + 11
constexpr int C1_ROW = C1_PS * 3;          // floats per patch row
constexpr int C1_GROUPS = 46;              // 363 -> 368 = 46 groups of 8 k

__global__ __launch_bounds__(256) void k_lpips_conv1(const float* __restrict__ in, const float* __restrict__ wpack,
                                                     const float* __restrict__ bias, float* __restrict__ out, int H, int W,
                                                     int Ho, int Wo) {
  __shared__ __attribute__((aligned(16))) float patch[C1_PS * C1_ROW];
  __shared__ __attribute__((aligned(16))) int kofft[C1_GROUPS * 8];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int tiles_x = (Wo + 15) >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy0 = ty * 16, ox0 = tx * 16, img = blockIdx.z;
  const int iy0 = oy0 * 4 - 2, ix0 = ox0 * 4 - 2;
  const float* src = in + (size_t)img * H * W * 3;

  for (int e = tid; e < C1_PS * C1_ROW; e += 256) {
    const int py = e / C1_ROW, rem = e - py * C1_ROW, px = rem / 3, c = rem - px * 3;
    const int iy = iy0 + py, ix = ix0 + px;
    float v = 0.f;
    if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = src[((size_t)iy * W + ix) * 3 + c];
    patch[e] = v;
  }
  // k = (ky * 11 + kx) * 3 + c = ky * 33 + (kx * 3 + c) -> patch offset ky * row + (kx * 3 + c); padded k: weight 0
  for (int k = tid; k < C1_GROUPS * 8; k += 256) kofft[k] = k < 363 ? (k / 33) * C1_ROW + (k % 33) : 0;
  __syncthreads();

  f32x16_l acc[2][2];
  zero_acc(acc);
  int base[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int m = (wave * 2 + mb) * 32 + li;
    base[mb] = (m >> 4) * 4 * C1_ROW + (m & 15) * 12;
  }
  const float4* wq = (const float4*)wpack + lane;
  for (int g = 0; g < C1_GROUPS; ++g) {
    const int4 ko = *(const int4*)&kofft[8 * g + 4 * lh];
    const float4 w0 = wq[(size_t)g * 64], w1 = wq[(size_t)(C1_GROUPS + g) * 64];
    float4 p0, p1;
    p0.x = patch[base[0] + ko.x]; p0.y = patch[base[0] + ko.y]; p0.z = patch[base[0] + ko.z]; p0.w = patch[base[0] + ko.w];
    p1.x = patch[base[1] + ko.x]; p1.y = patch[base[1] + ko.y]; p1.z = patch[base[1] + ko.z]; p1.w = patch[base[1] + ko.w];
    mfma_group(acc, w0, w1, p0, p1);
  }
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int m = (wave * 2 + mb) * 32 + li;
    const int oy = oy0 + (m >> 4), ox = ox0 + (m & 15);
    if (oy >= Ho || ox >= Wo) continue;
    float* dst = out + (((size_t)img * Ho + oy) * Wo + ox) * 64;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) store_relu(acc[mb][nb], bias + nb * 32 + 16 * lh, dst + nb * 32 + 16 * lh);
  }
}

// ------------------------------------------------------------------ conv2 .. conv5
constexpr int LP_CHUNK = 32;               // input channels per LDS patch
constexpr int LP_PITCH = 36;               // floats per patch pixel: 16 consecutive pixels cover all 64 banks

template <int KS>
__global__ __launch_bounds__(256) void k_lpips_conv(const float* __restrict__ in, const float* __restrict__ wpack,
                                                    const float* __restrict__ bias, float* __restrict__ out, int H, int W,
                                                    int Cin, int Cout) {
  constexpr int PS = 16 + KS - 1, PAD = KS / 2, TAPS = KS * KS;
  __shared__ __attribute__((aligned(16))) float patch[PS * PS * LP_PITCH];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int tiles_x = (W + 15) >> 4;
  const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
  const int oy0 = ty * 16, ox0 = tx * 16, img = blockIdx.z, nb0 = blockIdx.y * 2;
  const int nchunks = Cin / LP_CHUNK;
  const float* src = in + (size_t)img * H * W * Cin;

  f32x16_l acc[2][2];
  zero_acc(acc);
  int pbase[2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) pbase[mb] = ((wave * 4 + mb * 2 + (li >> 4)) * PS + (li & 15)) * LP_PITCH + 4 * lh;
  // weights: [N block][chunk][tap][group][lane] float4
  const float4* wq0 = (const float4*)wpack + (size_t)nb0 * nchunks * TAPS * 4 * 64 + lane;
  const float4* wq1 = wq0 + (size_t)nchunks * TAPS * 4 * 64;

  for (int ck = 0; ck < nchunks; ++ck) {
    if (ck) __syncthreads();               // every wave has finished reading the previous chunk
    for (int e = tid; e < PS * PS * 8; e += 256) {
      const int pp = e >> 3, q = e & 7, py = pp / PS, px = pp - py * PS;
      const int iy = oy0 + py - PAD, ix = ox0 + px - PAD;
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (iy >= 0 && iy < H && ix >= 0 && ix < W) v = *(const float4*)(src + ((size_t)iy * W + ix) * Cin + ck * LP_CHUNK + 4 * q);
      *(float4*)&patch[pp * LP_PITCH + 4 * q] = v;
    }
    __syncthreads();
    for (int tap = 0; tap < TAPS; ++tap) {
      const int toff = ((tap / KS) * PS + (tap % KS)) * LP_PITCH;
      const size_t wo = ((size_t)ck * TAPS + tap) * 4 * 64;
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const float4 w0 = wq0[wo + g * 64], w1 = wq1[wo + g * 64];
        const float4 p0 = *(const float4*)&patch[pbase[0] + toff + 8 * g];
        const float4 p1 = *(const float4*)&patch[pbase[1] + toff + 8 * g];
        mfma_group(acc, w0, w1, p0, p1);
      }
    }
  }
#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int oy = oy0 + wave * 4 + mb * 2 + (li >> 4), ox = ox0 + (li & 15);
    if (oy >= H || ox >= W) continue;
    float* dst = out + (((size_t)img * H + oy) * W + ox) * Cout;
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int n = (nb0 + nb) * 32 + 16 * lh;
      store_relu(acc[mb][nb], bias + n, dst + n);
    }
  }
}

// ------------------------------------------------------------------ max-pool 3 x 3 / 2, floor mode (every window inside)
__global__ __launch_bounds__(256) void k_lpips_pool(const float* __restrict__ in, float* __restrict__ out, int H, int W,
                                                    int Ho, int Wo, int C4, long long total) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int c = (int)(idx % C4);
  long long r = idx / C4;
  const int ox = (int)(r % Wo); r /= Wo;
  const int oy = (int)(r % Ho);
  const int img = (int)(r / Ho);
  const float4* src = (const float4*)in + (((size_t)img * H + 2 * oy) * W + 2 * ox) * C4 + c;
  float4 m = src[0];
#pragma unroll
  for (int dy = 0; dy < 3; ++dy)
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
      const float4 v = src[((size_t)dy * W + dx) * C4];
      m.x = fmaxf(m.x, v.x); m.y = fmaxf(m.y, v.y); m.z = fmaxf(m.z, v.z); m.w = fmaxf(m.w, v.w);
    }
  ((float4*)out)[idx] = m;
}

// ------------------------------------------------------------------ distance of one tap
// feat (2B, HW, C): pair b = images b and B + b.  A wave takes one pixel at a time: 64 lanes x NC channels each, the
// two norms by a butterfly (every lane gets the same bits), the lin-weighted squared difference accumulated per lane in
// double; lanes, waves and (k_lpips_finish) workgroups are then added in a fixed order.  part[B][nblk].
// The butterflies run upwards (kUp: offsets 1 .. 32) and the waves are added serially, unlike the other metric kernels
// (dsx_reduce.h): these sums round, so another order would give other bits than the ones recorded for this metric.
template <int NC>
__global__ __launch_bounds__(256) void k_lpips_dist(const float* __restrict__ feat, int B, int HW, const float* __restrict__ lin,
                                                    int ppb, double* __restrict__ part) {
  constexpr int C = NC * 64;
  __shared__ double sw[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y;
  const float* f0 = feat + (size_t)b * HW * C;
  const float* f1 = feat + (size_t)(B + b) * HW * C;
  float w[NC];
#pragma unroll
  for (int j = 0; j < NC; ++j) w[j] = lin[lane + 64 * j];
  const int p_end = min(HW, (int)(blockIdx.x + 1) * ppb);
  double acc = 0.0;
  for (int p = blockIdx.x * ppb + wave; p < p_end; p += 4) {
    float a[NC], c[NC], s0 = 0.f, s1 = 0.f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      a[j] = f0[(size_t)p * C + lane + 64 * j];
      c[j] = f1[(size_t)p * C + lane + 64 * j];
      s0 = fmaf(a[j], a[j], s0);
      s1 = fmaf(c[j], c[j], s1);
    }
    s0 = wave_reduce<RedSum, kUp>(s0);
    s1 = wave_reduce<RedSum, kUp>(s1);
    const float n0 = sqrtf(s0) + 1e-10f, n1 = sqrtf(s1) + 1e-10f;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const float d = __fsub_rn(__fdiv_rn(a[j], n0), __fdiv_rn(c[j], n1));
      acc += (double)(w[j] * (d * d));
    }
  }
  acc = block_reduce<RedSum, Serial, kUp>(acc, sw);
  if (threadIdx.x == 0) part[(size_t)b * gridDim.x + blockIdx.x] = acc;
}

__global__ __launch_bounds__(64) void k_lpips_finish(const double* __restrict__ part, LpipsTaps taps, int B, int b_off,
                                                     float* __restrict__ out, float* __restrict__ per_tap) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double total = 0.0;
  for (int t = 0; t < 5; ++t) {
    const double* row = part + taps.off[t] + (size_t)b * taps.nblk[t];
    double s = 0.0;
    for (int i = 0; i < taps.nblk[t]; ++i) s += row[i];
    s /= (double)taps.hw[t];
    if (per_tap) per_tap[(size_t)(b_off + b) * 5 + t] = (float)s;
    total += s;
  }
  out[b_off + b] = (float)total;
}

hipError_t launched() { return hipGetLastError(); }

}  // namespace

hipError_t launch_lpips_input_nchw(const float* in0, const float* in1, int B, int H, int W, float* out, hipStream_t st) {
  const long long n = 2ll * B * H * W;
  hipLaunchKernelGGL(k_lpips_input_nchw, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, in0, in1, B, (long long)H * W, out);
  return launched();
}
hipError_t launch_lpips_input_frames(const float* tgt, const float* prd, int n, int H, int W, int C, int ch, const float* mm,
                                     float* out, hipStream_t st) {
  const long long tot = 2ll * n * H * W;
  hipLaunchKernelGGL(k_lpips_input_frames, dim3((unsigned)((tot + 255) / 256)), dim3(256), 0, st, tgt, prd, n, (long long)H * W, C,
                     ch, mm, out);
  return launched();
}
hipError_t launch_lpips_minmax(const float* x, long long pixels, int C, int ch, float* part, float* mm, hipStream_t st) {
  const int blocks = lpips_minmax_blocks(pixels);
  hipLaunchKernelGGL(k_lpips_minmax, dim3(blocks), dim3(256), 0, st, x, pixels, C, ch, part);
  hipLaunchKernelGGL(k_lpips_minmax_fin, dim3(1), dim3(64), 0, st, (const float*)part, blocks, mm);
  return launched();
}
int lpips_minmax_blocks(long long pixels) {
  const long long b = (pixels + 255) / 256;
  return (int)(b > 1024 ? 1024 : (b < 1 ? 1 : b));
}
hipError_t launch_lpips_conv1(const float* in, const float* wpack, const float* bias, float* out, int nimg, int H, int W, int Ho,
                              int Wo, hipStream_t st) {
  const unsigned tiles = (unsigned)(((Ho + 15) / 16) * ((Wo + 15) / 16));
  hipLaunchKernelGGL(k_lpips_conv1, dim3(tiles, 1, (unsigned)nimg), dim3(256), 0, st, in, wpack, bias, out, H, W, Ho, Wo);
  return launched();
}
hipError_t launch_lpips_conv(int ks, const float* in, const float* wpack, const float* bias, float* out, int nimg, int H, int W,
                             int Cin, int Cout, hipStream_t st) {
  if ((ks != 3 && ks != 5) || Cin % LP_CHUNK || Cout % 64) return hipErrorInvalidValue;
  const dim3 grid((unsigned)(((H + 15) / 16) * ((W + 15) / 16)), (unsigned)(Cout / 64), (unsigned)nimg);
  if (ks == 5) hipLaunchKernelGGL(k_lpips_conv<5>, grid, dim3(256), 0, st, in, wpack, bias, out, H, W, Cin, Cout);
  else hipLaunchKernelGGL(k_lpips_conv<3>, grid, dim3(256), 0, st, in, wpack, bias, out, H, W, Cin, Cout);
  return launched();
}
hipError_t launch_lpips_pool(const float* in, float* out, int nimg, int H, int W, int Ho, int Wo, int C, hipStream_t st) {
  const long long total = (long long)nimg * Ho * Wo * (C / 4);
  hipLaunchKernelGGL(k_lpips_pool, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, in, out, H, W, Ho, Wo, C / 4, total);
  return launched();
}
int lpips_dist_blocks(int HW) {
  const int b = (HW + 63) / 64;
  return b > 1024 ? 1024 : (b < 1 ? 1 : b);
}
hipError_t launch_lpips_dist(const float* feat, int B, int HW, int C, const float* lin, double* part, hipStream_t st) {
  const int nblk = lpips_dist_blocks(HW), ppb = (HW + nblk - 1) / nblk;
  const dim3 grid((unsigned)nblk, (unsigned)B);
  switch (C) {
    case 64: hipLaunchKernelGGL(k_lpips_dist<1>, grid, dim3(256), 0, st, feat, B, HW, lin, ppb, part); break;
    case 192: hipLaunchKernelGGL(k_lpips_dist<3>, grid, dim3(256), 0, st, feat, B, HW, lin, ppb, part); break;
    case 256: hipLaunchKernelGGL(k_lpips_dist<4>, grid, dim3(256), 0, st, feat, B, HW, lin, ppb, part); break;
    case 384: hipLaunchKernelGGL(k_lpips_dist<6>, grid, dim3(256), 0, st, feat, B, HW, lin, ppb, part); break;
    default: return hipErrorInvalidValue;
  }
  return launched();
}
hipError_t launch_lpips_finish(const double* part, const LpipsTaps& taps, int B, int b_off, float* out, float* per_tap,
                               hipStream_t st) {
  hipLaunchKernelGGL(k_lpips_finish, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, part, taps, B, b_off, out, per_tap);
  return launched();
}

}  // namespace dsx
