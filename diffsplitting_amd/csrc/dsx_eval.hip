// dsx_eval.hip — the evaluation kernels (gfx950) that are not tiling, none of which runs inside a sampling step:
// the Welford moments over repeated samples, the TimePredictor's range table, SSIM + PSNR of image pairs, and the
// per-sample L1 / L2 reduction of the training objective (the noising step in front of the UNet forward is k_q_sample,
// dsx_steps.hip).  The tile kernels are dsx_tiles.hip; the reductions: dsx_reduce.h.  Host side: dsx_eval.cpp.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

// Mean and spread over N posterior samples, Welford's recurrence in double, one launch per sample and one to finish:
//   r == 0: mean = x, M2 = 0;   else d = x - mean;  mean' = mean + d / (r + 1);  M2' = M2 + d * (x - mean')
//   finish: mean_out = (float)mean;  std_out = n > 1 ? (float)sqrt(M2 / (n - 1)) : 0
// Every operation is rounded on its own, so a numpy float64 restatement of these lines gives the same bits.  The
// __d*_rn forms are plain operators in the toolchain's headers and may be contracted once inlined: the product and the
// sums go through mul_d / add_d / sub_d (dsx_kernels.h), which take the `contract` flag off their own instruction.
__global__ __launch_bounds__(256) void k_moments_update(const float* __restrict__ x, double* __restrict__ mean,
                                                        double* __restrict__ m2, long long count, int r) {
  const double rn = (double)(r + 1);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const double xv = (double)x[i];
    if (r == 0) { mean[i] = xv; m2[i] = 0.0; continue; }
    const double m = mean[i], d = sub_d(xv, m);
    const double m1 = add_d(m, d / rn);
    mean[i] = m1;
    m2[i] = add_d(m2[i], mul_d(d, sub_d(xv, m1)));
  }
}
__global__ __launch_bounds__(256) void k_moments_finish(const double* __restrict__ mean, const double* __restrict__ m2,
                                                        long long count, int n, float* __restrict__ mean_out,
                                                        float* __restrict__ std_out) {
  const double nm1 = (double)(n - 1);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    mean_out[i] = (float)mean[i];
    if (std_out) std_out[i] = n > 1 ? (float)sqrt(m2[i] / nm1) : 0.0f;
  }
}
hipError_t launch_moments_update(const float* x, double* mean, double* m2, long long count, int r, hipStream_t st) {
  hipLaunchKernelGGL(k_moments_update, dim3(grid_for(count)), dim3(256), 0, st, x, mean, m2, count, r);
  return hipGetLastError();
}
hipError_t launch_moments_finish(const double* mean, const double* m2, long long count, int n, float* mean_out,
                                 float* std_out, hipStream_t st) {
  hipLaunchKernelGGL(k_moments_finish, dim3(grid_for(count)), dim3(256), 0, st, mean, m2, count, n, mean_out, std_out);
  return hipGetLastError();
}

// (mul_d / add_d, one IEEE operation each, live in dsx_kernels.h)
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
  __shared__ double red[4 * kMixTB * 2];       // [wave][t][{min, max}]
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
#pragma unroll
  for (int j = 0; j < kMixTB; ++j) {
    block_park<RedMin>(mn[j], red, kMixTB * 2, 2 * j);
    block_park<RedMax>(mx[j], red, kMixTB * 2, 2 * j + 1);
  }
  __syncthreads();
  if (threadIdx.x < kMixTB * 2) {
    const int j = threadIdx.x >> 1, kk = threadIdx.x & 1;
    if (tb + j <= n)
      part[((size_t)blockIdx.y * (n + 1) + (tb + j)) * 2 + kk] =
          kk ? block_combine<RedMax, Pairwise>(red, kMixTB * 2, threadIdx.x)
             : block_combine<RedMin, Pairwise>(red, kMixTB * 2, threadIdx.x);
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
__global__ __launch_bounds__(256) void k_image_metrics(const float* __restrict__ a, const float* __restrict__ b, int H,
                                                       int W, int quantize, float lo, float hi, float rng, double c1,
                                                       double c2, SsimWindow win, int tiles_x, double* __restrict__ part) {
  __shared__ float sa[kSsimIn][kSsimIn], sb[kSsimIn][kSsimIn];
  __shared__ double hm[5][kSsimIn][kSsimT];
  __shared__ double red[4 * 2];                // [wave][{SSIM sum, fp64 SSD}]
  __shared__ unsigned long long redq[4];       // [wave] integer SSD
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
  block_park<RedSum>(acc, red, 2, 0);
  if (q) block_park<RedSum>(ssdq, redq);       // q is the same in every thread
  else block_park<RedSum>(ssd, red, 2, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)plane * gridDim.x + tile) * 2;
    o[0] = block_combine<RedSum, Pairwise>(red, 2, 0);
    o[1] = q ? __longlong_as_double((long long)block_combine<RedSum, Pairwise>(redq))
             : block_combine<RedSum, Pairwise>(red, 2, 1);
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

// ---------------------------------------------------------------------------
// Per-sample sum |a - b| (L1Loss) or sum (a - b)^2 (MSELoss) over (C, H, W): difference, square and accumulation in
// double.  Workgroup (x, b) owns elements [x * kLossChunk, (x + 1) * kLossChunk) of sample b -- loss_blocks(n) of them,
// a function of the shape alone -- and reduces thread -> wave shuffles -> 4 waves in a fixed order; k_loss_finish adds a
// sample's partials front to back.  No atomics: equal inputs give bitwise-equal outputs.
// ---------------------------------------------------------------------------
constexpr int kLossChunk = 4096;   // 16 elements per thread
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
  s = block_reduce<RedSum, Pairwise>(s, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
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
