// dsx_msssim.hip — multi-scale SSIM of plane pairs (gfx950), the definition in include/dsx.h (dsx_msssim).  Per call:
//   k_msssim_stats   (range-invariant form only) the nine plane statistics, one fixed-order double reduction per chunk
//   k_msssim_coef    per plane the two affine maps applied on the load of scale 0 and the constants c1, c2
//   k_msssim_scale   per scale: sum of the cs map and of the SSIM map over every 32 x 32 tile of the valid region
//   k_msssim_pool    between scales: 2 x 2 mean pooling of both planes, fp32 (+ affine) -> double, then double -> double
//   k_msssim_finish  per (plane, scale) the tile partials added in an order the shape alone fixes, over the pixel count
// No atomics anywhere: equal inputs give equal bits.  The reductions: dsx_reduce.h.  Host side: dsx_eval.cpp.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

// per plane: coef[plane * kMsCoef + ..] = {mean g, 1 / std g, mean p, alpha, c1, c2, 0, 0};  the loads of scale 0 are
// g' = (g - coef[0]) * coef[1] and p' = (p - coef[2]) * coef[3] in double ({0, 1, 0, 1} when not range-invariant: exact)
constexpr int kMsCoef = 8;
using MsRow = RedRow<5, 2>;            // PsnrSums' row (sum p, sum p^2, sum g, sum g^2, sum g p, min g, max g), min p, max p
constexpr int kMsStats = MsRow::kSlots;
constexpr int kMsStatChunk = 16384;    // elements of a plane per workgroup: 64 per thread

__global__ __launch_bounds__(256) void k_msssim_stats(const float* __restrict__ p, const float* __restrict__ g,
                                                      long long n, double* __restrict__ part) {
  __shared__ double red[4 * kMsStats];
  const long long base = (long long)blockIdx.y * n;
  const long long i0 = (long long)blockIdx.x * kMsStatChunk, i1 = min(n, i0 + kMsStatChunk);
  PsnrSums acc;
  double pmin = INFINITY, pmax = -INFINITY;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    const float pv = p[base + i];
    acc.add(pv, g[base + i]);
    pmin = fmin(pmin, (double)pv); pmax = fmax(pmax, (double)pv);
  }
  const double v[kMsStats] = {acc.sp, acc.spp, acc.sg, acc.sgg, acc.sgp, acc.mn, acc.mx, pmin, pmax};
  MsRow::park(v, red);
  __syncthreads();
  if (threadIdx.x < kMsStats)
    part[((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kMsStats + threadIdx.x] = MsRow::combine(red, threadIdx.x);
}

// one workgroup per plane.  Thread t adds the chunk rows t, t + 256, .. front to back, then the block reduction: the
// order is a function of nblk alone.  The transform of core/psnr.py's RangeInvariantPsnr from the sums:
//   std g = sqrt((sum g^2 - n mean_g^2) / (n - 1));  alpha = (sum g p - n mean_g mean_p) / std g / (sum p^2 - n mean_p^2)
//   L = (max g - min g) / std g.  A constant plane is recognised by min == max (exact), not by a rounded variance.
// The raw sums against the centred moments of range_invariant_psnr_curve (core/psnr.py): Cgg = sum g^2 - n mean_g^2,
// Cgp = sum g p - n mean_g mean_p, Cpp = sum p^2 - n mean_p^2; range_invariant_psnr_from_sums is the same closed form.
__global__ __launch_bounds__(256) void k_msssim_coef(const double* __restrict__ part, int nblk, double n,
                                                     int range_invariant, double c1, double c2,
                                                     double* __restrict__ coef) {
  __shared__ double red[4 * kMsStats];
  double* o = coef + (size_t)blockIdx.x * kMsCoef;
  if (!range_invariant) {                      // uniform over the grid
    if (threadIdx.x == 0) { o[0] = 0; o[1] = 1; o[2] = 0; o[3] = 1; o[4] = c1; o[5] = c2; o[6] = 0; o[7] = 0; }
    return;
  }
  double v[kMsStats];
  MsRow::init(v);
  for (int k = threadIdx.x; k < nblk; k += 256) MsRow::fold(v, part + ((size_t)blockIdx.x * nblk + k) * kMsStats);
  MsRow::park(v, red);
  __syncthreads();
  if (threadIdx.x == 0) {
    double s[kMsStats];
#pragma unroll
    for (int j = 0; j < kMsStats; ++j) s[j] = MsRow::combine(red, j);
    const double sp = s[0], spp = s[1], sg = s[2], sgg = s[3], sgp = s[4];
    const double gmin = s[5], gmax = s[6], pmin = s[7], pmax = s[8];
    const double mg = sg / n, mp = sp / n;
    double sd = sqrt(fmax(sgg - sg * mg, 0.0) / (n - 1.0));
    double alpha = ((sgp - sg * mp) / sd) / (spp - sp * mp);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    if (!(gmax > gmin)) { sd = nan; alpha = nan; }        // std g == 0 (or a NaN input): NaN for this plane
    if (!(pmax > pmin)) alpha = nan;                      // sum p~ p~ == 0
    const double L = (gmax - gmin) / sd;
    o[0] = mg; o[1] = 1.0 / sd; o[2] = mp; o[3] = alpha;
    o[4] = (0.01 * L) * (0.01 * L); o[5] = (0.03 * L) * (0.03 * L); o[6] = 0; o[7] = 0;
  }
}

// k_image_metrics' tiling (dsx_eval.hip): one workgroup per (32 x 32 tile of the valid region, plane), the 42 x 42 input
// tile staged in LDS -- here as doubles: fp32 with the plane's affine map applied on the load at scale 0 (T = float),
// the pooled double planes after that (T = double).  The horizontal 11-tap pass over the five moments and the vertical
// pass run once per 16-row half of the tile over a ring of 26 rows of horizontal sums, which keeps the workgroup at
// 61 KiB of LDS and two workgroups on a CU.  Taps in ascending order; per pixel
//   cs = (2 s12 + c2) / (s11 + s22 + c2),  ssim = (2 mu1 mu2 + c1) / (mu1^2 + mu2^2 + c1) * cs
// part[plane][tile] = {sum cs, sum ssim} by the fixed-order block reduction.
constexpr int kMsT = 32, kMsIn = kMsT + 10, kMsHalf = 16, kMsHRows = kMsHalf + 10;
template <class T>
__global__ __launch_bounds__(256) void k_msssim_scale(const T* __restrict__ a, const T* __restrict__ b, int H, int W,
                                                      const double* __restrict__ coef, SsimWindow win, int tiles_x,
                                                      double* __restrict__ part) {
  __shared__ double sa[kMsIn][kMsIn], sb[kMsIn][kMsIn];
  __shared__ double hm[5][kMsHRows][kMsT];
  __shared__ double red[4 * 2];
  const int tile = blockIdx.x, plane = blockIdx.y;
  const int y0 = (tile / tiles_x) * kMsT, x0 = (tile % tiles_x) * kMsT;      // output tile = input rows/cols + 5
  const size_t pl = (size_t)plane * H * W;
  const double* cf = coef + (size_t)plane * kMsCoef;
  const double c1 = cf[4], c2 = cf[5];
  double am = 0, as = 1, bm = 0, bs = 1;
  if (sizeof(T) == sizeof(float)) { bm = cf[0]; bs = cf[1]; am = cf[2]; as = cf[3]; }   // a = prediction, b = target
  for (int i = threadIdx.x; i < kMsIn * kMsIn; i += 256) {
    const int r = i / kMsIn, c = i % kMsIn, y = y0 + r, x = x0 + c;
    double va = 0, vb = 0;
    if (y < H && x < W) {
      va = (double)a[pl + (size_t)y * W + x];
      vb = (double)b[pl + (size_t)y * W + x];
      if (sizeof(T) == sizeof(float)) { va = (va - am) * as; vb = (vb - bm) * bs; }
    }
    sa[r][c] = va; sb[r][c] = vb;
  }
  const int col = threadIdx.x & (kMsT - 1), r8 = threadIdx.x / kMsT;
  constexpr int kRows = kMsHalf / (256 / kMsT);                               // 2 output rows per thread and half
  double acc_cs = 0, acc_ss = 0;
  for (int half = 0; half < kMsT / kMsHalf; ++half) {
    const int h0 = half * kMsHalf;
    __syncthreads();                           // the staged tile is complete / the previous half's hm has been read
    if (y0 + h0 >= H - 10) continue;           // uniform: no output row in this half (the barriers stay matched: none follows)
    // hm is a ring of 26 rows: input row y sits in slot y % 26.  The first half fills rows 0..25, the second keeps
    // rows 16..25 and replaces the others with rows 26..41, so every input row is filtered once
    for (int y = (half ? kMsHRows : 0) + r8; y < h0 + kMsHRows; y += 256 / kMsT) {
      double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
#pragma unroll
      for (int k = 0; k < 11; ++k) {
        const double u = sa[y][col + k], v = sb[y][col + k], w = win.w[k];
        m0 += w * u; m1 += w * v; m2 += w * (u * u); m3 += w * (v * v); m4 += w * (u * v);
      }
      const int r = y % kMsHRows;
      hm[0][r][col] = m0; hm[1][r][col] = m1; hm[2][r][col] = m2; hm[3][r][col] = m3; hm[4][r][col] = m4;
    }
    __syncthreads();
    const int rv = r8 * kRows;
    if (x0 + col < W - 10) {
      double mu1[kRows] = {}, mu2[kRows] = {}, e11[kRows] = {}, e22[kRows] = {}, e12[kRows] = {};
#pragma unroll
      for (int k = 0; k < kRows + 10; ++k) {
        const int r = (h0 + rv + k) % kMsHRows;
        const double h0v = hm[0][r][col], h1 = hm[1][r][col], h2 = hm[2][r][col], h3 = hm[3][r][col], h4 = hm[4][r][col];
#pragma unroll
        for (int j = 0; j < kRows; ++j) {
          if (k - j >= 0 && k - j < 11) {
            const double w = win.w[k - j];
            mu1[j] += w * h0v; mu2[j] += w * h1; e11[j] += w * h2; e22[j] += w * h3; e12[j] += w * h4;
          }
        }
      }
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (y0 + h0 + rv + j < H - 10) {
          // every operation rounded on its own (no fma): equal planes then give numerators equal to their
          // denominators bit for bit, and both maps are exactly 1
          const double mu11 = mul_d(mu1[j], mu1[j]), mu22 = mul_d(mu2[j], mu2[j]), mu12 = mul_d(mu1[j], mu2[j]);
          const double s11 = add_d(e11[j], -mu11), s22 = add_d(e22[j], -mu22), s12 = add_d(e12[j], -mu12);
          const double cs = add_d(mul_d(2.0, s12), c2) / add_d(add_d(s11, s22), c2);
          acc_cs += cs;
          acc_ss += mul_d(add_d(mul_d(2.0, mu12), c1) / add_d(add_d(mu11, mu22), c1), cs);
        }
      }
    }
  }
  __syncthreads();
  block_park<RedSum>(acc_cs, red, 2, 0);
  block_park<RedSum>(acc_ss, red, 2, 1);
  __syncthreads();
  if (threadIdx.x < 2)
    part[((size_t)plane * gridDim.x + tile) * 2 + threadIdx.x] = block_combine<RedSum, Pairwise>(red, 2, threadIdx.x);
}

// 2 x 2 mean pooling of both planes of every pair: out (Ho, Wo) = (H / 2, W / 2), an odd last row / column dropped;
// ((x00 + x01) + (x10 + x11)) * 0.25 in double, stored as double.  T = float: the planes of scale 0 under their affine maps.
template <class T>
__global__ __launch_bounds__(256) void k_msssim_pool(const T* __restrict__ a, const T* __restrict__ b, int planes, int H,
                                                     int W, const double* __restrict__ coef, double* __restrict__ oa,
                                                     double* __restrict__ ob) {
  const int Ho = H / 2, Wo = W / 2;
  const long long per = (long long)Ho * Wo, total = per * planes;
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const int plane = (int)(i / per);
    const long long q = i - (long long)plane * per;
    const int y = (int)(q / Wo), x = (int)(q - (long long)y * Wo);
    const size_t src = (size_t)plane * H * W + (size_t)(2 * y) * W + 2 * x;
    double a00 = (double)a[src], a01 = (double)a[src + 1], a10 = (double)a[src + W], a11 = (double)a[src + W + 1];
    double b00 = (double)b[src], b01 = (double)b[src + 1], b10 = (double)b[src + W], b11 = (double)b[src + W + 1];
    if (sizeof(T) == sizeof(float)) {
      const double* cf = coef + (size_t)plane * kMsCoef;
      const double bm = cf[0], bs = cf[1], am = cf[2], as = cf[3];
      a00 = (a00 - am) * as; a01 = (a01 - am) * as; a10 = (a10 - am) * as; a11 = (a11 - am) * as;
      b00 = (b00 - bm) * bs; b01 = (b01 - bm) * bs; b10 = (b10 - bm) * bs; b11 = (b11 - bm) * bs;
    }
    oa[i] = ((a00 + a01) + (a10 + a11)) * 0.25;
    ob[i] = ((b00 + b01) + (b10 + b11)) * 0.25;
  }
}

// one workgroup per (scale, plane): thread t adds the tiles t, t + 256, .. front to back, then the fixed-order block
// reduction -- the order is a function of the tile count, that is of the shape, alone.  out[plane][scale] = the two means.
__global__ __launch_bounds__(256) void k_msssim_finish(const double* __restrict__ part, MsssimLayout lay,
                                                       double* __restrict__ out) {
  __shared__ double red[4 * 2];
  const int s = blockIdx.x, plane = blockIdx.y, tiles = lay.tiles[s];
  const double* p = part + lay.off[s] + (size_t)plane * tiles * 2;
  double cs = 0, ss = 0;
  for (int t = threadIdx.x; t < tiles; t += 256) { cs += p[2 * t]; ss += p[2 * t + 1]; }
  block_park<RedSum>(cs, red, 2, 0);
  block_park<RedSum>(ss, red, 2, 1);
  __syncthreads();
  if (threadIdx.x < 2)
    out[((size_t)plane * gridDim.x + s) * 2 + threadIdx.x] = block_combine<RedSum, Pairwise>(red, 2, threadIdx.x) / lay.count[s];
}

int msssim_stat_blocks(long long n) { return (int)((n + kMsStatChunk - 1) / kMsStatChunk); }

// the workspace of a call, in doubles per plane pair (every segment holds `planes` times its share, in this order):
// coefficients, statistics partials, the output means, the tile partials of every scale, the pooled planes of scales >= 1
size_t msssim_layout(int H, int W, int scales, MsssimLayout* lay) {
  MsssimLayout l{};
  size_t tiles = 0, pooled = 0;
  int h = H, w = W;
  for (int s = 0; s < scales; ++s) {
    l.H[s] = h; l.W[s] = w;
    l.tiles[s] = image_metrics_tiles(h, w);
    l.count[s] = (double)(h - 10) * (double)(w - 10);
    tiles += (size_t)l.tiles[s] * 2;
    if (s) pooled += (size_t)h * w * 2;
    h /= 2; w /= 2;
  }
  if (lay) *lay = l;
  return (size_t)kMsCoef + (size_t)msssim_stat_blocks((long long)H * W) * kMsStats + (size_t)scales * 2 + tiles + pooled;
}

hipError_t launch_msssim(const float* pred, const float* target, int planes, int H, int W, int scales, int range_invariant,
                         double c1, double c2, const SsimWindow& win, double* ws, double** out_dev, hipStream_t st) {
  MsssimLayout lay;
  msssim_layout(H, W, scales, &lay);
  const size_t P = (size_t)planes;
  const int nblk = msssim_stat_blocks((long long)H * W);
  double* coef = ws;
  double* stat = coef + P * kMsCoef;
  double* out = stat + P * nblk * kMsStats;
  double* part = out + P * scales * 2;
  size_t off = 0;
  for (int s = 0; s < scales; ++s) { lay.off[s] = (long long)off; off += P * lay.tiles[s] * 2; }
  double* pyr = part + off;
  hipError_t e;
  if (range_invariant) {
    hipLaunchKernelGGL(k_msssim_stats, dim3((unsigned)nblk, (unsigned)planes), dim3(256), 0, st, pred, target,
                       (long long)H * W, stat);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  hipLaunchKernelGGL(k_msssim_coef, dim3((unsigned)planes), dim3(256), 0, st, stat, nblk, (double)H * (double)W,
                     range_invariant, c1, c2, coef);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  const double *ca = nullptr, *cb = nullptr;   // the pooled planes of the current scale (s >= 1)
  for (int s = 0; s < scales; ++s) {
    const int h = lay.H[s], w = lay.W[s], tiles_x = (w - 10 + kMsT - 1) / kMsT;
    const dim3 grid((unsigned)lay.tiles[s], (unsigned)planes);
    if (s == 0)
      hipLaunchKernelGGL(k_msssim_scale<float>, grid, dim3(256), 0, st, pred, target, h, w, coef, win, tiles_x,
                         part + lay.off[s]);
    else
      hipLaunchKernelGGL(k_msssim_scale<double>, grid, dim3(256), 0, st, ca, cb, h, w, coef, win, tiles_x,
                         part + lay.off[s]);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (s + 1 == scales) break;
    const size_t per = (size_t)(h / 2) * (w / 2) * P;
    double *na = pyr, *nb = pyr + per;
    pyr += 2 * per;
    const unsigned g = (unsigned)grid_for((long long)per);
    if (s == 0)
      hipLaunchKernelGGL(k_msssim_pool<float>, dim3(g), dim3(256), 0, st, pred, target, planes, h, w, coef, na, nb);
    else
      hipLaunchKernelGGL(k_msssim_pool<double>, dim3(g), dim3(256), 0, st, ca, cb, planes, h, w, coef, na, nb);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    ca = na; cb = nb;
  }
  hipLaunchKernelGGL(k_msssim_finish, dim3((unsigned)scales, (unsigned)planes), dim3(256), 0, st, part, lay, out);
  *out_dev = out;
  return hipGetLastError();
}

}  // namespace dsx
