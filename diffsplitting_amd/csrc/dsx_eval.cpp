// dsx_eval.cpp — the evaluation entry points that are not tiling: image metrics (SSIM + SSD), multi-scale SSIM, the
// validation report of the training loop, the range table of the mixed inputs and the Welford moments over repeated
// samples.  Kernels: dsx_eval.hip, dsx_msssim.hip, dsx_validate.hip.  C ABI in include/dsx.h.
#include "dsx_rt.h"

// SSIM + SSD of image pairs (core/metrics.py:62-92), optionally on the tensor2img quantisation (:14-34)
extern "C" int dsx_image_metrics_blocks(int H, int W) {
  if (H < 11 || W < 11) return fail(DSX_ERR_INVALID, "SSIM needs H, W >= 11 (got %d x %d)", H, W);
  return image_metrics_tiles(H, W);
}
extern "C" int dsx_image_metrics(const float* a, const float* b, int B, int C, int H, int W, int quantize, double lo,
                                 double hi, double data_range, double* partials_dev, double* out_ssim,
                                 double* out_ssd, void* stream) {
  if (!a || !b || !partials_dev || !out_ssim || !out_ssd || B < 1 || C < 1)
    return fail(DSX_ERR_INVALID, "bad argument");
  if (H < 11 || W < 11) return fail(DSX_ERR_INVALID, "SSIM needs H, W >= 11 (got %d x %d)", H, W);
  if ((int64_t)B * C > 65535) return fail(DSX_ERR_INVALID, "B * C = %lld image planes, at most 65535", (long long)B * C);
  if (!(data_range > 0) || !std::isfinite(data_range)) return fail(DSX_ERR_INVALID, "data_range must be positive");
  if (quantize && !(std::isfinite(lo) && std::isfinite(hi) && hi > lo))
    return fail(DSX_ERR_INVALID, "quantisation needs finite min_max with lo < hi");
  // cv2.getGaussianKernel(11, 1.5): exp(-x^2 / (2 sigma^2)) scaled by 1 / sum, in double
  SsimWindow win;
  double sum = 0;
  for (int i = 0; i < 11; ++i) { const double x = i - 5.0; win.w[i] = std::exp((-0.5 / (1.5 * 1.5)) * x * x); sum += win.w[i]; }
  sum = 1.0 / sum;
  for (int i = 0; i < 11; ++i) win.w[i] *= sum;
  const double c1 = (0.01 * data_range) * (0.01 * data_range), c2 = (0.03 * data_range) * (0.03 * data_range);
  // tensor2img's arithmetic: clamp bounds as fp32, hi - lo in double then fp32 (torch divides by a Python float)
  const int planes = B * C, tiles = image_metrics_tiles(H, W);
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch_image_metrics(a, b, planes, H, W, quantize ? 1 : 0, (float)lo, (float)hi, (float)(hi - lo), c1, c2,
                               win, partials_dev, st));
  std::vector<double> part((size_t)planes * tiles * 2);
  HIP_TRY(hipMemcpyAsync(part.data(), partials_dev, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  const double valid = (double)C * (H - 10) * (W - 10);
  for (int i = 0; i < B; ++i) {
    double s = 0, d = 0;
    uint64_t dq = 0;
    for (size_t j = (size_t)i * C * tiles; j < (size_t)(i + 1) * C * tiles; ++j) {
      s += part[j * 2];
      if (quantize) { uint64_t u; std::memcpy(&u, &part[j * 2 + 1], 8); dq += u; }
      else d += part[j * 2 + 1];
    }
    out_ssim[i] = s / valid;
    out_ssd[i] = quantize ? (double)dq : d;
  }
  return DSX_OK;
}

// multi-scale SSIM (include/dsx.h): every launch on the caller's stream, one synchronisation to read the means
static int msssim_check_shape(int H, int W, int scales) {
  if (scales < 1 || scales > 5) return fail(DSX_ERR_INVALID, "MS-SSIM: %d scales, must be in 1..5", scales);
  if (H < 1 || W < 1 || ((H < W ? H : W) >> (scales - 1)) < 11)
    return fail(DSX_ERR_INVALID, "MS-SSIM with %d scales needs min(H, W) >= %d (the coarsest scale still holds the 11 x 11 "
                "window), got %d x %d", scales, 11 << (scales - 1), H, W);
  if ((int64_t)H * W > INT32_MAX) return fail(DSX_ERR_INVALID, "MS-SSIM: plane too large");
  return DSX_OK;
}
extern "C" int64_t dsx_msssim_workspace(int H, int W, int scales) {
  const int rc = msssim_check_shape(H, W, scales);
  if (rc) return rc;
  return (int64_t)(msssim_layout(H, W, scales, nullptr) * sizeof(double));
}
extern "C" int dsx_msssim(const float* pred, const float* target, int planes, int H, int W, int scales, int range_invariant,
                          double data_range, void* workspace, size_t workspace_bytes, double* out, void* stream) {
  const int64_t per_plane = dsx_msssim_workspace(H, W, scales);
  if (per_plane < 0) return (int)per_plane;
  if (!pred || !target || !workspace || !out) return fail(DSX_ERR_INVALID, "MS-SSIM: null argument");
  if (planes < 1 || planes > 65535) return fail(DSX_ERR_INVALID, "MS-SSIM: %d image planes, must be in 1..65535", planes);
  if (!range_invariant && (!(data_range > 0) || !std::isfinite(data_range)))
    return fail(DSX_ERR_INVALID, "MS-SSIM: data_range must be positive (or range_invariant set)");
  if (workspace_bytes < (size_t)per_plane * planes)
    return fail(DSX_ERR_INVALID, "MS-SSIM: workspace of %zu bytes, %d planes need %zu", workspace_bytes, planes,
                (size_t)per_plane * planes);
  if ((uintptr_t)workspace % sizeof(double)) return fail(DSX_ERR_INVALID, "MS-SSIM: the workspace must be 8-byte aligned");
  SsimWindow win;                              // the window of dsx_image_metrics, computed the same way
  double sum = 0;
  for (int i = 0; i < 11; ++i) { const double x = i - 5.0; win.w[i] = std::exp((-0.5 / (1.5 * 1.5)) * x * x); sum += win.w[i]; }
  sum = 1.0 / sum;
  for (int i = 0; i < 11; ++i) win.w[i] *= sum;
  const double L = range_invariant ? 0.0 : data_range;
  hipStream_t st = (hipStream_t)stream;
  double* out_dev = nullptr;
  HIP_TRY(launch_msssim(pred, target, planes, H, W, scales, range_invariant ? 1 : 0, (0.01 * L) * (0.01 * L),
                        (0.03 * L) * (0.03 * L), win, (double*)workspace, &out_dev, st));
  HIP_TRY(hipMemcpyAsync(out, out_dev, (size_t)planes * scales * 2 * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return DSX_OK;
}

// the validation report of the training loop (split.py:174-241): two launches, nothing allocated or synchronised
extern "C" int dsx_val_report(const float* input, const float* target, const float* prediction, int B, int Cin, int C,
                              int H, int W, double mean_input, double std_input, const double* mean_target,
                              const double* std_target, uint16_t* input_q, uint16_t* target_q, uint16_t* pred_q,
                              uint16_t* input_n, uint16_t* target_n, uint16_t* pred_n, uint64_t* partial_dev,
                              uint64_t* stats_dev, void* stream) {
  if (B < 1 || Cin < 1 || C < 1 || H < 1 || W < 1)
    return fail(DSX_ERR_INVALID, "val_report: empty shape (%d, %d + %d, %d, %d)", B, Cin, C, H, W);
  if (C > kValMaxC) return fail(DSX_ERR_INVALID, "val_report: %d target channels, at most %d", C, kValMaxC);
  if ((int64_t)H * W > INT32_MAX) return fail(DSX_ERR_INVALID, "val_report: plane too large");
  if ((int64_t)B * ((int64_t)C + Cin) > 65535)
    return fail(DSX_ERR_INVALID, "val_report: B * (C + Cin) = %lld image planes, at most 65535", (long long)B * ((long long)C + Cin));
  if (!input || !target || !prediction || !mean_target || !std_target || !input_q || !target_q || !pred_q || !partial_dev ||
      !stats_dev)
    return fail(DSX_ERR_INVALID, "val_report: null argument");
  if ((input_n == nullptr) != (target_n == nullptr) || (input_n == nullptr) != (pred_n == nullptr))
    return fail(DSX_ERR_INVALID, "val_report: the three numerator arrays are given together, or none");
  ValArgs a{};
  a.input = input; a.target = target; a.pred = prediction;
  a.input_q = input_q; a.target_q = target_q; a.pred_q = pred_q;
  a.input_n = input_n; a.target_n = target_n; a.pred_n = pred_n;
  a.part = (unsigned long long*)partial_dev; a.stats = (unsigned long long*)stats_dev;
  a.mean_in = mean_input; a.std_in = std_input;
  for (int c = 0; c < C; ++c) { a.mean_t[c] = mean_target[c]; a.std_t[c] = std_target[c]; }
  a.B = B; a.Cin = Cin; a.C = C; a.HW = (int64_t)H * W; a.nblk = val_blocks(a.HW);
  HIP_TRY(launch_val_report(a, (hipStream_t)stream));
  return DSX_OK;
}

// the four statistics of the two target channels: finite, no zero standard deviation (also dsx_tiles.cpp)
int dsx::norm4_ok(const double norm[4]) {
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(norm[i])) return fail(DSX_ERR_INVALID, "normalisation statistics must be finite");
  if (norm[1] == 0.0 || norm[3] == 0.0) return fail(DSX_ERR_INVALID, "zero standard deviation");
  return DSX_OK;
}
// the range table of the mixed inputs in one launch; the min / max over the partial rows on the host (exact)
extern "C" int dsx_mix_range_blocks(int64_t pixels, int n_timesteps) {
  if (pixels < 1) return fail(DSX_ERR_INVALID, "mix_range: no pixels");
  if (n_timesteps < 1 || n_timesteps > 1024) return fail(DSX_ERR_INVALID, "n_timesteps = %d, must be in 1..1024", n_timesteps);
  return mix_range_blocks(pixels);
}
extern "C" int dsx_mix_range(const float* frames0, const float* frames1, int64_t pixels, const double norm[4],
                             int n_timesteps, double* partials_dev, double* out_minmax, void* stream) {
  const int rows = dsx_mix_range_blocks(pixels, n_timesteps);
  if (rows < 0) return rows;
  if (!norm) return fail(DSX_ERR_INVALID, "null argument");
  int rc = norm4_ok(norm);
  if (rc) return rc;
  if (!frames0 || !frames1 || !partials_dev || !out_minmax) return fail(DSX_ERR_INVALID, "null argument");
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch_mix_range(frames0, frames1, pixels, norm, n_timesteps, partials_dev, st));
  const size_t row = (size_t)(n_timesteps + 1) * 2;
  std::vector<double> part((size_t)rows * row);
  HIP_TRY(hipMemcpyAsync(part.data(), partials_dev, part.size() * sizeof(double), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  for (size_t i = 0; i < row; i += 2) {
    double lo = part[i], hi = part[i + 1];
    for (int r = 1; r < rows; ++r) { lo = std::fmin(lo, part[r * row + i]); hi = std::fmax(hi, part[r * row + i + 1]); }
    out_minmax[i] = lo; out_minmax[i + 1] = hi;
  }
  return DSX_OK;
}

// mean and spread over repeated samples (Welford in double; launch_moments_* in dsx_eval.hip)
extern "C" int dsx_moments_update(const float* x, double* mean, double* m2, int64_t count, int r, void* stream) {
  if (!x || !mean || !m2) return fail(DSX_ERR_INVALID, "moments_update: null argument");
  if (count < 1) return fail(DSX_ERR_INVALID, "moments_update: count = %lld, must be positive", (long long)count);
  if (r < 0 || r >= (1 << 24)) return fail(DSX_ERR_INVALID, "moments_update: r = %d, must be in 0..2^24 - 1", r);
  HIP_TRY(launch_moments_update(x, mean, m2, (long long)count, r, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_moments_finish(const double* mean, const double* m2, int64_t count, int n, float* mean_out,
                                  float* std_out, void* stream) {
  if (!mean || !m2 || !mean_out) return fail(DSX_ERR_INVALID, "moments_finish: null argument (only std_out may be NULL)");
  if (count < 1) return fail(DSX_ERR_INVALID, "moments_finish: count = %lld, must be positive", (long long)count);
  if (n < 1 || n > (1 << 24)) return fail(DSX_ERR_INVALID, "moments_finish: n = %d, must be in 1..2^24", n);
  HIP_TRY(launch_moments_finish(mean, m2, (long long)count, n, mean_out, std_out, (hipStream_t)stream));
  return DSX_OK;
}
