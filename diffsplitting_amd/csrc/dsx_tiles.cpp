// dsx_tiles.cpp — tiling: the tile planner (host integer math), the per-call gather / stitch forms, image metrics,
// mixed-input evaluation and the tile plan with device-resident tables.  C ABI in include/dsx.h.
#include "dsx_rt.h"

// ------------------------------------------------------------------ tiling (host integer math)
namespace {
struct TilePlanner {
  int64_t D[3], g[3], p[3];
  int mode;
  int64_t dim_count(int d) const {  // tiling_manager.py:34-50
    if (g[d] == 1 && p[d] == 1) return D[d];
    const int64_t ex = p[d] - g[d];
    if (mode == DSX_TILING_PAD) return (D[d] + g[d] - 1) / g[d];
    const int64_t num = D[d] - ex;
    if (mode == DSX_TILING_SHIFT) return num <= 0 ? 0 : (num + g[d] - 1) / g[d];
    return num < 0 ? 0 : num / g[d];
  }
  int64_t grid_count(int d) const {  // :58-68
    int64_t n = 1;
    for (int k = d + 1; k < 3; ++k) n *= dim_count(k);
    return n;
  }
  int64_t total() const { return grid_count(0) * dim_count(0); }
  int64_t grid_start(int d, int64_t k) const {  // :121-143
    const int64_t ex = (p[d] - g[d]) / 2;
    if (g[d] == 1 && p[d] == 1) return k;
    if (mode == DSX_TILING_PAD) return k * g[d];
    if (mode == DSX_TILING_TRIM) return k * g[d] + ex;
    if (k < dim_count(d) - 1) return k * g[d] + ex;
    return D[d] - g[d] - ex;
  }
  void location(int64_t idx, int64_t loc[3]) const {  // :145-154
    for (int d = 0; d < 3; ++d) {
      const int64_t gc = grid_count(d);
      loc[d] = grid_start(d, idx / gc);
      idx %= gc;
    }
  }
};
static int make_planner(const int64_t* ds, const int64_t* gs, const int64_t* ps, int mode, TilePlanner& t) {
  if (!ds || !gs || !ps) return fail(DSX_ERR_INVALID, "null shape");
  if (mode < 0 || mode > 2) return fail(DSX_ERR_INVALID, "bad tiling mode");
  for (int d = 0; d < 3; ++d) {
    t.D[d] = ds[d]; t.g[d] = gs[d]; t.p[d] = ps[d];
    if (ds[d] < 1 || gs[d] < 1 || ps[d] < gs[d] || ((ps[d] - gs[d]) & 1))  // tiling_manager.py:21-29
      return fail(DSX_ERR_INVALID, "patch must be >= grid with even padding in dim %d", d);
  }
  t.mode = mode;
  return DSX_OK;
}
}  // namespace

extern "C" int64_t dsx_tile_plan(const int64_t data_shape[3], const int64_t grid_shape[3],
                                 const int64_t patch_shape[3], int mode, int64_t* grid_start,
                                 int64_t* patch_start, int64_t capacity) {
  TilePlanner t;
  int rc = make_planner(data_shape, grid_shape, patch_shape, mode, t);
  if (rc) return rc;
  const int64_t n = t.total();
  if (grid_start || patch_start) {
    if (capacity < n) return fail(DSX_ERR_INVALID, "capacity %lld < %lld tiles", (long long)capacity, (long long)n);
    for (int64_t i = 0; i < n; ++i) {
      int64_t loc[3];
      t.location(i, loc);
      for (int d = 0; d < 3; ++d) {
        if (grid_start) grid_start[i * 3 + d] = loc[d];
        if (patch_start) patch_start[i * 3 + d] = loc[d] - (t.p[d] - t.g[d]) / 2;
      }
    }
  }
  return n;
}

extern "C" int dsx_tile_regions(const int64_t data_shape[3], const int64_t grid_shape[3],
                                const int64_t patch_shape[3], int mode, int32_t* regions, int64_t capacity) {
  TilePlanner t;
  int rc = make_planner(data_shape, grid_shape, patch_shape, mode, t);
  if (rc) return rc;
  if (!regions) return fail(DSX_ERR_INVALID, "null regions");
  const int64_t n = t.total();
  if (capacity < n) return fail(DSX_ERR_INVALID, "capacity too small");
  for (int64_t i = 0; i < n; ++i) {
    int64_t gs[3], vgs[3], vge[3], ps[3];
    t.location(i, gs);
    for (int d = 0; d < 3; ++d) {  // tile_stitcher.py:26-56
      const int64_t ge = gs[d] + t.g[d];
      ps[d] = gs[d] - (t.p[d] - t.g[d]) / 2;
      const int64_t pe = ps[d] + t.p[d];
      vgs[d] = gs[d]; vge[d] = ge;
      if (mode == DSX_TILING_SHIFT) {
        if (ps[d] == 0) vgs[d] = 0;
        if (pe == t.D[d]) vge[d] = t.D[d];
      }
    }
    int32_t* r = regions + i * 8;
    r[0] = (int32_t)vgs[0]; r[1] = (int32_t)vgs[1]; r[2] = (int32_t)vgs[2];
    r[3] = (int32_t)(vge[1] - vgs[1]); r[4] = (int32_t)(vge[2] - vgs[2]);
    r[5] = (int32_t)(vgs[1] - ps[1]); r[6] = (int32_t)(vgs[2] - ps[2]); r[7] = 0;
  }
  return DSX_OK;
}

// ---- legacy per-call forms: the caller passes host tables, which are uploaded for the call (one small allocation,
// one synchronous copy into a DevBuf of the call, freed on every path).  The stall-free forms are the dsx_tileplan_*
// entry points below.
namespace {
// starts[i] = (int) patch start of tile tile_ids[i] (or tile i); returns the id of the first tile that does not lie
// inside the frames (the conversion stops there), -1 if every tile does
static int64_t convert_starts(const int64_t* patch_start, const int64_t* tile_ids, int64_t count, const int64_t data_shape[3],
                              const int64_t patch_shape[3], std::vector<int>& starts) {
  starts.resize((size_t)count * 3);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t id = tile_ids ? tile_ids[i] : i;
    for (int d = 0; d < 3; ++d) starts[i * 3 + d] = (int)patch_start[id * 3 + d];
    if (starts[i * 3] < 0 || starts[i * 3] >= data_shape[0] || starts[i * 3 + 1] < 0 ||
        starts[i * 3 + 1] + patch_shape[1] > data_shape[1] || starts[i * 3 + 2] < 0 ||
        starts[i * 3 + 2] + patch_shape[2] > data_shape[2])
      return id;
  }
  return -1;
}
static int check_starts(const int64_t* patch_start, const int64_t* tile_ids, int64_t count, const int64_t data_shape[3],
                        const int64_t patch_shape[3], std::vector<int>& starts) {
  const int64_t bad = convert_starts(patch_start, tile_ids, count, data_shape, patch_shape, starts);
  return bad < 0 ? DSX_OK : fail(DSX_ERR_INVALID, "tile %lld lies outside the frames", (long long)bad);
}
static int check_regions(const int32_t* regions, int64_t count, const int64_t data_shape[3], int ph, int pw) {
  for (int64_t i = 0; i < count; ++i) {
    const int32_t* r = regions + i * 8;
    if (r[0] < 0 || r[0] >= data_shape[0] || r[1] < 0 || r[1] + r[3] > data_shape[1] || r[2] < 0 ||
        r[2] + r[4] > data_shape[2] || r[5] < 0 || r[5] + r[3] > ph || r[6] < 0 || r[6] + r[4] > pw)
      return fail(DSX_ERR_INVALID, "region %lld out of bounds", (long long)i);
  }
  return DSX_OK;
}
}  // namespace

extern "C" int dsx_tiles_gather(const float* frames, const int64_t data_shape[3], const int64_t patch_shape[3],
                                const int64_t* patch_start, const int64_t* tile_ids, int64_t count,
                                float* tiles, void* stream) {
  if (!frames || !data_shape || !patch_shape || !patch_start || !tiles || count < 0)
    return fail(DSX_ERR_INVALID, "bad argument");
  if (count == 0) return DSX_OK;
  std::vector<int> starts;
  int rc = check_starts(patch_start, tile_ids, count, data_shape, patch_shape, starts);
  if (rc) return rc;
  DevBuf d;
  HIP_TRY(d.upload(starts.data(), starts.size() * 4));
  HIP_TRY(launch_tiles_gather(frames, (int)data_shape[1], (int)data_shape[2], (int)patch_shape[1],
                              (int)patch_shape[2], (const int*)d.p, TileSeq{0, 1, count}, tiles, (hipStream_t)stream));
  return DSX_OK;   // ~DevBuf waits for the launch (DevBuf::reset)
}

extern "C" int dsx_stitch(const float* tiles, int64_t count, int C, int ph, int pw, const int32_t* regions,
                          float* canvas, const int64_t data_shape[3], void* stream) {
  if (!tiles || !regions || !canvas || !data_shape || count < 0 || C < 1)
    return fail(DSX_ERR_INVALID, "bad argument");
  if (count == 0) return DSX_OK;
  int rc = check_regions(regions, count, data_shape, ph, pw);
  if (rc) return rc;
  DevBuf d;
  HIP_TRY(d.upload(regions, (size_t)count * 32));
  const StitchSrc src{tiles, 0, ph, pw, nullptr, 0, 1};
  HIP_TRY(launch_stitch(src, C, (const int*)d.p, TileSeq{0, 1, count}, canvas, (int)data_shape[1], (int)data_shape[2],
                        nullptr, nullptr, 0, (hipStream_t)stream));
  return DSX_OK;
}

// stitch + RangeInvariantPsnr partial sums in one pass over the tiles (no second pass over the canvas)
extern "C" int dsx_stitch_psnr_blocks(int ph, int pw) {
  int gx = (ph * pw + 255) / 256;
  return gx > 16 ? 16 : (gx < 1 ? 1 : gx);
}
extern "C" int dsx_stitch_psnr(const float* tiles, int64_t count, int C, int ph, int pw, const int32_t* regions,
                               float* canvas, const int64_t data_shape[3], const float* gt_canvas, double* partials_dev,
                               void* stream) {
  if (!tiles || !regions || !canvas || !data_shape || !gt_canvas || !partials_dev || count < 0 || C < 1 || C > 4)
    return fail(DSX_ERR_INVALID, "bad argument (1 <= C <= 4)");
  if (count == 0) return DSX_OK;
  int rc = check_regions(regions, count, data_shape, ph, pw);
  if (rc) return rc;
  DevBuf d;
  HIP_TRY(d.upload(regions, (size_t)count * 32));
  const StitchSrc src{tiles, 0, ph, pw, nullptr, 0, 1};
  HIP_TRY(launch_stitch(src, C, (const int*)d.p, TileSeq{0, 1, count}, canvas, (int)data_shape[1], (int)data_shape[2],
                        gt_canvas, partials_dev, dsx_stitch_psnr_blocks(ph, pw), (hipStream_t)stream));
  return DSX_OK;
}

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

// tiles of both channels cut out of device-resident frames AND normalised in the same pass: the batch source of tiled
// prediction without the per-tile host crop + host->device copy of the reference's DataLoader(batch_size = 1)
extern "C" int dsx_tiles_gather_norm(const float* frames0, const float* frames1, const int64_t data_shape[3],
                                     const int64_t patch_shape[3], const int64_t* patch_start, const int64_t* tile_ids,
                                     int64_t count, float w0, float w1, const double norm[6], int from_norm_target,
                                     float* tiles_in, float* tiles_target, void* stream) {
  if (!frames0 || !frames1 || !data_shape || !patch_shape || !patch_start || !norm || !tiles_in || !tiles_target || count < 0)
    return fail(DSX_ERR_INVALID, "bad argument");
  if (norm[1] == 0.0 || norm[3] == 0.0 || norm[5] == 0.0) return fail(DSX_ERR_INVALID, "zero standard deviation");
  if (count == 0) return DSX_OK;
  std::vector<int> starts;
  int rc = check_starts(patch_start, tile_ids, count, data_shape, patch_shape, starts);
  if (rc) return rc;
  DevBuf d;
  HIP_TRY(d.upload(starts.data(), starts.size() * 4));
  HIP_TRY(launch_tiles_gather_norm(frames0, frames1, (int)data_shape[1], (int)data_shape[2], (int)patch_shape[1],
                                   (int)patch_shape[2], (const int*)d.p, TileSeq{0, 1, count}, w0, w1, norm,
                                   from_norm_target, tiles_in, tiles_target, (hipStream_t)stream));
  return DSX_OK;
}

// the same for frames with colour planes (data_type 'cifar10'): every argument is checked on the host, on the int64
// values, before anything is uploaded or launched
extern "C" int dsx_tiles_gather_norm_planes(const float* frames0, const float* frames1, const int64_t data_shape[4],
                                            const int64_t patch_hw[2], const int64_t* patch_start, const int64_t* tile_ids,
                                            int64_t count, float w0, float w1, double mean_input, double std_input,
                                            const double* mean_target, const double* std_target, float* tiles_in,
                                            float* tiles_target, void* stream) {
  if (!frames0 || !frames1 || !data_shape || !patch_hw || !patch_start || !mean_target || !std_target || !tiles_in ||
      !tiles_target)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: null argument");
  const int64_t N = data_shape[0], Cc = data_shape[1], H = data_shape[2], W = data_shape[3], ph = patch_hw[0], pw = patch_hw[1];
  if (Cc < 1 || Cc > kPlanesMaxC)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: %lld colour planes, must be in 1..%d", (long long)Cc, kPlanesMaxC);
  if (N < 1 || H < 1 || W < 1 || N > INT32_MAX || H > INT32_MAX || W > INT32_MAX)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: bad frame shape (%lld, %lld, %lld, %lld)", (long long)N, (long long)Cc,
                (long long)H, (long long)W);
  if (ph < 1 || pw < 1 || ph > H || pw > W)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: patch %lld x %lld does not fit the %lld x %lld frames", (long long)ph,
                (long long)pw, (long long)H, (long long)W);
  if (ph * pw > INT32_MAX) return fail(DSX_ERR_INVALID, "gather_norm_planes: patch too large");
  if (!std::isfinite(mean_input) || !std::isfinite(std_input) || std_input == 0.0)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: mean_input / std_input must be finite with non-zero std");
  for (int c = 0; c < 2 * Cc; ++c)
    if (!std::isfinite(mean_target[c]) || !std::isfinite(std_target[c]) || std_target[c] == 0.0)
      return fail(DSX_ERR_INVALID, "gather_norm_planes: statistics of target plane %d must be finite with non-zero std", c);
  if (count < 0 || count > 65535)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: count = %lld, at most 65535 items per call", (long long)count);
  if (count == 0) return DSX_OK;
  std::vector<int> starts((size_t)count * 3);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t id = tile_ids ? tile_ids[i] : i;
    if (id < 0) return fail(DSX_ERR_INVALID, "gather_norm_planes: negative tile id");
    const int64_t n = patch_start[id * 3], y = patch_start[id * 3 + 1], x = patch_start[id * 3 + 2];
    if (n < 0 || n >= N || y < 0 || y > H - ph || x < 0 || x > W - pw)
      return fail(DSX_ERR_INVALID, "gather_norm_planes: item %lld at (%lld, %lld, %lld) lies outside the frames", (long long)i,
                  (long long)n, (long long)y, (long long)x);
    starts[i * 3] = (int)n; starts[i * 3 + 1] = (int)y; starts[i * 3 + 2] = (int)x;
  }
  DevBuf d;
  HIP_TRY(d.upload(starts.data(), starts.size() * 4));
  HIP_TRY(launch_tiles_gather_norm_planes(frames0, frames1, (int)Cc, (int)H, (int)W, (int)ph, (int)pw, (const int*)d.p,
                                          TileSeq{0, 1, count}, w0, w1, mean_input, std_input, mean_target, std_target,
                                          tiles_in, tiles_target, (hipStream_t)stream));
  return DSX_OK;   // ~DevBuf waits for the launch
}

// ---- mixed-input evaluation (the TimePredictor's inputs): host-side argument checks shared by both gather_mix forms
namespace {
static int norm4_ok(const double norm[4]) {
  for (int i = 0; i < 4; ++i)
    if (!std::isfinite(norm[i])) return fail(DSX_ERR_INVALID, "normalisation statistics must be finite");
  if (norm[1] == 0.0 || norm[3] == 0.0) return fail(DSX_ERR_INVALID, "zero standard deviation");
  return DSX_OK;
}
static int mix_weights(double t, const double* lohi, const float* target, const float* mix, const float* cls,
                       MixWeights& mw) {
  if (!target && !mix && !cls) return fail(DSX_ERR_INVALID, "gather_mix: every output pointer is NULL");
  if (!std::isfinite(t)) return fail(DSX_ERR_INVALID, "mixing weight t must be finite");
  mw = MixWeights{(float)(1.0 - t), (float)t, 0.f, 1.f, 0.f, 1.f};
  if (cls) {
    if (!lohi) return fail(DSX_ERR_INVALID, "the classifier view needs the (lo, hi) pairs of its two table rows");
    for (int c = 0; c < 2; ++c) {
      const double lo = lohi[2 * c], hi = lohi[2 * c + 1];
      if (!std::isfinite(lo) || !std::isfinite(hi) || hi - lo == 0.0)
        return fail(DSX_ERR_INVALID, "table row of channel %d: lo and hi must be finite and differ", c);
    }
    mw.lo0 = (float)lohi[0]; mw.rng0 = (float)(lohi[1] - lohi[0]);
    mw.lo1 = (float)lohi[2]; mw.rng1 = (float)(lohi[3] - lohi[2]);
  }
  return DSX_OK;
}
}  // namespace

extern "C" int dsx_tiles_gather_mix(const float* frames0, const float* frames1, const int64_t data_shape[3],
                                    const int64_t patch_shape[3], const int64_t* patch_start, const int64_t* tile_ids,
                                    int64_t count, const double norm[4], double t, const double* lohi, float* target,
                                    float* mix, float* cls, void* stream) {
  MixWeights mw;
  int rc = mix_weights(t, lohi, target, mix, cls, mw);
  if (rc) return rc;
  if (!norm) return fail(DSX_ERR_INVALID, "null argument");
  if ((rc = norm4_ok(norm))) return rc;
  if (!frames0 || !frames1 || !data_shape || !patch_shape || !patch_start || count < 0)
    return fail(DSX_ERR_INVALID, "bad argument");
  if (count > 65535) return fail(DSX_ERR_INVALID, "at most 65535 tiles per call");
  if (count == 0) return DSX_OK;
  std::vector<int> starts;
  if ((rc = check_starts(patch_start, tile_ids, count, data_shape, patch_shape, starts))) return rc;
  DevBuf d;
  HIP_TRY(d.upload(starts.data(), starts.size() * 4));
  HIP_TRY(launch_tiles_gather_mix(frames0, frames1, (int)data_shape[1], (int)data_shape[2], (int)patch_shape[1],
                                  (int)patch_shape[2], (const int*)d.p, TileSeq{0, 1, count}, norm, mw, target, mix, cls,
                                  (hipStream_t)stream));
  return DSX_OK;
}

// one t and one pair of table rows per item; every refusal names the item, and nothing touches the device before the
// last of them has passed.  The records (start + weights) go up in the one table the call uploads.
extern "C" int dsx_tiles_gather_mix_items(const float* frames0, const float* frames1, const int64_t data_shape[3],
                                          const int64_t patch_shape[3], const int64_t* patch_start, int64_t count,
                                          const double norm[4], const double* t_host, const double* lohi_host,
                                          float* target, float* mix, float* cls, void* stream) {
  if (!target && !mix && !cls) return fail(DSX_ERR_INVALID, "gather_mix_items: every output pointer is NULL");
  if (!frames0 || !frames1 || !data_shape || !patch_shape || !patch_start || !norm || !t_host)
    return fail(DSX_ERR_INVALID, "gather_mix_items: null argument");
  if (cls && !lohi_host)
    return fail(DSX_ERR_INVALID, "gather_mix_items: the classifier view needs the (lo, hi) pairs of every item's two table rows");
  int rc = norm4_ok(norm);
  if (rc) return rc;
  const int64_t N = data_shape[0], H = data_shape[1], W = data_shape[2], ph = patch_shape[1], pw = patch_shape[2];
  if (N < 1 || H < 1 || W < 1 || N > INT32_MAX || H > INT32_MAX || W > INT32_MAX)
    return fail(DSX_ERR_INVALID, "gather_mix_items: bad frame shape (%lld, %lld, %lld)", (long long)N, (long long)H, (long long)W);
  if (ph < 1 || pw < 1 || ph > H || pw > W || ph * pw > INT32_MAX)
    return fail(DSX_ERR_INVALID, "gather_mix_items: patch %lld x %lld does not fit the %lld x %lld frames", (long long)ph,
                (long long)pw, (long long)H, (long long)W);
  if (count < 0 || count > 65535)
    return fail(DSX_ERR_INVALID, "gather_mix_items: count = %lld, at most 65535 items per call", (long long)count);
  if (count == 0) return DSX_OK;
  std::vector<MixItem> items((size_t)count);
  for (int64_t i = 0; i < count; ++i) {
    const double t = t_host[i];
    if (!std::isfinite(t)) return fail(DSX_ERR_INVALID, "gather_mix_items: item %lld: mixing weight t must be finite", (long long)i);
    MixWeights mw{(float)(1.0 - t), (float)t, 0.f, 1.f, 0.f, 1.f};
    if (cls) {
      const double* lohi = lohi_host + i * 4;
      for (int c = 0; c < 2; ++c) {
        const double lo = lohi[2 * c], hi = lohi[2 * c + 1];
        if (!std::isfinite(lo) || !std::isfinite(hi) || hi - lo == 0.0)
          return fail(DSX_ERR_INVALID, "gather_mix_items: item %lld: table row of channel %d: lo and hi must be finite and differ",
                      (long long)i, c);
      }
      mw.lo0 = (float)lohi[0]; mw.rng0 = (float)(lohi[1] - lohi[0]);
      mw.lo1 = (float)lohi[2]; mw.rng1 = (float)(lohi[3] - lohi[2]);
    }
    const int64_t n = patch_start[i * 3], y = patch_start[i * 3 + 1], x = patch_start[i * 3 + 2];
    if (n < 0 || n >= N || y < 0 || y > H - ph || x < 0 || x > W - pw)
      return fail(DSX_ERR_INVALID, "gather_mix_items: item %lld at (%lld, %lld, %lld) lies outside the frames", (long long)i,
                  (long long)n, (long long)y, (long long)x);
    items[i] = MixItem{(int)n, (int)y, (int)x, mw};
  }
  DevBuf d;
  HIP_TRY(d.upload(items.data(), items.size() * sizeof(MixItem)));
  HIP_TRY(launch_tiles_gather_mix_items(frames0, frames1, (int)H, (int)W, (int)ph, (int)pw, d.as<MixItem>(), count, norm,
                                        target, mix, cls, (hipStream_t)stream));
  return DSX_OK;   // ~DevBuf waits for the launch
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

// ------------------------------------------------------------------ tile plan with device-resident tables
// One handle per (data, grid, patch, mode): patch starts and valid regions of every tile are uploaded ONCE; every call
// names its tiles as the arithmetic sequence first, first + stride, ... (a rank's shard r, r + W, ... or a batch of
// it) and the kernels index the plan's tables by tile id.  No allocation, copy or synchronisation per call.
struct dsx_tileplan {
  TilePlanner t;
  int64_t total = 0;
  std::vector<int32_t> starts, regions;          // [total][3], [total][8]
  DevBuf d_starts;                               // int, one device allocation: starts, then regions
  int* d_regions = nullptr;                      // (points into d_starts)
  struct Offsets {                               // pack layout for `world` ranks (dsx_tileplan_pack_layout)
    int world = 0;
    std::vector<int64_t> off, rank_pixels;
    DevBuf d_off;                                // long long [total]
  };
  std::vector<Offsets> offs;
};

static void plan_layout(const dsx_tileplan* p, int world, dsx_tileplan::Offsets& o) {
  o.world = world;
  o.off.assign((size_t)p->total, 0);
  o.rank_pixels.assign((size_t)world, 0);
  for (int64_t id = 0; id < p->total; ++id) {    // rank q's run: its tiles q, q + world, ... back to back
    const int q = (int)(id % world);
    o.off[id] = o.rank_pixels[q];
    o.rank_pixels[q] += (int64_t)p->regions[id * 8 + 3] * p->regions[id * 8 + 4];
  }
}

extern "C" int dsx_tileplan_create(const int64_t data_shape[3], const int64_t grid_shape[3], const int64_t patch_shape[3],
                                   int mode, dsx_tileplan** out) {
  if (!out) return fail(DSX_ERR_INVALID, "null argument");
  auto p = std::make_unique<dsx_tileplan>();
  int rc = make_planner(data_shape, grid_shape, patch_shape, mode, p->t);
  if (rc) return rc;
  for (int d = 0; d < 3; ++d)
    if (data_shape[d] >= (1LL << 31)) return fail(DSX_ERR_INVALID, "data extent exceeds 32 bits");
  p->total = p->t.total();
  p->regions.resize((size_t)p->total * 8);
  std::vector<int64_t> ps((size_t)p->total * 3);
  if (p->total) {
    if (dsx_tile_plan(data_shape, grid_shape, patch_shape, mode, nullptr, ps.data(), p->total) < 0) return DSX_ERR_INVALID;
    rc = dsx_tile_regions(data_shape, grid_shape, patch_shape, mode, p->regions.data(), p->total);
    if (rc) return rc;
    const int64_t bad = convert_starts(ps.data(), nullptr, p->total, data_shape, patch_shape, p->starts);
    if (bad >= 0)
      return fail(DSX_ERR_INVALID, "tile %lld lies outside the frames (this tiling mode needs padded frames)", (long long)bad);
    rc = check_regions(p->regions.data(), p->total, data_shape, (int)patch_shape[1], (int)patch_shape[2]);
    if (rc) return rc;
    // stitch_predictions pastes tile after tile (tile_stitcher.py:68-80): where two valid regions overlap -- the
    // shifted last tile of a ragged extent re-covers a strip of the tile before it -- the LATER tile's pixels stay.
    // The device pastes all tiles at once, so the earlier tile's region is clipped to what survives: every canvas
    // pixel is then written exactly once, by the tile the sequential loop leaves there (and is packed only once).
    const int64_t cy = p->t.dim_count(1), cx = p->t.dim_count(2);
    for (int64_t i = 0; i < p->total; ++i) {
      int32_t* r = p->regions.data() + i * 8;
      const int64_t iy = (i / cx) % cy, ix = i % cx;
      if (cy >= 2 && iy == cy - 2) {
        const int32_t* last = p->regions.data() + (i + cx) * 8;          // same frame and column, last row of tiles
        if (last[1] < r[1] + r[3]) r[3] = std::max(0, last[1] - r[1]);
      }
      if (cx >= 2 && ix == cx - 2) {
        const int32_t* last = p->regions.data() + (i + 1) * 8;
        if (last[2] < r[2] + r[4]) r[4] = std::max(0, last[2] - r[2]);
      }
    }
  }
  *out = p.release();
  return DSX_OK;
}
extern "C" void dsx_tileplan_destroy(dsx_tileplan* p) { delete p; }
extern "C" int64_t dsx_tileplan_total(const dsx_tileplan* p) { return p ? p->total : 0; }
// the paste regions the plan's device kernels use (dsx_tile_regions clipped where a later tile overwrites)
extern "C" int dsx_tileplan_regions(const dsx_tileplan* p, int32_t* regions, int64_t capacity) {
  if (!p || !regions) return fail(DSX_ERR_INVALID, "null argument");
  if (capacity < p->total) return fail(DSX_ERR_INVALID, "capacity too small");
  memcpy(regions, p->regions.data(), (size_t)p->total * 32);
  return DSX_OK;
}

// host only: pixel offset of every tile inside its rank's packed run and the pixels of every rank's run
extern "C" int dsx_tileplan_pack_layout(const dsx_tileplan* p, int world, int64_t* off, int64_t* rank_pixels) {
  if (!p || world < 1) return fail(DSX_ERR_INVALID, "bad argument");
  dsx_tileplan::Offsets o;
  plan_layout(p, world, o);
  if (off) memcpy(off, o.off.data(), o.off.size() * 8);
  if (rank_pixels) memcpy(rank_pixels, o.rank_pixels.data(), o.rank_pixels.size() * 8);
  return DSX_OK;
}

static int plan_device(dsx_tileplan* p) {       // first device use: upload the tables (once)
  if (p->d_starts.p || p->total == 0) return DSX_OK;
  const size_t nb = (size_t)p->total * (3 + 8) * 4;
  DevBuf d;
  HIP_TRY(d.alloc(nb));
  int* d_regions = d.as<int>() + p->total * 3;
  hipError_t e = hipMemcpy(d.p, p->starts.data(), (size_t)p->total * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_regions, p->regions.data(), (size_t)p->total * 32, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(DSX_ERR_HIP, "upload of the tile tables failed: %s", hipGetErrorString(e));
  p->d_starts = std::move(d);
  p->d_regions = d_regions;
  return DSX_OK;
}
static int plan_offsets(dsx_tileplan* p, int world, const dsx_tileplan::Offsets** out) {
  for (auto& o : p->offs) if (o.world == world) { *out = &o; return DSX_OK; }
  dsx_tileplan::Offsets o;
  plan_layout(p, world, o);
  if (p->total) {
    HIP_TRY(o.d_off.alloc((size_t)p->total * 8));
    if (hipMemcpy(o.d_off.p, o.off.data(), (size_t)p->total * 8, hipMemcpyHostToDevice) != hipSuccess)
      return fail(DSX_ERR_HIP, "upload of the pack offsets failed");
  }
  p->offs.push_back(std::move(o));
  *out = &p->offs.back();
  return DSX_OK;
}
static int seq_ok(const dsx_tileplan* p, int64_t first, int64_t stride, int64_t count) {
  if (first < 0 || stride < 1 || count < 0) return fail(DSX_ERR_INVALID, "bad tile sequence");
  if (count > 0 && first + (count - 1) * stride >= p->total) return fail(DSX_ERR_INVALID, "tile sequence leaves the plan (%lld tiles)", (long long)p->total);
  if (count > 65535) return fail(DSX_ERR_INVALID, "at most 65535 tiles per call");
  return DSX_OK;
}

extern "C" int dsx_tileplan_gather(dsx_tileplan* p, const float* frames, int64_t first, int64_t stride, int64_t count,
                                   float* tiles, void* stream) {
  if (!p || !frames || !tiles) return fail(DSX_ERR_INVALID, "null argument");
  int rc = seq_ok(p, first, stride, count);
  if (rc || count == 0) return rc;
  if ((rc = plan_device(p))) return rc;
  HIP_TRY(launch_tiles_gather(frames, (int)p->t.D[1], (int)p->t.D[2], (int)p->t.p[1], (int)p->t.p[2], p->d_starts.as<int>(),
                              TileSeq{first, stride, count}, tiles, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_tileplan_gather_norm(dsx_tileplan* p, const float* frames0, const float* frames1, int64_t first,
                                        int64_t stride, int64_t count, float w0, float w1, const double norm[6],
                                        int from_norm_target, float* tiles_in, float* tiles_target, void* stream) {
  if (!p || !frames0 || !frames1 || !norm || !tiles_in || !tiles_target) return fail(DSX_ERR_INVALID, "null argument");
  if (norm[1] == 0.0 || norm[3] == 0.0 || norm[5] == 0.0) return fail(DSX_ERR_INVALID, "zero standard deviation");
  int rc = seq_ok(p, first, stride, count);
  if (rc || count == 0) return rc;
  if ((rc = plan_device(p))) return rc;
  HIP_TRY(launch_tiles_gather_norm(frames0, frames1, (int)p->t.D[1], (int)p->t.D[2], (int)p->t.p[1], (int)p->t.p[2],
                                   p->d_starts.as<int>(), TileSeq{first, stride, count}, w0, w1, norm, from_norm_target, tiles_in,
                                   tiles_target, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_tileplan_gather_mix(dsx_tileplan* p, const float* frames0, const float* frames1, int64_t first,
                                       int64_t stride, int64_t count, const double norm[4], double t, const double* lohi,
                                       float* target, float* mix, float* cls, void* stream) {
  MixWeights mw;
  int rc = mix_weights(t, lohi, target, mix, cls, mw);
  if (rc) return rc;
  if (!p || !frames0 || !frames1 || !norm) return fail(DSX_ERR_INVALID, "null argument");
  if ((rc = norm4_ok(norm))) return rc;
  rc = seq_ok(p, first, stride, count);
  if (rc || count == 0) return rc;
  if ((rc = plan_device(p))) return rc;
  HIP_TRY(launch_tiles_gather_mix(frames0, frames1, (int)p->t.D[1], (int)p->t.D[2], (int)p->t.p[1], (int)p->t.p[2],
                                  p->d_starts.as<int>(), TileSeq{first, stride, count}, norm, mw, target, mix, cls,
                                  (hipStream_t)stream));
  return DSX_OK;
}
// the network input of an input-only stack, kept in its file width: every argument is checked on the host before
// anything touches the device (the refusals need no GPU)
extern "C" int dsx_tileplan_gather_input(dsx_tileplan* p, const void* frames, int pix_type, int64_t first, int64_t stride,
                                         int64_t count, double mean_input, double std_input, double upper_clip,
                                         float* tiles_in, void* stream) {
  if (!p || !frames || !tiles_in) return fail(DSX_ERR_INVALID, "gather_input: null argument");
  if (pix_type != DSX_PIX_U8 && pix_type != DSX_PIX_U16 && pix_type != DSX_PIX_F32)
    return fail(DSX_ERR_INVALID, "gather_input: pixel type %d, must be uint8 (%d), uint16 (%d) or float32 (%d)", pix_type,
                DSX_PIX_U8, DSX_PIX_U16, DSX_PIX_F32);
  if (count < 1 || count > 65535)
    return fail(DSX_ERR_INVALID, "gather_input: count = %lld, must be in 1..65535", (long long)count);
  if (first < 0 || stride < 1 || first >= p->total || (count - 1) > (p->total - 1 - first) / stride)
    return fail(DSX_ERR_INVALID, "gather_input: tiles %lld + k * %lld (%lld of them) leave the plan (%lld tiles)",
                (long long)first, (long long)stride, (long long)count, (long long)p->total);
  if (!std::isfinite(mean_input)) return fail(DSX_ERR_INVALID, "gather_input: mean_input must be finite");
  if (!std::isfinite(std_input) || !(std_input > 0.0))
    return fail(DSX_ERR_INVALID, "gather_input: std_input must be finite and positive");
  if (upper_clip != upper_clip) return fail(DSX_ERR_INVALID, "gather_input: upper_clip is NaN");
  if (p->t.p[1] * p->t.p[2] > INT32_MAX) return fail(DSX_ERR_INVALID, "gather_input: patch too large");
  int rc = plan_device(p);
  if (rc) return rc;
  HIP_TRY(launch_tiles_gather_input(frames, pix_type == DSX_PIX_U8 ? 1 : pix_type == DSX_PIX_U16 ? 2 : 4,
                                    pix_type == DSX_PIX_F32, (int)p->t.D[1], (int)p->t.D[2], (int)p->t.p[1], (int)p->t.p[2],
                                    p->d_starts.as<int>(), TileSeq{first, stride, count}, mean_input, std_input,
                                    upper_clip, tiles_in, (hipStream_t)stream));
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

// paste whole predicted tiles (count, C, ph, pw) of the sequence; gt_canvas != NULL: also the PSNR partial sums
// (count * dsx_stitch_psnr_blocks * C * 8 doubles, as dsx_stitch_psnr)
extern "C" int dsx_tileplan_stitch(dsx_tileplan* p, const float* tiles, int C, int64_t first, int64_t stride, int64_t count,
                                   float* canvas, const float* gt_canvas, double* partials_dev, void* stream) {
  if (!p || !tiles || !canvas || C < 1) return fail(DSX_ERR_INVALID, "bad argument");
  if (gt_canvas && (!partials_dev || C > 4)) return fail(DSX_ERR_INVALID, "PSNR sums need a partials buffer and C <= 4");
  int rc = seq_ok(p, first, stride, count);
  if (rc || count == 0) return rc;
  if ((rc = plan_device(p))) return rc;
  const int ph = (int)p->t.p[1], pw = (int)p->t.p[2];
  const StitchSrc src{tiles, 0, ph, pw, nullptr, 0, 1};
  HIP_TRY(launch_stitch(src, C, p->d_regions, TileSeq{first, stride, count}, canvas, (int)p->t.D[1], (int)p->t.D[2],
                        gt_canvas, partials_dev, dsx_stitch_psnr_blocks(ph, pw), (hipStream_t)stream));
  return DSX_OK;
}
// valid regions of the sequence's predicted tiles -> this rank's packed run (`flat_rank`: the start of the run of rank
// first % world; tiles land at their final offsets, so batches of a shard pack into one buffer independently)
extern "C" int dsx_tileplan_pack(dsx_tileplan* p, const float* tiles, int C, int world, int64_t first, int64_t count,
                                 float* flat_rank, void* stream) {
  if (!p || !tiles || !flat_rank || C < 1 || world < 1) return fail(DSX_ERR_INVALID, "bad argument");
  int rc = seq_ok(p, first, world, count);
  if (rc || count == 0) return rc;
  if ((rc = plan_device(p))) return rc;
  const dsx_tileplan::Offsets* o = nullptr;
  if ((rc = plan_offsets(p, world, &o))) return rc;
  HIP_TRY(launch_tiles_pack(tiles, C, (int)p->t.p[1], (int)p->t.p[2], p->d_regions, o->d_off.as<long long>(), TileSeq{first, world, count},
                            flat_rank, (hipStream_t)stream));
  return DSX_OK;
}
// paste ALL tiles from the gathered exchange buffer [world][rank_stride_elems] (rank q's run at q * rank_stride_elems)
extern "C" int dsx_tileplan_paste_packed(dsx_tileplan* p, const float* flat_all, int C, int world, int64_t rank_stride_elems,
                                         float* canvas, const float* gt_canvas, double* partials_dev, void* stream) {
  if (!p || !flat_all || !canvas || C < 1 || world < 1) return fail(DSX_ERR_INVALID, "bad argument");
  if (gt_canvas && (!partials_dev || C > 4)) return fail(DSX_ERR_INVALID, "PSNR sums need a partials buffer and C <= 4");
  if (p->total == 0) return DSX_OK;
  int rc = seq_ok(p, 0, 1, p->total);
  if (rc) return rc;
  if ((rc = plan_device(p))) return rc;
  const dsx_tileplan::Offsets* o = nullptr;
  if ((rc = plan_offsets(p, world, &o))) return rc;
  for (int q = 0; q < world; ++q)
    if (o->rank_pixels[q] * C > rank_stride_elems) return fail(DSX_ERR_INVALID, "rank stride smaller than rank %d's run", q);
  const int ph = (int)p->t.p[1], pw = (int)p->t.p[2];
  const StitchSrc src{flat_all, 1, ph, pw, o->d_off.as<long long>(), rank_stride_elems, world};
  HIP_TRY(launch_stitch(src, C, p->d_regions, TileSeq{0, 1, p->total}, canvas, (int)p->t.D[1], (int)p->t.D[2], gt_canvas,
                        partials_dev, dsx_stitch_psnr_blocks(ph, pw), (hipStream_t)stream));
  return DSX_OK;
}
