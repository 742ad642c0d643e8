// dsx_tiles.cpp — tiling: the tile planner (host integer math), the checks and the two geometry makers that every
// gather shares, the per-call gather / stitch forms and the tile plan with device-resident tables.  Kernels:
// dsx_tiles.hip.  C ABI in include/dsx.h.
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

// ------------------------------------------------------------------ what the gather / stitch entry points check
// Each check is stated once.  Every extern "C" gather is its own argument checks, one geom_of_* call and one launch;
// nothing touches the device before the last host check of a call has passed (the refusals need no GPU).
namespace {
// tiles / items of one call: they are the grid's y (or z).  `least` is 0 where an empty call is allowed.
static int count_ok(const char* what, const char* label, int64_t count, int least) {
  if (count >= least && count <= kMaxItemsPerLaunch) return DSX_OK;
  return fail(DSX_ERR_INVALID, "%s: count = %lld, must be in %d..%lld %ss per call", what, (long long)count, least,
              kMaxItemsPerLaunch, label);
}
// (N, H, W) frames within 32 bits and a ph x pw patch that fits them
static int frames_ok(const char* what, int64_t N, int64_t H, int64_t W, int64_t ph, int64_t pw) {
  if (N < 1 || H < 1 || W < 1 || N > INT32_MAX || H > INT32_MAX || W > INT32_MAX)
    return fail(DSX_ERR_INVALID, "%s: bad frame shape (%lld, %lld, %lld)", what, (long long)N, (long long)H, (long long)W);
  if (ph < 1 || pw < 1 || ph > H || pw > W || ph * pw > INT32_MAX)
    return fail(DSX_ERR_INVALID, "%s: patch %lld x %lld does not fit the %lld x %lld frames", what, (long long)ph,
                (long long)pw, (long long)H, (long long)W);
  return DSX_OK;
}
// the one location test, on the int64 values: the ph x pw patch at s = (frame, y, x) lies inside the (N, H, W) frames
static bool inside(int64_t N, int64_t H, int64_t W, int64_t ph, int64_t pw, const int64_t s[3]) {
  return s[0] >= 0 && s[0] < N && s[1] >= 0 && s[1] <= H - ph && s[2] >= 0 && s[2] <= W - pw;
}
static int outside(const char* what, const char* label, int64_t which, const int64_t s[3]) {
  return fail(DSX_ERR_INVALID, "%s: %s %lld at (%lld, %lld, %lld) lies outside the frames", what, label, (long long)which,
              (long long)s[0], (long long)s[1], (long long)s[2]);
}
// The geometry of a per-call form: the rows tile_ids[i] (or i) of the caller's host table patch_start[..] = (frame, y, x)
// are checked and uploaded for the call -- one small allocation and one synchronous copy into `d`, which the caller
// frees on every path (~DevBuf waits for the launch).  `label` is what the caller's rows are, "tile" or "item"; a refusal
// names the row.  The stall-free forms are the dsx_tileplan_* entry points below.  count == 0: OK, nothing else is
// looked at and nothing is uploaded; the caller returns.
static int geom_of_host(const char* what, const char* label, int64_t N, int64_t H, int64_t W, int64_t ph, int64_t pw,
                        const int64_t* patch_start, const int64_t* tile_ids, int64_t count, DevBuf& d, TileGeom& g) {
  int rc = count_ok(what, label, count, 0);
  if (rc || count == 0 || (rc = frames_ok(what, N, H, W, ph, pw))) return rc;
  std::vector<int> starts((size_t)count * 3);
  for (int64_t i = 0; i < count; ++i) {
    const int64_t id = tile_ids ? tile_ids[i] : i;
    if (id < 0) return fail(DSX_ERR_INVALID, "%s: negative tile id", what);
    const int64_t* s = patch_start + id * 3;
    if (!inside(N, H, W, ph, pw, s)) return outside(what, label, id, s);
    for (int k = 0; k < 3; ++k) starts[i * 3 + k] = (int)s[k];
  }
  HIP_TRY(d.upload(starts.data(), starts.size() * 4));
  g = TileGeom{(int)H, (int)W, (int)ph, (int)pw, d.as<int>(), TileSeq{0, 1, count}};
  return DSX_OK;
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
// the mixing weight t and, with a classifier view, the (lo, hi) pairs of its two table rows -> the kernels' weights.
// item >= 0: the refusal names the item; -1: the call has one t
static int mix_weights(const char* what, int64_t item, double t, const double* lohi, bool cls, MixWeights& mw) {
  char who[40] = "";
  if (item >= 0) snprintf(who, sizeof who, "item %lld: ", (long long)item);
  if (!std::isfinite(t)) return fail(DSX_ERR_INVALID, "%s: %smixing weight t must be finite", what, who);
  mw = MixWeights{(float)(1.0 - t), (float)t, 0.f, 1.f, 0.f, 1.f};
  if (!cls) return DSX_OK;
  if (!lohi) return fail(DSX_ERR_INVALID, "%s: the classifier view needs the (lo, hi) pairs of its two table rows", what);
  for (int c = 0; c < 2; ++c) {
    const double lo = lohi[2 * c], hi = lohi[2 * c + 1];
    if (!std::isfinite(lo) || !std::isfinite(hi) || hi - lo == 0.0)
      return fail(DSX_ERR_INVALID, "%s: %stable row of channel %d: lo and hi must be finite and differ", what, who, c);
  }
  mw.lo0 = (float)lohi[0]; mw.rng0 = (float)(lohi[1] - lohi[0]);
  mw.lo1 = (float)lohi[2]; mw.rng1 = (float)(lohi[3] - lohi[2]);
  return DSX_OK;
}
// the one body of dsx_stitch / dsx_stitch_psnr (gt == NULL: plain paste): the caller's host regions go up for the call
static int stitch_host(const char* what, const float* tiles, int64_t count, int C, int ph, int pw, const int32_t* regions,
                       float* canvas, const int64_t data_shape[3], const float* gt, double* partials_dev, void* stream) {
  if (!tiles || !regions || !canvas || !data_shape || C < 1) return fail(DSX_ERR_INVALID, "%s: bad argument", what);
  int rc = count_ok(what, "tile", count, 0);
  if (rc || count == 0 || (rc = check_regions(regions, count, data_shape, ph, pw))) return rc;
  DevBuf d;
  HIP_TRY(d.upload(regions, (size_t)count * 32));
  const StitchSrc src{tiles, 0, ph, pw, nullptr, 0, 1};
  HIP_TRY(launch_stitch(src, C, d.as<int>(), TileSeq{0, 1, count}, canvas, (int)data_shape[1], (int)data_shape[2], gt,
                        partials_dev, dsx_stitch_psnr_blocks(ph, pw), (hipStream_t)stream));
  return DSX_OK;   // ~DevBuf waits for the launch (DevBuf::reset)
}
}  // namespace

extern "C" int dsx_tiles_gather(const float* frames, const int64_t data_shape[3], const int64_t patch_shape[3],
                                const int64_t* patch_start, const int64_t* tile_ids, int64_t count,
                                float* tiles, void* stream) {
  if (!frames || !data_shape || !patch_shape || !patch_start || !tiles) return fail(DSX_ERR_INVALID, "bad argument");
  DevBuf d;
  TileGeom g;
  const int rc = geom_of_host("gather", "tile", data_shape[0], data_shape[1], data_shape[2], patch_shape[1], patch_shape[2],
                              patch_start, tile_ids, count, d, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather(frames, g, tiles, (hipStream_t)stream));
  return DSX_OK;
}

extern "C" int dsx_stitch(const float* tiles, int64_t count, int C, int ph, int pw, const int32_t* regions,
                          float* canvas, const int64_t data_shape[3], void* stream) {
  return stitch_host("stitch", tiles, count, C, ph, pw, regions, canvas, data_shape, nullptr, nullptr, stream);
}
// stitch + RangeInvariantPsnr partial sums in one pass over the tiles (no second pass over the canvas)
extern "C" int dsx_stitch_psnr_blocks(int ph, int pw) {
  int gx = (ph * pw + 255) / 256;
  return gx > 16 ? 16 : (gx < 1 ? 1 : gx);
}
extern "C" int dsx_stitch_psnr(const float* tiles, int64_t count, int C, int ph, int pw, const int32_t* regions,
                               float* canvas, const int64_t data_shape[3], const float* gt_canvas, double* partials_dev,
                               void* stream) {
  if (!gt_canvas || !partials_dev || C > kPsnrMaxC) return fail(DSX_ERR_INVALID, "bad argument (1 <= C <= %d)", kPsnrMaxC);
  return stitch_host("stitch_psnr", tiles, count, C, ph, pw, regions, canvas, data_shape, gt_canvas, partials_dev, stream);
}

// tiles of both channels cut out of device-resident frames AND normalised in the same pass: the batch source of tiled
// prediction without the per-tile host crop + host->device copy of the reference's DataLoader(batch_size = 1)
extern "C" int dsx_tiles_gather_norm(const float* frames0, const float* frames1, const int64_t data_shape[3],
                                     const int64_t patch_shape[3], const int64_t* patch_start, const int64_t* tile_ids,
                                     int64_t count, float w0, float w1, const double norm[6], int from_norm_target,
                                     float* tiles_in, float* tiles_target, void* stream) {
  if (!frames0 || !frames1 || !data_shape || !patch_shape || !patch_start || !norm || !tiles_in || !tiles_target)
    return fail(DSX_ERR_INVALID, "bad argument");
  if (norm[1] == 0.0 || norm[3] == 0.0 || norm[5] == 0.0) return fail(DSX_ERR_INVALID, "zero standard deviation");
  DevBuf d;
  TileGeom g;
  const int rc = geom_of_host("gather_norm", "tile", data_shape[0], data_shape[1], data_shape[2], patch_shape[1],
                              patch_shape[2], patch_start, tile_ids, count, d, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather_norm(frames0, frames1, g, w0, w1, norm, from_norm_target, tiles_in, tiles_target,
                                   (hipStream_t)stream));
  return DSX_OK;
}

// the same for frames with colour planes (data_type 'cifar10')
extern "C" int dsx_tiles_gather_norm_planes(const float* frames0, const float* frames1, const int64_t data_shape[4],
                                            const int64_t patch_hw[2], const int64_t* patch_start, const int64_t* tile_ids,
                                            int64_t count, float w0, float w1, double mean_input, double std_input,
                                            const double* mean_target, const double* std_target, float* tiles_in,
                                            float* tiles_target, void* stream) {
  if (!frames0 || !frames1 || !data_shape || !patch_hw || !patch_start || !mean_target || !std_target || !tiles_in ||
      !tiles_target)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: null argument");
  const int64_t Cc = data_shape[1];
  if (Cc < 1 || Cc > kPlanesMaxC)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: %lld colour planes, must be in 1..%d", (long long)Cc, kPlanesMaxC);
  if (!std::isfinite(mean_input) || !std::isfinite(std_input) || std_input == 0.0)
    return fail(DSX_ERR_INVALID, "gather_norm_planes: mean_input / std_input must be finite with non-zero std");
  for (int c = 0; c < 2 * Cc; ++c)
    if (!std::isfinite(mean_target[c]) || !std::isfinite(std_target[c]) || std_target[c] == 0.0)
      return fail(DSX_ERR_INVALID, "gather_norm_planes: statistics of target plane %d must be finite with non-zero std", c);
  DevBuf d;
  TileGeom g;
  const int rc = geom_of_host("gather_norm_planes", "item", data_shape[0], data_shape[2], data_shape[3], patch_hw[0],
                              patch_hw[1], patch_start, tile_ids, count, d, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather_norm_planes(frames0, frames1, (int)Cc, g, w0, w1, mean_input, std_input, mean_target,
                                          std_target, tiles_in, tiles_target, (hipStream_t)stream));
  return DSX_OK;
}

// ---- mixed-input evaluation (the TimePredictor's inputs)
extern "C" int dsx_tiles_gather_mix(const float* frames0, const float* frames1, const int64_t data_shape[3],
                                    const int64_t patch_shape[3], const int64_t* patch_start, const int64_t* tile_ids,
                                    int64_t count, const double norm[4], double t, const double* lohi, float* target,
                                    float* mix, float* cls, void* stream) {
  if (!target && !mix && !cls) return fail(DSX_ERR_INVALID, "gather_mix: every output pointer is NULL");
  MixWeights mw;
  int rc = mix_weights("gather_mix", -1, t, lohi, cls != nullptr, mw);
  if (rc) return rc;
  if (!norm) return fail(DSX_ERR_INVALID, "null argument");
  if ((rc = norm4_ok(norm))) return rc;
  if (!frames0 || !frames1 || !data_shape || !patch_shape || !patch_start) return fail(DSX_ERR_INVALID, "bad argument");
  DevBuf d;
  TileGeom g;
  rc = geom_of_host("gather_mix", "tile", data_shape[0], data_shape[1], data_shape[2], patch_shape[1], patch_shape[2],
                    patch_start, tile_ids, count, d, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather_mix(frames0, frames1, g, norm, mw, target, mix, cls, (hipStream_t)stream));
  return DSX_OK;
}

// one t and one pair of table rows per item; every refusal names the item.  The records (start + weights) go up in the
// one table the call uploads.
extern "C" int dsx_tiles_gather_mix_items(const float* frames0, const float* frames1, const int64_t data_shape[3],
                                          const int64_t patch_shape[3], const int64_t* patch_start, int64_t count,
                                          const double norm[4], const double* t_host, const double* lohi_host,
                                          float* target, float* mix, float* cls, void* stream) {
  const char* what = "gather_mix_items";
  if (!target && !mix && !cls) return fail(DSX_ERR_INVALID, "gather_mix_items: every output pointer is NULL");
  if (!frames0 || !frames1 || !data_shape || !patch_shape || !patch_start || !norm || !t_host)
    return fail(DSX_ERR_INVALID, "gather_mix_items: null argument");
  if (cls && !lohi_host)
    return fail(DSX_ERR_INVALID, "gather_mix_items: the classifier view needs the (lo, hi) pairs of every item's two table rows");
  int rc = norm4_ok(norm);
  if (rc) return rc;
  const int64_t N = data_shape[0], H = data_shape[1], W = data_shape[2], ph = patch_shape[1], pw = patch_shape[2];
  if ((rc = frames_ok(what, N, H, W, ph, pw)) || (rc = count_ok(what, "item", count, 0)) || count == 0) return rc;
  std::vector<MixItem> items((size_t)count);
  for (int64_t i = 0; i < count; ++i) {
    MixWeights mw;
    if ((rc = mix_weights(what, i, t_host[i], cls ? lohi_host + i * 4 : nullptr, cls != nullptr, mw))) return rc;
    const int64_t* s = patch_start + i * 3;
    if (!inside(N, H, W, ph, pw, s)) return outside(what, "item", i, s);
    items[i] = MixItem{(int)s[0], (int)s[1], (int)s[2], mw};
  }
  DevBuf d;
  HIP_TRY(d.upload(items.data(), items.size() * sizeof(MixItem)));
  const TileGeom g{(int)H, (int)W, (int)ph, (int)pw, nullptr, TileSeq{0, 1, count}};
  HIP_TRY(launch_tiles_gather_mix_items(frames0, frames1, g, d.as<MixItem>(), norm, target, mix, cls, (hipStream_t)stream));
  return DSX_OK;   // ~DevBuf waits for the launch
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
  // blended stitching: per canvas row (first tile row, count), per canvas column (first tile column, count) -- the
  // tiles that cover it are one contiguous index range along each axis -- and the separable window wy[ph], wx[pw]
  std::vector<int32_t> rows, cols;               // [H][2], [W][2]
  bool covers = false;                           // every canvas pixel has a contributor
  int *d_rows = nullptr, *d_cols = nullptr;      // (point into d_starts)
  std::vector<float> window;                     // wy then wx; empty until dsx_tileplan_set_window
  bool window_stale = false;                     // the host window is newer than d_window
  DevBuf d_window;                               // float [ph + pw]
  struct Offsets {                               // pack layout for `world` ranks (dsx_tileplan_pack_layout)
    int world = 0;
    std::vector<int64_t> off, rank_pixels;
    DevBuf d_off;                                // long long [total]
  };
  std::vector<Offsets> offs;
  struct Band {                                  // the near-line masks of one band (dsx_tileplan_crop_lines) on the device
    int band = 0;
    DevBuf d;                                    // uint8 [H + W]: rows, then columns
  };
  std::vector<Band> bands;
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

// Along axis d the patch starts of the tile rows (columns) are s[0] < s[1] < ... (SHIFT: 0, g, 2g, .., D - p), all with
// the same extent, so the tiles that cover coordinate v are one contiguous index range: tab[v] = (first, count).
// False where the starts do not increase strictly or some coordinate has no tile (TRIM leaves a border uncovered).
static bool axis_contributors(const dsx_tileplan* p, int d, std::vector<int32_t>& tab) {
  const int64_t n = p->t.dim_count(d), D = p->t.D[d], ext = p->t.p[d], step = d == 1 ? p->t.dim_count(2) : 1;
  tab.assign((size_t)D * 2, 0);
  bool ok = p->total > 0;
  for (int64_t k = 0; k < n && ok; ++k) {
    const int64_t s = p->starts[(size_t)(k * step) * 3 + d];
    if (k > 0 && s <= p->starts[(size_t)((k - 1) * step) * 3 + d]) ok = false;
    for (int64_t v = s; v < s + ext && ok; ++v) {
      if (tab[v * 2 + 1] == 0) tab[v * 2] = (int32_t)k;
      ++tab[v * 2 + 1];
    }
  }
  for (int64_t v = 0; v < D && ok; ++v) ok = tab[v * 2 + 1] > 0;
  return ok;
}
static void plan_contributors(dsx_tileplan* p) {
  const bool flat = p->t.g[0] == 1 && p->t.p[0] == 1;      // one frame per tile: ids are (frame, tile row, tile column)
  const bool oky = axis_contributors(p, 1, p->rows), okx = axis_contributors(p, 2, p->cols);
  p->covers = flat && oky && okx;
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
    for (int64_t i = 0; i < p->total; ++i)
      if (!inside(data_shape[0], data_shape[1], data_shape[2], patch_shape[1], patch_shape[2], ps.data() + i * 3))
        return fail(DSX_ERR_INVALID, "tile %lld lies outside the frames (this tiling mode needs padded frames)", (long long)i);
    p->starts.assign(ps.begin(), ps.end());      // every value lies inside the frames, whose extents fit 32 bits
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
  plan_contributors(p.get());
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
  const size_t nb = ((size_t)p->total * (3 + 8) + p->rows.size() + p->cols.size()) * 4;
  DevBuf d;
  HIP_TRY(d.alloc(nb));
  int* d_regions = d.as<int>() + p->total * 3;
  int* d_rows = d_regions + p->total * 8;
  int* d_cols = d_rows + p->rows.size();
  hipError_t e = hipMemcpy(d.p, p->starts.data(), (size_t)p->total * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_regions, p->regions.data(), (size_t)p->total * 32, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_rows, p->rows.data(), p->rows.size() * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(d_cols, p->cols.data(), p->cols.size() * 4, hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(DSX_ERR_HIP, "upload of the tile tables failed: %s", hipGetErrorString(e));
  p->d_starts = std::move(d);
  p->d_regions = d_regions;
  p->d_rows = d_rows;
  p->d_cols = d_cols;
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
// The geometry of a plan form: the tiles first + k * stride, k < count, of the plan, whose tables go up on the first
// device use.  The sequence check divides instead of multiplying, so no stride or count overflows it.  count == 0
// (where `least` allows it): OK, nothing is uploaded and `g` is not set; the caller returns.
static int geom_of_plan(const char* what, dsx_tileplan* p, int64_t first, int64_t stride, int64_t count, TileGeom& g,
                        int least = 0) {
  if (!p) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  int rc = count_ok(what, "tile", count, least);
  if (rc) return rc;
  if (first < 0 || stride < 1 || (count > 0 && (first >= p->total || count - 1 > (p->total - 1 - first) / stride)))
    return fail(DSX_ERR_INVALID, "%s: tiles %lld + k * %lld (%lld of them) leave the plan (%lld tiles)", what,
                (long long)first, (long long)stride, (long long)count, (long long)p->total);
  if (count == 0 || (rc = plan_device(p))) return rc;
  g = TileGeom{(int)p->t.D[1], (int)p->t.D[2], (int)p->t.p[1], (int)p->t.p[2], p->d_starts.as<int>(),
               TileSeq{first, stride, count}};
  return DSX_OK;
}

extern "C" int dsx_tileplan_gather(dsx_tileplan* p, const float* frames, int64_t first, int64_t stride, int64_t count,
                                   float* tiles, void* stream) {
  if (!frames || !tiles) return fail(DSX_ERR_INVALID, "null argument");
  TileGeom g;
  const int rc = geom_of_plan("tileplan_gather", p, first, stride, count, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather(frames, g, tiles, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_tileplan_gather_norm(dsx_tileplan* p, const float* frames0, const float* frames1, int64_t first,
                                        int64_t stride, int64_t count, float w0, float w1, const double norm[6],
                                        int from_norm_target, float* tiles_in, float* tiles_target, void* stream) {
  if (!frames0 || !frames1 || !norm || !tiles_in || !tiles_target) return fail(DSX_ERR_INVALID, "null argument");
  if (norm[1] == 0.0 || norm[3] == 0.0 || norm[5] == 0.0) return fail(DSX_ERR_INVALID, "zero standard deviation");
  TileGeom g;
  const int rc = geom_of_plan("tileplan_gather_norm", p, first, stride, count, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather_norm(frames0, frames1, g, w0, w1, norm, from_norm_target, tiles_in, tiles_target,
                                   (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_tileplan_gather_mix(dsx_tileplan* p, const float* frames0, const float* frames1, int64_t first,
                                       int64_t stride, int64_t count, const double norm[4], double t, const double* lohi,
                                       float* target, float* mix, float* cls, void* stream) {
  if (!target && !mix && !cls) return fail(DSX_ERR_INVALID, "gather_mix: every output pointer is NULL");
  MixWeights mw;
  int rc = mix_weights("gather_mix", -1, t, lohi, cls != nullptr, mw);
  if (rc) return rc;
  if (!frames0 || !frames1 || !norm) return fail(DSX_ERR_INVALID, "null argument");
  if ((rc = norm4_ok(norm))) return rc;
  TileGeom g;
  rc = geom_of_plan("tileplan_gather_mix", p, first, stride, count, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather_mix(frames0, frames1, g, norm, mw, target, mix, cls, (hipStream_t)stream));
  return DSX_OK;
}
// the network input of an input-only stack, kept in its file width
extern "C" int dsx_tileplan_gather_input(dsx_tileplan* p, const void* frames, int pix_type, int64_t first, int64_t stride,
                                         int64_t count, double mean_input, double std_input, double upper_clip,
                                         float* tiles_in, void* stream) {
  if (!p || !frames || !tiles_in) return fail(DSX_ERR_INVALID, "gather_input: null argument");
  if (pix_type != DSX_PIX_U8 && pix_type != DSX_PIX_U16 && pix_type != DSX_PIX_F32)
    return fail(DSX_ERR_INVALID, "gather_input: pixel type %d, must be uint8 (%d), uint16 (%d) or float32 (%d)", pix_type,
                DSX_PIX_U8, DSX_PIX_U16, DSX_PIX_F32);
  if (!std::isfinite(mean_input)) return fail(DSX_ERR_INVALID, "gather_input: mean_input must be finite");
  if (!std::isfinite(std_input) || !(std_input > 0.0))
    return fail(DSX_ERR_INVALID, "gather_input: std_input must be finite and positive");
  if (upper_clip != upper_clip) return fail(DSX_ERR_INVALID, "gather_input: upper_clip is NaN");
  if (p->t.p[1] * p->t.p[2] > INT32_MAX) return fail(DSX_ERR_INVALID, "gather_input: patch too large");
  TileGeom g;
  const int rc = geom_of_plan("gather_input", p, first, stride, count, g, 1);
  if (rc) return rc;
  HIP_TRY(launch_tiles_gather_input(frames, pix_type == DSX_PIX_U8 ? 1 : pix_type == DSX_PIX_U16 ? 2 : 4,
                                    pix_type == DSX_PIX_F32, g, mean_input, std_input, upper_clip, tiles_in,
                                    (hipStream_t)stream));
  return DSX_OK;
}

// what every call that names noise fields refuses alike: the field ids of the plan's frames and the draw ordinal
static int field_ids_ok(const char* what, const dsx_tileplan* p, uint64_t id_base, uint32_t draw) {
  const uint64_t frames = (uint64_t)p->t.D[0];
  if (id_base >= DSX_STREAM_ID_LIMIT || id_base + (frames - 1) >= DSX_STREAM_ID_LIMIT)
    return fail(DSX_ERR_INVALID, "%s: id_base = %llu with %llu frames: every field id must be below 2^40", what,
                (unsigned long long)id_base, (unsigned long long)frames);
  if (draw >= DSX_STREAM_DRAW_LIMIT)
    return fail(DSX_ERR_INVALID, "%s: draw ordinal %u, must be below 2^24", what, (unsigned)draw);
  return DSX_OK;
}
// a (C, ph, pw) tile is indexed with 32 bits
static int tile_elems_ok(const char* what, const dsx_tileplan* p, int C) {
  const long long ph = p->t.p[1], pw = p->t.p[2];
  if ((int64_t)C <= INT32_MAX / (ph * pw)) return DSX_OK;
  return fail(DSX_ERR_INVALID, "%s: C * patch = %d * %lld x %lld exceeds 32 bits", what, C, ph, pw);
}

// frame-keyed noise of the sequence's tiles: the crops of the noise field (seed, id_base + frame, draw)
extern "C" int dsx_tileplan_randn(dsx_tileplan* p, int C, int64_t first, int64_t stride, int64_t count, uint64_t seed,
                                  uint64_t id_base, uint32_t draw, float* out_dev, void* stream) {
  const char* what = "tileplan_randn";
  if (!p) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  if (C < 1) return fail(DSX_ERR_INVALID, "%s: C = %d, must be at least 1", what, C);
  if (const int rc = field_ids_ok(what, p, id_base, draw)) return rc;
  if (const int rc = tile_elems_ok(what, p, C)) return rc;
  if (!out_dev && count != 0) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  TileGeom g;
  const int rc = geom_of_plan(what, p, first, stride, count, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_randn(g, C, seed, id_base, draw, out_dev, (hipStream_t)stream));
  return DSX_OK;
}

// paste whole predicted tiles (count, C, ph, pw) of the sequence; gt_canvas != NULL: also the PSNR partial sums
// (count * dsx_stitch_psnr_blocks * C * 8 doubles, as dsx_stitch_psnr)
extern "C" int dsx_tileplan_stitch(dsx_tileplan* p, const float* tiles, int C, int64_t first, int64_t stride, int64_t count,
                                   float* canvas, const float* gt_canvas, double* partials_dev, void* stream) {
  if (!tiles || !canvas || C < 1) return fail(DSX_ERR_INVALID, "bad argument");
  if (gt_canvas && (!partials_dev || C > kPsnrMaxC))
    return fail(DSX_ERR_INVALID, "PSNR sums need a partials buffer and C <= %d", kPsnrMaxC);
  TileGeom g;
  const int rc = geom_of_plan("tileplan_stitch", p, first, stride, count, g);
  if (rc || count == 0) return rc;
  const StitchSrc src{tiles, 0, g.ph, g.pw, nullptr, 0, 1};
  HIP_TRY(launch_stitch(src, C, p->d_regions, g.seq, canvas, g.H, g.W, gt_canvas, partials_dev,
                        dsx_stitch_psnr_blocks(g.ph, g.pw), (hipStream_t)stream));
  return DSX_OK;
}
// valid regions of the sequence's predicted tiles -> this rank's packed run (`flat_rank`: the start of the run of rank
// first % world; tiles land at their final offsets, so batches of a shard pack into one buffer independently)
extern "C" int dsx_tileplan_pack(dsx_tileplan* p, const float* tiles, int C, int world, int64_t first, int64_t count,
                                 float* flat_rank, void* stream) {
  if (!tiles || !flat_rank || C < 1 || world < 1) return fail(DSX_ERR_INVALID, "bad argument");
  TileGeom g;
  int rc = geom_of_plan("tileplan_pack", p, first, world, count, g);
  if (rc || count == 0) return rc;
  const dsx_tileplan::Offsets* o = nullptr;
  if ((rc = plan_offsets(p, world, &o))) return rc;
  HIP_TRY(launch_tiles_pack(tiles, C, g.ph, g.pw, p->d_regions, o->d_off.as<long long>(), g.seq, flat_rank,
                            (hipStream_t)stream));
  return DSX_OK;
}
// paste ALL tiles from the gathered exchange buffer [world][rank_stride_elems] (rank q's run at q * rank_stride_elems)
extern "C" int dsx_tileplan_paste_packed(dsx_tileplan* p, const float* flat_all, int C, int world, int64_t rank_stride_elems,
                                         float* canvas, const float* gt_canvas, double* partials_dev, void* stream) {
  if (!p || !flat_all || !canvas || C < 1 || world < 1) return fail(DSX_ERR_INVALID, "bad argument");
  if (gt_canvas && (!partials_dev || C > kPsnrMaxC))
    return fail(DSX_ERR_INVALID, "PSNR sums need a partials buffer and C <= %d", kPsnrMaxC);
  if (p->total == 0) return DSX_OK;
  TileGeom g;
  int rc = geom_of_plan("tileplan_paste_packed", p, 0, 1, p->total, g);
  if (rc) return rc;
  const dsx_tileplan::Offsets* o = nullptr;
  if ((rc = plan_offsets(p, world, &o))) return rc;
  for (int q = 0; q < world; ++q)
    if (o->rank_pixels[q] * C > rank_stride_elems) return fail(DSX_ERR_INVALID, "rank stride smaller than rank %d's run", q);
  const StitchSrc src{flat_all, 1, g.ph, g.pw, o->d_off.as<long long>(), rank_stride_elems, world};
  HIP_TRY(launch_stitch(src, C, p->d_regions, g.seq, canvas, g.H, g.W, gt_canvas, partials_dev,
                        dsx_stitch_psnr_blocks(g.ph, g.pw), (hipStream_t)stream));
  return DSX_OK;
}

// ------------------------------------------------------------------ blended stitching (contract: include/dsx.h)
extern "C" int dsx_tileplan_contributors(const dsx_tileplan* p, int32_t* rows, int32_t* cols) {
  if (!p || !rows || !cols) return fail(DSX_ERR_INVALID, "tileplan_contributors: null argument");
  if (!p->covers)
    return fail(DSX_ERR_INVALID, "tileplan_contributors: the plan's tiles do not cover the frames (SHIFT tiling of (1, g, g) "
                                 "grids does)");
  memcpy(rows, p->rows.data(), p->rows.size() * 4);
  memcpy(cols, p->cols.data(), p->cols.size() * 4);
  return DSX_OK;
}
extern "C" int dsx_tileplan_set_window(dsx_tileplan* p, const float* wy_host, const float* wx_host) {
  const char* what = "tileplan_set_window";
  if (!p || !wy_host || !wx_host) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  const int64_t ph = p->t.p[1], pw = p->t.p[2];
  for (int64_t i = 0; i < ph + pw; ++i) {
    const float w = i < ph ? wy_host[i] : wx_host[i - ph];
    if (!std::isfinite(w) || !(w > 0.f))
      return fail(DSX_ERR_INVALID, "%s: %s[%lld] = %g: every window value must be finite and > 0", what, i < ph ? "wy" : "wx",
                  (long long)(i < ph ? i : i - ph), (double)w);
  }
  p->window.assign(wy_host, wy_host + ph);
  p->window.insert(p->window.end(), wx_host, wx_host + pw);
  p->window_stale = true;                          // goes up once, at the next blend
  return DSX_OK;
}
extern "C" int dsx_tileplan_blend_blocks(const dsx_tileplan* p) {
  if (!p) return 0;
  const BlendGrid bg = blend_grid(p->t.D[1], p->t.D[2]);
  return bg.segs * bg.rows;
}
// what dsx_tileplan_blend and dsx_tileplan_blend_step refuse alike, on the host alone
// (windowed == false: dsx_tileplan_disagreement, which needs neither a canvas nor a window)
static int blend_checks(const char* what, const dsx_tileplan* p, const float* tiles_dev, int C, int world,
                        int64_t rank_stride_elems, const float* canvas_dev, const float* gt_canvas_dev,
                        const double* partials_dev, bool windowed = true) {
  if (!p || !tiles_dev || (windowed && !canvas_dev)) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  if (C < 1) return fail(DSX_ERR_INVALID, "%s: C = %d, must be at least 1", what, C);
  if (world < 1) return fail(DSX_ERR_INVALID, "%s: world = %d, must be at least 1", what, world);
  if (gt_canvas_dev && (!partials_dev || C > kPsnrMaxC))
    return fail(DSX_ERR_INVALID, "%s: PSNR sums need a partials buffer and C <= %d", what, kPsnrMaxC);
  if (!p->covers)
    return fail(DSX_ERR_INVALID, "%s: the plan's tiles do not cover the frames (SHIFT tiling of (1, g, g) grids does)", what);
  if (windowed && p->window.empty()) return fail(DSX_ERR_INVALID, "%s: the plan has no window: call dsx_tileplan_set_window first", what);
  if (p->t.D[0] > 65535) return fail(DSX_ERR_INVALID, "%s: %lld frames, at most 65535 per plan", what, (long long)p->t.D[0]);
  if (p->total > INT32_MAX) return fail(DSX_ERR_INVALID, "%s: %lld tiles, the tile id must fit 31 bits", what, (long long)p->total);
  if (const int rc = tile_elems_ok(what, p, C)) return rc;
  const int64_t most = (p->total + world - 1) / world;       // tiles of rank 0, the longest slot
  if (world > 1 && (rank_stride_elems < 0 || most > rank_stride_elems / (p->t.p[1] * p->t.p[2] * C)))
    return fail(DSX_ERR_INVALID, "%s: rank_stride_elems = %lld is smaller than rank 0's %lld whole tiles", what,
                (long long)rank_stride_elems, (long long)most);
  return DSX_OK;
}
// the tables and the window on the device (first use), then the one launch of both calls
static int blend_launch(const char* what, dsx_tileplan* p, BlendArgs a, void* stream) {
  int rc = plan_device(p);
  if (rc) return rc;
  if (p->window_stale) {
    if (!p->d_window.p) HIP_TRY(p->d_window.alloc(p->window.size() * 4));
    if (hipMemcpy(p->d_window.p, p->window.data(), p->window.size() * 4, hipMemcpyHostToDevice) != hipSuccess)
      return fail(DSX_ERR_HIP, "%s: upload of the window failed", what);
    p->window_stale = false;
  }
  a.N = (int)p->t.D[0]; a.H = (int)p->t.D[1]; a.W = (int)p->t.D[2]; a.ph = (int)p->t.p[1]; a.pw = (int)p->t.p[2];
  a.ny = (int)p->t.dim_count(1); a.nx = (int)p->t.dim_count(2);
  a.starts = p->d_starts.as<int>(); a.rows = p->d_rows; a.cols = p->d_cols;
  a.wy = p->d_window.as<float>(); a.wx = p->d_window.as<float>() + p->t.p[1];
  HIP_TRY(launch_blend(a, (hipStream_t)stream));
  return DSX_OK;
}
extern "C" int dsx_tileplan_blend(dsx_tileplan* p, const float* tiles_dev, int C, int world, int64_t rank_stride_elems,
                                  float* canvas_dev, const float* gt_canvas_dev, double* partials_dev, void* stream) {
  const char* what = "tileplan_blend";
  const int rc = blend_checks(what, p, tiles_dev, C, world, rank_stride_elems, canvas_dev, gt_canvas_dev, partials_dev);
  if (rc) return rc;
  BlendArgs a{};
  a.tiles = tiles_dev; a.C = C; a.world = world; a.rank_stride = rank_stride_elems;
  a.canvas = canvas_dev; a.gt = gt_canvas_dev; a.part = partials_dev;
  return blend_launch(what, p, a, stream);
}
// the blend as the x0 of one reverse step on the frame state (contract: include/dsx.h)
extern "C" int dsx_tileplan_blend_step(dsx_tileplan* p, const float* x0_tiles_dev, int C, int world,
                                       int64_t rank_stride_elems, float* state_dev, float c_x0, float c_xt, float sigma,
                                       uint64_t seed, uint64_t id_base, uint32_t draw, void* stream) {
  const char* what = "tileplan_blend_step";
  if (const int rc = blend_checks(what, p, x0_tiles_dev, C, world, rank_stride_elems, state_dev, nullptr, nullptr)) return rc;
  if (const int rc = field_ids_ok(what, p, id_base, draw)) return rc;
  if (!std::isfinite(c_x0) || !std::isfinite(c_xt) || !std::isfinite(sigma))
    return fail(DSX_ERR_INVALID, "%s: c_x0 = %g, c_xt = %g, sigma = %g: every coefficient must be finite", what,
                (double)c_x0, (double)c_xt, (double)sigma);
  BlendArgs a{};
  a.tiles = x0_tiles_dev; a.C = C; a.world = world; a.rank_stride = rank_stride_elems;
  a.canvas = state_dev;
  a.step = 1; a.c_x0 = c_x0; a.c_xt = c_xt; a.sigma = sigma; a.seed = seed; a.id_base = id_base; a.draw = draw;
  return blend_launch(what, p, a, stream);
}
// ------------------------------------------------------------------ tile disagreement (contract: include/dsx.h)
// The clipped paste regions partition every frame into nx column ranges times ny row ranges.  Along axis d the range of
// tile row (column) k is that of tile k * step of frame 0; a range the clip emptied owns nothing.  A coordinate v >= 1
// whose owner differs from that of v - 1 is a crop line L, and every v with L - band <= v < L + band is near it.
static void axis_near(const dsx_tileplan* p, int d, int band, uint8_t* near) {
  const int64_t n = p->t.dim_count(d), D = p->t.D[d], step = d == 1 ? p->t.dim_count(2) : 1;
  std::vector<int32_t> owner((size_t)D, -1);
  for (int64_t k = 0; k < n; ++k) {
    const int32_t* r = p->regions.data() + (size_t)(k * step) * 8;
    for (int64_t v = r[d]; v < (int64_t)r[d] + r[2 + d]; ++v) owner[v] = (int32_t)k;
  }
  memset(near, 0, (size_t)D);
  for (int64_t L = 1; L < D; ++L) {
    if (owner[L] == owner[L - 1]) continue;
    for (int64_t v = std::max<int64_t>(0, L - band); v < std::min<int64_t>(D, L + band); ++v) near[v] = 1;
  }
}
static int band_ok(const char* what, int band) {
  if (band >= 1 && band <= 65535) return DSX_OK;
  return fail(DSX_ERR_INVALID, "%s: band = %d, must be in 1..65535", what, band);
}
static int covers_ok(const char* what, const dsx_tileplan* p) {
  if (p->covers) return DSX_OK;
  return fail(DSX_ERR_INVALID, "%s: the plan's tiles do not cover the frames (SHIFT tiling of (1, g, g) grids does)", what);
}
extern "C" int dsx_tileplan_crop_lines(const dsx_tileplan* p, int band, uint8_t* rows, uint8_t* cols) {
  const char* what = "tileplan_crop_lines";
  if (!p || !rows || !cols) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  if (const int rc = band_ok(what, band)) return rc;
  if (const int rc = covers_ok(what, p)) return rc;
  axis_near(p, 1, band, rows);
  axis_near(p, 2, band, cols);
  return DSX_OK;
}
// the masks of `band` on the device: built and uploaded at the first call that names the band, then kept with the plan
static int plan_band(dsx_tileplan* p, int band, const uint8_t** near_y, const uint8_t** near_x) {
  const int64_t H = p->t.D[1], W = p->t.D[2];
  for (auto& b : p->bands)
    if (b.band == band) { *near_y = b.d.as<uint8_t>(); *near_x = b.d.as<uint8_t>() + H; return DSX_OK; }
  std::vector<uint8_t> m((size_t)(H + W));
  axis_near(p, 1, band, m.data());
  axis_near(p, 2, band, m.data() + H);
  dsx_tileplan::Band b;
  b.band = band;
  HIP_TRY(b.d.alloc(m.size()));
  if (hipMemcpy(b.d.p, m.data(), m.size(), hipMemcpyHostToDevice) != hipSuccess)
    return fail(DSX_ERR_HIP, "tileplan_disagreement: upload of the band masks failed");
  p->bands.push_back(std::move(b));
  *near_y = p->bands.back().d.as<uint8_t>();
  *near_x = *near_y + H;
  return DSX_OK;
}
extern "C" int dsx_tileplan_disagreement(dsx_tileplan* p, const float* tiles_dev, int C, int world, int64_t rank_stride_elems,
                                         int band, float* map_dev, double* partials_dev, void* stream) {
  const char* what = "tileplan_disagreement";
  if (!p || !tiles_dev || !partials_dev) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  if (C < 1 || C > kPsnrMaxC) return fail(DSX_ERR_INVALID, "%s: C = %d, must be in 1..%d", what, C, kPsnrMaxC);
  if (const int rc = band_ok(what, band)) return rc;
  if (const int rc = blend_checks(what, p, tiles_dev, C, world, rank_stride_elems, nullptr, nullptr, nullptr, false)) return rc;
  int rc = plan_device(p);
  if (rc) return rc;
  DisagreeArgs a{};
  if ((rc = plan_band(p, band, &a.near_y, &a.near_x))) return rc;
  a.tiles = tiles_dev; a.C = C; a.world = world; a.rank_stride = rank_stride_elems;
  a.N = (int)p->t.D[0]; a.H = (int)p->t.D[1]; a.W = (int)p->t.D[2]; a.ph = (int)p->t.p[1]; a.pw = (int)p->t.p[2];
  a.ny = (int)p->t.dim_count(1); a.nx = (int)p->t.dim_count(2);
  a.starts = p->d_starts.as<int>(); a.rows = p->d_rows; a.cols = p->d_cols;
  a.map = map_dev; a.part = partials_dev;
  HIP_TRY(launch_disagreement(a, (hipStream_t)stream));
  return DSX_OK;
}
// tiles first + k * stride of the plan out of a (N,H,W,C) frame state -> (count, C, ph, pw)
extern "C" int dsx_tileplan_gather_canvas(dsx_tileplan* p, const float* canvas_dev, int C, int64_t first, int64_t stride,
                                          int64_t count, float* tiles_dev, void* stream) {
  const char* what = "tileplan_gather_canvas";
  if (!p) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  if (C < 1) return fail(DSX_ERR_INVALID, "%s: C = %d, must be at least 1", what, C);
  if (const int rc = tile_elems_ok(what, p, C)) return rc;
  if ((!canvas_dev || !tiles_dev) && count != 0) return fail(DSX_ERR_INVALID, "%s: null argument", what);
  TileGeom g;
  const int rc = geom_of_plan(what, p, first, stride, count, g);
  if (rc || count == 0) return rc;
  HIP_TRY(launch_tiles_gather_canvas(canvas_dev, C, g, tiles_dev, (hipStream_t)stream));
  return DSX_OK;
}
