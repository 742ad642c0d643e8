// dsx_resize.cpp — host side of the SR3 image path (include/dsx.h, kernels: dsx_resize.hip): PIL's coefficient
// tables (host only), the resize plan with its tiling and device tables, and the two drivers.
#include "dsx_rt.h"

namespace {

constexpr int kPrecisionBits = 32 - 8 - 2;     // PIL's PRECISION_BITS
constexpr int kLdsBudget = 48 * 1024;          // bytes of LDS a pass may ask for
constexpr long long kMaxImageBytes = (1ll << 31) - 1;

double filter_support(int filter) { return filter == DSX_RESIZE_BILINEAR ? 1.0 : 2.0; }

double bilinear_filter(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}

double bicubic_filter(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}

int check_coeff_args(int in_size, int out_size, int filter) {
  if (in_size < 1 || out_size < 1) return fail(DSX_ERR_INVALID, "resize: sizes must be >= 1 (got %d -> %d)", in_size, out_size);
  if (filter != DSX_RESIZE_BILINEAR && filter != DSX_RESIZE_BICUBIC)
    return fail(DSX_ERR_INVALID, "resize: filter id %d is not DSX_RESIZE_BILINEAR (2) or DSX_RESIZE_BICUBIC (3)", filter);
  return DSX_OK;
}

int coeff_ksize(int in_size, int out_size, int filter) {
  const double scale = (double)in_size / out_size;
  const double support = filter_support(filter) * (scale < 1.0 ? 1.0 : scale);
  return (int)std::ceil(support) * 2 + 1;
}

// precompute_coeffs + normalize_coeffs_8bpc (Resample.c): every intermediate a double rounded on its own, sums in tap
// order.  k holds out_size rows of `cap` ints, zero past a row's n taps.
#pragma clang fp contract(off)
void fill_coeffs(int in_size, int out_size, int filter, int32_t* xmin, int32_t* n, int32_t* k, int cap) {
  const double scale = (double)in_size / out_size;
  const double filterscale = scale < 1.0 ? 1.0 : scale;
  const double support = filter_support(filter) * filterscale;
  const double ss = 1.0 / filterscale;
  std::vector<double> w((size_t)cap);
  for (int xx = 0; xx < out_size; ++xx) {
    const double center = (xx + 0.5) * scale;
    int lo = (int)(center - support + 0.5);
    if (lo < 0) lo = 0;
    int hi = (int)(center + support + 0.5);
    if (hi > in_size) hi = in_size;
    const int cnt = hi - lo;
    double ww = 0.0;
    for (int x = 0; x < cnt; ++x) {
      const double arg = (x + lo - center + 0.5) * ss;
      w[x] = filter == DSX_RESIZE_BILINEAR ? bilinear_filter(arg) : bicubic_filter(arg);
      ww += w[x];
    }
    xmin[xx] = lo;
    n[xx] = cnt;
    int32_t* row = k + (size_t)xx * cap;
    for (int x = 0; x < cap; ++x) row[x] = 0;
    for (int x = 0; x < cnt; ++x) {
      const double v = ww != 0.0 ? w[x] / ww : w[x];
      row[x] = v < 0 ? (int)(-0.5 + v * (1 << kPrecisionBits)) : (int)(0.5 + v * (1 << kPrecisionBits));
    }
  }
}

struct Table {               // one axis
  std::vector<int32_t> xmin, n, k;
  int ksize = 0;
  size_t dev_xmin = 0, dev_n = 0, dev_k = 0;   // int offsets into the plan's device buffer
  void build(int in_size, int out_size, int filter) {
    ksize = coeff_ksize(in_size, out_size, filter);
    xmin.resize(out_size); n.resize(out_size); k.resize((size_t)out_size * ksize);
    fill_coeffs(in_size, out_size, filter, xmin.data(), n.data(), k.data(), ksize);
  }
  // source samples covered by the outputs [first, first + count)
  int span(int first, int count) const { return xmin[first + count - 1] + n[first + count - 1] - xmin[first]; }
  int max_span(int first, int total, int S) const {
    int m = 0;
    for (int s0 = 0; s0 < total; s0 += S) m = std::max(m, span(first + s0, std::min(S, total - s0)));
    return m;
  }
};

struct Tiling { int S = 0, T = 0, pitch = 0, lds = 0; };

int round16(int v) { return (v + 15) & ~15; }

}  // namespace

struct dsx_resize_plan {
  int in_h = 0, in_w = 0, out_h = 0, out_w = 0, top = 0, left = 0, ch = 0, cw = 0, filter = 0, C = 0;
  bool need_h = false, need_v = false;
  int row0 = 0, nrows = 0;       // source rows the horizontal pass makes: what the cropped output rows read
  Table h, v;
  Tiling th, tv;
  DevBuf dev;                    // both tables (uploaded at first use)
};

namespace {

// horizontal: S output columns and T rows per workgroup
int tile_horizontal(dsx_resize_plan* p) {
  const Table& t = p->h;
  int S = std::max(1, std::min({p->cw, 64, 16384 / (t.ksize * 4)}));
  for (;; S = std::max(1, S / 2)) {
    const int tab = resize_tab_bytes(S, t.ksize);
    const int pitch = round16(t.max_span(p->left, p->cw, S) * p->C + 19);
    if (tab + pitch <= kLdsBudget) {
      const int T = std::max(1, std::min({p->nrows, 64, (kLdsBudget - tab) / pitch}));
      p->th = Tiling{S, T, pitch, tab + T * pitch};
      return DSX_OK;
    }
    if (S == 1)
      return fail(DSX_ERR_INVALID, "resize %d -> %d columns: one output's %d taps and source span do not fit %d bytes of LDS",
                  p->in_w, p->out_w, t.ksize, kLdsBudget);
  }
}

// vertical: S output rows and T bytes of every row per workgroup
int tile_vertical(dsx_resize_plan* p) {
  const Table& t = p->v;
  const int wb = p->cw * p->C;
  for (int T = std::min(wb, 128);; T = std::max(16, T / 2)) {
    const int pitch = round16(T + 19);
    for (int S = std::max(1, std::min({p->ch, 32, 16384 / (t.ksize * 4)}));; S = std::max(1, S / 2)) {
      const int tab = resize_tab_bytes(S, t.ksize);
      const long long need = tab + (long long)t.max_span(p->top, p->ch, S) * pitch;
      if (need <= kLdsBudget) {
        p->tv = Tiling{S, T, pitch, (int)need};
        return DSX_OK;
      }
      if (S == 1) break;
    }
    if (T <= 16)
      return fail(DSX_ERR_INVALID, "resize %d -> %d rows: one output's %d taps and source rows do not fit %d bytes of LDS",
                  p->in_h, p->out_h, t.ksize, kLdsBudget);
  }
}

int ensure_device(dsx_resize_plan* p) {
  if (p->dev.p || (!p->need_h && !p->need_v)) return DSX_OK;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return fail(DSX_ERR_HIP, "no HIP device visible: the resize runs on the device only (no CPU fallback)");
  }
  std::vector<int32_t> all;
  auto put = [&](const std::vector<int32_t>& v) { const size_t at = all.size(); all.insert(all.end(), v.begin(), v.end()); return at; };
  for (Table* t : {&p->h, &p->v}) { t->dev_xmin = put(t->xmin); t->dev_n = put(t->n); t->dev_k = put(t->k); }
  HIP_TRY(p->dev.upload(all.data(), all.size() * sizeof(int32_t)));
  return DSX_OK;
}

ResizePassArgs pass_args(const dsx_resize_plan* p, const Table& t, const Tiling& tl, int B) {
  ResizePassArgs a{};
  const int* d = p->dev.as<int>();
  a.xmin = d + t.dev_xmin; a.n = d + t.dev_n; a.k = d + t.dev_k;
  a.ksize = t.ksize; a.C = p->C; a.S = tl.S; a.T = tl.T; a.lds_pitch = tl.pitch; a.lds_bytes = tl.lds; a.B = B;
  return a;
}

}  // namespace

// PIL's precompute_coeffs + normalize_coeffs_8bpc (libImaging/Resample.c) for one axis
extern "C" int dsx_resize_coeffs(int in_size, int out_size, int filter, int32_t* xmin_out, int32_t* n_out, int32_t* k_out,
                                 int cap) {
  int rc = check_coeff_args(in_size, out_size, filter);
  if (rc) return rc;
  const int ksize = coeff_ksize(in_size, out_size, filter);
  if (!xmin_out && !n_out && !k_out) return ksize;
  if (!xmin_out || !n_out || !k_out) return fail(DSX_ERR_INVALID, "resize coefficients: pass all three outputs or none");
  if (cap < ksize) return fail(DSX_ERR_INVALID, "resize coefficients: row capacity %d is below the %d taps needed", cap, ksize);
  fill_coeffs(in_size, out_size, filter, xmin_out, n_out, k_out, cap);
  return ksize;
}

extern "C" int dsx_resize_plan_create(int in_h, int in_w, int out_h, int out_w, int crop_top, int crop_left, int crop_h,
                                      int crop_w, int filter, int C, dsx_resize_plan** out) {
  if (!out) return fail(DSX_ERR_INVALID, "bad argument");
  int rc = check_coeff_args(in_h, out_h, filter);
  if (rc || (rc = check_coeff_args(in_w, out_w, filter))) return rc;
  if (C != 1 && C != 3) return fail(DSX_ERR_INVALID, "resize: C = %d channels, the kernels take 1 or 3", C);
  if (crop_top < 0 || crop_left < 0 || crop_h < 1 || crop_w < 1 || crop_top > out_h - crop_h || crop_left > out_w - crop_w)
    return fail(DSX_ERR_INVALID, "resize: crop window (top %d, left %d, %d x %d) lies outside the resized image %d x %d",
                crop_top, crop_left, crop_h, crop_w, out_h, out_w);
  if ((long long)in_h * in_w * C > kMaxImageBytes || (long long)out_h * out_w * C > kMaxImageBytes)
    return fail(DSX_ERR_INVALID, "resize: an image of %d x %d -> %d x %d x %d bytes passes 32-bit offsets", in_h, in_w, out_h,
                out_w, C);
  auto p = std::make_unique<dsx_resize_plan>();
  p->in_h = in_h; p->in_w = in_w; p->out_h = out_h; p->out_w = out_w;
  p->top = crop_top; p->left = crop_left; p->ch = crop_h; p->cw = crop_w; p->filter = filter; p->C = C;
  p->need_h = in_w != out_w;         // ImagingResample skips a pass that keeps the length
  p->need_v = in_h != out_h;
  p->row0 = crop_top; p->nrows = crop_h;
  if (p->need_v) {
    p->v.build(in_h, out_h, filter);
    p->row0 = p->v.xmin[crop_top];
    p->nrows = p->v.span(crop_top, crop_h);
    if ((rc = tile_vertical(p.get()))) return rc;
  }
  if (p->need_h) {
    p->h.build(in_w, out_w, filter);
    if ((rc = tile_horizontal(p.get()))) return rc;
  }
  *out = p.release();
  return DSX_OK;
}

extern "C" void dsx_resize_plan_destroy(dsx_resize_plan* plan) { delete plan; }

extern "C" size_t dsx_resize_workspace_bytes(const dsx_resize_plan* plan, int B) {
  if (!plan || B < 1 || !(plan->need_h && plan->need_v)) return 0;
  return (size_t)B * plan->nrows * plan->cw * plan->C;
}

// Image.resize((out_w, out_h), filter) then the crop, on B images [B][in_h][in_w][C] -> [B][crop_h][crop_w][C]
extern "C" int dsx_resize_u8(dsx_resize_plan* p, const uint8_t* src_dev, int B, uint8_t* dst_dev, uint8_t* workspace_dev,
                             void* stream) {
  if (!p || !src_dev || !dst_dev) return fail(DSX_ERR_INVALID, "bad argument");
  if (B < 1 || B > 65535) return fail(DSX_ERR_INVALID, "resize: a batch of %d images, 1 .. 65535 per call", B);
  if (p->need_h && p->need_v && !workspace_dev)
    return fail(DSX_ERR_INVALID, "resize: this plan needs a workspace of dsx_resize_workspace_bytes(plan, B) bytes");
  int rc = ensure_device(p);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int C = p->C, src_pitch = p->in_w * C, dst_pitch = p->cw * C;
  const long long src_img = (long long)p->in_h * src_pitch, dst_img = (long long)p->ch * dst_pitch;
  if (!p->need_h && !p->need_v) {      // the image stays: only the crop
    // with every row kept, the rows of the whole batch are one pitch apart: one copy; else image by image
    const int calls = p->ch == p->in_h ? 1 : B;
    const size_t rows = p->ch == p->in_h ? (size_t)B * p->ch : (size_t)p->ch;
    for (int b = 0; b < calls; ++b)
      HIP_TRY(hipMemcpy2DAsync(dst_dev + b * dst_img, (size_t)dst_pitch,
                               src_dev + b * src_img + (size_t)p->top * src_pitch + (size_t)p->left * C, (size_t)src_pitch,
                               (size_t)dst_pitch, rows, hipMemcpyDeviceToDevice, st));
    return DSX_OK;
  }
  if (p->need_h) {
    ResizePassArgs a = pass_args(p, p->h, p->th, B);
    a.src = src_dev + (long long)p->row0 * src_pitch;
    a.src_img = src_img; a.src_pitch = src_pitch;
    a.dst = p->need_v ? workspace_dev : dst_dev;
    a.dst_img = (long long)p->nrows * dst_pitch; a.dst_pitch = dst_pitch;
    a.t0 = p->left; a.n_out = p->cw; a.n_other = p->nrows;
    HIP_TRY(launch_resize_h_u8(a, st));
  }
  if (p->need_v) {
    ResizePassArgs a = pass_args(p, p->v, p->tv, B);
    if (p->need_h) {
      a.src = workspace_dev; a.src_img = (long long)p->nrows * dst_pitch; a.src_pitch = dst_pitch; a.base = p->row0;
    } else {
      a.src = src_dev + (long long)p->left * C; a.src_img = src_img; a.src_pitch = src_pitch; a.base = 0;
    }
    a.dst = dst_dev; a.dst_img = dst_img; a.dst_pitch = dst_pitch;
    a.t0 = p->top; a.n_out = p->ch; a.n_other = dst_pitch;
    HIP_TRY(launch_resize_v_u8(a, st));
  }
  return DSX_OK;
}

// torchvision's ToTensor and the min_max map of transform_augment (data/util.py:74-83)
extern "C" int dsx_u8_to_tensor(const uint8_t* src_dev, int B, int H, int W, int C, float lo, float hi, float* dst_dev,
                                void* stream) {
  if (!src_dev || !dst_dev) return fail(DSX_ERR_INVALID, "bad argument");
  if (B < 1 || H < 1 || W < 1 || (C != 1 && C != 3))
    return fail(DSX_ERR_INVALID, "u8_to_tensor: B %d, H %d, W %d must be >= 1 and C = %d one of 1, 3", B, H, W, C);
  if ((long long)B * (((long long)H * W + 3) / 4) > (1ll << 38))     // 2^31 workgroups of 256 threads, halved
    return fail(DSX_ERR_INVALID, "u8_to_tensor: %d images of %d x %d pass one launch", B, H, W);
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return fail(DSX_ERR_HIP, "no HIP device visible: u8_to_tensor runs on the device only (no CPU fallback)");
  }
  HIP_TRY(launch_u8_to_tensor(src_dev, B, (long long)H * W, C, lo, hi, dst_dev, (hipStream_t)stream));
  return DSX_OK;
}
