// dsx_consistency.cpp — the entry points of the data-consistency pass: residual map, report rows and the conditioned
// mean and spread (dsx_consistency).  Kernels: dsx_consistency.hip.  C ABI and the contract in include/dsx.h.
#include "dsx_rt.h"

static const int64_t kConMaxPlane = (int64_t)1 << 40;

static int con_check_plane(int64_t plane) {
  if (plane < 1 || plane > kConMaxPlane)
    return fail(DSX_ERR_INVALID, "consistency: plane = %lld pixels, must be in 1..2^40", (long long)plane);
  return DSX_OK;
}

extern "C" int dsx_consistency_blocks(int64_t plane) {
  if (int rc = con_check_plane(plane)) return rc;
  return consistency_blocks((long long)plane);
}

namespace {
struct Range { const char* name; uintptr_t lo, hi; };   // [lo, hi) in bytes; lo == 0: not given
bool overlap(const Range& p, const Range& q) { return p.lo && q.lo && p.lo < q.hi && q.lo < p.hi; }
}  // namespace

// everything is checked before any device work; two launches on the caller's stream, nothing synchronised
extern "C" int dsx_consistency(const void* input_dev, int pix, const float* mean_dev, const float* std_dev, int64_t frames,
                               int64_t plane, int C, const double* scale_host, const double* shift_host,
                               const double* weight_host, double clip, double noise_var, float* map_dev,
                               float* out_mean_dev, float* out_std_dev, double* out_dev, double* partial_dev,
                               void* stream) {
  if (!input_dev || !mean_dev || !scale_host || !shift_host || !weight_host)
    return fail(DSX_ERR_INVALID, "consistency: null argument");
  if (frames < 1 || frames > 65535)
    return fail(DSX_ERR_INVALID, "consistency: %lld frames, must be in 1..65535", (long long)frames);
  if (int rc = con_check_plane(plane)) return rc;
  if (C < 1 || C > kConMaxC) return fail(DSX_ERR_INVALID, "consistency: C = %d channels, must be in 1..%d", C, kConMaxC);
  if (pix != DSX_PIX_U8 && pix != DSX_PIX_U16 && pix != DSX_PIX_F32)
    return fail(DSX_ERR_INVALID, "consistency: pix = %d, must be DSX_PIX_U8, DSX_PIX_U16 or DSX_PIX_F32", pix);
  ConArgs a{};
  bool any_w = false;
  for (int c = 0; c < C; ++c) {
    const double s = scale_host[c], b = shift_host[c], w = weight_host[c];
    if (!std::isfinite(s) || !std::isfinite(b) || !std::isfinite(w))
      return fail(DSX_ERR_INVALID, "consistency: scale, shift or weight of channel %d is not finite (%g, %g, %g)", c, s, b, w);
    if (!(s > 0)) return fail(DSX_ERR_INVALID, "consistency: scale[%d] = %g, must be > 0", c, s);
    any_w = any_w || w != 0;
    a.a[c] = s; a.b[c] = b; a.w[c] = w;
  }
  if (!std::isfinite(clip)) return fail(DSX_ERR_INVALID, "consistency: clip = %g is not finite (negative: no clip)", clip);
  if (!std::isfinite(noise_var)) return fail(DSX_ERR_INVALID, "consistency: noise_var = %g is not finite", noise_var);
  if (noise_var < 0) return fail(DSX_ERR_INVALID, "consistency: noise_var = %g, must not be negative", noise_var);
  if (!any_w) return fail(DSX_ERR_INVALID, "consistency: every weight is 0, the observation says nothing");
  if (out_std_dev && !std_dev)
    return fail(DSX_ERR_INVALID, "consistency: out_std_dev without std_dev; there is no spread to condition");
  if (!map_dev && !out_mean_dev && !out_std_dev && !out_dev)
    return fail(DSX_ERR_INVALID, "consistency: no output: give map_dev, out_mean_dev, out_std_dev or out_dev");
  if (out_dev && !partial_dev) return fail(DSX_ERR_INVALID, "consistency: out_dev needs partial_dev");

  const int blocks = consistency_blocks((long long)plane);
  const size_t esz = pix == DSX_PIX_U8 ? 1 : (pix == DSX_PIX_U16 ? 2 : 4);
  const uintptr_t px = (uintptr_t)frames * (uintptr_t)plane, canvas = px * (uintptr_t)C * 4;
  auto range = [](const char* name, const void* p, uintptr_t bytes) { return Range{name, (uintptr_t)p, (uintptr_t)p + bytes}; };
  const Range ins[3] = {range("input_dev", input_dev, px * esz), range("mean_dev", mean_dev, canvas),
                        range("std_dev", std_dev, canvas)};
  const Range outs[5] = {range("map_dev", map_dev, px * 4), range("out_mean_dev", out_mean_dev, canvas),
                         range("out_std_dev", out_std_dev, canvas),
                         range("out_dev", out_dev, (uintptr_t)frames * kConSlots * 8),
                         range("partial_dev", out_dev ? partial_dev : nullptr, (uintptr_t)frames * blocks * kConSlots * 8)};
  for (int o = 0; o < 5; ++o) {
    for (int i = 0; i < 3; ++i) {
      const bool in_place = (o == 1 && i == 1 && out_mean_dev == mean_dev) || (o == 2 && i == 2 && out_std_dev == std_dev);
      if (!in_place && overlap(outs[o], ins[i]))
        return fail(DSX_ERR_INVALID, "consistency: %s overlaps %s (in place means out_mean_dev == mean_dev, "
                    "out_std_dev == std_dev exactly)", outs[o].name, ins[i].name);
    }
    for (int q = o + 1; q < 5; ++q)
      if (overlap(outs[o], outs[q]))
        return fail(DSX_ERR_INVALID, "consistency: %s overlaps %s", outs[o].name, outs[q].name);
  }

  a.in = input_dev; a.mean = mean_dev; a.sd = std_dev;
  a.map = map_dev; a.omean = out_mean_dev; a.osd = out_std_dev;
  a.part = out_dev ? partial_dev : nullptr; a.out = out_dev;
  a.plane = (long long)plane; a.span = consistency_span((long long)plane);
  a.pix = pix; a.C = C;
  a.clip = clip; a.noise_var = noise_var;
  auto aligned = [](const void* p, size_t to) { return (uintptr_t)p % to == 0; };   // a null pointer passes
  const bool vec = plane % 4 == 0 && aligned(input_dev, 4 * esz) && aligned(mean_dev, 16) && aligned(std_dev, 16) &&
                   aligned(map_dev, 16) && aligned(out_mean_dev, 16) && aligned(out_std_dev, 16);
  HIP_TRY(launch_consistency(a, (int)frames, vec, (hipStream_t)stream));
  return DSX_OK;
}
