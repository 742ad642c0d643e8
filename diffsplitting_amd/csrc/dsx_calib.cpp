// dsx_calib.cpp — the entry points of the spread calibration: per-bin counts and sums, coverage (dsx_calibration).
// Kernels: dsx_calib.hip.  C ABI and the contract in include/dsx.h.
#include "dsx_rt.h"

static const int64_t kCalMaxN = (int64_t)1 << 40;

static int cal_check_n(int64_t n) {
  if (n < 1 || n > kCalMaxN)
    return fail(DSX_ERR_INVALID, "calibration: n = %lld pixels, must be in 1..2^40", (long long)n);
  return DSX_OK;
}

extern "C" int dsx_calibration_blocks(int64_t n) {
  if (int rc = cal_check_n(n)) return rc;
  return calibration_blocks((long long)n);
}

// everything is checked before any device work; two launches on the caller's stream, nothing synchronised
extern "C" int dsx_calibration(const float* mean_dev, const float* std_dev, const float* target_dev, int64_t n, int C,
                               const double* edges_host, int nbins, const double* z_host, int nz, double* partial_dev,
                               double* out_dev, void* stream) {
  if (!mean_dev || !std_dev || !target_dev || !partial_dev || !out_dev)
    return fail(DSX_ERR_INVALID, "calibration: null argument");
  if (int rc = cal_check_n(n)) return rc;
  if (C < 1 || C > kCalMaxC) return fail(DSX_ERR_INVALID, "calibration: C = %d channels, must be in 1..%d", C, kCalMaxC);
  if (nbins < 1 || nbins > kCalMaxBins)
    return fail(DSX_ERR_INVALID, "calibration: nbins = %d, must be in 1..%d", nbins, kCalMaxBins);
  if (nz < 0 || nz > kCalMaxZ) return fail(DSX_ERR_INVALID, "calibration: nz = %d, must be in 0..%d", nz, kCalMaxZ);
  if ((nbins > 1 && !edges_host) || (nz > 0 && !z_host)) return fail(DSX_ERR_INVALID, "calibration: null argument");
  CalArgs a{};
  const int m = nbins - 1;
  for (int c = 0; c < C; ++c)
    for (int j = 0; j < m; ++j) {
      const double e = edges_host[c * m + j];
      if (!std::isfinite(e)) return fail(DSX_ERR_INVALID, "calibration: edge %d of channel %d is not finite", j, c);
      if (j > 0 && e < edges_host[c * m + j - 1])
        return fail(DSX_ERR_INVALID, "calibration: the edges of channel %d descend at %d (%.17g after %.17g)", c, j, e,
                    edges_host[c * m + j - 1]);
      a.edges[c * m + j] = e;
    }
  for (int k = 0; k < nz; ++k) {
    if (!std::isfinite(z_host[k]) || z_host[k] < 0)
      return fail(DSX_ERR_INVALID, "calibration: z[%d] = %g, must be finite and not negative", k, z_host[k]);
    a.z[k] = z_host[k];
  }
  a.mean = mean_dev; a.sd = std_dev; a.target = target_dev;
  a.elems = (long long)n * C; a.span = calibration_span((long long)n) * C;
  a.C = C; a.nbins = nbins; a.nz = nz;
  a.part = partial_dev; a.out = out_dev;
  const bool vec = a.elems % 4 == 0 && (uintptr_t)mean_dev % 16 == 0 && (uintptr_t)std_dev % 16 == 0 &&
                   (uintptr_t)target_dev % 16 == 0;
  HIP_TRY(launch_calibration(a, vec, (hipStream_t)stream));
  return DSX_OK;
}
