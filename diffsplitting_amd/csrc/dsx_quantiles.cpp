// dsx_quantiles.cpp — the entry point of the per-element quantiles and ranks across a stack of samples
// (dsx_sample_quantiles).  Kernel: dsx_quantiles.hip.  C ABI and the contract in include/dsx.h.
#include "dsx_rt.h"

// do the byte ranges [a, a + na) and [b, b + nb) share a byte?
static bool quant_overlap(const void* a, double na, const void* b, double nb) {
  const double a0 = (double)(uintptr_t)a, b0 = (double)(uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

// everything is checked before any device work; one launch on the caller's stream, nothing synchronised
extern "C" int dsx_sample_quantiles(const float* x_dev, int64_t sample_stride, int n, int64_t count, const double* q_host,
                                    int nq, float* out_dev, const float* target_dev, float* rank_dev, void* stream) {
  if (!x_dev) return fail(DSX_ERR_INVALID, "sample_quantiles: x_dev is NULL");
  if (n < 1 || n > kQuantMaxN) return fail(DSX_ERR_INVALID, "sample_quantiles: n = %d samples, must be in 1..%d", n, kQuantMaxN);
  if (nq < 0 || nq > kQuantMaxQ)
    return fail(DSX_ERR_INVALID, "sample_quantiles: nq = %d quantiles, must be in 0..%d", nq, kQuantMaxQ);
  if ((target_dev == nullptr) != (rank_dev == nullptr))
    return fail(DSX_ERR_INVALID, "sample_quantiles: target_dev and rank_dev are given together, or neither");
  if (nq == 0 && !rank_dev) return fail(DSX_ERR_INVALID, "sample_quantiles: nq = 0 and no rank output: nothing to compute");
  if (nq > 0 && (!q_host || !out_dev)) return fail(DSX_ERR_INVALID, "sample_quantiles: nq = %d needs q_host and out_dev", nq);
  if (count < 1) return fail(DSX_ERR_INVALID, "sample_quantiles: count = %lld elements, must be at least 1", (long long)count);
  if (sample_stride < count)
    return fail(DSX_ERR_INVALID, "sample_quantiles: sample_stride = %lld is below count = %lld", (long long)sample_stride,
                (long long)count);
  QuantArgs a{};
  for (int k = 0; k < nq; ++k) {
    const double q = q_host[k];
    if (!std::isfinite(q) || q < 0.0 || q > 1.0)
      return fail(DSX_ERR_INVALID, "sample_quantiles: q[%d] = %g, must be finite and in [0, 1]", k, q);
    const double pos = (double)(n - 1) * q, lo = std::floor(pos);
    a.lo[k] = (int)lo;
    a.hi[k] = std::min(a.lo[k] + 1, n - 1);
    a.t[k] = pos - lo;
  }
  const double in_bytes = 4.0 * ((double)(n - 1) * (double)sample_stride + (double)count);
  if (nq > 0 && quant_overlap(out_dev, 4.0 * nq * (double)count, x_dev, in_bytes))
    return fail(DSX_ERR_INVALID, "sample_quantiles: out_dev overlaps the samples");
  if (rank_dev && quant_overlap(rank_dev, 4.0 * (double)count, x_dev, in_bytes))
    return fail(DSX_ERR_INVALID, "sample_quantiles: rank_dev overlaps the samples");
  a.x = x_dev; a.stride = sample_stride; a.count = count;
  a.n = n; a.nq = nq;
  a.out = nq > 0 ? out_dev : nullptr; a.target = target_dev; a.rank = rank_dev;
  // the wide path: every base, the stride and the count a multiple of the elements one thread takes
  const int e = quantiles_per_thread(quantiles_wires(n));
  const uintptr_t bases = (uintptr_t)x_dev | (uintptr_t)a.out | (uintptr_t)target_dev | (uintptr_t)rank_dev;
  const bool wide = bases % (4 * e) == 0 && sample_stride % e == 0 && count % e == 0;
  HIP_TRY(launch_quantiles(a, wide, (hipStream_t)stream));
  return DSX_OK;
}
