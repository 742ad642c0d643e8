// dsx_refine.cpp — the entry points of the mixing-time refinement: the centred second moments of plane triples
// (dsx_comoments).  Kernels: dsx_refine.hip.  C ABI and the curve's formulae in include/dsx.h.
#include "dsx_rt.h"

extern "C" int dsx_comoments_blocks(int64_t n) {
  if (n < 1) return fail(DSX_ERR_INVALID, "comoments: n = %lld pixels, must be positive", (long long)n);
  return comoments_blocks((long long)n);
}

// everything is checked before any device work; two launches on the caller's stream, nothing synchronised
extern "C" int dsx_comoments(const float* g, const float* p1, const float* p2, int64_t planes, int64_t n,
                             const int64_t strides[6], double* partial_dev, double* out_dev, void* stream) {
  if (!g || !p1 || !p2 || !strides || !partial_dev || !out_dev) return fail(DSX_ERR_INVALID, "comoments: null argument");
  if (n < 1) return fail(DSX_ERR_INVALID, "comoments: n = %lld pixels, must be positive", (long long)n);
  if (planes < 0 || planes > 65535)
    return fail(DSX_ERR_INVALID, "comoments: %lld planes, must be in 0..65535", (long long)planes);
  static const char* const kName[3] = {"g", "p1", "p2"};
  for (int k = 0; k < 3; ++k) {
    const int64_t ps = strides[2 * k], px = strides[2 * k + 1];
    if (ps < 1 || px < 1)
      return fail(DSX_ERR_INVALID, "comoments: strides of %s = {%lld, %lld}, each must be at least 1", kName[k],
                  (long long)ps, (long long)px);
    if (px > (INT64_MAX - 1) / n) return fail(DSX_ERR_INVALID, "comoments: the pixel stride of %s times n overflows", kName[k]);
    if (planes > 1 && ps < (n - 1) * px + 1)
      return fail(DSX_ERR_INVALID, "comoments: the planes of %s overlap: plane stride %lld, a plane spans %lld elements",
                  kName[k], (long long)ps, (long long)((n - 1) * px + 1));
  }
  if (planes == 0) return DSX_OK;
  ComArgs a{};
  a.g = g; a.p1 = p1; a.p2 = p2;
  a.n = (long long)n; a.span = comoments_span((long long)n);
  bool vec = n % 4 == 0;
  const float* base[3] = {g, p1, p2};
  for (int k = 0; k < 3; ++k) {
    a.stride[2 * k] = strides[2 * k]; a.stride[2 * k + 1] = strides[2 * k + 1];
    vec = vec && strides[2 * k + 1] == 1 && (uintptr_t)base[k] % 16 == 0 && (planes == 1 || strides[2 * k] % 4 == 0);
  }
  a.part = partial_dev; a.out = out_dev;
  HIP_TRY(launch_comoments(a, (int)planes, vec, (hipStream_t)stream));
  return DSX_OK;
}
