// dsx_select.cpp — frame statistics without a sort: dsx_order_stats drives the radix-select passes of dsx_select.hip
// (one histogram launch per pass, the bin holding the rank chosen on the host from exact integer counts), and
// dsx_frames_to_f32 widens integer frame stacks on the device.  C ABI in include/dsx.h.
#include "dsx_rt.h"

#include <numeric>

namespace {
constexpr int kPasses = 6;
constexpr int kShift[kPasses] = {53, 42, 31, 20, 9, 0};
constexpr int kBits[kPasses] = {11, 11, 11, 11, 11, 9};
}  // namespace

extern "C" size_t dsx_order_stats_workspace_bytes(int64_t count, int n_ranks) {
  (void)count; (void)n_ranks;              // one histogram, whatever the size: no per-element temporary
  return (size_t)kSelectBins * sizeof(unsigned long long);
}

extern "C" int dsx_order_stats(const float* a, const float* b, int64_t count, double w0, double w1, const int64_t* ranks,
                               int n_ranks, double* out, void* workspace, void* stream) {
  if (!a || !ranks || !out || !workspace) return fail(DSX_ERR_INVALID, "order_stats: null argument");
  if (count < 1 || count > (1ll << 40)) return fail(DSX_ERR_INVALID, "order_stats: count = %lld, must be in 1..2^40", (long long)count);
  if (n_ranks < 1 || n_ranks > 4096) return fail(DSX_ERR_INVALID, "order_stats: n_ranks = %d, must be in 1..4096", n_ranks);
  for (int i = 0; i < n_ranks; ++i)
    if (ranks[i] < 0 || ranks[i] >= count)
      return fail(DSX_ERR_INVALID, "order_stats: rank %lld (entry %d) outside [0, %lld)", (long long)ranks[i], i, (long long)count);
  if (b && !(std::isfinite(w0) && std::isfinite(w1))) return fail(DSX_ERR_INVALID, "order_stats: weights must be finite");
  hipStream_t st = (hipStream_t)stream;
  // ranks in ascending order: neighbours share their upper digits, and with them the histograms of those passes
  std::vector<int> order((size_t)n_ranks);
  std::iota(order.begin(), order.end(), 0);
  std::sort(order.begin(), order.end(), [&](int x, int y) { return ranks[x] < ranks[y]; });
  struct Cached { bool valid = false; unsigned long long prefix = 0; std::vector<unsigned long long> h; };
  Cached cache[kPasses];
  for (int k : order) {
    unsigned long long prefix = 0, below = (unsigned long long)ranks[k], inside = (unsigned long long)count;
    for (int p = 0; p < kPasses; ++p) {
      Cached& c = cache[p];
      const int bins = 1 << kBits[p];
      if (!c.valid || c.prefix != prefix) {
        SelectArgs s{a, b, (long long)count, w0, w1, prefix, kShift[p], kBits[p], kShift[p] + kBits[p],
                     (unsigned long long*)workspace};
        c.h.resize((size_t)bins);
        c.valid = false;
        HIP_TRY(hipMemsetAsync(workspace, 0, (size_t)bins * sizeof(unsigned long long), st));
        HIP_TRY(launch_select_hist(s, st));
        HIP_TRY(hipMemcpyAsync(c.h.data(), workspace, (size_t)bins * sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        c.prefix = prefix;
        c.valid = true;
      }
      unsigned long long total = 0;
      for (int i = 0; i < bins; ++i) total += c.h[(size_t)i];
      if (total != inside)                 // every element has exactly one image; NaN keys or frames written meanwhile
        return fail(DSX_ERR_STATE, "order_stats: pass %d counted %llu elements where %llu were expected (inputs changed "
                    "during the call?)", p, total, inside);
      int bin = 0;
      while (below >= c.h[(size_t)bin]) below -= c.h[(size_t)bin++];   // below < total: ends inside the table
      inside = c.h[(size_t)bin];
      prefix = (prefix << kBits[p]) | (unsigned long long)bin;
    }
    const unsigned long long bits = (prefix >> 63) ? prefix ^ 0x8000000000000000ull : ~prefix;
    memcpy(&out[k], &bits, sizeof bits);
  }
  return DSX_OK;
}

extern "C" int dsx_frames_to_f32(const void* src, int src_dtype, int64_t count, double upper_clip, float* dst, void* stream) {
  if (!src || !dst) return fail(DSX_ERR_INVALID, "frames_to_f32: null argument");
  if (src_dtype != DSX_PIX_U8 && src_dtype != DSX_PIX_U16)
    return fail(DSX_ERR_INVALID, "frames_to_f32: source type %d, must be uint8 (%d) or uint16 (%d)", src_dtype, DSX_PIX_U8, DSX_PIX_U16);
  if (count < 1) return fail(DSX_ERR_INVALID, "frames_to_f32: count = %lld, must be positive", (long long)count);
  if (upper_clip != upper_clip) return fail(DSX_ERR_INVALID, "frames_to_f32: upper_clip is NaN");
  HIP_TRY(launch_widen(src, src_dtype == DSX_PIX_U16 ? 2 : 1, (long long)count, upper_clip, dst, (hipStream_t)stream));
  return DSX_OK;
}
