// dsx_lpips.cpp — host side of the LPIPS metric (include/dsx.h, kernels: dsx_lpips.hip): weight validation and
// packing (host only), the workspace, and the two drivers (image pairs, stitched frames in chunks).
#include "dsx_rt.h"

namespace {

struct ConvSpec { const char* key; int cout, cin, ks; };
// AlexNet's feature convs under the key names of lpips.LPIPS.state_dict() (torchvision features.{0,3,6,8,10})
const ConvSpec kConv[5] = {{"net.slice1.0", 64, 3, 11}, {"net.slice2.3", 192, 64, 5}, {"net.slice3.6", 384, 192, 3},
                           {"net.slice4.8", 256, 384, 3}, {"net.slice5.10", 256, 256, 3}};
const int kTapC[5] = {64, 192, 384, 256, 256};

// sizes of every stage for an H x W input
struct Geo {
  int H, W, H1, W1, P1h, P1w, P2h, P2w;
};
int conv1_out(int n) { return (n + 4 - 11) / 4 + 1; }
int pool_out(int n) { return (n - 3) / 2 + 1; }

// output channel held by row i of an N block (dsx_kernels.h)
int row_channel(int i) { return 16 * ((i >> 2) & 1) + (i & 3) + 4 * (i >> 3); }

}  // namespace

struct dsx_lpips {
  std::vector<float> host;         // packed image: conv1..5 weights, 5 biases, 5 lin vectors (floats, 64-float aligned)
  size_t w_off[5], b_off[5], l_off[5];
  DevBuf dev;                      // the same on the device (uploaded at first use)
  DevBuf ws;                       // one workspace per (pairs, H, W)
  int ws_pairs = 0, ws_H = 0, ws_W = 0;
  size_t ws_bytes = 0;
  Geo geo{};                       // of the workspace
  int table_pairs = 0;             // > 0: the workspace holds every stage of one dsx_lpips_forward of that many pairs
  // bump-allocated views into ws
  float *x0 = nullptr, *f1 = nullptr, *p1 = nullptr, *f2 = nullptr, *p2 = nullptr, *f3 = nullptr, *f4 = nullptr, *f5 = nullptr;
  float *mm = nullptr, *mm_part = nullptr;
  double* part = nullptr;
  LpipsTaps taps{};
};

namespace {

int geometry(int H, int W, Geo& g) {
  if (H < 31 || W < 31)
    return fail(DSX_ERR_INVALID, "LPIPS(alex) needs H, W >= 31: below that the second max-pool has no output (got %d x %d)", H, W);
  g.H = H; g.W = W;
  g.H1 = conv1_out(H); g.W1 = conv1_out(W);
  g.P1h = pool_out(g.H1); g.P1w = pool_out(g.W1);
  g.P2h = pool_out(g.P1h); g.P2w = pool_out(g.P1w);
  return DSX_OK;
}

// bytes of the largest tensor of a batch of `pairs` pairs: the kernels index with 32-bit element offsets inside a pixel
// row only, but the planner's 2 GiB refusal is kept for every tensor
int check_sizes(const Geo& g, long long pairs) {
  const long long nimg = 2 * pairs;
  const long long big = std::max((long long)g.H * g.W * 3, (long long)g.H1 * g.W1 * 64) * nimg * 4;
  if (pairs < 1 || nimg > 65535) return fail(DSX_ERR_INVALID, "LPIPS batch of %lld pairs: 1 .. 32767 per call", pairs);
  if (big >= (1ll << 31))
    return fail(DSX_ERR_INVALID, "LPIPS: a tensor of %lld bytes for %lld pairs of %d x %d passes 32-bit byte offsets (2 GiB); "
                "use fewer pairs per call", big, pairs, g.H, g.W);
  return DSX_OK;
}

int ensure_device(dsx_lpips* h) {
  if (h->dev.p) return DSX_OK;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n < 1) {
    (void)hipGetLastError();
    return fail(DSX_ERR_HIP, "no HIP device visible: LPIPS runs on the device only (no CPU fallback)");
  }
  HIP_TRY(h->dev.upload(h->host.data(), h->host.size() * sizeof(float)));
  return DSX_OK;
}

int ensure_workspace(dsx_lpips* h, const Geo& g, int pairs) {
  if (h->ws.p && h->ws_pairs == pairs && h->ws_H == g.H && h->ws_W == g.W) return DSX_OK;
  const size_t nimg = 2 * (size_t)pairs;
  size_t used = 0;
  auto bump = [&](size_t bytes) { const size_t at = used; used += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_x0 = bump(nimg * g.H * g.W * 3 * 4);
  const size_t o_f1 = bump(nimg * g.H1 * g.W1 * 64 * 4);
  const size_t o_p1 = bump(nimg * g.P1h * g.P1w * 64 * 4);
  const size_t o_f2 = bump(nimg * g.P1h * g.P1w * 192 * 4);
  const size_t o_p2 = bump(nimg * g.P2h * g.P2w * 192 * 4);
  const size_t o_f3 = bump(nimg * g.P2h * g.P2w * 384 * 4);
  const size_t o_f4 = bump(nimg * g.P2h * g.P2w * 256 * 4);
  const size_t o_f5 = bump(nimg * g.P2h * g.P2w * 256 * 4);
  const int hw[5] = {g.H1 * g.W1, g.P1h * g.P1w, g.P2h * g.P2w, g.P2h * g.P2w, g.P2h * g.P2w};
  long long rows = 0;
  for (int t = 0; t < 5; ++t) {
    h->taps.off[t] = rows;
    h->taps.nblk[t] = lpips_dist_blocks(hw[t]);
    h->taps.hw[t] = hw[t];
    rows += (long long)pairs * h->taps.nblk[t];
  }
  const size_t o_part = bump((size_t)rows * 8);
  const size_t o_mm = bump(256);
  const size_t o_mmp = bump((size_t)1024 * 2 * 4);   // lpips_minmax_blocks <= 1024
  h->ws_pairs = 0;
  HIP_TRY(h->ws.alloc(used));
  h->ws_bytes = used;
  h->geo = g;
  char* b = (char*)h->ws.p;
  h->x0 = (float*)(b + o_x0); h->f1 = (float*)(b + o_f1); h->p1 = (float*)(b + o_p1); h->f2 = (float*)(b + o_f2);
  h->p2 = (float*)(b + o_p2); h->f3 = (float*)(b + o_f3); h->f4 = (float*)(b + o_f4); h->f5 = (float*)(b + o_f5);
  h->part = (double*)(b + o_part); h->mm = (float*)(b + o_mm); h->mm_part = (float*)(b + o_mmp);
  h->ws_pairs = pairs; h->ws_H = g.H; h->ws_W = g.W;
  return DSX_OK;
}

// trunk + distances of the `n` pairs staged in x0 (n <= ws_pairs) -> out[b_off + b], per_tap[(b_off + b) * 5 + tap]
int run_trunk(dsx_lpips* h, const Geo& g, int n, int b_off, float* out, float* per_tap, hipStream_t st) {
  const float* d = h->dev.as<float>();
  const int nimg = 2 * n;
  LpipsTaps taps = h->taps;            // rows of a tap: n pairs of this call
  long long rows = 0;
  for (int t = 0; t < 5; ++t) { taps.off[t] = rows; rows += (long long)n * taps.nblk[t]; }
  HIP_TRY(launch_lpips_conv1(h->x0, d + h->w_off[0], d + h->b_off[0], h->f1, nimg, g.H, g.W, g.H1, g.W1, st));
  HIP_TRY(launch_lpips_dist(h->f1, n, g.H1 * g.W1, 64, d + h->l_off[0], h->part + taps.off[0], st));
  HIP_TRY(launch_lpips_pool(h->f1, h->p1, nimg, g.H1, g.W1, g.P1h, g.P1w, 64, st));
  HIP_TRY(launch_lpips_conv(5, h->p1, d + h->w_off[1], d + h->b_off[1], h->f2, nimg, g.P1h, g.P1w, 64, 192, st));
  HIP_TRY(launch_lpips_dist(h->f2, n, g.P1h * g.P1w, 192, d + h->l_off[1], h->part + taps.off[1], st));
  HIP_TRY(launch_lpips_pool(h->f2, h->p2, nimg, g.P1h, g.P1w, g.P2h, g.P2w, 192, st));
  HIP_TRY(launch_lpips_conv(3, h->p2, d + h->w_off[2], d + h->b_off[2], h->f3, nimg, g.P2h, g.P2w, 192, 384, st));
  HIP_TRY(launch_lpips_dist(h->f3, n, g.P2h * g.P2w, 384, d + h->l_off[2], h->part + taps.off[2], st));
  HIP_TRY(launch_lpips_conv(3, h->f3, d + h->w_off[3], d + h->b_off[3], h->f4, nimg, g.P2h, g.P2w, 384, 256, st));
  HIP_TRY(launch_lpips_dist(h->f4, n, g.P2h * g.P2w, 256, d + h->l_off[3], h->part + taps.off[3], st));
  HIP_TRY(launch_lpips_conv(3, h->f4, d + h->w_off[4], d + h->b_off[4], h->f5, nimg, g.P2h, g.P2w, 256, 256, st));
  HIP_TRY(launch_lpips_dist(h->f5, n, g.P2h * g.P2w, 256, d + h->l_off[4], h->part + taps.off[4], st));
  HIP_TRY(launch_lpips_finish(h->part, taps, n, b_off, out, per_tap, st));
  return DSX_OK;
}

}  // namespace

// lpips.LPIPS(net='alex') holds torchvision's AlexNet features (five convs) and five 1 x 1 `lin` heads; this packs them
extern "C" int dsx_lpips_create(const float* const* trunk_host, const int64_t* trunk_numel, const float* const* lin_host,
                                const int64_t* lin_numel, dsx_lpips** out) {
  if (!trunk_host || !trunk_numel || !lin_host || !lin_numel || !out) return fail(DSX_ERR_INVALID, "bad argument");
  for (int l = 0; l < 5; ++l) {
    const ConvSpec& s = kConv[l];
    const int64_t wn = (int64_t)s.cout * s.cin * s.ks * s.ks;
    if (!trunk_host[2 * l] || trunk_numel[2 * l] != wn)
      return fail(DSX_ERR_INVALID, "%s.weight: expected (%d, %d, %d, %d) = %lld elements, got %lld", s.key, s.cout, s.cin, s.ks,
                  s.ks, (long long)wn, (long long)trunk_numel[2 * l]);
    if (!trunk_host[2 * l + 1] || trunk_numel[2 * l + 1] != s.cout)
      return fail(DSX_ERR_INVALID, "%s.bias: expected (%d,) elements, got %lld", s.key, s.cout, (long long)trunk_numel[2 * l + 1]);
    if (!lin_host[l] || lin_numel[l] != kTapC[l])
      return fail(DSX_ERR_INVALID, "lin%d.model.1.weight: expected (1, %d, 1, 1) = %d elements, got %lld", l, kTapC[l], kTapC[l],
                  (long long)lin_numel[l]);
  }
  auto h = std::make_unique<dsx_lpips>();
  size_t used = 0;
  auto bump = [&](size_t floats) { const size_t at = used; used += (floats + 63) & ~(size_t)63; return at; };
  h->w_off[0] = bump((size_t)2 * 46 * 64 * 4);
  for (int l = 1; l < 5; ++l) h->w_off[l] = bump((size_t)kConv[l].cout * kConv[l].cin * kConv[l].ks * kConv[l].ks);
  for (int l = 0; l < 5; ++l) h->b_off[l] = bump(kConv[l].cout);
  for (int l = 0; l < 5; ++l) h->l_off[l] = bump(kTapC[l]);
  h->host.assign(used, 0.f);
  {  // conv1: k = (ky * 11 + kx) * 3 + c along the MFMA K dimension, 363 padded to 368 with zero weights
    const float* w = trunk_host[0];
    float* p = h->host.data() + h->w_off[0];
    for (int nb = 0; nb < 2; ++nb)
      for (int g = 0; g < 46; ++g)
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < 4; ++s) {
            const int k = 8 * g + 4 * (lane >> 5) + s, n = nb * 32 + row_channel(lane & 31);
            if (k >= 363) continue;
            const int c = k % 3, kx = (k / 3) % 11, ky = k / 33;
            p[(((size_t)nb * 46 + g) * 64 + lane) * 4 + s] = w[(((size_t)n * 3 + c) * 11 + ky) * 11 + kx];
          }
  }
  for (int l = 1; l < 5; ++l) {
    const ConvSpec& s = kConv[l];
    const int taps = s.ks * s.ks, nchunks = s.cin / 32;
    const float* w = trunk_host[2 * l];
    float* p = h->host.data() + h->w_off[l];
    for (int nb = 0; nb < s.cout / 32; ++nb)
      for (int ck = 0; ck < nchunks; ++ck)
        for (int tap = 0; tap < taps; ++tap)
          for (int g = 0; g < 4; ++g)
            for (int lane = 0; lane < 64; ++lane)
              for (int q = 0; q < 4; ++q) {
                const int c = ck * 32 + 8 * g + 4 * (lane >> 5) + q, n = nb * 32 + row_channel(lane & 31);
                p[(((((size_t)nb * nchunks + ck) * taps + tap) * 4 + g) * 64 + lane) * 4 + q] =
                    w[((size_t)n * s.cin + c) * taps + tap];
              }
  }
  for (int l = 0; l < 5; ++l) {
    std::memcpy(h->host.data() + h->b_off[l], trunk_host[2 * l + 1], (size_t)kConv[l].cout * 4);
    std::memcpy(h->host.data() + h->l_off[l], lin_host[l], (size_t)kTapC[l] * 4);
  }
  *out = h.release();
  return DSX_OK;
}

extern "C" void dsx_lpips_destroy(dsx_lpips* h) { delete h; }

// LPIPS.forward(in0, in1) with normalize=False, spatial=False: (B, 3, H, W) pairs in [-1, 1] -> B values
extern "C" int dsx_lpips_forward(dsx_lpips* h, const float* in0_nchw_dev, const float* in1_nchw_dev, int B, int H, int W,
                                 float* out_dev, float* per_tap_dev, void* stream) {
  if (!h || !in0_nchw_dev || !in1_nchw_dev || !out_dev) return fail(DSX_ERR_INVALID, "bad argument");
  Geo g;
  int rc = geometry(H, W, g);
  if (rc) return rc;
  if ((rc = check_sizes(g, B))) return rc;
  if ((rc = ensure_device(h))) return rc;
  h->table_pairs = 0;
  if ((rc = ensure_workspace(h, g, B))) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch_lpips_input_nchw(in0_nchw_dev, in1_nchw_dev, B, H, W, h->x0, st));
  if ((rc = run_trunk(h, g, B, 0, out_dev, per_tap_dev, st))) return rc;
  h->table_pairs = B;
  return DSX_OK;
}

extern "C" int dsx_lpips_layers(const dsx_lpips* h, dsx_lpips_layer_table* table) {
  if (!h || !table) return fail(DSX_ERR_INVALID, "bad argument");
  if (h->table_pairs < 1 || !h->ws.p)
    return fail(DSX_ERR_INVALID, "LPIPS layer table: the workspace holds no whole forward (call it after dsx_lpips_forward; "
                "dsx_lpips_frames reuses the workspace per chunk)");
  const Geo& g = h->geo;
  const float* stage[DSX_LPIPS_STAGES] = {h->x0, h->f1, h->p1, h->f2, h->p2, h->f3, h->f4, h->f5};
  const int sh[DSX_LPIPS_STAGES] = {g.H, g.H1, g.P1h, g.P1h, g.P2h, g.P2h, g.P2h, g.P2h};
  const int sw[DSX_LPIPS_STAGES] = {g.W, g.W1, g.P1w, g.P1w, g.P2w, g.P2w, g.P2w, g.P2w};
  const int sc[DSX_LPIPS_STAGES] = {3, 64, 64, 192, 192, 384, 256, 256};
  *table = dsx_lpips_layer_table{};
  table->pairs = h->table_pairs;
  table->nimg = 2 * h->table_pairs;
  for (int s = 0; s < DSX_LPIPS_STAGES; ++s) {
    table->H[s] = sh[s]; table->W[s] = sw[s]; table->C[s] = sc[s];
    table->stage[s] = (uint64_t)(uintptr_t)stage[s];
  }
  for (int t = 0; t < 5; ++t) {   // a forward runs ws_pairs pairs: the rows of run_trunk lie where ensure_workspace put them
    table->nblk[t] = h->taps.nblk[t];
    table->hw[t] = h->taps.hw[t];
    table->part[t] = (uint64_t)(uintptr_t)(h->part + h->taps.off[t]);
  }
  return DSX_OK;
}

extern "C" int dsx_lpips_copy_workspace(const dsx_lpips* h, uint64_t src, size_t bytes, void* dst_dev, void* stream) {
  if (!h || !dst_dev) return fail(DSX_ERR_INVALID, "bad argument");
  const uint64_t lo = (uint64_t)(uintptr_t)h->ws.p, hi = lo + h->ws_bytes;
  if (!h->ws.p || src < lo || src > hi || bytes > hi - src) return fail(DSX_ERR_INVALID, "range is not inside the workspace");
  HIP_TRY(hipMemcpyAsync(dst_dev, (const void*)(uintptr_t)src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return DSX_OK;
}

// compute_lpips of the evaluation notebooks for one channel: min-max map with the TARGET channel's range over all N
// frames, three equal channels, one LPIPS value per frame; `chunk` frames per pass (0: as many as fit ~1.5 GiB)
extern "C" int dsx_lpips_frames(dsx_lpips* h, const float* target_nhwc_dev, const float* pred_nhwc_dev, int N, int H, int W,
                                int C, int channel, int chunk, float* out_dev, void* stream) {
  if (!h || !target_nhwc_dev || !pred_nhwc_dev || !out_dev || N < 1 || C < 1 || channel < 0 || channel >= C || chunk < 0)
    return fail(DSX_ERR_INVALID, "bad argument (N >= 1, 0 <= channel < C, chunk >= 0)");
  Geo g;
  int rc = geometry(H, W, g);
  if (rc) return rc;
  if (chunk == 0) {
    const double per_pair = 2.0 * 4 * ((double)H * W * 3 + (double)g.H1 * g.W1 * 64 + (double)g.P1h * g.P1w * 256 +
                                       (double)g.P2h * g.P2w * (192 + 384 + 512));
    chunk = (int)std::max(1.0, std::min((double)N, 1.5 * 1073741824.0 / per_pair));
  }
  if (chunk > N) chunk = N;
  if ((rc = check_sizes(g, chunk))) return rc;
  if ((rc = ensure_device(h))) return rc;
  const long long pixels = (long long)N * H * W;
  h->table_pairs = 0;
  if ((rc = ensure_workspace(h, g, chunk))) return rc;
  hipStream_t st = (hipStream_t)stream;
  HIP_TRY(launch_lpips_minmax(target_nhwc_dev, pixels, C, channel, h->mm_part, h->mm, st));
  const size_t frame = (size_t)H * W * C;
  for (int f = 0; f < N; f += chunk) {
    const int n = std::min(chunk, N - f);
    HIP_TRY(launch_lpips_input_frames(target_nhwc_dev + f * frame, pred_nhwc_dev + f * frame, n, H, W, C, channel, h->mm,
                                      h->x0, st));
    if ((rc = run_trunk(h, g, n, f, out_dev, nullptr, st))) return rc;
  }
  return DSX_OK;
}
