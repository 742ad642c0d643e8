// dsx_plan.cpp — the launch planner: the tuning knobs, the per-conv decision (decide_conv), workspace reservation and
// the launches of the per-(B, H, W) plan as plain data (build_plan, run_planner), the plan dump and the host-only dry
// run.  C ABI in include/dsx.h.
#include "dsx_rt.h"

// ------------------------------------------------------------------ planner knobs (PlanKnobs: dsx_rt.h)
// a tile preference list "0,2,3,4"; an empty string keeps `dflt`
static std::vector<int> tile_order(const char* e, const std::vector<int>& dflt) {
  if (!*e) return dflt;
  std::vector<int> v;
  for (const char* p = e; *p;) {
    v.push_back(atoi(p));
    while (*p && *p != ',') ++p;
    if (*p == ',') ++p;
  }
  return v;
}

PlanKnobs dsx::read_plan_knobs() {
  PlanKnobs k;
  static const struct { const char* name; int PlanKnobs::*field; } ints[] = {
      {"DSX_FIRST", &PlanKnobs::first}, {"DSX_IMG", &PlanKnobs::img}, {"DSX_WS", &PlanKnobs::ws},
      {"DSX_WS_1X1", &PlanKnobs::ws_1x1}, {"DSX_WS_MIN_GRID", &PlanKnobs::ws_min_grid}, {"DSX_WS_G2", &PlanKnobs::ws_g2},
      {"DSX_WS_G2_MIN64", &PlanKnobs::ws_g2_min64}, {"DSX_WS_G2_MIN128", &PlanKnobs::ws_g2_min128},
      {"DSX_WS_G4_MIN64", &PlanKnobs::ws_g4_min64}, {"DSX_WS_C4", &PlanKnobs::ws_c4},
      {"DSX_WS_C4_MIN", &PlanKnobs::ws_c4_min}, {"DSX_WS_DIRECT", &PlanKnobs::ws_direct}, {"DSX_WS_MAP3", &PlanKnobs::ws_map3},
      {"DSX_XCD_BANDS", &PlanKnobs::xcd_bands}, {"DSX_HOST_FIN", &PlanKnobs::host_fin},
      {"DSX_PREFETCH", &PlanKnobs::prefetch}, {"DSX_PREFETCH_WS", &PlanKnobs::prefetch_ws},
      {"DSX_FUSE_STATS", &PlanKnobs::fuse_stats}, {"DSX_NARROW_G2", &PlanKnobs::narrow_g2},
      {"DSX_MIN_GRID", &PlanKnobs::min_grid}, {"DSX_SPLITK", &PlanKnobs::splitk}, {"DSX_ATTN_CS", &PlanKnobs::attn_cs},
#ifdef DSX_DIAG
      {"DSX_ABLATE", &PlanKnobs::ablate},
#endif
  };
  static const struct { const char* name; std::vector<int> PlanKnobs::*field; } lists[] = {
      {"DSX_TILES_WIDE", &PlanKnobs::tiles_wide}, {"DSX_TILES_NARROW", &PlanKnobs::tiles_narrow},
      {"DSX_TILES_SLIM", &PlanKnobs::tiles_slim}, {"DSX_TILES_WIDE_SPLIT", &PlanKnobs::tiles_wide_split},
      {"DSX_TILES_NARROW_SPLIT", &PlanKnobs::tiles_narrow_split}, {"DSX_TILES_NARROW_G2", &PlanKnobs::tiles_narrow_g2},
      {"DSX_TILES_WS_WIDE", &PlanKnobs::tiles_ws_wide}, {"DSX_TILES_WS_WIDE_1X1", &PlanKnobs::tiles_ws_wide_1x1},
      {"DSX_TILES_WS_WIDE_1X1_RAW", &PlanKnobs::tiles_ws_wide_1x1_raw}, {"DSX_TILES_WS_NARROW", &PlanKnobs::tiles_ws_narrow},
  };
  for (const auto& e : ints)
    if (const char* v = getenv(e.name)) k.*e.field = atoi(v);
  for (const auto& e : lists)
    if (const char* v = getenv(e.name)) k.*e.field = tile_order(v, k.*e.field);
  const char* impl = getenv("DSX_CONV_IMPL");
  k.conv_naive = impl && !strcmp(impl, "naive");
  if (const char* path = getenv("DSX_PLAN_DUMP")) k.plan_dump = path;
  if (const char* se = getenv("DSX_STAMP_OP")) {
    const char* comma = strchr(se, ',');
    k.stamp_op = atoi(se);
    k.stamp_block = comma ? atoi(comma + 1) : 0;
  }
  return k;
}

hipError_t dsx::launch_op(const PlanOp& o, hipStream_t st) {
  switch (o.launcher) {
    case L_CONV_FIRST: return launch_conv_first(o.dtype, o.args.conv, st);
    case L_CONV_IMG: return launch_conv_img(o.dtype, o.ks, o.args.conv, st);
    case L_CONV_WS: return launch_conv_ws(o.dtype, o.tile, o.ks, o.args.conv, st);
    case L_CONV_MFMA: return launch_conv(o.dtype, o.tile, o.ks, o.stride, o.args.conv, st);
    case L_SPLITK_REDUCE: return launch_splitk_reduce(o.args.reduce, st);
    case L_CONV_NAIVE: return launch_conv_naive(o.args.naive, st);
    case L_CHAN_STATS: {
      const ChanStatsArgs& c = o.args.stats;
      return launch_chan_stats(c.x, c.xbf, c.B, c.HW, c.C, c.nchunk, c.part, st);
    }
    case L_GN_FINALIZE: return launch_gn_finalize(o.args.fin, st);
    case L_ATTN: return launch_attn(o.args.attn, o.col_split != 0, st);
  }
  return hipErrorInvalidValue;
}

// PlanKnobs::plan_dump: one line per PlanOp, the argument struct of its launcher as hex bytes.  The bytes include the
// structs' padding (zero with this compiler, not by the language): compare dumps of builds with one compiler and layout.
static int dump_plan(const dsx_exec* ex) {
  static const struct { const char* name; size_t bytes; } L[] = {
      {"conv_first", sizeof(ConvArgs)}, {"conv_img", sizeof(ConvArgs)}, {"conv_ws", sizeof(ConvArgs)},
      {"conv_mfma", sizeof(ConvArgs)}, {"splitk_reduce", sizeof(SplitKReduceArgs)}, {"conv_naive", sizeof(NaiveConvArgs)},
      {"chan_stats", sizeof(ChanStatsArgs)}, {"gn_finalize", sizeof(GnFinArgs)}, {"attn", sizeof(AttnArgs)}};
  FILE* f = fopen(ex->knobs.plan_dump.c_str(), "w");
  if (!f) return fail(DSX_ERR_INVALID, "DSX_PLAN_DUMP: cannot write %s", ex->knobs.plan_dump.c_str());
  for (size_t i = 0; i < ex->ops.size(); ++i) {
    const PlanOp& o = ex->ops[i];
    // (a finalize launch is named by the kernel its launch rule picks: gn_finalize or gn_finalize_wide)
    const char* name = (o.launcher == L_GN_FINALIZE && gn_finalize_is_wide(o.args.fin)) ? "gn_finalize_wide" : L[o.launcher].name;
    fprintf(f, "%zu kind=%d desc=\"%s\" flops=%.17g bytes=%.17g launcher=%s dtype=%d tile=%d ks=%d stride=%d col_split=%d args=",
            i, o.kind, o.desc.c_str(), o.flops, o.bytes, name, o.dtype, o.tile, o.ks, o.stride, o.col_split);
    const unsigned char* p = (const unsigned char*)&o.args;
    for (size_t b = 0; b < L[o.launcher].bytes; ++b) fprintf(f, "%02x", p[b]);
    fputc('\n', f);
  }
  fclose(f);
  return DSX_OK;
}

// appends a launch to the plan and returns its index (the caller fills in the scalar parameters and `args`)
static int add_op(dsx_exec* ex, int kind, const std::string& desc, double flops, double bytes, Launcher launcher) {
  PlanOp op;
  op.kind = kind; op.desc = desc; op.flops = flops; op.bytes = bytes; op.launcher = launcher;
  ex->ops.push_back(op);
  return (int)ex->ops.size() - 1;
}
static std::string fmt(const char* f, ...) {
  char buf[256];
  va_list ap;
  va_start(ap, f);
  vsnprintf(buf, sizeof buf, f, ap);
  va_end(ap);
  return buf;
}

static char* ws_alloc(dsx_exec* ex, size_t bytes) {
  size_t off = (ex->ws_used + 255) & ~(size_t)255;
  ex->ws_used = off + bytes;
  if (ex->sizing) return nullptr;
  return ex->ws + off;
}
// activations are stored in the MFMA operand type (bf16 build: bf16); `f32` forces fp32 (network output)
static Tensor new_tensor(dsx_exec* ex, int C, int H, int W, bool f32 = false) {
  Tensor t;
  t.C = C; t.H = H; t.W = W;
  t.st = f32 ? 0 : ex->m->dtype;
  t.p = ws_alloc(ex, (size_t)ex->B * H * W * C * t.esz());
  t.id = (int)ex->stats.size();
  ex->stats.push_back(StatInfo());
  return t;
}

static int ilog2(int v) { int l = 0; while ((1 << (l + 1)) <= v) ++l; return l; }
static int pow2_divisor(int v, int cap) {  // largest power of two dividing v, <= cap
  int p = 1;
  while (p * 2 <= cap && v % (p * 2) == 0) p *= 2;
  return p;
}

// geometry of `tile` for this conv (unsplit); false if the tile cannot be used
static bool tile_geometry(int dtype, int tile, int ks, int stride, int ablate, const ConvArgs& a, ConvArgs& c) {
  if (tile < 0 || tile >= TILE_COUNT) return false;
  if (stride == 2 && tile != TILE_64x64) return false;
  const ConvTileInfo ti = conv_tile_info(tile);
  c = a;
  const int TW = pow2_divisor(a.Wo, 16);
  const int TH = pow2_divisor(a.Ho, std::max(1, ti.BM / TW));
  const int TB = ti.BM / (TW * TH);
  if (TB < 1 || TW * TH * TB != ti.BM) return false;
  c.tw_log2 = ilog2(TW); c.th_log2 = ilog2(TH); c.tb_log2 = ilog2(TB);
  c.tiles_x = a.Wo / TW; c.tiles_y = a.Ho / TH;
  c.m_tiles = c.tiles_x * c.tiles_y * ((a.B + TB - 1) / TB);
  c.n_tiles = (c.nblocks * 32 + ti.BN - 1) / ti.BN;
  c.ksplit = 1; c.groups_per_split = a.kchunks / conv_chunk_multiple(ks); c.slab_stride = 0;
  c.lds_row = conv_lds_row(ks, stride, c.tw_log2, conv_chunk_multiple(ks));
  c.ablate = ablate;
  return conv_lds_bytes(dtype, tile, ks, stride, c) != 0;
}

// geometry of `tile` on the two-chunk (cpg = 2) variant of k_conv_mfma: one image per M tile, one N tile, every two
// 64-byte chunks one staged group; false if the tile cannot be used
static bool g2_geometry(int dtype, int tile, const ConvArgs& a, ConvArgs& g) {
  const ConvTileInfo ti = conv_tile_info(tile);
  const int TW = pow2_divisor(a.Wo, 16), TH = pow2_divisor(a.Ho, std::max(1, ti.BM / TW));
  if (TW * TH != ti.BM) return false;
  g = a;
  g.cpg = 2;
  g.tw_log2 = ilog2(TW); g.th_log2 = ilog2(TH); g.tb_log2 = 0;
  g.tiles_x = a.Wo / TW; g.tiles_y = a.Ho / TH;
  g.m_tiles = g.tiles_x * g.tiles_y * a.B;
  g.n_tiles = 1;
  g.ksplit = 1; g.groups_per_split = a.kchunks / 2; g.slab_stride = 0;
  g.lds_row = conv_lds_row(3, 1, g.tw_log2, 2);
  g.ablate = 0;
  return conv_lds_bytes(dtype, tile, 3, 1, g) != 0;
}

namespace {
// Everything a planning decision about one conv may depend on: integers and booleans, no pointer.  Both planner passes
// build the same ConvShape, so they decide alike by construction.
struct ConvShape {
  int B, Hs, Ws, Ho, Wo, C0, C1, Cout, ks, stride;
  bool up, swish, has_gn, has_resid, has_film;
  int resid_ld, out_ld;
  int out_st;              // storage kind of the output
  int kchunks, nblocks;
  bool want_stats;         // a GroupNorm will read the output
  bool may_host_fin;       // plan_res: a residual 1 x 1 conv whose block's second GroupNorm has fused statistics
  bool has_naive;          // the model carries the plain direct-conv weights (read off a pointer of the model, which
                           // is the same in both passes: not a workspace address)
};
enum ConvKernel { CONV_FIRST, CONV_IMG, CONV_WS, CONV_MFMA, CONV_MFMA_G2, CONV_SPLITK, CONV_NAIVE };
enum StatSource { STATS_NONE, STATS_EPILOGUE, STATS_REDUCE };   // who produces the output's GroupNorm partial sums
enum PivotKind { PIVOT_NONE, PIVOT_BIAS, PIVOT_BIAS_FILM };     // what they are shifted by (StatPivot)
// What decide_conv chose.  plan_conv reserves and emits from this alone.
struct ConvChoice {
  ConvKernel kernel;
  int tile;                // TILE_* of the MFMA kernels, -1 otherwise
  ConvArgs geo;            // every pointer member null: the shape, the tile geometry, ws_cpg / lds_row, the split-K
                           // slicing and (CONV_WS) the ws_map / workgroups-per-N / fastdiv block
  StatSource stats;
  int stat_nchunk;         // rows per image of the partial sums
  PivotKind pivot;
  bool gn_in_kernel;       // the kernel finalizes the GroupNorm in front of it (no scale / shift, no finalize launch)
  bool hosts_fin;          // its loader waves run the next GroupNorm finalize
};
}  // namespace

// tile + geometry (+ split-K) of one MFMA conv; returns false if no MFMA config fits.
// Pass 0: the warp-specialised persistent kernel: the widest tile (least re-staging of the activations per output
//         channel) that still gives >= ws_min_grid work items.
// Pass 1: the first tile of the preference list whose plain grid fills the chip.
// Pass 2: small-M layers — the first tile of the split list, K split across workgroups
//         (slabs + a reduce launch) until the grid fills the chip.
// Narrow outputs (<= 32 channels) go to the two-chunk variant of k_conv_mfma first (PlanKnobs::narrow_g2).
static bool decide_tile(const PlanKnobs& k, int dtype, int ks, int stride, bool ws_allowed, ConvArgs& a, int& tile_out) {
  const bool is_wide = a.Cout > 64;
  const int kgroups = a.kchunks / conv_chunk_multiple(ks);
  ConvArgs c;
  const int gw2 = 2 * (dtype != DSX_DTYPE_F32 ? 32 : 16);          // channels per two-chunk group
  if (k.narrow_g2 && ks == 3 && stride == 1 && a.Cout <= 32 && a.stage_mode == 0 && a.kchunks % 2 == 0 &&
      a.C0 % gw2 == 0 && a.C1 % gw2 == 0 && !a.up) {
    for (int tile : k.tiles_narrow_g2)
      if (g2_geometry(dtype, tile, a, c)) { a = c; tile_out = tile; return true; }
  }
  if (ws_allowed) {
    const std::vector<int>& ws_wide =
        ks == 1 ? ((a.has_gn || a.swish) ? k.tiles_ws_wide_1x1 : k.tiles_ws_wide_1x1_raw) : k.tiles_ws_wide;
    for (int tile : (is_wide ? ws_wide : k.tiles_ws_narrow)) {
      if (!tile_geometry(dtype, tile, ks, stride, k.ablate, a, c)) continue;
      if (conv_ws_lds_bytes(dtype, tile, ks, c) == 0) continue;
      if ((long long)c.m_tiles * c.n_tiles >= k.ws_min_grid) { a = c; tile_out = tile; return true; }
    }
  }
  for (int tile : (is_wide ? k.tiles_wide : (a.Cout <= 32 ? k.tiles_slim : k.tiles_narrow))) {
    if (!tile_geometry(dtype, tile, ks, stride, k.ablate, a, c)) continue;
    if ((long long)c.m_tiles * c.n_tiles >= k.min_grid) { a = c; tile_out = tile; return true; }
  }
  int best = -1;
  long long best_eff = -1;
  ConvArgs best_a = a;
  for (int tile : (is_wide ? k.tiles_wide_split : (a.Cout <= 32 ? k.tiles_slim : k.tiles_narrow_split))) {
    if (!tile_geometry(dtype, tile, ks, stride, k.ablate, a, c)) continue;
    const long long grid = (long long)c.m_tiles * c.n_tiles;
    long long eff = grid;
    if (k.splitk && grid < k.min_grid && kgroups >= 4 && (a.Cout % 16) == 0 && a.out_ld == a.Cout) {
      const int want = (int)((k.min_grid + grid - 1) / grid);
      int S = std::min(want, kgroups / 2);  // at least two channel groups per slice
      const int gps = (kgroups + S - 1) / S;
      S = (kgroups + gps - 1) / gps;
      if (S > 1) {
        c.ksplit = S; c.groups_per_split = gps;
        c.slab_stride = (long long)a.B * a.Ho * a.Wo * a.Cout;
        eff = grid * S;
      }
    }
    if (eff > best_eff) { best = tile; best_a = c; best_eff = eff; }
    if (eff >= k.min_grid) break;
  }
  if (best < 0) return false;
  a = best_a;
  tile_out = best;
  return true;
}

// workgroups per N tile of a k_conv_ws launch (whole XCD groups per N tile, see the kernel)
static int ws_wg_per_n(const ConvArgs& a) {
  int wpn = std::min(a.m_tiles, std::max(1, 256 / std::max(1, a.n_tiles)));
  if (a.n_tiles <= 8 && 8 % a.n_tiles == 0) {
    const int unit = 8 / a.n_tiles;
    wpn = std::max(unit, wpn / unit * unit);
    if (wpn > a.m_tiles) wpn = (a.m_tiles + unit - 1) / unit * unit;
  }
  return wpn;
}

// k_conv_ws, chunks per (tile, group) item: several 64-byte chunks where the geometry allows it (PlanKnobs::ws_g2, ws_c4),
// and whether a plain 1 x 1 conv takes the direct row of those chunks (PlanKnobs::ws_direct)
static void decide_ws_chunks(const PlanKnobs& k, int dtype, int ks, int tile, ConvArgs& a) {
  auto take = [&](bool wanted, int cpg) {
    ConvArgs t = a;
    t.ws_cpg = cpg; t.lds_row = conv_lds_row(ks, 1, a.tw_log2, cpg);
    if (wanted && conv_ws_lds_bytes(dtype, tile, ks, t) != 0) { a.ws_cpg = cpg; a.lds_row = t.lds_row; }
  };
  if (ks == 3) {
    const int min_chunks = conv_tile_info(tile).BM == 64 ? k.ws_g2_min64 : k.ws_g2_min128;
    take(k.ws_g2 && a.kchunks >= min_chunks, 2);
    take(k.ws_g2 && a.kchunks >= k.ws_g4_min64, 4);
  }
  if (ks == 1) take(k.ws_c4 && a.kchunks >= k.ws_c4_min, 4);   // 128 input channels per item
  // a plain 1 x 1 conv (no GroupNorm, no Swish in front; whole groups from either source: the staging mode 0 that
  // k_conv_ws requires anyway) takes the direct row of its (type, tile, chunks per item) where one is compiled
  if (ks == 1 && k.ws_direct && !a.has_gn && !a.swish) {
    ConvArgs t = a;
    t.ws_direct = 1;
    if (conv_ws_lds_bytes(dtype, tile, ks, t) != 0) a.ws_direct = 1;
  }
}

// k_conv_ws, blockIdx -> work mapping and its division-free start-up: quotients and fastdiv magics (ConvArgs::ws_map)
static int decide_ws_startup(const PlanKnobs& k, int ks, ConvArgs& w) {
  w.xcd_bands = k.xcd_bands;
  w.ws_wg_per_n = ws_wg_per_n(w);
  // 1 x 1 convs with several N tiles: an XCD takes every N tile of its M tiles (PlanKnobs::ws_map3)
  const bool map3 = k.ws_map3 && ks == 1 && w.n_tiles >= 2 && w.n_tiles <= 32;
  if (map3) {
    int wpn3 = std::max(8, (256 / w.n_tiles) / 8 * 8);
    if (wpn3 > w.m_tiles) wpn3 = (w.m_tiles + 7) / 8 * 8;
    w.ws_wg_per_n = wpn3;
  }
  const int NT = w.n_tiles, wpn = w.ws_wg_per_n, per_img = w.tiles_x * w.tiles_y;
  w.ws_map = map3 ? 3 : ((NT <= 8 && 8 % NT == 0 && wpn % (8 / NT) == 0) ? 0 : ((NT % 8) == 0 ? 1 : 2));
  w.ws_nt_log2 = NT <= 8 ? ilog2(NT) : 0;
  w.ws_per = map3 ? NT : (NT >> 3);
  w.ws_adv_x = wpn % w.tiles_x; w.ws_adv_y = (wpn / w.tiles_x) % w.tiles_y; w.ws_adv_b = wpn / per_img;
  const int PW = ((1 << w.tw_log2) - 1) + ks;                       // stride 1
  const int upg = 4 * (w.ws_cpg ? w.ws_cpg : conv_chunk_multiple(ks));   // 16-byte units per pixel and group
  const int pstep = 256 / upg;                                      // loader threads / units per pixel
  w.ws_dpy = pstep / PW; w.ws_dpx = pstep - w.ws_dpy * PW;
  w.mg_tiles_x = fastdiv_magic((unsigned)w.tiles_x); w.mg_per_img = fastdiv_magic((unsigned)per_img);
  w.mg_pw = fastdiv_magic((unsigned)PW); w.mg_wpn = fastdiv_magic((unsigned)wpn);
  w.mg_per = fastdiv_magic((unsigned)std::max(1, w.ws_per));
  w.ws_bigdiv = ((long long)w.m_tiles + wpn >= 65536 || w.tiles_x >= 65536 || per_img >= 65536) ? 1 : 0;
  // the magics are exact for dividends below 65536; check the ones this launch can produce (a few thousand
  // multiplications per conv at plan time) rather than trust the bound
  auto exact = [](unsigned d, unsigned magic, unsigned nmax) {
    for (unsigned n = 0; n <= nmax; ++n) {
      const unsigned q = magic ? (unsigned)(((unsigned long long)n * magic) >> 32) : n;
      if (q != n / d) return false;
    }
    return true;
  };
  const unsigned grid = (unsigned)(NT * wpn);
  const unsigned nt_max = w.ws_bigdiv ? 0u : (unsigned)(w.m_tiles + wpn);
  if (!exact((unsigned)w.tiles_x, w.mg_tiles_x, grid) || !exact((unsigned)per_img, w.mg_per_img, grid) ||
      !exact((unsigned)PW, w.mg_pw, 255u) || !exact((unsigned)wpn, w.mg_wpn, std::max(grid, nt_max)) ||
      !exact((unsigned)std::max(1, w.ws_per), w.mg_per, grid >> 3))
    return fail(DSX_ERR_INVALID, "planner: fastdiv magic not exact for conv %dx%d @%dx%d", ks, ks, w.Ho, w.Wo);
  return DSX_OK;
}

// Every decision about one conv, from its shape alone: kernel family, tile and geometry, where the GroupNorm statistics
// of its output come from, who finalizes the GroupNorm in front of it, whether it hosts the next finalize.  It sees no
// executor, tensor or device address (the geometry helpers get a ConvArgs whose pointers are all null), so the sizing
// pass and the planning pass cannot decide differently.
static int decide_conv(const PlanKnobs& k, int dtype, int norm_groups, const ConvShape& s, ConvChoice& ch) {
  ch = ConvChoice{};
  ch.tile = -1;
  ConvArgs& a = ch.geo;
  a.C0 = s.C0; a.C1 = s.C1;
  a.B = s.B; a.Hs = s.Hs; a.Ws = s.Ws; a.up = s.up ? 1 : 0;
  a.Ho = s.Ho; a.Wo = s.Wo;
  a.swish = s.swish ? 1 : 0;
  a.has_gn = s.has_gn ? 1 : 0;
  a.act_bf16 = dtype;   // storage kind of the sources / residual
  a.out_bf16 = s.out_st;
  {
    const int gw = conv_chunk_multiple(s.ks) * (dtype != 0 ? 32 : 16);  // channels per staged group
    const int um = dtype != 0 ? 7 : 3;                                   // channels per 16-byte unit - 1
    a.stage_mode = ((a.C0 & um) || (a.C1 & um)) ? 2 : ((a.C1 == 0 || a.C0 % gw == 0) ? 0 : 1);
  }
  a.resid_ld = s.resid_ld; a.out_ld = s.out_ld; a.Cout = s.Cout;
  a.nblocks = s.nblocks; a.kchunks = s.kchunks;
  const int ks = s.ks, stride = s.stride;
  // ---- the UNet's first conv (few input channels): im2col-in-K kernel.  (Preserved: this used to test the FiLM
  // pointer, which is null while sizing; has_film is what the planning pass saw.)
  if (!k.conv_naive && k.first && !s.has_film && !s.has_resid && conv_first_applicable(ks, stride, a, s.has_gn)) {
    ch.kernel = CONV_FIRST;
    if (s.want_stats) { ch.stats = STATS_EPILOGUE; ch.stat_nchunk = (a.Ho >> 4) * (a.Wo >> 4) * 4; ch.pivot = PIVOT_BIAS; }   // the kernel sums x - bias
    return DSX_OK;
  }
  // ---- 8 x 8 maps: the image-resident kernel (GroupNorm finalised in its prologue, statistics in its epilogue).
  // (Preserved: conv_img_applicable tests `a.resid && (a.resid_ld & 3)` on a pointer that is null here; has_resid
  // stands for it, as the planning pass saw it.)
  if (!k.conv_naive && k.img && !(s.has_resid && (s.resid_ld & 3)) &&
      conv_img_applicable(dtype, ks, stride, a, s.has_gn, norm_groups)) {
    ch.kernel = CONV_IMG;
    ch.gn_in_kernel = s.has_gn;
    if (s.want_stats) { ch.stats = STATS_EPILOGUE; ch.stat_nchunk = 1; }
    return DSX_OK;
  }
  const bool ws_allowed = k.ws && (ks != 1 || k.ws_1x1) && stride == 1 && a.stage_mode == 0;
  if (k.conv_naive || !decide_tile(k, dtype, ks, stride, ws_allowed, a, ch.tile)) {
    if (!s.has_naive)
      return fail(DSX_ERR_INVALID, "no MFMA tile fits conv %dx%d (%dx%d out, B=%d); set DSX_CONV_IMPL=naive", ks, ks,
                  a.Ho, a.Wo, a.B);
    ch.kernel = CONV_NAIVE;
    return DSX_OK;
  }
  // (Preserved: k_conv_ws whenever its conditions hold for the tile that was picked, whichever pass of decide_tile
  // picked it -- so also with fewer than ws_min_grid items when a fallback pass chose the tile and split-K did not apply.)
  const int tile = ch.tile;
  const bool use_ws = ws_allowed && a.cpg != 2 && a.ksplit == 1 && conv_ws_lds_bytes(dtype, tile, ks, a) != 0;
  ch.kernel = a.ksplit > 1 ? CONV_SPLITK : (use_ws ? CONV_WS : (a.cpg == 2 ? CONV_MFMA_G2 : CONV_MFMA));
  if (use_ws) decide_ws_chunks(k, dtype, ks, tile, a);
  // (Tried and rejected in round 3, measured: the GroupNorm finalised by the consuming conv's own compute waves during
  // their start-up wait -- 14 to 22 k_gn_finalize launches fewer, but every such conv started 3-7 us later, the same
  // or more than the launch it replaced cost inside the captured graph: step +0.4 .. +1.1 %.  DESIGN.md section 4.)
  const ConvTileInfo ti = conv_tile_info(tile, use_ws);
  if (k.fuse_stats && s.want_stats && ti.fuses_stats &&
      a.ksplit == 1 && a.tb_log2 == 0 && (a.Cout & 15) == 0 && a.out_ld == a.Cout && (a.resid_ld & 7) == 0) {
    ch.stats = STATS_EPILOGUE;
    ch.stat_nchunk = a.tiles_x * a.tiles_y * ti.WM;
  }
  if (a.ksplit > 1 && k.fuse_stats && s.want_stats && a.Cout % 64 == 0 && a.out_ld == a.Cout && (a.Ho * a.Wo) % 16 == 0) {
    ch.stats = STATS_REDUCE;   // statistics in the reduce launch, shifted by bias + film
    ch.stat_nchunk = a.Ho * a.Wo / 16;
    ch.pivot = PIVOT_BIAS_FILM;
  }
  ch.hosts_fin = s.may_host_fin && k.host_fin && use_ws;
  return use_ws ? decide_ws_startup(k, ks, a) : DSX_OK;
}

struct ConvSpec {
  const ConvW* w;
  Tensor x0, x1;       // x1.p == nullptr / C == 0: single source
  bool up = false;
  int stride = 1;
  const GnW* gn = nullptr;   // GroupNorm over cat(x0, x1) in front of the conv (finalised by k_gn_finalize, or inside
                             // the consumer by k_conv_img)
  bool has_resid = false;
  bool host_fin = false;     // plan_res: this residual 1 x 1 conv may host the finalize of the block's second GroupNorm
  bool swish = false;
  int film_off = -1;         // FiLM vector of the conv: offset into dsx_exec::film (row stride dsx_model::F), -1: none
  const void* resid = nullptr; int resid_ld = 0;   // (the pointer is null while sizing: decisions read has_resid)
  Tensor out;
  bool want_stats = false;   // a GroupNorm will read `out`: produce its statistics in the epilogue
  bool bias_in_film = false; // the conv bias is already part of the FiLM vector (dsx_model_finalize)
};

// reserves the k_chan_stats partial sums of `t` unless a producer already planned its statistics; true if it did
static bool reserve_stats(dsx_exec* ex, const Tensor& t) {
  StatInfo& si = ex->stats[t.id];
  if (si.planned) return false;
  int nchunk = std::max(1, 512 / ex->B);
  nchunk = std::min(nchunk, std::max(1, t.H * t.W / 16));
  nchunk = std::min(nchunk, 64);
  si.nchunk = nchunk;
  si.part = ws_alloc(ex, (size_t)ex->B * nchunk * t.C * 2 * sizeof(double));
  si.planned = true;
  si.f32 = false;
  return true;
}
static void emit_stats(dsx_exec* ex, const Tensor& t) {
  const StatInfo& si = ex->stats[t.id];
  const int HW = t.H * t.W;
  const int i = add_op(ex, DSX_OP_GN_STATS, fmt("gn_stats C=%d @%dx%d", t.C, t.H, t.W), 0.0,
                       (t.st ? 2.0 : 4.0) * ex->B * HW * t.C, L_CHAN_STATS);
  ChanStatsArgs& c = ex->ops[i].args.stats;
  c.x = t.p; c.xbf = t.st; c.B = ex->B; c.HW = HW; c.C = t.C; c.nchunk = si.nchunk; c.part = (double*)si.part;
}

// the GroupNorm partial sums of `t` come from the epilogue of the launch being planned (fp32 rows [B][nchunk][C][2])
static float* plan_fused_stats(dsx_exec* ex, const Tensor& t, int nchunk, int C) {
  StatInfo& si = ex->stats[t.id];
  si.nchunk = nchunk;
  si.part = ws_alloc(ex, (size_t)ex->B * nchunk * C * 2 * sizeof(float));
  si.planned = true;
  si.f32 = true;
  return (float*)si.part;
}

// GroupNorm over cat(t0, t1) -> device scale/shift [B][C]: a k_gn_finalize launch, or (hosted) the arguments of the
// residual 1 x 1 conv in front that runs it.  Returns the op whose prefetch slot the consuming conv may fill.
static int emit_gn_finalize(dsx_exec* ex, const GnW& g, const Tensor& t0, const Tensor* t1, float* scale, float* shift,
                            bool hosted) {
  GnFinArgs a{};
  a.part0 = ex->stats[t0.id].part; a.C0 = t0.C; a.nchunk0 = ex->stats[t0.id].nchunk;
  a.f32_0 = ex->stats[t0.id].f32 ? 1 : 0;
  a.part1 = t1 ? ex->stats[t1->id].part : nullptr; a.C1 = t1 ? t1->C : 0;
  a.nchunk1 = t1 ? ex->stats[t1->id].nchunk : 0;
  a.f32_1 = (t1 && ex->stats[t1->id].f32) ? 1 : 0;
  a.piv0 = ex->stats[t0.id].piv;
  if (t1) a.piv1 = ex->stats[t1->id].piv;
  a.B = ex->B; a.groups = ex->m->cfg.norm_groups; a.count = (double)t0.H * t0.W;
  a.gamma = g.gamma; a.beta = g.beta; a.eps = 1e-5f;
  a.scale = scale; a.shift = shift;
  if (hosted && ex->fin_host_op >= 0) {
    const int host = ex->fin_host_op;
    ex->fin_host_op = -1;
    ex->ops[host].args.conv.fin_on = 1;
    ex->ops[host].args.conv.fin = a;
    return host;
  }
  const int i = add_op(ex, DSX_OP_GN_FINALIZE, fmt("gn_finalize C=%d", a.C0 + a.C1), 0.0, 0.0, L_GN_FINALIZE);
  ex->ops[i].args.fin = a;
  return i;
}

static dsx_layer_info new_layer(dsx_exec* ex, int kind, int op_begin) {
  dsx_layer_info L;
  memset(&L, 0, sizeof L);
  L.kind = kind;
  L.op_begin = op_begin; L.op_end = (int)ex->ops.size(); L.op_main = L.op_end - 1;
  L.B = ex->B;
  L.gn_gamma_param = L.gn_beta_param = L.w_param = L.b_param = -1;
  return L;
}

// the launches of one conv, from its choice and its bound arguments; `fin_op`: the finalize planned for it (-1: none).
// Returns the index of the conv launch itself.
static int emit_conv_ops(dsx_exec* ex, const ConvChoice& ch, const ConvArgs& a, int ks, int stride, int fin_op,
                         float* slab, float* reduce_stats, const float* naive_w) {
  const PlanKnobs& k = ex->knobs;
  const int dtype = ex->m->dtype, tile = ch.tile, cin = a.C0 + a.C1;
  const double npix = (double)a.B * a.Ho * a.Wo;
  const double flops = 2.0 * npix * a.Cout * cin * ks * ks;
  const double esz = dtype != 0 ? 2.0 : 4.0;   // activation element size in HBM
  const double bytes = esz * ((double)a.B * a.Hs * a.Ws * cin + npix * a.Cout * (a.resid ? 1 : 0)) +
                       (a.out_bf16 ? 2.0 : 4.0) * npix * a.Cout + (double)a.Cout * cin * ks * ks * esz;
  auto conv_op = [&](const std::string& desc, Launcher l, const ConvArgs& args) {
    const int i = add_op(ex, DSX_OP_CONV_MFMA, desc, flops, bytes, l);
    PlanOp& o = ex->ops[i];
    o.dtype = dtype; o.tile = tile; o.ks = ks; o.stride = stride; o.args.conv = args;
    return i;
  };
  if (ch.kernel == CONV_FIRST)
    return conv_op(fmt("conv3x3 %d->%d @%dx%d first", cin, a.Cout, a.Ho, a.Wo), L_CONV_FIRST, a);
  if (ch.kernel == CONV_IMG) {
    // the previous image-resident conv warms the L2s for this one: one slice per N block
    if (k.prefetch && ex->prev_img_op >= 0)
      ex->ops[ex->prev_img_op].args.conv.pf = PrefetchArgs{a.wpack, (unsigned)((size_t)a.kchunks * ks * ks * 2 * 1024), a.nblocks, nullptr};
    return ex->prev_img_op = conv_op(fmt("conv%dx%d %d->%d @%dx%d img", ks, ks, cin, a.Cout, a.Ho, a.Wo), L_CONV_IMG, a);
  }
  if (ch.kernel == CONV_NAIVE) {
    const int i = add_op(ex, DSX_OP_CONV_NAIVE, fmt("conv%dx%d-naive %d->%d @%dx%d", ks, ks, cin, a.Cout, a.Ho, a.Wo),
                         flops, bytes, L_CONV_NAIVE);
    NaiveConvArgs& na = ex->ops[i].args.naive;
    na.c = a; na.w = naive_w; na.ks = ks; na.stride = stride; na.sigmoid_out = 0;
    return i;
  }
  const ConvTileInfo ti = conv_tile_info(tile);
  const std::string d = fmt("conv%dx%d%s%s %d->%d @%dx%d tile%dx%d", ks, ks, stride == 2 ? "s2" : "",
                            a.up ? "up" : "", cin, a.Cout, a.Ho, a.Wo, ti.BM, ti.BN);
  if (ch.kernel == CONV_SPLITK) {
    ConvArgs p = a;  // slices write raw sums into fp32 slabs; a reduce launch applies the epilogue
    p.out = slab; p.out_bf16 = 0;
    const int main_op = conv_op(d + fmt(" splitK%d", a.ksplit), L_CONV_MFMA, p);
    const long long M = (long long)a.B * a.Ho * a.Wo;
    const int i = add_op(ex, DSX_OP_SPLITK_REDUCE, fmt("splitk_reduce x%d %d ch @%dx%d", a.ksplit, a.Cout, a.Ho, a.Wo), 0.0,
                         (4.0 * a.ksplit + esz) * (double)M * a.Cout, L_SPLITK_REDUCE);
    SplitKReduceArgs& ra = ex->ops[i].args.reduce;
    ra.slab = slab; ra.nsplit = a.ksplit; ra.slab_stride = a.slab_stride;
    ra.M = M; ra.N = a.Cout; ra.HW = a.Ho * a.Wo;
    ra.bias = a.bias; ra.film = a.film; ra.film_bs = a.film_bs;
    ra.resid = a.resid; ra.resid_ld = a.resid_ld; ra.out = a.out; ra.act_bf16 = a.act_bf16;
    ra.stat_part = reduce_stats;
    return main_op;
  }
  if (ch.kernel != CONV_WS) return conv_op(a.cpg == 2 ? d + " g2" : d, L_CONV_MFMA, a);
  // this conv's finalize pulls the weight slices into the L2 of the XCD group that will read them (k_conv_ws keys its
  // N tile on blockIdx % 8 in exactly ws_map 0 and 1); no finalize in front (1 x 1 without GroupNorm, upsampling
  // conv): the previous k_conv_ws launch carries it
  const bool keyed = a.ws_map == 0 || a.ws_map == 1;
  const size_t wblock = (size_t)a.kchunks * ks * ks * 2 * 1024;     // bytes of one 32-channel N block's fragments
  const PrefetchArgs mine{a.wpack, (unsigned)(wblock * (ti.BN / 32)), a.n_tiles, nullptr};
  if (k.prefetch && fin_op >= 0 && keyed) {
    PlanOp& f = ex->ops[fin_op];
    (f.launcher == L_GN_FINALIZE ? f.args.fin.pf : f.args.conv.fin.pf) = mine;
  } else if (k.prefetch && k.prefetch_ws && ex->prev_ws_op >= 0 && keyed) {
    ex->ops[ex->prev_ws_op].args.conv.pf = mine;
  }
  const char* cpg = a.ws_cpg == 4 ? " ws c4" : ((a.ws_cpg == 2 && !ch.hosts_fin) ? " ws c2" : " ws");
  ex->prev_ws_op = conv_op(d + cpg + (ch.hosts_fin ? " +gn" : ""), L_CONV_WS, a);
  if (ch.hosts_fin) ex->fin_host_op = ex->prev_ws_op;
  return ex->prev_ws_op;
}

static ConvShape conv_shape(const dsx_exec* ex, const ConvSpec& s) {
  ConvShape h{};
  h.B = ex->B; h.Hs = s.x0.H; h.Ws = s.x0.W; h.Ho = s.out.H; h.Wo = s.out.W;
  h.C0 = s.x0.C; h.C1 = s.x1.C; h.Cout = s.w->cout; h.ks = s.w->ks; h.stride = s.stride;
  h.up = s.up; h.swish = s.swish; h.has_gn = s.gn != nullptr; h.has_resid = s.has_resid; h.has_film = s.film_off >= 0;
  h.resid_ld = s.resid_ld; h.out_ld = s.out.C; h.out_st = s.out.st;
  h.kchunks = s.w->kchunks; h.nblocks = s.w->nblocks;
  h.want_stats = s.want_stats; h.may_host_fin = s.host_fin; h.has_naive = s.w->naive != nullptr;
  return h;
}

// One conv of the plan: decide (from the shape alone), reserve (every workspace byte of this conv, both passes), emit
// (planning pass only: the launches and the layer-table entry, from the choice and the addresses just reserved).
static int plan_conv(dsx_exec* ex, const ConvSpec& s) {
  const PlanKnobs& k = ex->knobs;
  const ConvShape shape = conv_shape(ex, s);
  if (shape.C0 + shape.C1 != s.w->cin) return fail(DSX_ERR_INVALID, "conv channel mismatch");
  {
    // the conv kernels address their sources with 32-bit byte offsets (0x80000000 = forced out of bounds, the
    // zero padding): a source tensor of 2 GiB or more would silently read as zeros
    const long long esz_src = ex->m->dtype != DSX_DTYPE_F32 ? 2 : 4;
    const long long src_bytes = (long long)shape.B * shape.Hs * shape.Ws * std::max(shape.C0, shape.C1) * esz_src;
    if (src_bytes >= (1LL << 31))
      return fail(DSX_ERR_INVALID,
                  "conv source of %lld bytes (B=%d, %dx%d, %d channels) exceeds the 2 GiB the kernels address; "
                  "use a smaller batch per executor", src_bytes, shape.B, shape.Hs, shape.Ws, std::max(shape.C0, shape.C1));
  }
  ConvChoice ch;
  if (int rc = decide_conv(k, ex->m->dtype, ex->m->cfg.norm_groups, shape, ch)) return rc;

  // ---- reserve: all workspace of this conv, in this order in both passes
  ConvArgs a = ch.geo;
  if (ex->conv_ordinal++ == k.stamp_op) {   // diagnostics: in-kernel phase stamps of this launch
    a.stamp = (unsigned long long*)ws_alloc(ex, 128 * 8);
    a.stamp_block = k.stamp_block;
    ex->stamp_buf = a.stamp;
  }
  const Tensor* x1 = s.x1.C ? &s.x1 : nullptr;
  bool new_stats0 = false, new_stats1 = false;
  float *gn_scale = nullptr, *gn_shift = nullptr;
  bool fin_hosted = false;
  if (s.gn) {   // statistics of the sources no producer fused; every kernel but k_conv_img takes a finalized scale / shift
    new_stats0 = reserve_stats(ex, s.x0);
    if (x1) new_stats1 = reserve_stats(ex, *x1);
    if (!ch.gn_in_kernel) {
      gn_scale = (float*)ws_alloc(ex, (size_t)ex->B * (shape.C0 + shape.C1) * sizeof(float));
      gn_shift = (float*)ws_alloc(ex, (size_t)ex->B * (shape.C0 + shape.C1) * sizeof(float));
      fin_hosted = ex->fin_host_armed;     // the launch in front is a residual 1 x 1 conv whose loader waves do it
      ex->fin_host_armed = false;
    }
  }
  if (ch.stats == STATS_EPILOGUE) a.stat_part = plan_fused_stats(ex, s.out, ch.stat_nchunk, a.Cout);
  float* slab = ch.kernel == CONV_SPLITK ? (float*)ws_alloc(ex, (size_t)a.ksplit * a.slab_stride * sizeof(float)) : nullptr;
  float* reduce_stats = ch.stats == STATS_REDUCE ? plan_fused_stats(ex, s.out, ch.stat_nchunk, a.Cout) : nullptr;
  ex->launches += (new_stats0 ? 1 : 0) + (new_stats1 ? 1 : 0) + ((s.gn && !ch.gn_in_kernel && !fin_hosted) ? 1 : 0) + 1 +
                  (ch.kernel == CONV_SPLITK ? 1 : 0);
  if (ch.hosts_fin) ex->fin_host_armed = true;
  // the addresses the choice leaves open (null while sizing)
  a.src0 = s.x0.p; a.src1 = x1 ? x1->p : nullptr;
  a.wpack = ch.kernel == CONV_FIRST ? s.w->pack_first : s.w->pack;
  a.bias = s.bias_in_film ? nullptr : s.w->bias;
  if (s.film_off >= 0 && !ex->sizing) { a.film = ex->film + s.film_off; a.film_bs = ex->m->F; }
  a.resid = s.resid; a.out = s.out.p;
  a.gn_scale = gn_scale; a.gn_shift = gn_shift;
  if (ch.kernel == CONV_WS) a.handoff_timeouts = ex->handoff_timeouts;
  if (ch.pivot == PIVOT_BIAS) ex->stats[s.out.id].piv = StatPivot{a.bias, nullptr, 0};
  if (ch.pivot == PIVOT_BIAS_FILM) ex->stats[s.out.id].piv = StatPivot{a.bias, a.film, a.film_bs};
  if (ex->sizing) return DSX_OK;

  // ---- emit
  const int op0 = (int)ex->ops.size();
  if (new_stats0) emit_stats(ex, s.x0);
  if (new_stats1) emit_stats(ex, *x1);
  int fin_op = -1;
  if (s.gn && ch.gn_in_kernel) {
    const StatInfo& s0 = ex->stats[s.x0.id];
    a.gn_part0 = s0.part; a.gn_nchunk0 = s0.nchunk; a.gn_pf32_0 = s0.f32 ? 1 : 0; a.gn_piv0 = s0.piv;
    if (x1) {
      const StatInfo& s1 = ex->stats[x1->id];
      a.gn_part1 = s1.part; a.gn_nchunk1 = s1.nchunk; a.gn_pf32_1 = s1.f32 ? 1 : 0; a.gn_piv1 = s1.piv;
    }
    a.gn_gamma = s.gn->gamma; a.gn_beta = s.gn->beta; a.gn_groups = ex->m->cfg.norm_groups; a.gn_eps = 1e-5f;
  } else if (s.gn) {
    fin_op = emit_gn_finalize(ex, *s.gn, s.x0, x1, gn_scale, gn_shift, fin_hosted);
  }
  const int main_op = emit_conv_ops(ex, ch, a, shape.ks, shape.stride, fin_op, slab, reduce_stats, s.w->naive);

  dsx_layer_info L = new_layer(ex, DSX_LAYER_CONV, op0);
  L.op_main = main_op;
  L.ks = shape.ks; L.stride = s.stride; L.up = s.up ? 1 : 0; L.swish = s.swish ? 1 : 0;
  L.Hs = s.x0.H; L.Ws = s.x0.W; L.Ho = s.out.H; L.Wo = s.out.W;
  L.C0 = s.x0.C; L.C1 = s.x1.C; L.src_dtype = s.x0.st;
  L.src0 = (uint64_t)(uintptr_t)s.x0.p; L.src1 = x1 ? (uint64_t)(uintptr_t)x1->p : 0;
  if (s.gn) { L.gn_gamma_param = s.gn->pg; L.gn_beta_param = s.gn->pb; }
  L.gn_in_kernel = ch.gn_in_kernel ? 1 : 0;
  L.gn_scale = (uint64_t)(uintptr_t)gn_scale; L.gn_shift = (uint64_t)(uintptr_t)gn_shift;
  L.w_param = s.w->pw; L.b_param = s.w->pb; L.bias_in_film = s.bias_in_film ? 1 : 0;
  if (s.film_off >= 0) { L.film = (uint64_t)(uintptr_t)ex->film; L.film_off = s.film_off; L.film_bs = ex->m->F; }
  L.resid = (uint64_t)(uintptr_t)s.resid; L.resid_ld = s.resid_ld;
  L.out = (uint64_t)(uintptr_t)s.out.p; L.out_ld = s.out.C; L.Cout = s.w->cout; L.out_dtype = s.out.st;
  ex->layers.push_back(L);
  return DSX_OK;
}

static int plan_res(dsx_exec* ex, const Module& md, const Tensor& x0, const Tensor* x1, Tensor& y) {
  int rc;
  const int H = x0.H, W = x0.W;
  Tensor h = new_tensor(ex, md.cout, H, W);
  ConvSpec c1{};
  c1.w = &md.conv1; c1.x0 = x0; if (x1) c1.x1 = *x1;
  c1.gn = &md.gn1; c1.swish = true;
  c1.film_off = md.film_off;
  c1.bias_in_film = md.film_off >= 0 && md.conv1.pb >= 0;
  c1.out = h; c1.want_stats = true;
  if ((rc = plan_conv(ex, c1))) return rc;
  Tensor r;
  if (md.has_res) {
    r = new_tensor(ex, md.cout, H, W);
    ConvSpec cr{};
    cr.w = &md.res; cr.x0 = x0; if (x1) cr.x1 = *x1; cr.out = r;
    // the hosted finalize reads h's GroupNorm partial sums: only when conv1's epilogue produced them (fused statistics;
    // `planned` follows from conv1's ConvChoice).  Otherwise c2 adds a k_chan_stats launch
    // AFTER this conv and the finalize must stay behind it as a launch of its own.
    cr.host_fin = ex->stats[h.id].planned;
    if ((rc = plan_conv(ex, cr))) return rc;
  } else {
    r = x0;
  }
  Tensor o = new_tensor(ex, md.cout, H, W);
  ConvSpec c2{};
  c2.w = &md.conv2; c2.x0 = h; c2.gn = &md.gn2; c2.swish = true;
  c2.resid = r.p; c2.resid_ld = md.cout; c2.has_resid = true; c2.out = o; c2.want_stats = true;
  if ((rc = plan_conv(ex, c2))) return rc;
  ex->fin_host_armed = false; ex->fin_host_op = -1;
  if (!md.attn) { y = o; return DSX_OK; }
  // SelfAttention (unet.py:113-142)
  const int C = md.cout, L = H * W, B = ex->B;
  Tensor qkv = new_tensor(ex, 3 * C, H, W);
  ConvSpec cq{};
  cq.w = &md.qkv; cq.x0 = o; cq.gn = &md.gna; cq.out = qkv;
  if ((rc = plan_conv(ex, cq))) return rc;
  Tensor av = new_tensor(ex, C, H, W);
  ex->launches += 1;
  if (!attn_supported(C, L)) return fail(DSX_ERR_INVALID, "attention with head dimension %d is not supported (8..1024, multiple of 8)", C);
  if (!ex->sizing) {
    AttnArgs g{};
    g.q = qkv.p; g.k = qkv.at(C); g.v = qkv.at(2 * (size_t)C); g.ld = 3 * C;
    g.out = av.p; g.ldo = C; g.storage = qkv.st;
    g.B = B; g.L = L; g.C = C; g.div = sqrtf((float)C); g.inv_div = 1.0f / g.div;
    const double esz = qkv.st ? 2.0 : 4.0;
    const int op0 = add_op(ex, DSX_OP_ATTN_GEMM, fmt("attn fused L=%d d=%d", L, C), 4.0 * B * L * (double)L * C,
                           B * esz * 4.0 * L * C, L_ATTN);
    ex->ops[op0].col_split = ex->knobs.attn_cs == 2 ? 1 : 0;
    ex->ops[op0].args.attn = g;
    dsx_layer_info li = new_layer(ex, DSX_LAYER_ATTN, op0);
    li.Hs = li.Ho = H; li.Ws = li.Wo = W; li.C0 = li.C1 = C; li.src_dtype = qkv.st;
    li.src0 = (uint64_t)(uintptr_t)g.q; li.src1 = (uint64_t)(uintptr_t)g.k; li.resid = (uint64_t)(uintptr_t)g.v;
    li.ld = g.ld;
    li.out = (uint64_t)(uintptr_t)av.p; li.out_ld = C; li.Cout = C; li.out_dtype = av.st;
    ex->layers.push_back(li);
  }
  Tensor o2 = new_tensor(ex, C, H, W);
  ConvSpec co{};
  co.w = &md.out; co.x0 = av; co.resid = o.p; co.resid_ld = C; co.has_resid = true; co.out = o2; co.want_stats = true;
  if ((rc = plan_conv(ex, co))) return rc;
  y = o2;
  return DSX_OK;
}

static int build_plan(dsx_exec* ex) {
  dsx_model* m = ex->m;
  ex->ws_used = 0;
  ex->ops.clear();
  ex->conv_ordinal = 0;
  ex->prev_img_op = ex->prev_ws_op = ex->fin_host_op = -1;
  ex->fin_host_armed = false;
  ex->stats.clear();
  ex->layers.clear();
  ex->launches = 0;
  const int B = ex->B;
  ex->step_ctr = (int*)ws_alloc(ex, 256);
  ex->loop_params = (unsigned long long*)(ex->sizing ? nullptr : (char*)ex->step_ctr + 64);
  ex->handoff_timeouts = (unsigned*)(ex->sizing ? nullptr : (char*)ex->step_ctr + 128);   // (zeroed with the block at create)
  ex->time_buf = (float*)ws_alloc(ex, (size_t)B * sizeof(float));
  ex->film = m->F ? (float*)ws_alloc(ex, (size_t)B * m->F * sizeof(float)) : nullptr;
  ex->in_cond = Tensor();
  if (ex->cond_c) ex->in_cond = new_tensor(ex, ex->cond_c, ex->H, ex->W);
  ex->in_x = new_tensor(ex, ex->x_c, ex->H, ex->W);
  ex->x_state = ex->in_x.st ? (float*)ws_alloc(ex, (size_t)B * ex->H * ex->W * ex->x_c * sizeof(float))
                              : (float*)ex->in_x.p;
  if (!ex->sizing) {
    if (ex->film) {
      dsx_layer_info L = new_layer(ex, DSX_LAYER_FILM, 0);
      L.op_main = -1;
      L.film = L.out = (uint64_t)(uintptr_t)ex->film; L.film_bs = L.Cout = L.out_ld = m->F;
      ex->layers.push_back(L);
    }
    for (const Tensor* t : {&ex->in_cond, &ex->in_x}) {
      if (!t->C) continue;
      dsx_layer_info L = new_layer(ex, DSX_LAYER_INPUT, 0);
      L.op_main = -1;
      L.Ho = L.Hs = ex->H; L.Wo = L.Ws = ex->W;
      L.C0 = t == &ex->in_x ? ex->cond_c : 0;
      L.out = (uint64_t)(uintptr_t)t->p; L.Cout = L.out_ld = t->C; L.out_dtype = t->st;
      ex->layers.push_back(L);
    }
  }
  std::vector<Tensor> feats;
  Tensor x;
  int rc;
  for (auto& md : m->mods) {
    if (md.kind == 0) {
      Tensor o = new_tensor(ex, md.cout, ex->H, ex->W);
      ConvSpec c{};
      c.w = &md.conv;
      if (ex->cond_c) { c.x0 = ex->in_cond; c.x1 = ex->in_x; } else c.x0 = ex->in_x;
      c.out = o; c.want_stats = true;
      if ((rc = plan_conv(ex, c))) return rc;
      x = o; feats.push_back(x);
    } else if (md.kind == 2) {
      if ((x.H & 1) || (x.W & 1)) return fail(DSX_ERR_INVALID, "H and W must be divisible by 2^(levels-1)");
      Tensor o = new_tensor(ex, md.cout, x.H / 2, x.W / 2);
      ConvSpec c{};
      c.w = &md.conv; c.x0 = x; c.stride = 2; c.out = o; c.want_stats = true;
      if ((rc = plan_conv(ex, c))) return rc;
      x = o; feats.push_back(x);
    } else if (md.kind == 3) {
      Tensor o = new_tensor(ex, md.cout, x.H * 2, x.W * 2);
      ConvSpec c{};
      c.w = &md.conv; c.x0 = x; c.up = true; c.out = o; c.want_stats = true;
      if ((rc = plan_conv(ex, c))) return rc;
      x = o;
    } else if (md.kind == 1) {
      Tensor y;
      if (md.section == 2) {
        Tensor skip = feats.back();
        feats.pop_back();
        if (skip.H != x.H || skip.W != x.W || skip.C != md.skip) return fail(DSX_ERR_INVALID, "skip mismatch");
        if ((rc = plan_res(ex, md, x, &skip, y))) return rc;
      } else {
        if ((rc = plan_res(ex, md, x, nullptr, y))) return rc;
      }
      x = y;
      if (md.section == 0) feats.push_back(x);
    } else {
      Tensor o = new_tensor(ex, md.cout, x.H, x.W, /*f32=*/true);   // the network's output feeds the fp32 sampler update
      ConvSpec c{};
      c.w = &md.conv; c.x0 = x; c.gn = &md.gn1; c.swish = true; c.out = o;
      if ((rc = plan_conv(ex, c))) return rc;
      x = o;
    }
  }
  ex->out = x;
  if (ex->out.st) return fail(DSX_ERR_STATE, "internal error: the network output must be an fp32 tensor");
  return ex->knobs.plan_dump.empty() ? DSX_OK : dump_plan(ex);
}

// Both planner passes.  The sizing pass walks the plan without a workspace and records no launch; the planning pass
// walks it again over the workspace: `fake_base` (dsx_plan_dry_run: an address that is never dereferenced), or device
// memory allocated here.  They must reserve exactly the same bytes.
int dsx::run_planner(dsx_exec* ex, char* fake_base, size_t* sizing_bytes) {
  ex->sizing = true;
  int rc = build_plan(ex);
  const size_t sized = ex->ws_used;
  if (sizing_bytes) *sizing_bytes = sized;
  if (rc) return rc;
  ex->ws_bytes = sized + 4096;
  ex->ws = fake_base;
  if (!fake_base) {
    const hipError_t e = ex->ws_mem.alloc(ex->ws_bytes);
    if (e != hipSuccess)
      return fail(DSX_ERR_HIP, "hipMalloc(%zu) for the activation workspace failed: %s", ex->ws_bytes, hipGetErrorString(e));
    ex->ws = ex->ws_mem.as<char>();
  }
  ex->sizing = false;
  if ((rc = build_plan(ex))) return rc;
  // ws_used only grows, so a pass that ran past the workspace fails here too.  The dry run (fake base: nothing is ever
  // written) reports both counts to its caller instead, as include/dsx.h documents.
  if (!fake_base && ex->ws_used != sized)
    return fail(DSX_ERR_STATE, "planner: sizing pass reserved %zu bytes, planning pass used %zu", sized, ex->ws_used);
  return DSX_OK;
}

// Host-only: both planner passes for (cfg, dtype, B, H, W) without a device (the workspace base is a fake
// address that is never dereferenced).  Tests use it to pin that sizing and planning agree under every tile
// preference setting.
extern "C" int dsx_plan_dry_run(const dsx_unet_cfg* cfg, int dtype, int B, int H, int W, int cond_channels,
                                size_t* sizing_bytes, size_t* planning_bytes, int* launches) {
  if (!cfg || B < 1 || H < 1 || W < 1) return fail(DSX_ERR_INVALID, "bad argument");
  if (dtype != DSX_DTYPE_F32 && dtype != DSX_DTYPE_BF16 && dtype != DSX_DTYPE_F16) return fail(DSX_ERR_INVALID, "bad dtype");
  dsx_model* m = nullptr;
  int rc = dsx_model_create(cfg, &m);
  if (rc) return rc;
  const std::unique_ptr<dsx_model> model(m);
  if (cond_channels < 0 || cond_channels >= m->cfg.in_channel) return fail(DSX_ERR_INVALID, "bad cond_channels");
  m->dtype = dtype;
  for (auto& md : m->mods)
    for (ConvW* c : {&md.conv, &md.conv1, &md.conv2, &md.res, &md.qkv, &md.out})
      if (c->pw >= 0) conv_geometry(c->cout, c->cin, c->ks, dtype, c->kchunks, c->nblocks);
  const auto ex = new_exec(m, B, H, W, cond_channels);
  // never dereferenced, no launch happens; never freed either: dsx_exec::ws only borrows its base
  rc = run_planner(ex.get(), (char*)(uintptr_t)0x100000000ull, sizing_bytes);
  if (planning_bytes) *planning_bytes = ex->sizing ? 0 : ex->ws_used;
  if (launches) *launches = ex->launches;
  return rc;
}
