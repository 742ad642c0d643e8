// dsx_conv_variants.h — the ONE table of compiled conv kernel variants, for init, checks and launch.
//
// kVariants has one row per compiled instantiation of k_conv_mfma, k_conv_ws and k_conv_img.  conv_init sets every
// row's dynamic-LDS limit, the *_lds_bytes functions take "does this variant exist" and its constants from the row, and
// the launchers launch the row's kernel: a key without a row is hipErrorInvalidValue, never some other kernel.
// To add a variant, add ONE row to variants_of (or to ws_nb2_variants, if it has no fp32 build): the maker derives the
// kernel's template arguments and the row's constants from the same numbers.
//
// The three kernel templates are only declared here.  Each is defined in one file (dsx_conv_mfma.hip, dsx_conv_ws.hip,
// dsx_conv_img.hip), which reaches the table through find_variant: that file alone instantiates the template's rows and
// emits their code; every other file that includes the table refers to them as undefined symbols, resolved when the
// library is linked (with --no-undefined: a row whose kernel no file emits fails the build).  So a kernel is compiled
// exactly once.  The knobs that shape a row sit here beside the makers; those a kernel body reads, in its file.
#pragma once
#include "dsx_conv_common.h"

#ifndef DSX_RING_DEPTH
#define DSX_RING_DEPTH 6  // weight-fragment prefetch ring depth for 3x3 (divides 18)
#endif
#ifndef DSX_WS_DEPTH_EXPR
#define DSX_WS_DEPTH_EXPR (bm == 64 ? 5 : (bm == 256 ? 2 : (ks == 1 ? 3 : 4)))   // measured: one more group in flight than the HBM latency strictly needs (256-pixel tile: 2, its third MFMA image takes the LDS of the fourth ring slot)
#endif
#ifndef DSX_WS_DEPTH_C2_64
#define DSX_WS_DEPTH_C2_64 3
#endif
// 1 x 1 convs: weight fragments in flight per wave.  A group is only 4 steps (8-16 MFMAs), so a ring of one group
// (round 1) exposed a whole L2 round trip per group: 1800-2500 cycles for 256 cycles of MFMA work.
#ifndef DSX_RING_1X1_NB1
#define DSX_RING_1X1_NB1 16
#endif
#ifndef DSX_RING_1X1_NB2
#define DSX_RING_1X1_NB2 4
#endif

namespace dsx {

// (the launch bounds are stated here and not on the definitions: a row of the table names its specialization before
// the definition is seen, and the specialization takes its attributes from the declaration it was first named through)
template <typename DT, int MB, int WM, int WN, int KS, int S, int CPG, int D, int MAX_IT>
__global__ __launch_bounds__(256, ((KS == 3 && CPG == 2) ? 2   // two-chunk 3 x 3 variant: up to 11 staging units per thread in flight (spills at 168 VGPRs)
                                  : (MB == 1 ? (S == 2 ? 3 : 4) : (MB == 2 ? 3 : (MB == 4 ? 2 : 1))))) void k_conv_mfma(const ConvArgs a);   // dsx_conv_mfma.hip
template <typename DT, int MB, int WM, int WN, int NB, int KS, int CPG, int D, int NIT, int P, int LW, bool DIRECT>
__global__ __launch_bounds__(256 + 64 * LW, 1) void k_conv_ws(const ConvArgs a);   // dsx_conv_ws.hip
template <typename DT, int KS, int NPH> __global__ __launch_bounds__(512, 1) void k_conv_img(const ConvArgs a);   // dsx_conv_img.hip

enum ConvFamily { FAM_MFMA, FAM_WS, FAM_IMG };
struct ConvVariant {
  int family, dtype, tile, ks, stride, cpg;   // the key (with `direct`).  cpg: chunks per staged group (k_conv_img: NPH, and tile -1)
  void (*kern)(const ConvArgs);
  int block, lds_cap;   // threads per workgroup; dynamic-LDS limit: kLdsDefault, or kLdsMax (set by conv_init)
  int MB, WM, WN, NB;   // wave layout: the tile is 32 MB WM pixels x 32 WN NB channels; WM statistics rows per tile
  int max_px;           // patch pixels the staging registers are sized for
  int nit;              // 16-byte staging units per (loader) thread and group
  int depth, nbuf;      // k_conv_ws: raw groups in flight beyond the current one (P), MFMA images
  bool fuses_stats;     // the epilogue can emit the GroupNorm partial sums of the result
  bool direct;          // k_conv_ws, part of the key: the loaders DMA straight into the MFMA images (ConvArgs::ws_direct)
};
static constexpr int kLdsDefault = 64 * 1024, kLdsMax = 160 * 1024;
static constexpr int conv_cpg(int ks) { return ks == 1 ? 2 : 1; }   // the families' default chunks per group

// k_conv_mfma.  CPG 2 with a 3 x 3 is the two-chunk form (ConvArgs::cpg == 2): 64 input channels per staged group.  For
// the 64-channel layers of the 128^2 level the whole K extent is one group: load + GroupNorm/Swish + one barrier + 36
// MFMA steps + epilogue, three workgroups per CU overlapping each other's phases, instead of the persistent kernel's
// per-group hand-offs (which dominate when a tile has only two groups).
static constexpr int mfma_max_px(int bm, int ks, int stride, int cpg) {
  if (ks == 1) return bm;  // no halo
  if (stride == 2) return 400;
  if (cpg == 2) return bm == 256 ? 324 : 220;
  return bm == 256 ? 400 : (bm == 128 ? 220 : 144);
}
template <typename DT, int TILE, int MB, int WM, int WN, int KS, int S = 1, int CPG = conv_cpg(KS)>
constexpr ConvVariant mfma_row() {
  constexpr bool G2 = KS == 3 && CPG == 2;
  constexpr int D = KS == 1 ? 4 : (G2 ? 6 : DSX_RING_DEPTH);
  constexpr int PX = mfma_max_px(32 * MB * WM, KS, S, CPG);
  constexpr int MI = (PX * 4 * CPG + 255) / 256;   // 4 CPG 16-byte units per pixel and group, either storage type
  return {FAM_MFMA, Kind<DT>::value, TILE, KS, S, CPG, k_conv_mfma<DT, MB, WM, WN, KS, S, CPG, D, MI>, 256,
          G2 ? kLdsMax : kLdsDefault, MB, WM, WN, 1, PX, MI, 0, 2, MB <= 2, false};
}

// k_conv_ws.  Its waves are laid out differently from k_conv_mfma's: MB row blocks x NB N blocks per wave (the
// 128 x 128 tile is 2 x 2 waves of 64 x 64).
static constexpr int kWsLoaderWaves = 4;
// patch pixels the WS loaders are sized for: one image per tile, square-ish tiles (16x8 / 8x16 -> 18x10,
// 8x8 -> 10x10, 16x4 -> 18x6); other shapes fall back to k_conv_mfma
static constexpr int ws_max_px(int bm, int ks) { return ks == 1 ? bm : (bm == 256 ? 324 : (bm == 128 ? 180 : 108)); }
static constexpr int ws_depth(int bm, int ks, int cpg) {
  if (ks == 3 && cpg == 2) return bm == 64 ? DSX_WS_DEPTH_C2_64 : 2;   // two-chunk groups are twice as long (and twice the ring bytes)
  if (ks == 3 && cpg == 4) return 1;
  if (ks == 1 && cpg == 4) return bm == 64 ? 2 : 1;                     // four-chunk groups of a 1 x 1 conv
  return DSX_WS_DEPTH_EXPR;
}

// Loader -> compute hand-off of k_conv_ws.  NBUF == 2: two MFMA images, one workgroup barrier per (tile, group) item
// (strict alternation).  NBUF == 3 / 4: three / four images and LDS counters instead of the barrier -- FULL (one per
// loader wave: items converted) and FREE (one per compute wave: items consumed): the loaders may run two items
// ahead, i.e. they convert during the compute waves' epilogue instead of parking at the barrier, and the compute waves
// find the next tile's first groups ready.  Spins are bounded (a lost hand-off gives wrong pixels, never a hung GPU).
// Measured (round 3, A/B inside one gpurun call, three alternations): counters for the 256-pixel 3 x 3 tile only (the
// 64-channel layers of the 128^2 level: two groups per tile, so the loaders used to idle through every epilogue and
// the compute waves then waited 3500 cycles for the second group) -0.9 % on the step, those layers -10 %; for every
// 3 x 3 tile -0.5 % (deep-K layers lose 2 us each to the polling); four buffers no better than three.
#ifndef DSX_WS_NBUF_EXPR
#define DSX_WS_NBUF_EXPR(bm, ks, nb, cpg) ((bm) == 256 && (ks) == 3 ? 3 : 2)
#endif
static constexpr int ws_nbuf(int bm, int ks, int nb, int cpg) { return DSX_WS_NBUF_EXPR(bm, ks, nb, cpg); }

// DIRECT rows (1 x 1 convs with neither GroupNorm nor Swish in front): no raw ring and no conversion -- the LDS-DMAs fill
// the swizzled MFMA image of the item `depth` items ahead, and the LDS of the ring goes to more images: as many as the old
// path had items between the DMA request and the MFMAs (ring slots + the fetched item + the converted image).
static constexpr int ws_direct_images(int bm, int cpg) { return ws_depth(bm, 1, cpg) + 3; }

template <typename DT, int TILE, int MB, int WM, int WN, int NB, int KS, int CPG = conv_cpg(KS), bool DIRECT = false>
constexpr ConvVariant ws_row() {
  constexpr int BM = 32 * MB * WM;
  // weight ring, in steps: a full group for one N block per wave, half of it (same bytes, same time) for two
  // (1 x 1 with two N blocks per wave or MB 4: a deeper ring spills, and hipcc's spill path fails on this kernel)
  constexpr int D = KS == 1 ? ((NB == 2 || MB == 4) ? DSX_RING_1X1_NB2 : DSX_RING_1X1_NB1) : ((NB == 2 || MB == 4) ? 6 : 18);   // (MB 4: four MFMAs per step, and the registers are needed)
  constexpr int PX = ws_max_px(BM, KS);
  constexpr int NIT = (PX * 4 * CPG + kWsLoaderWaves * 64 - 1) / (kWsLoaderWaves * 64);
  static_assert(!DIRECT || (KS == 1 && NB == 1), "direct rows: 1 x 1 convs, one N block per wave");
  constexpr int NIMG = DIRECT ? ws_direct_images(BM, CPG) : ws_nbuf(BM, KS, NB, CPG);
  constexpr int P = DIRECT ? NIMG - 1 : ws_depth(BM, KS, CPG);
  return {FAM_WS, Kind<DT>::value, TILE, KS, 1, CPG, k_conv_ws<DT, MB, WM, WN, NB, KS, CPG, D, NIT, P, kWsLoaderWaves, DIRECT>,
          256 + 64 * kWsLoaderWaves, kLdsMax, MB, WM, WN, NB, PX, NIT, P, NIMG, true, DIRECT};
}

// k_conv_img.  NPH 2 / 4: unrolled for exactly that many channel phases; NPH 8: any count up to 8, read at run time
template <typename DT, int KS, int NPH> constexpr ConvVariant img_row() {
  return {FAM_IMG, Kind<DT>::value, -1, KS, 1, NPH, k_conv_img<DT, KS, NPH>, 512, kLdsMax, 0, 0, 0, 0, 0, 0, 0, 0, true, false};
}

template <int N> struct ConvVariants {
  ConvVariant row[N];
  constexpr const ConvVariant* begin() const { return row; }
  constexpr const ConvVariant* end() const { return row + N; }
};
template <int... N> constexpr ConvVariants<(N + ...)> concat(const ConvVariants<N>&... parts) {
  ConvVariants<(N + ...)> out{};
  int n = 0;
  auto append = [&](const auto& p) { for (const ConvVariant& v : p) out.row[n++] = v; };
  (append(parts), ...);
  return out;
}

// Which variants are compiled, per operand type.
template <typename DT> constexpr ConvVariants<37> variants_of() {
  return {{
      // k_conv_mfma: tile, MB, WM, WN, ks, stride (1), chunks per group (the default of ks)
      mfma_row<DT, TILE_256x128, 8, 1, 4, 1>(), mfma_row<DT, TILE_256x128, 8, 1, 4, 3>(),
      mfma_row<DT, TILE_128x128, 4, 1, 4, 1>(), mfma_row<DT, TILE_128x128, 4, 1, 4, 3>(),
      mfma_row<DT, TILE_64x128, 2, 1, 4, 1>(), mfma_row<DT, TILE_64x128, 2, 1, 4, 3>(),
      mfma_row<DT, TILE_256x64, 4, 2, 2, 1>(), mfma_row<DT, TILE_256x64, 4, 2, 2, 3>(),
      mfma_row<DT, TILE_128x64, 2, 2, 2, 1>(), mfma_row<DT, TILE_128x64, 2, 2, 2, 3>(),
      mfma_row<DT, TILE_128x64, 2, 2, 2, 3, 1, 2>(),   // two-chunk form: an experiment (PlanKnobs::tiles_narrow_g2)
      mfma_row<DT, TILE_64x64, 1, 2, 2, 1>(), mfma_row<DT, TILE_64x64, 1, 2, 2, 3>(),
      mfma_row<DT, TILE_64x64, 1, 2, 2, 3, 2>(),       // the stride-2 downsamples
      // layers with <= 32 output channels (the final conv, 16-channel Hagen levels): all four waves along M, no wave
      // multiplies padding columns; 256 x 32 (a 16 x 16 pixel tile) exists as the two-chunk form only
      mfma_row<DT, TILE_128x32, 1, 4, 1, 1>(), mfma_row<DT, TILE_128x32, 1, 4, 1, 3>(),
      mfma_row<DT, TILE_128x32, 1, 4, 1, 3, 1, 2>(), mfma_row<DT, TILE_256x32, 2, 4, 1, 3, 1, 2>(),
      // k_conv_ws: tile, MB, WM, WN, NB, ks, chunks per group (the default of ks)
      ws_row<DT, TILE_64x128, 2, 1, 4, 1, 1>(), ws_row<DT, TILE_64x128, 2, 1, 4, 1, 3>(),
      ws_row<DT, TILE_64x128, 2, 1, 4, 1, 1, 4>(),     // ConvArgs::ws_cpg: 128 input channels per item of a 1 x 1 conv,
      ws_row<DT, TILE_64x128, 2, 1, 4, 1, 3, 2>(),     // 64 (the 16 x 16 maps, where the loaders' per-item costs bound the item)
      ws_row<DT, TILE_64x128, 2, 1, 4, 1, 3, 4>(),     // or 128 of a 3 x 3 conv
      ws_row<DT, TILE_128x64, 2, 2, 2, 1, 1>(), ws_row<DT, TILE_128x64, 2, 2, 2, 1, 3>(),
      ws_row<DT, TILE_256x64, 4, 2, 2, 1, 3>(),        // 16 x 16 pixels: half the tiles (and epilogues) of 128 x 64
      ws_row<DT, TILE_64x64, 1, 2, 2, 1, 1>(), ws_row<DT, TILE_64x64, 1, 2, 2, 1, 3>(),
      // k_conv_ws, direct rows: the plain 1 x 1 convs (residual and attention-output convs), per (tile, chunks per item).
      // (No TILE_64x64 row: no launch of the benchmark takes that tile for a 1 x 1 conv, so it was never measured.)
      ws_row<DT, TILE_64x128, 2, 1, 4, 1, 1, 2, true>(), ws_row<DT, TILE_64x128, 2, 1, 4, 1, 1, 4, true>(),
      ws_row<DT, TILE_128x64, 2, 2, 2, 1, 1, 2, true>(),
      // k_conv_img: ks, NPH
      img_row<DT, 1, 2>(), img_row<DT, 1, 4>(), img_row<DT, 1, 8>(),
      img_row<DT, 3, 2>(), img_row<DT, 3, 4>(), img_row<DT, 3, 8>(),
  }};
}
// k_conv_ws with two N blocks per wave: the fp32 build does not fit the registers, so 16-bit operands only
template <typename DT> constexpr ConvVariants<4> ws_nb2_variants() {
  return {{ws_row<DT, TILE_128x128, 2, 2, 2, 2, 1>(), ws_row<DT, TILE_128x128, 2, 2, 2, 2, 3>(),
           ws_row<DT, TILE_128x128, 2, 2, 2, 2, 1, 4>(), ws_row<DT, TILE_128x128, 2, 2, 2, 2, 3, 2>()}};
}
static constexpr auto kVariants = concat(variants_of<float>(), variants_of<__bf16>(), variants_of<_Float16>(),
                                         ws_nb2_variants<__bf16>(), ws_nb2_variants<_Float16>());

// key -> row without a search (the planner asks a few times per conv and candidate tile)
static constexpr int kKeySlots = 3 * 3 * (TILE_COUNT + 1) * 2 * 2 * 4 * 2;
static constexpr int key_slot(int family, int dtype, int tile, int ks, int stride, int cpg, bool direct) {
  const int c = cpg == 1 ? 0 : (cpg == 2 ? 1 : (cpg == 4 ? 2 : (cpg == 8 ? 3 : -1)));
  if (family < 0 || family > FAM_IMG || dtype < 0 || dtype > 2 || tile < -1 || tile >= TILE_COUNT || (ks != 1 && ks != 3) ||
      (stride != 1 && stride != 2) || c < 0)
    return -1;
  return (((((family * 3 + dtype) * (TILE_COUNT + 1) + tile + 1) * 2 + ks / 2) * 2 + stride - 1) * 4 + c) * 2 + (direct ? 1 : 0);
}
struct VariantIndex { short row[kKeySlots]; bool unique; };
static constexpr VariantIndex index_variants() {
  VariantIndex ix{};
  for (short& r : ix.row) r = -1;
  ix.unique = true;
  short n = 0;
  for (const ConvVariant& v : kVariants) {
    const int s = key_slot(v.family, v.dtype, v.tile, v.ks, v.stride, v.cpg, v.direct);
    if (s < 0 || ix.row[s] >= 0) ix.unique = false;
    else ix.row[s] = n;
    ++n;
  }
  return ix;
}
static constexpr VariantIndex kIndex = index_variants();
static const ConvVariant* find_variant(int family, int dtype, int tile, int ks, int stride, int cpg, bool direct = false) {
  const int s = key_slot(family, dtype, tile, ks, stride, cpg, direct);
  return s >= 0 && kIndex.row[s] >= 0 ? &kVariants.row[kIndex.row[s]] : nullptr;
}

static int patch_pixels(int ks, int stride, const ConvArgs& a) {
  const int TW = 1 << a.tw_log2, TH = 1 << a.th_log2;
  return (((TH - 1) * stride + ks) * ((TW - 1) * stride + ks)) << a.tb_log2;
}
static hipError_t launch_variant(const ConvVariant& v, unsigned grid, size_t lds, const ConvArgs& a, hipStream_t st) {
  void* args[] = {(void*)&a};
  (void)hipLaunchKernel((const void*)v.kern, dim3(grid), dim3((unsigned)v.block), args, lds, st);
  return hipGetLastError();
}

}  // namespace dsx
