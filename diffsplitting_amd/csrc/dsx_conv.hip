// dsx_conv.hip — fused GroupNorm-apply + Swish + KxK convolution (+bias +FiLM
// +residual) as an implicit GEMM on gfx950 MFMA; NHWC activations in HBM in the MFMA operand type
// (fp32 in the parity build, bf16 in the bf16 build).
//
// Replaces the ATen op chain of Block / ResnetBlock / Upsample / Downsample /
// 1x1 convs of the reference UNets (model/sr3_modules/unet.py:58-110,
// model/ddpm_modules/unet.py:42-96): group_norm -> sigmoid -> mul -> conv2d ->
// add (FiLM) -> add (residual), and torch.cat / upsample_nearest2d in front of it.
//
// One translation unit per kernel family; a kernel's code does not depend on what else is compiled beside it:
//   dsx_conv_mfma.hip    k_conv_mfma: the tiled kernel (any stride, split-K, every staging mode); its header describes the
//                        work decomposition and the operand layouts that all families share
//   dsx_conv_ws.hip      k_conv_ws (+ dsx_conv_ws_item.inc): the warp-specialised persistent kernel most launches run on
//   dsx_conv_img.hip     k_conv_img: the image-resident kernel of the 8 x 8 feature maps
//   dsx_conv_direct.hip  k_conv_first (the UNet's first conv) and k_conv_naive (plain direct conv)
//   dsx_conv_common.h    device helpers that more than one family uses
//   dsx_conv_variants.h  the table of compiled variants (kVariants), its index and the launch helper
// This file keeps what spans the families: the compile-time checks over the whole table, conv_tile_info and conv_init.
#include "dsx_conv_variants.h"
#include <mutex>

namespace dsx {

int conv_chunk_multiple(int ks) { return conv_cpg(ks); }

static_assert(kIndex.unique, "kVariants: two rows share a key, or a key is outside key_slot's ranges");

static constexpr bool variants_consistent() {
  for (const ConvVariant& a : kVariants) {
    // the sizing rules assume these limits; block sizes are the kernels' __launch_bounds__
    const bool big = a.family != FAM_MFMA || (a.ks == 3 && a.cpg == 2);
    if (a.lds_cap != (big ? kLdsMax : kLdsDefault) || a.block != (a.family == FAM_MFMA ? 256 : 512)) return false;
    for (const ConvVariant& b : kVariants) {
      // one wave layout per (family, tile), and both families agree on what a tile's name means (conv_tile_info)
      if (a.tile == b.tile && (a.MB * a.WM != b.MB * b.WM || a.WN * a.NB != b.WN * b.NB)) return false;
      if (a.tile == b.tile && a.family == b.family && (a.WM != b.WM || a.fuses_stats != b.fuses_stats)) return false;
    }
  }
  return true;
}
static_assert(variants_consistent(), "kVariants: wrong LDS limit / block size, or two layouts for one tile");

ConvTileInfo conv_tile_info(int tile, bool ws) {
  for (const ConvVariant& v : kVariants)
    if (v.family == (ws ? FAM_WS : FAM_MFMA) && v.tile == tile) return {32 * v.MB * v.WM, 32 * v.WN * v.NB, v.WM, v.fuses_stats};
  return {0, 0, 0, false};
}

// conv_lds_row against the four pitch functions it replaced, for every (ks, stride, cpg) these stood for
namespace lds_row_was {
constexpr int banked(int rb, int tw_log2) {
  if (tw_log2 == 4) rb = (rb + 255) & ~255;
  else if (tw_log2 == 3) { rb = (rb + 127) & ~127; if (((rb >> 7) & 1) == 0) rb += 128; }
  return rb;
}
constexpr int plain(int ks, int stride, int tw_log2) {   // conv_lds_row(ks, stride, tw_log2)
  const int rb = ((((1 << tw_log2) - 1) * stride + ks) * (64 * conv_cpg(ks) + 16) + 15) & ~15;
  return (ks == 1 || stride != 1) ? rb : banked(rb, tw_log2);
}
constexpr int g2(int tw_log2) { return banked(((((1 << tw_log2) - 1) + 3) * (64 * 2 + 16) + 15) & ~15, tw_log2); }
constexpr int c3x3(int tw_log2, int cpg) { return banked(((((1 << tw_log2) - 1) + 3) * (64 * cpg + 16) + 15) & ~15, tw_log2); }
constexpr int c4_1x1(int tw_log2) { return (((1 << tw_log2) * (64 * 4 + 16)) + 15) & ~15; }
constexpr bool same() {
  for (int tw = 0; tw <= 4; ++tw) {
    for (int cpg = 1; cpg <= 4; cpg *= 2)
      if (conv_lds_row(3, 1, tw, cpg) != c3x3(tw, cpg)) return false;
    if (conv_lds_row(3, 1, tw, 1) != plain(3, 1, tw) || conv_lds_row(3, 1, tw, 2) != g2(tw)) return false;
    if (conv_lds_row(3, 2, tw, 1) != plain(3, 2, tw)) return false;
    if (conv_lds_row(1, 1, tw, 2) != plain(1, 1, tw) || conv_lds_row(1, 1, tw, 4) != c4_1x1(tw)) return false;
  }
  return true;
}
static_assert(same(), "conv_lds_row changed a row pitch");
}  // namespace lds_row_was

hipError_t conv_init() {
  static std::mutex mu;
  static bool done = false;
  std::lock_guard<std::mutex> lock(mu);   // executors may be created from several threads
  if (done) return hipSuccess;
  for (const ConvVariant& v : kVariants) {
    const hipError_t e = hipFuncSetAttribute((const void*)v.kern, hipFuncAttributeMaxDynamicSharedMemorySize, v.lds_cap);
    if (e != hipSuccess) return e;
  }
  done = true;
  return hipSuccess;
}

}  // namespace dsx
