// dsx_conv_ws.hip — k_conv_ws, the warp-specialised persistent form of the fused conv (dsx_conv.hip has the overview of
// the families; dsx_conv_mfma.hip describes the operand layouts).  The compute waves' (tile, group) item is
// dsx_conv_ws_item.inc.  The knobs that shape the table's rows (ring depths, images) are in dsx_conv_variants.h.
#include "dsx_conv_variants.h"
#include <algorithm>

// residual prefetch one tile ahead: only with one N block per wave.  With two, the register demand passes 256 and
// hipcc (ROCm 7.2) fails in its spill path ("Illegal instruction detected: Operand has incorrect register class
// V_CMP_NE_U32_e32 0, $src_private_base"); the same happens for a 64 x 256 tile (MB 2, WM 1, WN 4, NB 2).
#ifndef DSX_PRE_RESID_EXPR
#define DSX_PRE_RESID_EXPR (NB == 1 && MB <= 2)   // (MB 4 with 16-bit storage fits the registers but measured 3 % slower)
#endif
#ifndef DSX_PFF_EXPR
#define DSX_PFF_EXPR (NB == 2 ? 3 : 6)   // k_conv_ws: pixel fragments in flight ahead of the MFMAs (~190 cycles of MFMA work)
#endif
#ifndef DSX_WS_K0_EXPR
#define DSX_WS_K0_EXPR 64   // raw groups requested before the first wait (>= P + 1: the whole ring, the round-2 behaviour)
#endif
#ifndef DSX_EPI_PRIO_COND
#define DSX_EPI_PRIO_COND false
#endif
#ifndef DSX_STAMP_CVT_COND
#define DSX_STAMP_CVT_COND (tiC == 2 && gC == 0)   // which item the loader-conversion stamps 120-123 record (diagnostic builds)
#endif
#ifndef DSX_LOADER_PRIO
#define DSX_LOADER_PRIO 3   // (1 until the 16 x 16 MFMA shape made the loaders the bound of most items; A/B in one call: 3 -0.3 %, 0 +0.5 %)
#endif
#ifndef DSX_LOADER_PRIO_EXPR
#define DSX_LOADER_PRIO_EXPR DSX_LOADER_PRIO   // (may name MB, KS, NB: per-tile experiments)
#endif

namespace dsx {

// (the loader -> compute hand-off and its image counters: see ws_nbuf in dsx_conv_variants.h)
// a counter PER WAVE (four words, read with one ds_read_b128): a single shared counter would let three fast waves
// stand in for a slow one, and the image of the item that one is still reading would be overwritten
static __device__ __forceinline__ void lds_wait_all_ge(unsigned addr, int target, unsigned* timeouts) {
  for (int spin = 0; spin < (1 << 18); ++spin) {   // ~30 ms: a hand-off normally takes microseconds
    f32x4_t v;
    asm volatile("ds_read_b128 %0, %1\n\ts_waitcnt lgkmcnt(0)" : "=v"(v) : "v"(addr) : "memory");
    const int4 c = __builtin_bit_cast(int4, v);
    const int m = min(min(c.x, c.y), min(c.z, c.w));
    if (__builtin_amdgcn_readfirstlane(m) >= target) return;
    __builtin_amdgcn_s_sleep(1);
  }
  // gave up: the pixels of this launch are wrong -- say so (the host reads the counter: dsx_exec_handoff_timeouts)
  if (timeouts != nullptr && (threadIdx.x & 63) == 0) atomicAdd(timeouts, 1u);
}
static __device__ __forceinline__ void lds_signal(unsigned addr, int wave, int count) {   // this wave's word := count, behind its own LDS traffic
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  if ((threadIdx.x & 63) == 0) asm volatile("ds_write_b32 %0, %1" ::"v"(addr + 4u * (unsigned)wave), "v"(count) : "memory");
}

// ===========================================================================================
// Warp-specialised, persistent variant (stride 1, sources aligned to the channel group).
//
// Why: inside one wave the activation stream (HBM, ~3 us under load) and the weight-fragment stream
// (L2, ~0.6 us) share ONE in-order vmcnt queue, so neither can be prefetched deeper than the other
// allows, and every phase of k_conv_mfma (load wait, GN+Swish VALU, MFMA, epilogue) ends up serialised.
// Here a workgroup is 8 waves:
//   waves 4-7  LOADERS : LDS-DMA (buffer_load ... lds, no VGPRs) of the raw halo patch P groups ahead
//                        into a ring; units are read back one iteration before use, then GroupNorm
//                        affine + Swish + convert and the MFMA image of the NEXT group; their vmcnt
//                        only ever counts activation DMAs.  s_setprio 1 (see below).
//   waves 0-3  COMPUTE : weight-fragment ring + MFMA on the CURRENT group's image, epilogue + fused
//                        statistics at tile ends; their vmcnt only counts weight / epilogue loads.
// Both pipes of a SIMD stay busy (one loader + one compute wave per SIMD: VALU beside MFMA), the
// workgroup is persistent over M tiles of one N tile (the weight stream stays in L2, the pipelines run
// on across tile boundaries, per-workgroup setup is paid once), and there is one raw s_barrier per
// group (never __syncthreads: its vmcnt(0) would drain the DMA ring).
// ===========================================================================================
//
// DIRECT instantiations (ConvArgs::ws_direct: 1 x 1 convs with neither GroupNorm nor Swish in front).  The image the
// MFMAs read is the activation tile itself, so the loaders only issue LDS-DMAs -- straight into the image of the item P
// items ahead -- wait with a counted vmcnt for the next item's image and take the per-item barrier: no raw ring, no
// fetch, no convert.  An LDS-DMA instruction fills 1 KiB contiguously (lane l at +16 l), so the pixel pitch is the
// unpadded 64 CPG bytes and conflict-free operand reads come from a swizzle on the SOURCE side: LDS slot (pixel m,
// unit j) holds channel unit j ^ sigma(m), sigma(m) = (m >> 1) & 7 (CPG 2) or m & 15 (CPG 4), and the compute waves
// read unit u at slot u ^ sigma(m).  A b128 read group holds the 8 even pixels of a 16-pixel block at K slice s and the
// 8 odd ones at slice s ^ 2 (see mfma16_step).  CPG 2 (128-byte pitch): 16-byte bank slot = 8 (m & 1) + (u ^ sigma):
// the parities take different halves of the bank row, and inside one (m >> 1) & 7 runs over all 8 values.  CPG 4
// (256-byte pitch): slot = u ^ (m & 15): the low bit separates the parities (u and u ^ 2 agree in it), the other three
// run over all values inside a parity.  16 distinct slots either way.  All else (weight stream, MFMA order, epilogue,
// statistics) is the code of the other instantiations, so a direct launch writes the same bytes.
template <typename DT, int MB, int WM, int WN, int NB, int KS, int CPG, int D, int NIT, int P, int LW, bool DIRECT>
__global__ void k_conv_ws(const ConvArgs a) {   // (launch bounds: on the declaration in dsx_conv_variants.h)
  constexpr int LT = 64 * LW;                   // loader threads
  constexpr int S = 1;
  constexpr int KC = Chunk<DT>::KC;
  constexpr int CPU = Unit<DT>::N;              // channels per 16-byte unit (HBM, raw ring and LDS image alike)
  constexpr int ES = (int)sizeof(DT);
  constexpr int UPP = KC / CPU;
  constexpr int UPG = UPP * CPG;
  constexpr int UPG_LOG2 = UPG == 16 ? 4 : (UPG == 8 ? 3 : 2);
  constexpr int UB = 16;
  constexpr int PIXB = DIRECT ? 64 * CPG : 64 * CPG + 16;
  constexpr int TAPS = KS * KS;
  constexpr int PAD = KS / 2;
  constexpr int NSTEP = CPG * TAPS * 2;
  [[maybe_unused]] constexpr bool IS_BF16 = sizeof(DT) == 2;
  constexpr int RAWB = NIT * LT * 16;           // one raw ring slot
  constexpr int NSLOT = P + 1;
  static_assert(D <= NSTEP ? NSTEP % D == 0 : (D % NSTEP == 0 && D / NSTEP <= 8), "ring depth divides the steps per group, or is a multiple of them");
  static_assert(WM * WN == 4 && P * NIT < 64, "4 compute waves; vmcnt is 6 bits");

  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int tid = threadIdx.x;
  DSX_STAMP_T(63, tid == 0);                    // kernel entry (diagnostic builds): stamp 0 - stamp 63 = the start-up ramp
  const int lane = tid & 63;
  const int wave8 = __builtin_amdgcn_readfirstlane(tid >> 6);
  const bool loader = wave8 >= 4;
  const int wave = loader ? wave8 - 4 : wave8;  // index inside the role
  const int ltid = loader ? tid - 256 : tid;
  const int c16 = lane & 15, kq = lane >> 4;     // compute waves: MFMA column (pixel) / K slice and output row group (see mfma16_step)

  const int TW = 1 << a.tw_log2, TH = 1 << a.th_log2;
  const int PW = (TW - 1) * S + KS;
  const int PH = (TH - 1) * S + KS;
  const int PPI = PH * PW;
  const int PP = PPI << a.tb_log2;
  const int RB = a.lds_row;
  const int BUFB = DIRECT ? 32 * MB * WM * PIXB : (PH << a.tb_log2) * RB;   // (direct: pixel m of the tile at m PIXB)
  // [image 0 .. NBUF-1][GroupNorm scale/shift of three tiles' images][raw ring][FULL, FREE counters]
  constexpr int NBUF = ws_nbuf(32 * MB * WM, KS, NB, CPG);
  static_assert(NBUF >= 2 && NBUF <= 4, "two images and a barrier, or three / four and counters");
  constexpr int NIMG = DIRECT ? P + 1 : NBUF;   // images the items rotate through (direct: the barrier hand-off of NBUF == 2)
  static_assert(!DIRECT || (KS == 1 && NBUF == 2 && NIT * LT == 32 * MB * WM * UPG), "direct: 1 x 1, one barrier per item, whole DMA instructions");
  const int C = a.C0 + a.C1;
  const int AFFB = a.has_gn ? ((2 * C * 4 + 15) & ~15) : 0;     // bytes of one tile's {scale[C], shift[C]}
  float* const aff_base = (float*)(lds + NBUF * BUFB);
  unsigned char* const raw_base = lds + NBUF * BUFB + 3 * AFFB;
  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;  // LDS byte address of lds[0]
  const unsigned full_addr = lds0 + NBUF * BUFB + 3 * AFFB + NSLOT * RAWB;   // FULL[4 loader waves], FREE[4 compute waves] at +16 (NBUF == 3)
  const int G = a.kchunks / CPG;                // channel groups per tile (no split-K here; host: G >= 2, TB == 1)

  // persistent work list: this workgroup owns N tile `nt` and M tiles p, p+wpn, ...
  // XCD-aware: workgroups are dealt round-robin over the 8 XCDs (blockIdx % 8 labels the L2 they
  // share), so an N tile's workgroups are pinned to as few XCDs as possible and every L2 only
  // streams its own slice of the weights (placement affects speed only, never results).
  const int wpn = a.ws_wg_per_n;
  int nt, p0;
  {
    // (no integer divisions here or below: the host passes quotients and fastdiv magics, see ConvArgs::ws_map)
    const int bid = blockIdx.x, xcd = bid & 7, k = bid >> 3;
    if (a.ws_map == 0) {                         // n_tiles in {1, 2, 4, 8} and wpn a multiple of 8 / n_tiles
      const int lg = a.ws_nt_log2, band = xcd >> lg;
      nt = xcd & ((1 << lg) - 1);
      // each XCD owns a contiguous band of M tiles (neighbouring tiles share halo rows in its L2) ...
      if (a.xcd_bands) p0 = band * (wpn >> (3 - lg)) + k;
      else p0 = (k << (3 - lg)) + band;          // ... or tiles dealt round-robin (DSX_XCD_BANDS=0)
    } else if (a.ws_map == 1) {                  // n_tiles a multiple of 8
      const int kq = (int)fastdiv((unsigned)k, a.mg_per);
      nt = xcd + 8 * (k - kq * a.ws_per);
      p0 = kq;
    } else if (a.ws_map == 3) {                  // 1 x 1 convs: XCD x owns the M tiles p = x (mod 8) for EVERY N tile -- their
      const int j = (int)fastdiv((unsigned)k, a.mg_per);   // weights are small, the input is what the L2s would otherwise
      nt = k - j * a.ws_per;                     // all fetch; consecutive workgroups of an XCD share the M tile
      p0 = (j << 3) + xcd;                       // (host: ws_per = n_tiles, wpn a multiple of 8)
    } else {
      nt = (int)fastdiv((unsigned)bid, a.mg_wpn);
      p0 = bid - nt * wpn;
    }
  }
  // (m_tiles - p0 + wpn - 1) / wpn; one tile per workgroup is the common case
  const int ntile = wpn >= a.m_tiles ? (p0 < a.m_tiles ? 1 : 0)
                                     : (a.ws_bigdiv ? (a.m_tiles - p0 + wpn - 1) / wpn
                                                                : (int)fastdiv((unsigned)(a.m_tiles - p0 + wpn - 1), a.mg_wpn));
  const int total = ntile * G;                  // (tile, group) items, in order

  if (loader) {
    // ======================================================================= LOADER WAVES
    // The loader waves are dispatched after the compute waves, and vector issue on a SIMD is arbitrated by
    // priority, then age: as the younger wave their GroupNorm/Swish VALU stream only gets the slots the MFMA
    // wave leaves over, and they become the critical path.  Static priority for the whole kernel.
    __builtin_amdgcn_s_setprio(DSX_LOADER_PRIO_EXPR);
    if constexpr (DIRECT) {
      // unit it LT + ltid of an item is (pixel it (LT / UPG) + ltid / UPG, slot ltid % UPG): LT / UPG is a multiple of
      // 16, so sigma -- and with it the channel unit this thread fetches -- is the same for all of its units
      const int pix0 = ltid >> UPG_LOG2;
      const int srcu = (ltid & (UPG - 1)) ^ (CPG == 4 ? (pix0 & 15) : ((pix0 >> 1) & 7));
      int rel[NIT];             // source pixel offset relative to the tile's first pixel
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const int m = pix0 + it * (LT >> UPG_LOG2);
        rel[it] = (m >> a.tw_log2) * a.Ws + (m & (TW - 1));
      }
      const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc(
          (void*)a.src0, 0, (int)min((long long)a.B * a.Hs * a.Ws * a.C0 * ES, 0x7fffffffLL), 0x00020000);
      const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(a.src1 ? a.src1 : a.src0), 0,
          a.src1 ? (int)min((long long)a.B * a.Hs * a.Ws * a.C1 * ES, 0x7fffffffLL) : 0, 0x00020000);
      const int adv_x = a.ws_adv_x, adv_y = a.ws_adv_y, adv_b = a.ws_adv_b;
      int tx, ty, tb;                                                            // tile being issued
      {
        const int q1 = (int)fastdiv((unsigned)p0, a.mg_tiles_x);                  // p0 / tiles_x
        tb = (int)fastdiv((unsigned)p0, a.mg_per_img);
        tx = p0 - q1 * a.tiles_x;
        ty = q1 - tb * a.tiles_y;
      }
      auto tile_base = [&]() __attribute__((always_inline)) -> int {
        return (tb * a.Hs + (ty << a.th_log2)) * a.Ws + (tx << a.tw_log2);
      };
      int baseI = tile_base(), gI = 0, issued = 0, bufI = 0;
      // DMA item (tile, gI) into image bufI; every wave issues exactly NIT instructions.  Channel units past C are out
      // of the descriptor's range: the bounds check fills them with zeros
      auto issue_next = [&]() __attribute__((always_inline)) {
        const int c = gI * (CPG * KC) + srcu * CPU;
        const bool first = gI * (CPG * KC) < a.C0;            // uniform: a group never straddles the sources
        const int cs = first ? a.C0 : a.C1;
        const unsigned coff = c < C ? (unsigned)((first ? c : c - a.C0) * ES) : 0x80000000u;
        unsigned char* dst = lds + bufI * BUFB + wave * 1024;
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          const unsigned vo = c < C ? (unsigned)(baseI + rel[it]) * (unsigned)(cs * ES) + coff : 0x80000000u;
          auto ldst = (__attribute__((address_space(3))) void*)(dst + it * (LT * 16));
          if (first) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, ldst, 16, vo, 0, 0, 0);
          else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, ldst, 16, vo, 0, 0, 0);
        }
        ++issued;
        if (++bufI == NIMG) bufI = 0;
        if (++gI == G) {
          gI = 0;
          tx += adv_x;
          if (tx >= a.tiles_x) { tx -= a.tiles_x; ty += 1; }
          ty += adv_y;
          if (ty >= a.tiles_y) { ty -= a.tiles_y; tb += 1; }
          tb += adv_b;
          baseI = tile_base();
        }
      };
      // wait until the DMAs of an item have landed; `young` = items requested after it, which may stay in flight
      auto wait_young = [&](int young) __attribute__((always_inline)) {
        if (young >= P) wait_vmcnt<P * NIT>();
        else static_for<P>([&](auto jc) __attribute__((always_inline)) {
          if (young == decltype(jc)::value) wait_vmcnt<decltype(jc)::value * NIT>();
        });
        __builtin_amdgcn_sched_barrier(0);
      };
      DSX_STAMP_T(110, tid == 256);       // tables built
      while (issued < NIMG && issued < total) issue_next();   // every image is free
      DSX_STAMP_T(111, tid == 256);       // first DMAs issued
      ws_barrier();                       // (the compute waves' start-up barrier)
      if (total > 0) wait_young(issued - 1);
      DSX_STAMP_T(112, tid == 256);       // item 0 has landed
      ws_barrier();                       // image of item 0 is ready
      DSX_STAMP_T(64, tid == 256);
      for (int v = 0; v < total; ++v) {
        DSX_STAMP_T(65 + 4 * v, tid == 256 && v < 9);
        DSX_STAMP_T(66 + 4 * v, tid == 256 && v < 9);
        if (v + 1 < total) wait_young(issued - (v + 2));   // item v + 1 has landed (all of this wave's units of it)
        DSX_STAMP_T(67 + 4 * v, tid == 256 && v < 9);
        ws_barrier();                     // the compute waves are done with item v: its image is free, item v + 1 is complete
        DSX_STAMP_T(68 + 4 * v, tid == 256 && v < 9);
        if (issued < total) issue_next();   // item v + NIMG into the image of item v
      }
      return;
    }
    // Per-thread, tile-invariant description of its NIT units: LDS image offset, source pixel offset
    // relative to the tile's origin pixel, and which patch borders the unit lies on.  Per tile only the
    // origin offset and four "tile touches the image border" flags change (no divisions, no per-unit
    // bounds arithmetic): zero padding is exactly the border units of border tiles.
    struct TilePos { int tx, ty, b; };
    const int adv_x = a.ws_adv_x, adv_y = a.ws_adv_y, adv_b = a.ws_adv_b;
    auto tile_advance = [&](TilePos& t) __attribute__((always_inline)) {
      t.tx += adv_x;
      if (t.tx >= a.tiles_x) { t.tx -= a.tiles_x; t.ty += 1; }
      t.ty += adv_y;
      if (t.ty >= a.tiles_y) { t.ty -= a.tiles_y; t.b += 1; }
      t.b += adv_b;
    };
    auto tile_flags = [&](const TilePos& t) __attribute__((always_inline)) -> int {   // bit0 top, bit1 bottom, bit2 left, bit3 right
      return (PAD == 0) ? 0
                        : ((t.ty == 0 ? 1 : 0) | (t.ty == a.tiles_y - 1 ? 2 : 0) | (t.tx == 0 ? 4 : 0) |
                           (t.tx == a.tiles_x - 1 ? 8 : 0));
    };
    // source pixel index of the patch origin's *output* pixel (oy0, ox0); `rel` is added to it
    auto tile_base = [&](const TilePos& t) __attribute__((always_inline)) -> int {
      const int oy0 = t.ty << a.th_log2, ox0 = t.tx << a.tw_log2;   // even whenever a.up (TW, TH >= 2)
      return (t.b * a.Hs + (a.up ? oy0 >> 1 : oy0)) * a.Ws + (a.up ? ox0 >> 1 : ox0);
    };
    const int nunits = PP << UPG_LOG2;
    const int cvg = ltid & (UPG - 1);
    int loff[NIT];            // LDS image offset of each unit, -1: no such unit
    int rel[NIT];             // source pixel offset relative to tile_base
    int edge[NIT];            // border bits of the unit's patch pixel
    {
      constexpr int PSTEP = LT >> UPG_LOG2;
      const int pix0 = ltid >> UPG_LOG2;
      static_assert(PSTEP < 65536, "fastdiv range");
      int py = (int)fastdiv((unsigned)pix0, a.mg_pw);
      int px = pix0 - py * PW;
      const int dpy = a.ws_dpy, dpx = a.ws_dpx;   // PSTEP / PW and the remainder
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const bool have = ltid + it * LT < nunits;
        loff[it] = have ? py * RB + px * PIXB + cvg * UB : -1;
        const int ry = py - PAD, rx = px - PAD;   // relative to the tile's first output pixel (input grid)
        // nearest x2 upsample: source = floor(input / 2); the origin is even, so floor((o + r) / 2) = o/2 + (r >> 1)
        rel[it] = a.up ? (ry >> 1) * a.Ws + (rx >> 1) : ry * a.Ws + rx;
        edge[it] = (PAD == 0) ? 0 : ((py == 0 ? 1 : 0) | (py == PH - 1 ? 2 : 0) | (px == 0 ? 4 : 0) | (px == PW - 1 ? 8 : 0));
        px += dpx; py += dpy;
        if (px >= PW) { px -= PW; py += 1; }
      }
    }

    const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)a.src0, 0, (int)min((long long)a.B * a.Hs * a.Ws * a.C0 * ES, 0x7fffffffLL), 0x00020000);
    const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(
        (void*)(a.src1 ? a.src1 : a.src0), 0,
        a.src1 ? (int)min((long long)a.B * a.Hs * a.Ws * a.C1 * ES, 0x7fffffffLL) : 0, 0x00020000);

    TilePos posI;                                                                // tile being issued
    {
      const int q1 = (int)fastdiv((unsigned)p0, a.mg_tiles_x);                  // p0 / tiles_x
      posI.b = (int)fastdiv((unsigned)p0, a.mg_per_img);
      posI.tx = p0 - q1 * a.tiles_x;
      posI.ty = q1 - posI.b * a.tiles_y;
    }
    TilePos posC = posI;                                                         // tile being consumed
    int baseI = tile_base(posI), flagsI = tile_flags(posI), flagsC = flagsI;
    int gI = 0;               // group of the next item to issue
    int tiC = 0;              // tile of the next item to consume
    int gC = 0;               // its group
    int affslot = 0;          // tiC % 3: LDS slot of that tile's scale/shift

    // DMA the raw patch of item (tiI, gI) into ring slot `slot`; every wave issues exactly NIT instructions
    auto issue = [&](int slot) __attribute__((always_inline)) {
      const int c = gI * (CPG * KC) + cvg * CPU;
      const bool first = gI * (CPG * KC) < a.C0;            // uniform: a group never straddles the sources
      const int cs = first ? a.C0 : a.C1;
      const unsigned coff = c < C ? (unsigned)((first ? c : c - a.C0) * ES) : 0x80000000u;
      unsigned char* dst = raw_base + slot * RAWB + wave * 1024;
#pragma unroll
      for (int it = 0; it < NIT; ++it) {
        const bool ok = loff[it] >= 0 && (edge[it] & flagsI) == 0;
        const unsigned vo = ok ? (unsigned)(baseI + rel[it]) * (unsigned)(cs * ES) + coff : 0x80000000u;
        auto ldst = (__attribute__((address_space(3))) void*)(dst + it * (LT * 16));
        if (first) __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, ldst, 16, vo, 0, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, ldst, 16, vo, 0, 0, 0);
      }
      if (++gI == G) {
        gI = 0;
        tile_advance(posI);
        baseI = tile_base(posI); flagsI = tile_flags(posI);
      }
    };
    // Item (tiC, gC) goes raw slot -> registers (fetch) -> GroupNorm affine + Swish -> MFMA image (convert).
    // The two halves run one iteration apart: the LDS reads of item v+2 are issued before the barrier of
    // iteration v and are long complete when iteration v+1 converts them (the LDS queue is busy with the
    // compute waves' operand reads, so a read-then-wait inside one iteration costs hundreds of cycles).
    constexpr int NA = CPU / 4;          // 16-byte pieces of scale (and of shift) per unit
    f32x4_t av[2 * NA], rv[NIT];
    int cF = 0, flagsF = 0;              // channel offset / border flags of the fetched item
    bool gnF = false;
    // fetch: scale/shift (parked in LDS by the compute waves -- an ordinary global load here would make the
    // compiler wait vmcnt(0) and drain the DMA ring) and the raw units of item (tiC, gC); advances (tiC, gC)
    auto fetch = [&](int slot) __attribute__((always_inline)) {
      cF = gC * (CPG * KC) + cvg * CPU;
      flagsF = flagsC;
      gnF = a.gn_scale != nullptr && cF < C;
      if constexpr (NBUF >= 3) {
        // the scale/shift slot of tile t (t >= 3) is written by the compute waves' epilogue of tile t - 3, which is
        // over once they have consumed the first item of tile t - 2 (with the per-item barrier of NBUF == 2 the
        // three-tile lead alone guarantees this; running ahead, the loaders ask)
        if (gnF && gC == 0 && tiC >= 3) lds_wait_all_ge(full_addr + 16, (tiC - 2) * G + 1, a.handoff_timeouts);
      }
      const unsigned src = lds0 + NBUF * BUFB + 3 * AFFB + slot * RAWB + ltid * 16;
      if (gnF) {
        const unsigned af = lds0 + NBUF * BUFB + affslot * AFFB;   // slot tiC % 3
#pragma unroll
        for (int q = 0; q < NA; ++q) {
          asm volatile("ds_read_b128 %0, %1" : "=v"(av[q]) : "v"(af + (cF + 4 * q) * 4) : "memory");
          asm volatile("ds_read_b128 %0, %1" : "=v"(av[NA + q]) : "v"(af + (C + cF + 4 * q) * 4) : "memory");
        }
      }
#pragma unroll
      for (int it = 0; it < NIT; ++it)
        asm volatile("ds_read_b128 %0, %1" : "=v"(rv[it]) : "v"(src + it * (LT * 16)) : "memory");
      if (++gC == G) {
        gC = 0; ++tiC;
        if (++affslot == 3) affslot = 0;
        tile_advance(posC);
        flagsC = tile_flags(posC);
      }
    };
    auto convert = [&](int buf) __attribute__((always_inline)) {
      const unsigned dst = lds0 + buf * BUFB;
      // the wait, then empty volatile asms that every read's result passes through: volatile asms keep their
      // order, so no use of a result can be scheduled above the wait
      DSX_STAMP_T(120, tid == 256 && DSX_STAMP_CVT_COND);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
      for (int q = 0; q < 2 * NA; ++q) asm volatile("" : "+v"(av[q]));
#pragma unroll
      for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(rv[it]));
      DSX_STAMP_T(121, tid == 256 && DSX_STAMP_CVT_COND);
      // lanes without a GroupNorm in front (gnF is per lane: channels past C) multiply by 1 and add 0 -- exact -- so the
      // unit loop has one unconditional packed fma per pair instead of a select per element
      float sc[CPU], sh[CPU];
#pragma unroll
      for (int q = 0; q < NA; ++q) {
        sc[4 * q] = gnF ? av[q].x : 1.0f; sc[4 * q + 1] = gnF ? av[q].y : 1.0f;
        sc[4 * q + 2] = gnF ? av[q].z : 1.0f; sc[4 * q + 3] = gnF ? av[q].w : 1.0f;
        sh[4 * q] = gnF ? av[NA + q].x : 0.0f; sh[4 * q + 1] = gnF ? av[NA + q].y : 0.0f;
        sh[4 * q + 2] = gnF ? av[NA + q].z : 0.0f; sh[4 * q + 3] = gnF ? av[NA + q].w : 0.0f;
      }
      const bool any_gn = a.gn_scale != nullptr;   // uniform
      // one uniform branch around the whole unit loop (a branch per unit keeps the units' arithmetic from interleaving):
      // residual / attention-output 1 x 1 convs and the upsampling convs have no GroupNorm / Swish in front and copy
      // (1 x 1 only: in the 3 x 3 instantiations the extra branch cost the GroupNorm layers 3-4 %, more than the four
      // upsampling convs gained)
      const bool plain = KS == 1 && !(gnF || a.swish);
      if (plain) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          if (loff[it] >= 0) {
            uint4 w = __builtin_bit_cast(uint4, rv[it]);
            const unsigned keep = ((edge[it] & flagsF) == 0 && cF < C) ? 0xffffffffu : 0u;
            w.x &= keep; w.y &= keep; w.z &= keep; w.w &= keep;
            lds_write_b128_asm(dst + loff[it], __builtin_bit_cast(f32x4_t, w));
          }
        }
      } else {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
          if (loff[it] >= 0) {
            float v[CPU];
            Unit<DT>::unpack(__builtin_bit_cast(uint4, rv[it]), v);
            // the arithmetic runs in every lane; padding pixels (and channels past C) are forced to exactly 0
            // afterwards with one mask per packed register (padded AFTER the activation, as the reference does)
#ifndef DSX_ABL_CVT   // -DDSX_ABL_CVT: timing experiment, loaders skip the GroupNorm / Swish arithmetic (results wrong)
            if (any_gn) affine_vec(v, sc, sh);
            if (a.swish) swish_vec(v);
#endif
            if (it == NIT - 1) { asm volatile("" :: "v"(v[0]), "v"(v[CPU - 1])); DSX_STAMP_T(122, tid == 256 && DSX_STAMP_CVT_COND); }
            uint4 w = Unit<DT>::pack(v);
            const unsigned keep = ((edge[it] & flagsF) == 0 && cF < C) ? 0xffffffffu : 0u;
            w.x &= keep; w.y &= keep; w.z &= keep; w.w &= keep;
            lds_write_b128_asm(dst + loff[it], __builtin_bit_cast(f32x4_t, w));
          }
        }
      }
      DSX_STAMP_T(123, tid == 256 && DSX_STAMP_CVT_COND);
    };
    // wait until the DMAs of the item to fetch have landed; `young` = younger items that may stay in flight
    auto wait_young = [&](int young) __attribute__((always_inline)) {
      if (young >= P) wait_vmcnt<P * NIT>();
      else if (P > 1 && young == P - 1) wait_vmcnt<(P > 1 ? (P - 1) * NIT : 0)>();
      else if (P > 2 && young == P - 2) wait_vmcnt<(P > 2 ? (P - 2) * NIT : 0)>();
      else if (P > 3 && young == P - 3) wait_vmcnt<(P > 3 ? (P - 3) * NIT : 0)>();
      else wait_vmcnt<0>();
      __builtin_amdgcn_sched_barrier(0);
    };

    int issued = 0, slotI = 0, slotF = 0;   // items issued; ring slot of the next issue / next fetch
    auto issue_next = [&]() __attribute__((always_inline)) {
      issue(slotI);
      ++issued;
      if (++slotI == NSLOT) slotI = 0;
    };
    auto fetch_next = [&]() __attribute__((always_inline)) {
      fetch(slotF);
      if (++slotF == NSLOT) slotF = 0;
    };
    DSX_STAMP_T(110, tid == 256);       // tables built
    // Start-up ramp: with every CU issuing at once an LDS-DMA instruction takes ~200 cycles to issue, and the first
    // item's data has landed long before all P + 1 ring slots are requested.  Only the first K0 items are requested
    // up front; the ring fills up (at most two requests per iteration) while the first images are converted.
    // `young` of a wait is counted from `issued`: requests issued after the item waited for.
    constexpr int K0 = DSX_WS_K0_EXPR < NSLOT ? DSX_WS_K0_EXPR : NSLOT;
    while (issued < K0 && issued < total) issue_next();
    DSX_STAMP_T(111, tid == 256);       // first DMAs issued
    ws_barrier();                       // scale/shift of tiles 0 and 1 are in LDS
    wait_young(issued - 1);
    DSX_STAMP_T(112, tid == 256);       // item 0 has landed
    fetch_next();                       // item 0
    for (int k = 0; k < 2 && issued < total && issued < NSLOT; ++k) issue_next();   // (in flight during the conversion)
    convert(0);
    if constexpr (NBUF >= 3) { if (total > 0) lds_signal(full_addr, wave, 1); }   // item 0 is ready
    DSX_STAMP_T(113, tid == 256);       // item 0 converted
    if (total > 1) {
      wait_young(issued - 2);
      fetch_next();                     // item 1
    }
    if constexpr (NBUF == 2) ws_barrier();   // image of item 0 is ready
    DSX_STAMP_T(64, tid == 256);
    int bufL = 1;                       // image buffer of item v + 1
    for (int v = 0; v < total; ++v) {
      // the slots of items <= v were copied to registers an iteration or more ago: items up to v + NSLOT may be requested
      for (int k = 0; k < 2 && issued < total && issued < v + 1 + NSLOT; ++k) issue_next();
      DSX_STAMP_T(65 + 4 * v, tid == 256 && v < 9);
      if (v + 1 < total) {
        if constexpr (NBUF >= 3) {
          // buffer (v + 1) % NBUF held item v + 1 - NBUF: every compute wave must have released it (v + 2 - NBUF items consumed)
          if (v + 1 >= NBUF) lds_wait_all_ge(full_addr + 16, v + 2 - NBUF, a.handoff_timeouts);
          convert(bufL);
          lds_signal(full_addr, wave, v + 2);     // items 0 .. v + 1 are ready
        } else {
          convert((v + 1) & 1);
        }
      }
      if (++bufL == NBUF) bufL = 0;
      DSX_STAMP_T(66 + 4 * v, tid == 256 && v < 9);
      if (v + 2 < total) {
        wait_young(issued - (v + 3));
        fetch_next();                   // item v+2
      }
      DSX_STAMP_T(67 + 4 * v, tid == 256 && v < 9);
      if constexpr (NBUF == 2) ws_barrier();
      DSX_STAMP_T(68 + 4 * v, tid == 256 && v < 9);
    }
    return;
  }

  // ========================================================================= COMPUTE WAVES
  // Each wave owns MB row blocks of 32 pixels (two 16-pixel MFMA column blocks, ph = 0 / 1) x NB 32-channel N blocks.
  // A pixel fragment read from LDS feeds 2 NB MFMAs (both 16-channel halves of every N block).
  const int wm = wave / WN, wn = wave % WN;
  const int pq = ws16_pixel(c16);               // this lane's pixel inside a 16-pixel block
  constexpr int AD = DIRECT ? CPG : KS;         // fragment base addresses per row block: one per tap row, or (direct: the
                                                // swizzle reaches the chunk bits, so no `cg * 64` immediate) one per chunk
  int abase[MB][AD];                            // ph = 0; the ph = 1 block is `a16` bytes further (uniform)
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = (wm * MB + mb) * 32 + pq;
    if constexpr (DIRECT) {
      const int sg = CPG == 4 ? (m & 15) : ((m >> 1) & 7);   // sigma(m) == sigma(m + 16)
#pragma unroll
      for (int cg = 0; cg < AD; ++cg) abase[mb][cg] = m * PIXB + (((cg * 4 + ws16_slice(kq)) ^ sg) << 4);
      continue;
    }
    const int tx = m & (TW - 1);
    const int ty = (m >> a.tw_log2) & (TH - 1);
    const int tb = m >> (a.tw_log2 + a.th_log2);
#pragma unroll
    for (int dy = 0; dy < KS; ++dy)
      abase[mb][DIRECT ? 0 : dy] = (tb * PH + ty * S + dy) * RB + tx * S * PIXB + ws16_slice(kq) * 16;
  }
  // pixel m + 16 of a row block: 16 pixels to the right (tiles >= 32 wide), else 16 / TW rows down.  (host: TB == 1 and
  // TW a power of two <= 16 -- 2 and 4 included, see tile_geometry -- so TW TH >= 64 and the 32 pixels of a row block
  // are 32 / TW whole rows of one image.)
  const int a16 = DIRECT ? 16 * PIXB : (TW >= 32 ? 16 * S * PIXB : (16 >> a.tw_log2) * S * RB);
  const int blk0 = (nt * WN + wn) * NB;         // host: Cout % (32 * WN * NB) == 0, so every block exists
  const int wblock = G * (NSTEP * 1024);        // bytes of one N block's fragment stream
  const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const unsigned char*)a.wpack + (size_t)blk0 * wblock), 0, NB * wblock, 0x00020000);
  // pack_conv's stream holds, per (chunk, tap), two 1 KiB fragments of the 32x32x16 shape; the 16 x 16 fragments ch = 0 / 1
  // of the same 32 channels x 32 K are a per-lane gather from that 2 KiB pair (every byte of it is read exactly once)
  const int wlane[2] = {ws16_woff(lane, 0), ws16_woff(lane, 1)};
  static_assert(D % 2 == 0 && NSTEP % 2 == 0, "ring slots alternate between the two fragments of a pair");
  const int qtot = G * NSTEP;                   // the stream restarts at every tile (same N blocks)
  int qn = 0;                                   // next step (fragment) to prefetch (wraps); its parity is the static `ch`
  struct WFrag { uint4 v[NB]; };                // one step's weight fragments (by value: stays in registers)
  auto load_b = [&](auto chc) __attribute__((always_inline)) -> WFrag {
    constexpr int ch = decltype(chc)::value;
    WFrag f;
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
      f.v[nb] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsw, wlane[ch], nb * wblock + (qn >> 1) * 2048, 0));
    if (++qn == qtot) qn = 0;
    return f;
  };
  WFrag bq[D];
  static_for<D>([&](auto jc) __attribute__((always_inline)) {
    bq[decltype(jc)::value] = load_b(std::integral_constant<int, (decltype(jc)::value & 1)>{});
  });

  f32x16 acc[MB][NB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.0f;

  const bool do_stats = a.stat_part != nullptr;
  const int nbase = blk0 * 32 + 8 * kq;         // this lane's 8 consecutive channels of N block 0 (+32 per block)

  // Tile walk without divisions: (tx, ty, image) of tile p0 + k*wpn, advanced by the decomposed stride.
  struct TilePos { int tx, ty, b; };
  const int per_img = a.tiles_x * a.tiles_y;
  const int adv_x = a.ws_adv_x, adv_y = a.ws_adv_y, adv_b = a.ws_adv_b;
  auto tile_advance = [&](TilePos& t) __attribute__((always_inline)) {
    t.tx += adv_x;
    if (t.tx >= a.tiles_x) { t.tx -= a.tiles_x; t.ty += 1; }
    t.ty += adv_y;
    if (t.ty >= a.tiles_y) { t.ty -= a.tiles_y; t.b += 1; }
    t.b += adv_b;
  };
  // element offsets (32-bit; host: tensors < 2^31 elements) of this lane's output rows: a tile-invariant
  // per-row part, precomputed, plus a wave-uniform per-tile part -> no per-tile vector multiplies
  int orow[MB], rrow[MB];                       // ph = 0; the pixel of ph = 1 is `p16` output pixels further (uniform)
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = (wm * MB + mb) * 32 + pq;
    const int pix = (m >> a.tw_log2) * a.Wo + (m & (TW - 1));
    orow[mb] = pix * a.out_ld + nbase;
    rrow[mb] = pix * a.resid_ld + nbase;
  }
  const int p16 = TW >= 32 ? 16 : (16 >> a.tw_log2) * a.Wo;
  const int o16 = p16 * a.out_ld, r16 = p16 * a.resid_ld;
  auto tile_pixel0 = [&](const TilePos& t) __attribute__((always_inline)) -> int {   // first output pixel of tile t (uniform)
    return (t.b * a.Ho + (t.ty << a.th_log2)) * a.Wo + (t.tx << a.tw_log2);
  };
  TilePos cur;             // tile ti (being multiplied)
  {
    const int q1 = (int)fastdiv((unsigned)p0, a.mg_tiles_x);
    cur.b = (int)fastdiv((unsigned)p0, a.mg_per_img);
    cur.tx = p0 - q1 * a.tiles_x;
    cur.ty = q1 - cur.b * a.tiles_y;
  }
  TilePos nxt = cur;       // tile ti + 1
  tile_advance(nxt);
  TilePos nn = nxt;        // tile ti + 2
  tile_advance(nn);

  // GroupNorm scale/shift of image b -> LDS parity slot, for the loader waves (host: C <= 1024)
  auto load_aff = [&](int b, int slot) __attribute__((always_inline)) {
    if (DIRECT || a.gn_scale == nullptr || tid * 4 >= C) return;   // (direct: no GroupNorm in front, no slots in LDS)
    float* dst = aff_base + (size_t)slot * (AFFB / 4);
    *(float4*)(dst + tid * 4) = *(const float4*)(a.gn_scale + (size_t)b * C + tid * 4);
    *(float4*)(dst + C + tid * 4) = *(const float4*)(a.gn_shift + (size_t)b * C + tid * 4);
  };
  // Three slots (tile % 3).  The scale/shift of tile t is written by the epilogue of tile t-3, i.e. it is visible
  // after the barrier that ends item (t-2)*G, and the loaders first read it when they fetch item t*G, after the
  // barrier that ends item t*G - 3: safe for every G >= 2.  (With two slots and a lead of two tiles the fetch of a
  // G = 2 layer raced with the epilogue that writes the slot.)
  TilePos n3 = nn;         // tile ti + 3
  tile_advance(n3);
  load_aff(cur.b, 0);
  if (ntile > 1) load_aff(nxt.b, 1);
  if (ntile > 2) load_aff(nn.b, 2);

  // Epilogue operands live in registers and are fetched one tile ahead, at the start of the previous tile's
  // epilogue (right after its own operands were consumed): the loads then have the rest of that epilogue
  // plus the ring's steps to land before an in-order vmcnt wait of the weight ring can trip over them.
  // One per-channel addend: the FiLM vector of the tile's image (the host folds the conv bias into the FiLM
  // bias, see dsx_model_finalize) or, without FiLM, the conv bias, fetched once (the workgroup never changes
  // its N tile).  Missing operands stay 0.0f: adding them is exact.
  constexpr int NR = 8 / CPU;    // 16-byte pieces of a lane's 8 residual values of one pixel
  const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 addv[NB][2], affv[2];
  constexpr bool PRE_RESID = DSX_PRE_RESID_EXPR;   // else the residual is read in the epilogue
  uint4 residv[PRE_RESID ? MB : 1][NB][2][NR];   // [row block][N block][ph][piece]; storage type; all-zero bits are 0.0 in both
  // (a uniform branch, not `cond ? *ptr : zero4`: hipcc turns that select into a flat load through a pointer select
  // between the global vector and a private copy of zero4 -- scratch, flat loads, and the addrspacecast that its spill
  // path later fails on with "Operand has incorrect register class ... $src_private_base")
#pragma unroll
  for (int nb = 0; nb < NB; ++nb)
#pragma unroll
    for (int j = 0; j < 2; ++j) addv[nb][j] = zero4;
  if (a.bias && !a.film) {
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int j = 0; j < 2; ++j) addv[nb][j] = *(const float4*)(a.bias + nbase + 32 * nb + 4 * j);
  }
#pragma unroll
  for (int mb = 0; mb < (PRE_RESID ? MB : 1); ++mb)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
      for (int ph = 0; ph < 2; ++ph)
#pragma unroll
        for (int q = 0; q < NR; ++q) residv[mb][nb][ph][q] = make_uint4(0u, 0u, 0u, 0u);
  affv[0] = affv[1] = zero4;
  // t: the tile whose epilogue will use the operands; b_aff: image of the tile three after it
  auto prefetch_epilogue = [&](const TilePos& t, bool want_aff, int b_aff) __attribute__((always_inline)) {
    if (a.film) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          addv[nb][j] = *(const float4*)(a.film + (size_t)t.b * a.film_bs + nbase + 32 * nb + 4 * j);
    }
    if (PRE_RESID && a.resid) {
      const int r0 = tile_pixel0(t) * a.resid_ld;
#pragma unroll
      for (int mb = 0; mb < (PRE_RESID ? MB : 1); ++mb)
#pragma unroll
        for (int ph = 0; ph < 2; ++ph) {
          const DT* rp = (const DT*)a.resid + (r0 + rrow[mb] + ph * r16);
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int q = 0; q < NR; ++q) residv[mb][nb][ph][q] = *(const uint4*)(rp + 32 * nb + CPU * q);
        }
    }
    if (!DIRECT && want_aff && a.gn_scale != nullptr && tid * 4 < C) {
      affv[0] = *(const float4*)(a.gn_scale + (size_t)b_aff * C + tid * 4);
      affv[1] = *(const float4*)(a.gn_shift + (size_t)b_aff * C + tid * 4);
    }
  };
  prefetch_epilogue(cur, ntile > 3, n3.b);

  // Until the loaders have staged the first image the compute waves only wait (one DMA round trip plus a conversion).
  // A residual 1 x 1 conv uses that time for the finalize of the GroupNorm between the two 3 x 3 convs of its block
  // (its statistics were complete before this launch started): one (image, group) item per compute wave, plus that
  // GroupNorm's consumer's L2 weight prefetch -- one k_gn_finalize launch less per block.
  // Every launch also uses the wait to pull the NEXT conv launch's weight slices into the L2s that will read them.
  // (not in the two-N-block 3 x 3 instantiation: it is at the register limit, and the extra live values cost its main
  // loop 10 %)
  constexpr bool PF_OK = !(NB == 2 && KS == 3);
  // (folded into one register at once: these waves wait for the first image anyway, and the main loop has no registers to spare)
  unsigned fin_pf_acc = 0u;
  if constexpr (PF_OK) fin_pf_acc = l2_prefetch_fold(l2_prefetch(a.pf, blockIdx.x, gridDim.x, tid, 256));
  if constexpr (KS == 1) {
    if (a.fin_on) {
      fin_pf_acc |= l2_prefetch_fold(l2_prefetch(a.fin.pf, blockIdx.x, gridDim.x, tid, 256));
      const int nitems = a.fin.B * a.fin.groups;
      for (int item = (int)blockIdx.x * 4 + wave; item < nitems; item += (int)gridDim.x * 4)
        gn_finalize_item<1>(a.fin, item % a.fin.B, item / a.fin.B, lane, nullptr);
    }
  }

  if constexpr (NBUF >= 3) {
    if (tid < 8) ((unsigned*)(lds + NBUF * BUFB + 3 * AFFB + NSLOT * RAWB))[tid] = 0u;   // FULL[4], FREE[4]
  }
  ws_barrier();   // scale/shift (and the zeroed counters) visible to the loaders
  if constexpr (NBUF == 2) ws_barrier();   // image of item 0 is ready
  DSX_STAMP_T(0, tid == 0);
  int g = 0, ti = 0, aslot = 0;   // aslot == ti % 3
  int ibuf = 0;                   // image buffer of the current item (v % NBUF)
  // operand fragments (one 16-pixel column block x one 64-byte chunk each, feeding 2 NB MFMAs = 32 NB cycles) are read
  // PFF fragments ahead of their MFMAs into a ring of PFF + 1
  constexpr int NPAIR = NSTEP / 2;                 // (chunk, tap) pairs of an item: two weight fragments (ch = 0, 1) each
  constexpr int NF = 2 * MB;                       // pixel fragments per pair: (mb, ph)
  constexpr int FT = NPAIR * NF;                   // pixel fragments per item
  constexpr int PFF = (DSX_PFF_EXPR) < FT ? (DSX_PFF_EXPR) : FT - 1;
  static_assert(PFF >= 1 && PFF < FT && PFF <= 15, "lgkmcnt is 4 bits");
  // The ring slot of step s of item v is (v * NSTEP + s) % D: static for D <= NSTEP; for a ring of RP groups the item
  // loop is unrolled RP times (ring phase R = v % RP static in each copy).
  constexpr int RP = D > NSTEP ? D / NSTEP : 1;
  if constexpr (RP == 1) {
    for (int v = 0; v < total; ++v) {
      constexpr int R0 = 0;
#define DSX_WS_ITEM_NEXT continue
#include "dsx_conv_ws_item.inc"
#undef DSX_WS_ITEM_NEXT
    }
  } else {
    for (int v0 = 0; v0 < total; v0 += RP)
      static_for<RP>([&](auto rc_) __attribute__((always_inline)) {
        constexpr int R0 = decltype(rc_)::value * NSTEP;
        const int v = v0 + decltype(rc_)::value;
        if (v >= total) return;
#define DSX_WS_ITEM_NEXT return
#include "dsx_conv_ws_item.inc"
#undef DSX_WS_ITEM_NEXT
      });
  }
  if constexpr (PF_OK) l2_prefetch_retire(a.pf, fin_pf_acc);   // (both sinks are always null)
}

// ---- k_conv_ws.  Chunks per group: the family default, or ConvArgs::ws_cpg where that names a compiled form
static const ConvVariant* ws_variant(int dtype, int tile, int ks, const ConvArgs& a) {
  const int cpg = (ks == 3 && (a.ws_cpg == 2 || a.ws_cpg == 4)) ? a.ws_cpg : ((ks == 1 && a.ws_cpg == 4) ? 4 : conv_cpg(ks));
  return find_variant(FAM_WS, dtype, tile, ks, 1, cpg, a.ws_direct != 0);
}
size_t conv_ws_lds_bytes(int dtype, int tile, int ks, const ConvArgs& a) {
  const ConvVariant* v = ws_variant(dtype, tile, ks, a);
  if (!v) return 0;
  const int cpg = v->cpg;
  if (cpg != conv_cpg(ks)) {
    // several chunks per item: whole groups from either source, never on top of the two-chunk k_conv_mfma geometry
    const int gw = cpg * (dtype != 0 ? 32 : 16);
    if ((ks == 3 && a.cpg == 2) || a.kchunks % cpg || a.C0 % gw || a.C1 % gw) return 0;
    if ((1 << (a.tw_log2 + a.th_log2 + a.tb_log2)) != 32 * v->MB * v->WM) return 0;
    if (a.lds_row != conv_lds_row(ks, 1, a.tw_log2, cpg)) return 0;
  } else if (conv_lds_bytes(dtype, tile, ks, 1, a) == 0) return 0;   // the tile geometry and row pitch of k_conv_mfma
  if (patch_pixels(ks, 1, a) > v->max_px) return 0;
  if (a.up && (a.tw_log2 == 0 || a.th_log2 == 0)) return 0;   // the loaders assume an even tile origin when upsampling
  const int ph = ((1 << a.th_log2) - 1) + ks;
  const size_t bufb = (size_t)(ph << a.tb_log2) * a.lds_row;
  const size_t rawb = (size_t)v->nit * (kWsLoaderWaves * 64 * 16);
  const size_t affb = a.has_gn ? (((size_t)2 * (a.C0 + a.C1) * 4 + 15) & ~(size_t)15) : 0;  // never keyed on a pointer
  // direct rows: a plain 1 x 1 conv (nothing to apply between HBM and the MFMAs); LDS = the images alone
  if (v->direct && (ks != 1 || a.has_gn || a.swish || a.up)) return 0;
  const size_t total = v->direct ? (size_t)v->nbuf * (32 * v->MB * v->WM) * (64 * cpg)
                                 : v->nbuf * bufb + 3 * affb + (size_t)(v->depth + 1) * rawb + (v->nbuf >= 3 ? 32 : 0);
  if (a.tb_log2 != 0 || a.kchunks / cpg < 2) return 0;   // one image per tile, >= 2 channel groups
  // whole 32-channel blocks, float4 epilogue, scale/shift staged by 256 threads x float4
  if ((long long)a.B * a.Ho * a.Wo * std::max(a.out_ld, a.resid_ld) >= (1LL << 31)) return 0;   // 32-bit element offsets
  const int al = dtype != 0 ? 7 : 3;   // 16-byte rows in elements of the storage type
  if (a.Cout % (32 * v->WN * v->NB) != 0 || (a.out_ld & al) != 0 || (a.resid_ld & al) != 0 || a.C0 + a.C1 > 1024)
    return 0;
  if (dtype != 0 && !(a.act_bf16 && a.out_bf16)) return 0;   // this kernel reads and writes the storage type only
  return total <= (size_t)v->lds_cap ? total : 0;
}
hipError_t launch_conv_ws(int dtype, int tile, int ks, const ConvArgs& a, hipStream_t st) {
  const size_t lds = conv_ws_lds_bytes(dtype, tile, ks, a);
  if (lds == 0 || a.ksplit != 1 || a.ws_wg_per_n < 1 || a.stage_mode != 0) return hipErrorInvalidValue;
  if (a.bias && a.film) return hipErrorInvalidValue;   // the planner folds the conv bias into the FiLM bias
  return launch_variant(*ws_variant(dtype, tile, ks, a), (unsigned)(a.n_tiles * a.ws_wg_per_n), lds, a, st);
}

}  // namespace dsx
