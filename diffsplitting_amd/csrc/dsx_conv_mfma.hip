// dsx_conv_mfma.hip — k_conv_mfma, the tiled form of the fused conv (dsx_conv.hip has the overview of the families).
//
// Work decomposition (one 256-thread workgroup = 4 wave64):
//   output tile  : BM = TB x TH x TW output pixels  x  BN output channels
//   K loop       : chunks of 64 B of input channels per pixel (16 fp32 / 32 bf16)
//   A operand    : the (TH*S+KS-S) x (TW*S+KS-S) input halo patch of the chunk is
//                  loaded once (coalesced 16-byte units along C), normalised + activated
//                  in registers, converted, and parked in LDS with an 80-B pixel
//                  stride (conflict-free ds_read_b128); all KS*KS taps re-read it
//                  at constant LDS offsets -> 9x fewer global reads than im2col.
//   B operand    : weights pre-packed on the host in MFMA fragment order, so each
//                  lane's 16-B fragment is one fully coalesced global load (1 KiB
//                  per wave instruction), software-prefetched one step ahead; no
//                  LDS traffic for weights.
//   MFMA         : bf16  v_mfma_f32_32x32x16_bf16 (1 per 16-B fragment pair)
//                  fp32  v_mfma_f32_32x32x2_f32   (4 per 16-B fragment pair; exact
//                        fp32 FMA chain -> the <=1e-3 parity path)
//                  k_conv_ws (the persistent kernel most launches run on): the 16 x 16 shapes on the SAME packed
//                  weights -- v_mfma_f32_16x16x32_bf16 / _f16, v_mfma_f32_16x16x4_f32 (see mfma16_step: the chip holds
//                  a higher clock under them)
//   epilogue     : weights are the MFMA A operand (rows packed permuted), pixels the B operand: a lane
//                  holds one pixel x 16 consecutive channels (k_conv_ws: 8 channels of one pixel per 16-pixel block)
//                  -> 16-byte loads / NHWC stores only.
#include "dsx_conv_variants.h"

namespace dsx {

// MB   : 32-row M blocks per wave;  WM x WN waves (WM*WN == 4); every wave owns ONE
//        32-channel N block, so with WM == 1 no weight fragment is loaded twice.
// CPG  : channel chunks staged per barrier ("group"); 1 for 3x3, 2 for 1x1 (few steps per chunk)
// D    : depth of the weight-fragment prefetch ring (global -> VGPR), steps ahead
//
// Addressing is done by the memory pipeline, not the VALU: both operands come through
// buffer_load with a wave-uniform SGPR offset; out-of-range offsets (zero padding, channel
// tails, prefetch past the end) return 0 from the hardware bounds check, so the staging
// code has no predicates.  LDS image: pixel stride PIXB, row pitch `a.lds_row` chosen by the
// host so that ds_read_b128 of a 32-row fragment is bank-conflict-free (see conv_lds_row).
template <typename DT, int MB, int WM, int WN, int KS, int S, int CPG, int D, int MAX_IT>
__global__ void k_conv_mfma(const ConvArgs a) {   // (launch bounds: on the declaration in dsx_conv_variants.h)
  constexpr int KC = Chunk<DT>::KC;
  constexpr int CPU = Unit<DT>::N;            // channels per 16-byte staging unit
  constexpr int ES = (int)sizeof(DT);         // bytes per activation element in HBM
  constexpr int UPP = KC / CPU;               // staging units per pixel per chunk (4)
  constexpr int UPG = UPP * CPG;              // ... per group
  constexpr int UPG_LOG2 = UPG == 16 ? 4 : (UPG == 8 ? 3 : 2);
  constexpr int UB = 16;                      // LDS bytes per staging unit
  constexpr int PIXB = 64 * CPG + 16;         // LDS bytes per patch pixel
  constexpr int TAPS = KS * KS;
  constexpr int PAD = KS / 2;
  constexpr int NSTEP = CPG * TAPS * 2;       // MFMA steps per group: (chunk, tap, 32-B half)
  constexpr bool IS_BF16 = sizeof(DT) == 2;
  static_assert(NSTEP % D == 0, "ring depth must divide the steps per group");
  static_assert(WM * WN == 4 && UPP == 4, "4 waves; 64-byte chunks");

  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / WN, wn = wave % WN;
  const int li = lane & 31, lh = lane >> 5;

  const int TW = 1 << a.tw_log2, TH = 1 << a.th_log2;
  const int PW = (TW - 1) * S + KS;
  const int PH = (TH - 1) * S + KS;
  const int PPI = PH * PW;                       // patch pixels per image
  const int PP = PPI << a.tb_log2;               // patch pixels per tile
  const int RB = a.lds_row;                      // LDS bytes per patch row
  const int BUFB = (PH << a.tb_log2) * RB;       // one LDS buffer
  const bool multi_img = a.tb_log2 != 0;

  // ---- tile coordinates: blockIdx.x = (split * n_tiles + nt) * m_tiles + mt
  const int mt = blockIdx.x % a.m_tiles;
  const int rest = blockIdx.x / a.m_tiles;
  const int nt = rest % a.n_tiles;
  const int split = rest / a.n_tiles;
  const int txi = mt % a.tiles_x;
  const int tyi = (mt / a.tiles_x) % a.tiles_y;
  const int bg = mt / (a.tiles_x * a.tiles_y);
  const int oy0 = tyi << a.th_log2, ox0 = txi << a.tw_log2, b0 = bg << a.tb_log2;
  const int iy0 = oy0 * S - PAD, ix0 = ox0 * S - PAD;
  const int Hi = a.up ? a.Hs * 2 : a.Hs;
  const int Wi = a.up ? a.Ws * 2 : a.Ws;
  const int C = a.C0 + a.C1;
  const int kgroups = a.kchunks / CPG;
  const int g0 = split * a.groups_per_split;
  const int g1 = min(kgroups, g0 + a.groups_per_split);

  // ---- staging plan: source pixel and LDS slot of each of this thread's units.
  // Unit u = tid + 256*it covers patch pixel u >> UPG_LOG2; (tb, py, px) advance by a fixed stride
  // per `it`, so only the first unit needs integer divisions.
  const int nunits = PP << UPG_LOG2;
  const int cvg = tid & (UPG - 1);  // this thread's unit inside a group (same for all its units)
  int soff[MAX_IT];   // source pixel index, or -1 (zero padding / outside batch / no such unit)
  int loff[MAX_IT];   // LDS byte offset of the unit inside a buffer, or -1
  int simg[MAX_IT];   // image index (GroupNorm scale/shift lookup when a tile spans images)
  {
    constexpr int PSTEP = 256 >> UPG_LOG2;           // pixels between consecutive units of a thread
    const int pix0 = tid >> UPG_LOG2;
    int tb = pix0 / PPI;
    int rem = pix0 - tb * PPI;
    int py = rem / PW;
    int px = rem - py * PW;
    const int dpy = PSTEP / PW, dpx = PSTEP - dpy * PW;   // uniform
#pragma unroll
    for (int it = 0; it < MAX_IT; ++it) {
      int so = -1, lo = -1;
      const int b = b0 + tb;
      if (tid + it * 256 < nunits) {
        const int iy = iy0 + py, ix = ix0 + px;
        lo = (tb * PH + py) * RB + px * PIXB + cvg * UB;
        if (b < a.B && iy >= 0 && iy < Hi && ix >= 0 && ix < Wi) {
          const int sy = a.up ? (iy >> 1) : iy;
          const int sx = a.up ? (ix >> 1) : ix;
          so = (b * a.Hs + sy) * a.Ws + sx;
        }
      }
      soff[it] = so;
      loff[it] = lo;
      simg[it] = b;
      px += dpx; py += dpy;
      if (px >= PW) { px -= PW; py += 1; }
      while (py >= PH) { py -= PH; tb += 1; }
    }
  }

  // ---- A-fragment LDS addresses: one per (row block, tap row); tap column / chunk / half are immediates
  int abase[MB][KS];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    const int m = (wm * MB + mb) * 32 + li;
    const int tx = m & (TW - 1);
    const int ty = (m >> a.tw_log2) & (TH - 1);
    const int tb = m >> (a.tw_log2 + a.th_log2);
#pragma unroll
    for (int dy = 0; dy < KS; ++dy)
      abase[mb][dy] = (tb * PH + ty * S + dy) * RB + tx * S * PIXB + lh * 16;
  }

  // ---- buffer descriptors (wave-uniform): activations (two sources) and this wave's weight stream
  const __amdgpu_buffer_rsrc_t rs0 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)a.src0, 0, (int)min((long long)a.B * a.Hs * a.Ws * a.C0 * ES, 0x7fffffffLL), 0x00020000);
  const __amdgpu_buffer_rsrc_t rs1 = __builtin_amdgcn_make_buffer_rsrc(
      (void*)(a.src1 ? a.src1 : a.src0), 0,
      a.src1 ? (int)min((long long)a.B * a.Hs * a.Ws * a.C1 * ES, 0x7fffffffLL) : 0, 0x00020000);
  int blk = nt * WN + wn;
  if (blk >= a.nblocks) blk = a.nblocks - 1;  // results of a clamped block are never stored
  const long long wblock = (long long)kgroups * (NSTEP * 1024);  // bytes of one N block's fragment stream
  const __amdgpu_buffer_rsrc_t rsw = __builtin_amdgcn_make_buffer_rsrc(
      (void*)((const unsigned char*)a.wpack + (size_t)blk * wblock), 0, (int)wblock, 0x00020000);
  const int wlane = lane * 16;
  auto load_b = [&](int q) -> uint4 {  // step q of the stream; past the end -> zeros (bounds check)
    return __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rsw, wlane, q * 1024, 0));
  };
  uint4 bq[D];
#pragma unroll
  for (int j = 0; j < D; ++j) bq[j] = load_b(g0 * NSTEP + j);

  f32x16 acc[MB];
#pragma unroll
  for (int mb = 0; mb < MB; ++mb)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[mb][r] = 0.0f;

  uint4 stg[MAX_IT];   // raw 16-byte units (CPU channels in the storage type)
#pragma unroll
  for (int it = 0; it < MAX_IT; ++it) stg[it] = make_uint4(0u, 0u, 0u, 0u);

  // issue the global loads of group g into registers
  auto stage_load = [&](int g) {
    const int c = g * (CPG * KC) + cvg * CPU;
#ifdef DSX_DIAG
    if (a.ablate & 2) return;   // timing experiments only (DSX_ABLATE, diagnostic build): skip activation loads
#endif
    if (a.stage_mode == 0) {
      // fast path (both channel counts multiples of the group width): the whole workgroup reads ONE
      // source in this group -> wave-uniform descriptor, offsets by the memory pipeline, OOB -> 0
      const bool first = g * (CPG * KC) < a.C0;            // uniform
      const int cs = first ? a.C0 : a.C1;
      const unsigned coff = c < C ? (unsigned)((first ? c : c - a.C0) * ES) : 0x80000000u;
      if (first) {
#pragma unroll
        for (int it = 0; it < MAX_IT; ++it) {
          const unsigned vo = soff[it] >= 0 ? (unsigned)soff[it] * (unsigned)(cs * ES) + coff : 0x80000000u;
          stg[it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs0, vo, 0, 0));
        }
      } else {
#pragma unroll
        for (int it = 0; it < MAX_IT; ++it) {
          const unsigned vo = soff[it] >= 0 ? (unsigned)soff[it] * (unsigned)(cs * ES) + coff : 0x80000000u;
          stg[it] = __builtin_bit_cast(uint4, __builtin_amdgcn_raw_buffer_load_b128(rs1, vo, 0, 0));
        }
      }
    } else if (a.stage_mode == 1) {
      // channel counts multiples of the unit but a group may straddle the two sources: per-lane source select
#pragma unroll
      for (int it = 0; it < MAX_IT; ++it) {
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        const int so = soff[it];
        if (so >= 0) {
          if (c < a.C0) v = *(const uint4*)((const DT*)a.src0 + (size_t)so * a.C0 + c);
          else if (c < C) v = *(const uint4*)((const DT*)a.src1 + (size_t)so * a.C1 + (c - a.C0));
        }
        stg[it] = v;
      }
    } else {
#pragma unroll
      for (int it = 0; it < MAX_IT; ++it) {
        float e[CPU];
#pragma unroll
        for (int j = 0; j < CPU; ++j) e[j] = 0.f;
        const int so = soff[it];
        if (so >= 0) {
#pragma unroll
          for (int j = 0; j < CPU; ++j) {
            const int cc = c + j;
            if (cc < a.C0) e[j] = act_load<DT>(a.src0, (size_t)so * a.C0 + cc);
            else if (cc < C) e[j] = act_load<DT>(a.src1, (size_t)so * a.C1 + (cc - a.C0));
          }
        }
        stg[it] = Unit<DT>::pack(e);   // exact: the values came from the storage type
      }
    }
  };

  // GroupNorm affine + Swish in registers, convert, park in LDS buffer `buf`
  auto stage_store = [&](int g, int buf) {
    const int c = g * (CPG * KC) + cvg * CPU;
    unsigned char* dst = lds + buf * BUFB;
    const bool has_gn = a.gn_scale != nullptr && c < C;
    float sc[CPU], sh[CPU];
#pragma unroll
    for (int j = 0; j < CPU; ++j) { sc[j] = 1.f; sh[j] = 0.f; }
    auto load_affine = [&](int b) {
      const size_t gi = (size_t)b * C + c;
      if (!(a.stage_mode == 2)) {
#pragma unroll
        for (int q = 0; q < CPU / 4; ++q) {
          const float4 s4 = *(const float4*)(a.gn_scale + gi + 4 * q);
          const float4 h4 = *(const float4*)(a.gn_shift + gi + 4 * q);
          sc[4 * q] = s4.x; sc[4 * q + 1] = s4.y; sc[4 * q + 2] = s4.z; sc[4 * q + 3] = s4.w;
          sh[4 * q] = h4.x; sh[4 * q + 1] = h4.y; sh[4 * q + 2] = h4.z; sh[4 * q + 3] = h4.w;
        }
      } else {
#pragma unroll
        for (int j = 0; j < CPU; ++j) {
          sc[j] = (c + j < C) ? a.gn_scale[gi + j] : 0.f;
          sh[j] = (c + j < C) ? a.gn_shift[gi + j] : 0.f;
        }
      }
    };
    if (has_gn && !multi_img) load_affine(b0);  // one image per tile: same (b, c) for every unit
#pragma unroll
    for (int it = 0; it < MAX_IT; ++it) {
      if (loff[it] >= 0) {
        float v[CPU];
        Unit<DT>::unpack(stg[it], v);
        if (soff[it] >= 0 && c < C && !DSX_ABLATED(1)) {   // padding pixels stay exactly 0 (padded AFTER the activation)
          if (has_gn) {
            if (multi_img) load_affine(simg[it]);
            affine_vec(v, sc, sh);
          }
          if (a.swish) swish_vec(v);
          if ((a.stage_mode == 2)) {  // channels past C inside the last unit must stay 0
#pragma unroll
            for (int j = 1; j < CPU; ++j) if (c + j >= C) v[j] = 0.f;
          }
        }
        *(uint4*)(dst + loff[it]) = Unit<DT>::pack(v);
      }
    }
  };

  // ---- main loop over channel groups (double-buffered LDS, one barrier per group)
  DSX_STAMP(0);
  stage_load(g0);
  DSX_STAMP(1);
  stage_store(g0, 0);
  DSX_STAMP(2);
  __syncthreads();
  DSX_STAMP(3);

  const unsigned lds0 = (unsigned)(uintptr_t)(__attribute__((address_space(3))) unsigned char*)lds;  // LDS byte address of lds[0]
  constexpr int PF = 1;   // operand fragments are read one step ahead of their MFMAs (see lds_read_frag)
  for (int g = g0; g < g1; ++g) {
    const bool more = (g + 1) < g1;
    const int qbase = g * NSTEP;

    if (more) stage_load(g + 1);
    DSX_STAMP(8 + 4 * (g - g0));

    unsigned aaddr[MB][KS];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
      for (int dy = 0; dy < KS; ++dy) aaddr[mb][dy] = lds0 + ((g - g0) & 1) * BUFB + abase[mb][dy];
    f32x4_t fb[PF + 1][MB];
    auto read_step = [&](auto sc) {
      constexpr int s = decltype(sc)::value;
      constexpr int kTapSteps = TAPS * 2;
      constexpr int cg = s / kTapSteps, tap = (s >> 1) % TAPS, fs = s & 1;
      constexpr int dy = tap / KS, dx = tap % KS;
      constexpr int imm = dx * PIXB + cg * 64 + fs * 32;
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) lds_read_frag<imm>(fb[s % (PF + 1)][mb], aaddr[mb][dy]);
    };
    static_for<PF>(read_step);
    static_for<NSTEP>([&](auto sc) {
      constexpr int s = decltype(sc)::value;
      const uint4 bcur = bq[s % D];
      bq[s % D] = load_b(qbase + s + D);
      if constexpr (s + PF < NSTEP) read_step(std::integral_constant<int, s + PF>{});
      constexpr int ahead = (NSTEP - 1 - s < PF ? NSTEP - 1 - s : PF) * MB;   // younger reads that may stay in flight
      constexpr int cb = s % (PF + 1);
      static_assert(PF * MB <= 15, "lgkmcnt is 4 bits");
      if constexpr (MB == 1) wait_frags<ahead>(fb[cb][0]);
      else if constexpr (MB == 2) wait_frags<ahead>(fb[cb][0], fb[cb][1]);
      else if constexpr (MB == 4) wait_frags<ahead>(fb[cb][0], fb[cb][1], fb[cb][2], fb[cb][3]);
      else {
        wait_frags<ahead>(fb[cb][0], fb[cb][1], fb[cb][2], fb[cb][3]);   // the wait; the rest only need the ordering
#pragma unroll
        for (int mb = 4; mb < MB; ++mb) asm volatile("" : "+v"(fb[cb][mb]));
      }
#pragma unroll
      for (int mb = 0; mb < MB; ++mb) {
        // weights as the A operand, pixels as B: the accumulator then holds, per lane, one pixel's channels
        acc[mb] = mfma_step<DT>(bcur, fb[cb][mb], acc[mb]);
      }
    });

    DSX_STAMP(9 + 4 * (g - g0));
    if (more && !DSX_ABLATED(32)) stage_store(g + 1, (g + 1 - g0) & 1);
    DSX_STAMP(10 + 4 * (g - g0));
    __syncthreads();
    DSX_STAMP(11 + 4 * (g - g0));
  }
  DSX_STAMP(4);

  // ---- epilogue.  Accumulator layout (operands swapped): column = lane&31 = pixel of the row block,
  // register r = channel 16*(lane>>5) + r of this wave's 32-channel block (the weight rows are packed
  // permuted): 16 consecutive channels per lane -> 16-byte bias / FiLM / residual loads and NHWC stores.
  // Split-K slices write raw partial sums to their fp32 slab.  The GroupNorm statistics of the tensor being
  // written (sum, sum of squares per channel over this wave's pixels) are accumulated in the same pass.
  if (DSX_ABLATED(16)) return;
  const int nbase = (nt * WN + wn) * 32 + 16 * lh;
  const bool partial = a.ksplit > 1;
  const int okind = (IS_BF16 && a.out_bf16) ? Kind<DT>::value : 0;   // storage kind of `out`
  const bool obf = okind != 0;
  void* outp = partial ? (void*)((float*)a.out + (size_t)split * a.slab_stride) : a.out;
  const int oal = obf ? 7 : 3, ral = IS_BF16 ? 7 : 3;   // 16-byte alignment of rows, in elements
  const bool vec = (a.Cout & 15) == 0 && (a.out_ld & oal) == 0 && (!a.resid || (a.resid_ld & ral) == 0);
  // fused statistics are compiled only into the small-MB tiles: in the MB >= 4 tiles their registers
  // would cost a wave of occupancy (the host then falls back to k_chan_stats)
  constexpr bool STATS = MB <= 2;
  const bool do_stats = STATS && a.stat_part != nullptr;   // host guarantees: vec, one image per tile, no split-K
  float s1[16], s2[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) { s1[r] = 0.f; s2[r] = 0.f; }
#pragma unroll
  for (int mb = 0; mb < MB; ++mb) {
    // one row block at a time: keeps the epilogue's loads from being hoisted across blocks,
    // which would cost registers (and a wave of occupancy) in the main loop's favour
    __builtin_amdgcn_sched_barrier(0);
    const int m = (wm * MB + mb) * 32 + li;
    const int tx = m & (TW - 1);
    const int ty = (m >> a.tw_log2) & (TH - 1);
    const int b = b0 + (m >> (a.tw_log2 + a.th_log2));
    if (b >= a.B || nbase >= a.Cout) continue;
    const size_t opix = ((size_t)b * a.Ho + (oy0 + ty)) * a.Wo + (ox0 + tx);
    float x[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) x[r] = acc[mb][r];
    if (vec) {
      if (!partial) {
        if (a.bias) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { const float4 t = *(const float4*)(a.bias + nbase + 4 * j); x[4 * j] += t.x; x[4 * j + 1] += t.y; x[4 * j + 2] += t.z; x[4 * j + 3] += t.w; }
        }
        if (a.film) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { const float4 t = *(const float4*)(a.film + (size_t)b * a.film_bs + nbase + 4 * j); x[4 * j] += t.x; x[4 * j + 1] += t.y; x[4 * j + 2] += t.z; x[4 * j + 3] += t.w; }
        }
        if (a.resid) {
          const DT* rp = (const DT*)a.resid + opix * a.resid_ld + nbase;
#pragma unroll
          for (int q = 0; q < 16 / CPU; ++q) {
            float t[CPU];
            Unit<DT>::unpack(*(const uint4*)(rp + CPU * q), t);
#pragma unroll
            for (int j = 0; j < CPU; ++j) x[CPU * q + j] += t[j];
          }
        }
      }
      store16<true>(outp, opix * a.out_ld + nbase, x, okind, 16);
      if (do_stats) {
#pragma unroll
        for (int r = 0; r < 16; ++r) { s1[r] += x[r]; s2[r] += x[r] * x[r]; }
      }
    } else {
      const int valid = min(16, a.Cout - nbase);
      if (!partial) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          if (r >= valid) break;
          if (a.bias) x[r] += a.bias[nbase + r];
          if (a.film) x[r] += a.film[(size_t)b * a.film_bs + nbase + r];
          if (a.resid) x[r] += act_load<DT>(a.resid, opix * a.resid_ld + nbase + r);
        }
      }
      store16<false>(outp, opix * a.out_ld + nbase, x, okind, valid);
    }
  }
  DSX_STAMP(5);

  // ---- statistics: reduce over the 32 pixel lanes of each half-wave (DPP butterfly inside the 16-lane
  // rows, one cross-row exchange; fixed order -> bitwise reproducible).  One partial row per (tile, wm):
  // [b][chunk][channel][2] fp32.
  if (do_stats) {
    float w1 = row16_fold(s1, lane), w2 = row16_fold(s2, lane);
    w1 += __shfl_xor(w1, 16, 64);
    w2 += __shfl_xor(w2, 16, 64);
    const int chunk = (tyi * a.tiles_x + txi) * WM + wm;   // partial row inside the image
    const int nch = a.tiles_x * a.tiles_y * WM;
    const int n = nbase + row16_fold_reg(li);
    if (li < 16 && n < a.Cout) {
      float* p = a.stat_part + (((size_t)b0 * nch + chunk) * a.Cout + n) * 2;
      p[0] = w1; p[1] = w2;
    }
  }
  DSX_STAMP(6);
}

// ---- k_conv_mfma
static bool is_g2(int ks, int stride, const ConvArgs& a) { return a.cpg == 2 && ks == 3 && stride == 1; }
static const ConvVariant* mfma_variant(int dtype, int tile, int ks, int stride, const ConvArgs& a) {
  return find_variant(FAM_MFMA, dtype, tile, ks, stride, is_g2(ks, stride, a) ? 2 : conv_cpg(ks));
}
size_t conv_lds_bytes(int dtype, int tile, int ks, int stride, const ConvArgs& a) {
  const ConvVariant* v = mfma_variant(dtype, tile, ks, stride, a);
  if (!v) return 0;
  if ((1 << (a.tw_log2 + a.th_log2 + a.tb_log2)) != 32 * v->MB * v->WM) return 0;
  if (patch_pixels(ks, stride, a) > v->max_px || a.lds_row != conv_lds_row(ks, stride, a.tw_log2, v->cpg)) return 0;
  const int ph = ((1 << a.th_log2) - 1) * stride + ks;
  const size_t bufb = (size_t)(ph << a.tb_log2) * a.lds_row;
  size_t need = 2 * bufb;
  if (is_g2(ks, stride, a)) {   // one image per tile, whole groups of aligned sources
    if (a.tb_log2 != 0 || a.kchunks % 2 || a.stage_mode != 0) return 0;
    if (a.kchunks / 2 <= 1) need = bufb;   // a single group never touches the second buffer
  }
  return need <= (size_t)v->lds_cap ? need : 0;
}
hipError_t launch_conv(int dtype, int tile, int ks, int stride, const ConvArgs& a, hipStream_t st) {
  const size_t lds = conv_lds_bytes(dtype, tile, ks, stride, a);
  if (lds == 0 || a.ksplit < 1 || a.n_tiles < 1) return hipErrorInvalidValue;
  return launch_variant(*mfma_variant(dtype, tile, ks, stride, a), (unsigned)(a.m_tiles * a.n_tiles * a.ksplit), lds, a, st);
}

}  // namespace dsx
