// dsx_kernels.h — launch interface between the host runtime (dsx_*.cpp)
// and the gfx950 kernels (dsx_conv*.hip, dsx_ops.hip, dsx_attn.hip, dsx_tiles.hip, dsx_eval.hip, ...).  Internal;
// the public ABI is include/dsx.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace dsx {

// ---------------------------------------------------------------------------
// L2 weight prefetch for the NEXT conv launch.  A conv's weight stream is read once per step and comes from HBM
// (196 MB of weights per step do not stay in the 32 MB of L2); a wave can keep ~18 KiB of it in flight, so at HBM
// latency the stream, not the MFMAs, paces the small-map layers.  The launch in front of a conv (its k_gn_finalize, or
// the previous image-resident conv) therefore touches the 128-byte lines of the weight slices that the conv's
// workgroups on the same XCD will read, so that they wait in that XCD's L2.  Workgroups are dealt round-robin over the 8 XCDs: blocks with equal
// (linear id % 8) share an L2, and the consumer kernels key their N slices on that same label.  Placement only
// affects speed: a different dispatch order makes the prefetch useless, never wrong.
//   slices : `nslices` consecutive ranges of `slice_bytes` at `base`
//   label x needs slice x % nslices when nslices < 8 (8 % nslices == 0), else every slice s with s % 8 == x
// The loads are ordinary (compiler-counted) loads whose values are OR-ed into a word that is stored through `sink`
// at the end of the kernel; `sink` is always nullptr, so nothing is ever stored, but the loads cannot be dropped
// and no register is overwritten behind the compiler's back.
// ---------------------------------------------------------------------------
struct PrefetchArgs {
  const void* base;       // nullptr: nothing to prefetch
  unsigned slice_bytes;
  int nslices;
  unsigned* sink;         // always nullptr
};
// n / d for n, d < 65536 as a multiply-high: magic = d == 1 ? 0 : floor(2^32 / d) + 1 (exact: n * (magic * d - 2^32) < 2^32)
inline unsigned fastdiv_magic(unsigned d) { return d <= 1 ? 0u : (unsigned)((1ull << 32) / d) + 1u; }
#if defined(__HIPCC__)
__device__ __forceinline__ unsigned fastdiv(unsigned n, unsigned magic) { return magic ? __umulhi(n, magic) : n; }
// The loaded words stay in four registers of their own until l2_prefetch_retire: the first line a thread requests of
// each of its first four slices is a plain assignment, so no s_waitcnt stands between the prefetch and the kernel's own
// work (an `acc |= load` there made the issuing waves of k_conv_img wait vmcnt(0), i.e. for their whole weight stream,
// before they converted their slice of the image: they reached the workgroup barrier ~5 k cycles after the others).
// Further lines (a share longer than the thread count, more than four slices per label: not in the plans built here)
// are OR-ed in and do wait.
struct PfAcc { unsigned v[4]; };
__device__ __forceinline__ PfAcc l2_prefetch(const PrefetchArgs& pf, unsigned lin_block, unsigned nblocks_total, int tid, int nthreads) {
  PfAcc acc = {{0u, 0u, 0u, 0u}};
  if (pf.base == nullptr || pf.nslices <= 0) return acc;
  const unsigned label = lin_block & 7u, j = lin_block >> 3, n8 = (nblocks_total + 7u) >> 3;
  const unsigned lines = pf.slice_bytes >> 7;            // whole 128-byte lines (slices are multiples of 1 KiB)
  const unsigned per = (lines + n8 - 1u) / n8, l0 = j * per;
  const unsigned l1 = l0 + per < lines ? l0 + per : lines;
  const int s0 = pf.nslices < 8 ? (int)(label % (unsigned)pf.nslices) : (int)label;
  const int sstep = pf.nslices < 8 ? pf.nslices : 8;     // nslices < 8: exactly one slice
  int sl = s0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (sl < pf.nslices) {
      const char* b = (const char*)pf.base + (size_t)sl * pf.slice_bytes;
      unsigned l = l0 + (unsigned)tid;
      if (l < l1) acc.v[k] = *(const unsigned*)(b + (size_t)l * 128);
      for (l += (unsigned)nthreads; l < l1; l += (unsigned)nthreads) acc.v[k] |= *(const unsigned*)(b + (size_t)l * 128);
      sl += sstep;
    }
  }
  for (; sl < pf.nslices; sl += sstep) {
    const char* b = (const char*)pf.base + (size_t)sl * pf.slice_bytes;
    for (unsigned l = l0 + (unsigned)tid; l < l1; l += (unsigned)nthreads) acc.v[3] |= *(const unsigned*)(b + (size_t)l * 128);
  }
  return acc;
}
__device__ __forceinline__ unsigned l2_prefetch_fold(const PfAcc& acc) { return acc.v[0] | acc.v[1] | acc.v[2] | acc.v[3]; }   // waits for the loads
__device__ __forceinline__ void l2_prefetch_retire(const PrefetchArgs& pf, unsigned acc) {
  if (pf.sink != nullptr) *pf.sink = acc;
}
__device__ __forceinline__ void l2_prefetch_retire(const PrefetchArgs& pf, const PfAcc& acc) {
  if (pf.sink != nullptr) *pf.sink = acc.v[0] | acc.v[1] | acc.v[2] | acc.v[3];   // never taken: keeps the prefetch loads alive
}
#endif

// Shifted fp32 GroupNorm partials: a producer that has a per-(image, channel) pivot p = bias[c] + film[b][c] (either
// pointer may be null) sums x - p and (x - p)^2, so that a flat map whose level comes from the bias (a uniform background
// through the first conv) does not cancel in E[x^2] - E[x]^2; the consumer adds the pivot back in double.  Every tile of
// the map uses the same pivot; producer and consumer compute it with this one expression (bitwise the same value).
struct StatPivot {
  const float* bias;     // [C] or nullptr
  const float* film;     // [B][film_bs] or nullptr
  int film_bs;
};
#if defined(__HIPCC__)
__device__ __forceinline__ float stat_pivot(const StatPivot& p, int b, int c) {
  return (p.bias ? p.bias[c] : 0.f) + (p.film ? p.film[(size_t)b * p.film_bs + c] : 0.f);
}
// channel sums (s, q) of x - p over `count` pixels -> sums of x
__device__ __forceinline__ void stat_unshift(double& s, double& q, double p, double count) {
  q += 2.0 * p * s + count * p * p;
  s += count * p;
}
#endif

// GroupNorm of the concatenation of (t0, t1) -> scale/shift[b][C0+C1]
struct GnFinArgs {
  const void* part0; int C0, nchunk0, f32_0;   // partials: double (k_chan_stats) or float (conv epilogue)
  const void* part1; int C1, nchunk1, f32_1;
  StatPivot piv0, piv1;  // pivots of shifted fp32 partials (all-null: unshifted)
  int B, groups;
  double count;          // elements per channel (H*W)
  const float* gamma;    // [C0+C1]
  const float* beta;
  float eps;
  float* scale;          // [B][C0+C1]
  float* shift;
  PrefetchArgs pf;       // weight slices of the conv this GroupNorm feeds (see l2_prefetch)
};
// The launch rule of a finalize launch of its own: k_gn_finalize_wide (four waves per item) when a group has more than 512
// (channel, partial row) pairs (an upper bound: the longer source's rows for every channel), else k_gn_finalize.  One
// statement for launch_gn_finalize and for DSX_PLAN_DUMP, which names the launcher by it.
inline bool gn_finalize_is_wide(const GnFinArgs& a) {
  const int cpg = (a.C0 + a.C1) / a.groups;
  return (long long)cpg * (a.nchunk0 > a.nchunk1 ? a.nchunk0 : a.nchunk1) > 512;
}
#if defined(__HIPCC__)
// One (image, group) item of the GroupNorm finalize, by one wave (or NW waves): threads stride over (channel-in-group,
// chunk) partials, fixed assignment + fixed butterfly order -> bitwise reproducible.  Used by k_gn_finalize (one wave per
// workgroup) and by the loader waves of a residual 1 x 1 conv that hosts the finalize of the block's second GroupNorm.
// NW waves share the item (k_gn_finalize_wide: NW = 4 for the 128^2 / 64^2 maps with hundreds of partial rows); their
// wave sums meet in LDS (`red`, 2 * NW doubles) and are added in wave order.
template <int NW>
__device__ __forceinline__ void gn_finalize_item(const GnFinArgs& a, const int b, const int g, const int tid, double* red) {
  constexpr int NT = 64 * NW;
  const int C = a.C0 + a.C1;
  const int cpg = C / a.groups;
  const int c_lo = g * cpg;
  double s = 0, q = 0;
  // channels of this group that live in source 0 / source 1; the loads of a lane are independent, so
  // they are issued 8 at a time (the kernel is pure load latency otherwise)
  const int n0 = max(0, min(a.C0, c_lo + cpg) - c_lo);      // first n0 channels from source 0
  const int n1 = cpg - n0;
  auto accumulate = [&](const void* part, int is_f32, int nsrc, int nchunk, int Csrc, int cbase, const StatPivot& piv) __attribute__((always_inline)) {
    const bool shifted = piv.bias || piv.film;
    const int items = nsrc * nchunk;
    for (int i0 = tid; i0 < items; i0 += NT * 8) {
      double ps[8], pq[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int i = i0 + u * NT;
        ps[u] = 0; pq[u] = 0;
        if (i < items) {
          const int ch = i / nsrc, c = cbase + (i - ch * nsrc);
          const size_t idx = (((size_t)b * nchunk + ch) * Csrc + c) * 2;
          if (is_f32) { const float2 v = *(const float2*)((const float*)part + idx); ps[u] = v.x; pq[u] = v.y; }
          else { const double2 v = *(const double2*)((const double*)part + idx); ps[u] = v.x; pq[u] = v.y; }
          if (shifted) {   // sum over the chunks of (s + 2 p s_k) + count p^2: the count term once, with chunk 0
            const double p = (double)stat_pivot(piv, b, c);
            pq[u] += 2.0 * p * ps[u] + (ch == 0 ? a.count * p * p : 0.0);
            ps[u] += ch == 0 ? a.count * p : 0.0;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) { s += ps[u]; q += pq[u]; }
    }
  };
  // gamma / beta of this thread's channel: issued with the partial sums (one memory round trip, not two)
  const int c_own = c_lo + tid;
  const bool own = tid < cpg;
  const float g_own = own ? a.gamma[c_own] : 0.f, b_own = own ? a.beta[c_own] : 0.f;
  if (n0 > 0) accumulate(a.part0, a.f32_0, n0, a.nchunk0, a.C0, c_lo, a.piv0);
  if (n1 > 0) accumulate(a.part1, a.f32_1, n1, a.nchunk1, a.C1, c_lo + n0 - a.C0, a.piv1);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); q += __shfl_xor(q, o, 64); }
  if constexpr (NW > 1) {
    if ((tid & 63) == 0) { red[2 * (tid >> 6)] = s; red[2 * (tid >> 6) + 1] = q; }
    __syncthreads();
    s = 0; q = 0;
#pragma unroll
    for (int w = 0; w < NW; ++w) { s += red[2 * w]; q += red[2 * w + 1]; }
  }
  const double n = a.count * cpg;
  const double mean = s / n;
  double var = q / n - mean * mean;
  if (var < 0) var = 0;
  const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
  const float meanf = (float)mean;
  if (own) {
    const float sc = rstd * g_own;
    a.scale[(size_t)b * C + c_own] = sc;
    a.shift[(size_t)b * C + c_own] = b_own - meanf * sc;
  }
  // groups wider than the workgroup (norm_groups 1 .. 3 on wide levels and concats: tests/test_gpu_groups.py runs this
  // loop in k_gn_finalize at 65 .. 512 channels per group, in k_gn_finalize_wide above 256 and in the hosted finalize)
  for (int c = c_lo + tid + NT; c < c_lo + cpg; c += NT) {
    const float sc = rstd * a.gamma[c];
    a.scale[(size_t)b * C + c] = sc;
    a.shift[(size_t)b * C + c] = a.beta[c] - meanf * sc;
  }
}
#endif

// ---------------------------------------------------------------------------
// Fused conv:  out = conv_{KSxKS, stride S}( act( gn(x) ) ) + bias + film + resid
//   x is the channel-concatenation of up to two NHWC fp32 tensors (skip
//   connections are never materialised), optionally nearest-upsampled x2.
//   Implicit GEMM on MFMA: M = output pixels, N = Cout, K = taps x Cin.
// ---------------------------------------------------------------------------
// (tests/plan_dump.py mirrors the members up to `stat_part` to read DSX_PLAN_DUMP lines: keep it in step
// when a member is added, removed or reordered above that one.)
struct ConvArgs {
  const void* src0;       // NHWC activations in the storage type: fp32, or bf16 when act_bf16
  const void* src1;
  int act_bf16;           // storage kind of src0 / src1 / resid: 0 fp32, 1 bf16, 2 fp16 (the MFMA operand type)
  int out_bf16;           // storage kind of out (0 for split-K slabs and the network's final output)
  int C0, C1;             // channels per source (C1 == 0: single source)
  int B, Hs, Ws;          // source spatial size (before the optional upsample)
  int up;                 // 1: nearest x2 upsample fused into the patch load
  int Ho, Wo;             // output spatial size
  const float* gn_scale;  // [B][C0+C1] or nullptr:  v = x*scale + shift
  const float* gn_shift;
  int has_gn;             // GroupNorm affine fused (== gn_scale != nullptr once the workspace exists)
  int swish;              // v = v*sigmoid(v) after the affine
  int stage_mode;         // 0: sources aligned to the channel group (buffer loads); 1: 16-byte loads with
                          // per-lane source select; 2: channel counts not multiples of the 16-byte unit
                          // (4 fp32 / 8 bf16 channels): per-element loads
  const void* wpack;      // MFMA-fragment-ordered weights (fp32 or bf16)
  const float* bias;      // [Cout] or nullptr
  const float* film;      // film[b*film_bs + n] or nullptr (FiLM / time-embedding add)
  int film_bs;
  const void* resid;      // [B][Ho][Wo][resid_ld] (storage type) or nullptr
  int resid_ld;
  void* out;              // [B][Ho][Wo][out_ld]
  int out_ld;
  int Cout;
  int nblocks;            // ceil(Cout/32)
  int kchunks;            // ceil((C0+C1)/KC), padded to conv_chunk_multiple(ks)
  int tw_log2, th_log2, tb_log2;  // output tile = TB images x TH x TW pixels
  int tiles_x, tiles_y, m_tiles, n_tiles;
  int lds_row;            // LDS bytes per patch row (conv_lds_row)
  int cpg;                // 0: the kernel family's default chunks per staged group (1 for 3x3, 2 for 1x1);
                          // 2 with a 3x3: the two-chunk variant of k_conv_mfma (64 input channels per barrier: a
                          // 64-channel layer is ONE group, no K loop)
  int ws_wg_per_n;        // warp-specialised kernel: persistent workgroups per N tile (0: k_conv_mfma)
  int ws_cpg;             // k_conv_ws: chunks per (tile, group) item other than the family default -- 2 or 4 for a 3 x 3 conv, 4 for
                          // a 1 x 1 conv (lds_row = conv_lds_row of that many chunks); 64- and 128-pixel tiles: the loaders'
                          // per-item costs are paid once per 64 / 128 input channels
  int xcd_bands;          // k_conv_ws: an XCD's workgroups take a contiguous band of M tiles (else round-robin)
  // k_conv_ws start-up without integer divisions (a dozen of them cost ~2000 cycles before the first DMA could be issued):
  // the host passes the quotients it can compute and multiply-high magics (fastdiv) for the per-workgroup ones.
  int ws_map;             // blockIdx -> (N tile, first M tile): 0 N tiles dealt over XCDs (n_tiles in {1,2,4,8}), 1 n_tiles % 8 == 0, 2 plain,
                          // 3 M tiles dealt over XCDs, every N tile on each (1 x 1 convs; ws_per = n_tiles)
  int ws_nt_log2;         // ws_map 0: log2(n_tiles)
  int ws_per;             // ws_map 1: n_tiles / 8
  int ws_adv_x, ws_adv_y, ws_adv_b;   // tile walk stride wpn decomposed: wpn % tiles_x, (wpn / tiles_x) % tiles_y, wpn / (tiles_x * tiles_y)
  int ws_dpy, ws_dpx;     // loader tables: (loader threads / units per pixel) / PW and the remainder
  unsigned mg_tiles_x, mg_per_img, mg_pw, mg_wpn, mg_per;   // fastdiv magics (dividends < 65536, see fastdiv)
  int ws_bigdiv;          // m_tiles + wpn >= 65536: the tiles-per-workgroup quotient needs a real division
  float* stat_part;       // fused GroupNorm partials [B][tiles_x*tiles_y*WM][Cout][2] (fp32) or nullptr
  unsigned* handoff_timeouts;  // k_conv_ws with image counters: incremented when a bounded FULL / FREE spin gives up (never in
                               // a correct run; dsx_exec_handoff_timeouts reads it) -- a lost hand-off must not pass silently
  int ws_direct;          // k_conv_ws, 1 x 1 conv with neither GroupNorm nor Swish in front: the loader waves DMA the activation
                          // units straight into swizzled MFMA images (the DIRECT rows of the variant table; lds_row is unused)
  unsigned long long* stamp;  // diagnostic s_memtime stamps of workgroup `stamp_block` (or nullptr)
  int stamp_block;
  int ablate;             // -DDSX_DIAG builds only: DSX_ABLATE timing experiments (results are wrong when non-zero)
  // k_conv_img only (GroupNorm finalised inside the consumer): the partial sums of the sources as their producers
  // left them ([B][nchunk][C][2], double from k_chan_stats or float from a fused epilogue) and the affine parameters
  const void* gn_part0; int gn_nchunk0, gn_pf32_0;
  const void* gn_part1; int gn_nchunk1, gn_pf32_1;
  StatPivot gn_piv0, gn_piv1;   // pivots of shifted fp32 partials (GnFinArgs::piv0 / piv1)
  const float* gn_gamma; const float* gn_beta;
  int gn_groups; float gn_eps;
  PrefetchArgs pf;        // weight slices of the next conv launch (see l2_prefetch)
  int fin_on;             // k_conv_ws: the compute waves, idle until the first image is staged, finalize another GroupNorm
  GnFinArgs fin;          //   (the one between the two convs behind this residual 1 x 1 conv; fin.pf = its consumer's weights)
  int ksplit;             // split-K slices (1 = none); slice s writes raw sums to out + s*slab_stride
  int groups_per_split;   // channel groups per slice
  long long slab_stride;  // elements between slabs
};

// tile configurations compiled for the MFMA conv kernels
enum ConvTile { TILE_256x128 = 0, TILE_128x128, TILE_64x128, TILE_256x64, TILE_128x64, TILE_64x64, TILE_128x32, TILE_256x32, TILE_COUNT };
// pixels x output channels of a tile, waves along M (one statistics row per (tile, wm)), and whether the epilogue can
// emit the GroupNorm statistics of the result; `ws`: as k_conv_ws lays the tile out (k_conv_mfma otherwise).  All zero
// when the kernel is not compiled for the tile.
struct ConvTileInfo { int BM, BN, WM; bool fuses_stats; };
ConvTileInfo conv_tile_info(int tile, bool ws = false);
// input-channel chunks are staged in groups of this many (weights are packed/padded to it)
int conv_chunk_multiple(int ks);
// LDS bytes per patch row of a tile 2^tw_log2 pixels wide with `cpg` 64-byte chunks per pixel (the family default
// conv_chunk_multiple(ks), ConvArgs::cpg or ConvArgs::ws_cpg).  The A fragment of a 32-row block is read with
// ds_read_b128, whose 16-lane groups cover rows {0-3,12-15,20-27} / {4-11,16-19,28-31}: with 16-wide tiles the pitch must
// be a multiple of 256 B, with 8-wide tiles an odd multiple of 128 B, for the 16 reads to fall on 16 distinct 16-B slots.
constexpr int conv_lds_row(int ks, int stride, int tw_log2, int cpg) {
  const int pixb = 64 * cpg + 16;
  const int pw = ((1 << tw_log2) - 1) * stride + ks;
  int rb = (pw * pixb + 15) & ~15;
  if (ks == 1 || stride != 1) return rb;   // no halo: consecutive pixels already conflict-free
  if (tw_log2 == 4) rb = (rb + 255) & ~255;
  else if (tw_log2 == 3) { rb = (rb + 127) & ~127; if (((rb >> 7) & 1) == 0) rb += 128; }
  return rb;
}
// k_conv_mfma.  With ConvArgs::cpg == 2 and a 3 x 3 conv: its two-chunk-per-group form, TILE_128x64 (experiment) and the
// narrow-output tiles TILE_256x32 / TILE_128x32 (convs with <= 32 output channels, e.g. the UNet's final conv).
// LDS bytes needed by a launch; 0 if the geometry is not supported by `tile`
size_t conv_lds_bytes(int dtype, int tile, int ks, int stride, const ConvArgs& a);
hipError_t launch_conv(int dtype, int tile, int ks, int stride, const ConvArgs& a, hipStream_t st);
// warp-specialised persistent variant (stride 1, stage_mode 0, no split-K); 0 bytes = not applicable
size_t conv_ws_lds_bytes(int dtype, int tile, int ks, const ConvArgs& a);
hipError_t launch_conv_ws(int dtype, int tile, int ks, const ConvArgs& a, hipStream_t st);
// image-resident kernel for 8 x 8 feature maps (one workgroup = one image x 32 output channels, the whole K inside
// the workgroup, GroupNorm finalised in the prologue, statistics of the result in the epilogue): no split-K slabs,
// no reduce launch, no k_gn_finalize launch.  `gn` says whether a GroupNorm precedes the conv.
bool conv_img_applicable(int dtype, int ks, int stride, const ConvArgs& a, bool gn, int gn_groups);
hipError_t launch_conv_img(int dtype, int ks, const ConvArgs& a, hipStream_t st);
// first conv of the UNet (1..7 input channels): the 9 taps x Cin receptive field as ONE K dimension on the MFMA;
// a.wpack = the im2col-ordered pack (pack_first in dsx_model.cpp).  One GroupNorm partial row per (16x16 tile, wave).
bool conv_first_applicable(int ks, int stride, const ConvArgs& a, bool gn);
hipError_t launch_conv_first(int dtype, const ConvArgs& a, hipStream_t st);
// one-time function attributes (dynamic LDS limit); call outside any stream capture
hipError_t conv_init();
hipError_t ops_init();

// Plain direct convolution (one thread per output element), any odd KS, stride 1,
// weights [Cout][KS][KS][Cin] fp32.  Used for the 7x7 ForegroundMask conv and as
// an on-device cross-check of the MFMA path (DSX_CONV_IMPL=naive).
struct NaiveConvArgs {
  ConvArgs c;
  const float* w;  // [Cout][KS][KS][C]
  int ks, stride;
  int sigmoid_out;
};
hipError_t launch_conv_naive(const NaiveConvArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// GroupNorm statistics
// ---------------------------------------------------------------------------
// per-(image, pixel-chunk, channel) partial {sum, sumsq} in double:
//   part[((b*nchunk + ch)*C + c)*2 + {0,1}]
hipError_t launch_chan_stats(const void* x, int bf16, int B, int HW, int C, int nchunk, double* part,
                             hipStream_t st);
hipError_t launch_gn_finalize(const GnFinArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// time embedding + all FiLM vectors of one forward in one launch
// ---------------------------------------------------------------------------
struct TembArgs {
  int flavour;            // 0 sr3 (PositionalEncoding), 1 ddpm (TimeEmbedding)
  int B;                  // rows to produce
  int n_time;             // B or 1 (broadcast)
  const float* time;      // direct time values, or nullptr -> table[*step_ctr]
  const float* table;     // per-step tcond table (device); per_sample: [step][B]
  const int* step_ctr;
  int per_sample;
  int inner;              // C0
  const float* freq;      // [inner/2]
  const float* w1; const float* b1;   // [4*inner][inner], [4*inner]
  const float* w2; const float* b2;   // [inner][4*inner], [inner]
  const float* wf; const float* bf;   // all FiLM linears stacked: [F][inner], [F]
  int F;
  float* film;            // [B][F]
};
hipError_t launch_temb(const TembArgs& a, hipStream_t st);

// ---------------------------------------------------------------------------
// attention (single head, d = C):  S = QK^T/sqrt(C); P = softmax(S); O = PV
// ---------------------------------------------------------------------------
// out[m][n] = sum_s slab[s][m][n] + bias[n] + film[b][n] + resid[m][n]   (split-K epilogue)
struct SplitKReduceArgs {
  const float* slab; int nsplit; long long slab_stride;
  long long M; int N; int HW;            // b = m / HW
  const float* bias; const float* film; int film_bs;
  const void* resid; int resid_ld;
  void* out;
  int act_bf16;                          // storage kind of resid and out (0 fp32, 1 bf16, 2 fp16)
  float* stat_part;                      // nullptr, or GroupNorm partials [B][HW/16][N][2] of `out` (N % 64 == 0, HW % 16 == 0),
                                         // shifted by the pivot bias[n] + film[b][n] (StatPivot)
};
hipError_t launch_splitk_reduce(const SplitKReduceArgs& a, hipStream_t st);

// fused single-head attention (dsx_attn.hip): out[b][i][:] = softmax_j(q_i . k_j / div) . v_j ; no L x L tensor in HBM.
// q / k / v: token-major rows of `ld` elements (the three thirds of the qkv conv's output), out: rows of `ldo`.
// The kernel reads all three through ONE buffer descriptor per image, based at q's first row of that image and
// L * ld * ES bytes long: q, k and v must be column ranges of the same rows with k >= q and v >= q (their byte
// offsets from q are taken as unsigned), each range inside the row, and L * ld * ES < 2^31.  Three separate
// allocations cannot be expressed.  launch_attn checks alignment only; dsx_attention (dsx_exec.cpp) checks the rest
// for caller tensors, the planner satisfies it by construction (ld = 3C, q first).
struct AttnArgs {
  const void* q; const void* k; const void* v; int ld;
  void* out; int ldo;
  int storage;            // element type of q, k, v and out: 0 fp32, 1 bf16, 2 fp16
  int B, L, C;            // images, tokens per image, head dimension (= channels)
  float div, inv_div;     // sqrt(C) and its reciprocal
};
bool attn_supported(int C, int L);
// `col_split`: launches with few query tiles and 257..512 channels run two workgroups per tile, half of the output
// channels each (the planner's choice, PlanKnobs::attn_cs)
hipError_t launch_attn(const AttnArgs& a, bool col_split, hipStream_t st);

// ---------------------------------------------------------------------------
// layout, sampler update, RNG, tiling
// ---------------------------------------------------------------------------
// dst[b][hw][c] = src[(b*ctot + coff + c)*HW + hw]   (channel slice of an NCHW tensor -> NHWC)
hipError_t launch_nchw_slice_to_nhwc(const float* src, void* dst, int dst_bf16, int B, int C, int ctot, int coff,
                                     int HW, hipStream_t st);
hipError_t launch_nhwc_to_nchw(const float* src, float* dst, int B, int C, int H, int W, hipStream_t st);

// The loop update (k_update, dsx_steps.hip): one launch per step of dsx_sample_loop, dsx_sample_loop_streams and
// dsx_solver_loop.
constexpr int kUpdateCols = 7;
struct UpdateArgs {
  float* x;               // state, NHWC [B][H][W][C], always fp32
  void* x_act;            // the first conv's copy of the state in the activation storage type (16-bit builds),
                          // or nullptr when the conv reads `x` itself
  int x_act_kind;         // its storage kind (1 bf16, 2 fp16)
  const float* net;       // UNet output, NHWC
  float* x0_hist;         // the few-step solvers' previous predicted x0, NHWC fp32 like x: read where the row's cp != 0,
                          // written at every step; nullptr (ancestral loops): never read and never written
  int use_noise;          // 0 -> Philox normals keyed by (seed, step); 1 -> injected draws
  // per-call values live in device memory so that one captured graph serves every call:
  // loop_params[0] = Philox seed, loop_params[1] = address of the injected noise [steps][B][C][H][W] (NCHW,
  // reference draw order)
  const unsigned long long* loop_params;
  const float* tab;       // device table [kUpdateCols][n_steps]: tcond,a,b,c1,c2,cp,sigma (step_update's names)
  int n_steps;            // column stride of `tab` (its capacity)
  const int* step_ctr;
  int predict_eps, clip;
  int per_sample;         // the table columns hold [step][B] values instead of one per step (never with x0_hist)
  int B, C, H, W;
  // per-sample noise streams (include/dsx.h): device array of B sample ids, read at every step -> the stream form of
  // the kernel (element (b, c, hw) takes element c*H*W + hw of the stream (seed, ids[b] << 24 | step + 1)); nullptr ->
  // the default form, one stream per step at the flat NHWC index
  const unsigned long long* sample_ids;
};
hipError_t launch_update(const UpdateArgs& a, hipStream_t st);
// Per-sample noise streams without an executor: the Philox subsequences (id << 24 | draw) of up to kStreamRows samples
// travel in the kernel arguments; larger batches take several launches.
constexpr int kStreamRows = 32;
struct StreamIds { unsigned long long subseq[kStreamRows]; };
// f(b0, rows, s) for every run of up to kStreamRows samples of a batch: s.subseq[r] = ids[b0 + r] << 24 | draw
template <class F>
static inline hipError_t each_stream_chunk(int B, const uint64_t* ids, uint64_t draw, F&& f) {
  for (int b0 = 0; b0 < B; b0 += kStreamRows) {
    StreamIds s{};
    const int rows = B - b0 < kStreamRows ? B - b0 : kStreamRows;
    for (int r = 0; r < rows; ++r) s.subseq[r] = ((unsigned long long)ids[b0 + r] << 24) | draw;
    const hipError_t e = f(b0, rows, s);
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}
// out (rows, chw): row r = the first chw elements of the stream (seed, s.subseq[r]); rows <= kStreamRows
hipError_t launch_randn_samples(float* out, int rows, long long chw, unsigned long long seed, const StreamIds& s,
                                hipStream_t st);
hipError_t launch_advance(int* step_ctr, hipStream_t st);
hipError_t launch_randn(float* out, long long n, unsigned long long seed, unsigned long long subseq,
                        hipStream_t st);
// grid of a 256-thread grid-stride launch over `total` items
static inline unsigned grid_for(long long total) {
  long long g = (total + 255) / 256;
  return (unsigned)(g > 4096 ? 4096 : (g < 1 ? 1 : g));
}
#if defined(__HIPCC__)
// One IEEE operation each, never contracted into an fma: the pragma takes the `contract` flag off the instruction, and
// the backend fuses a product into a sum only when both carry it.
__device__ __forceinline__ float mul_f(float a, float b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ float add_f(float a, float b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ float sub_f(float a, float b) {
#pragma clang fp contract(off)
  return a - b;
}
__device__ __forceinline__ double mul_d(double a, double b) {
#pragma clang fp contract(off)
  return a * b;
}
__device__ __forceinline__ double add_d(double a, double b) {
#pragma clang fp contract(off)
  return a + b;
}
__device__ __forceinline__ double sub_d(double a, double b) {
#pragma clang fp contract(off)
  return a - b;
}

// ---------------------------------------------------------------------------
// The skeleton the NCHW pointwise kernels share (dsx_steps.hip, dsx_validate.hip).  A thread owns group i4: the four consecutive elements from 4 * i4 (= one
// Philox block of the flat normal stream, where one is drawn).  VEC: H * W is a multiple of 4 and every base pointer is 16-byte aligned, so
// a group lies inside one (b, c) row and is one 16-byte access in every tensor; otherwise its first `cnt` elements are
// accessed one by one.  Each body below is written once over the arrays of a group, so both instantiations give the
// same bits.
// ---------------------------------------------------------------------------
// the elements of a group that exist, unrolled: the arrays of a group stay in registers
#define DSX_EACH4(j, cnt) _Pragma("unroll") for (int j = 0; j < 4; ++j) if (j < (cnt))
// the flat indices of group i4 of n elements; returns how many of them exist
template <bool VEC>
__device__ __forceinline__ int group4(long long i4, long long n, long long at[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) at[j] = i4 * 4 + j;
  return VEC ? 4 : (int)min(4LL, n - i4 * 4);
}
// row[j] = at[j] / len: the (b, c) row with len = H*W, the sample with len = C*H*W.  VEC: one division per group.
template <bool VEC>
__device__ __forceinline__ void rows4(const long long at[4], int cnt, long long len, long long row[4]) {
  if (VEC) row[0] = row[1] = row[2] = row[3] = at[0] / len;
  else DSX_EACH4(j, cnt) row[j] = at[j] / len;
}
template <bool VEC>
__device__ __forceinline__ void load4(const float* p, const long long at[4], int cnt, float v[4]) {
  if (VEC) {
    const float4 t = *(const float4*)(p + at[0]);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    DSX_EACH4(j, cnt) v[j] = p[at[j]];
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, const long long at[4], int cnt, const float v[4]) {
  if (VEC) *(float4*)(p + at[0]) = make_float4(v[0], v[1], v[2], v[3]);
  else DSX_EACH4(j, cnt) p[at[j]] = v[j];
}
// the same group in a uint16 tensor: one 8-byte access under VEC (the base pointers then are 8-byte aligned)
template <bool VEC>
__device__ __forceinline__ void load4(const unsigned short* p, const long long at[4], int cnt, unsigned v[4]) {
  if (VEC) {
    const ushort4 t = *(const ushort4*)(p + at[0]);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
  } else {
    DSX_EACH4(j, cnt) v[j] = p[at[j]];
  }
}
template <bool VEC>
__device__ __forceinline__ void store4(unsigned short* p, const long long at[4], int cnt, const unsigned v[4]) {
  if (VEC) *(ushort4*)(p + at[0]) = make_ushort4((unsigned short)v[0], (unsigned short)v[1], (unsigned short)v[2], (unsigned short)v[3]);
  else DSX_EACH4(j, cnt) p[at[j]] = (unsigned short)v[j];
}
template <class... P>
static inline bool aligned16(const P*... p) { return ((... | (uintptr_t)p) & 15u) == 0; }   // nullptr counts as aligned

// The reverse update of every sampler -- ancestral (sr3 diffusion.py:141-175, ddpm diffusion.py:163-203, indi.py:62-69)
// and few-step (DDIM, DPM-Solver++(2M) in data prediction; model/solvers.py builds the rows) -- stated once for the
// loop (k_update) and the single step (k_step), both in dsx_steps.hip; every product and sum is rounded on its own, as
// the reference's ATen op sequence does:
//   x0   = predict_eps ? clamp(a*x - b*net) : net          (the clamp to +-1 only with clip)
//   mean = c1*x0 + c2*x
//   mean = cp != 0 ? mean + cp*x0_prev : mean              (the caller does not load x0_prev where cp == 0)
//   out  = use_z ? mean + z*sigma : mean
// An ancestral row is a solver row with cp == 0.  The solver tables (dsx_solver_table, dsx_solver_step) name and order
// their columns cx, c0: x0's coefficient c0 is c1 here and x's coefficient cx is c2 -- c1 = c0, c2 = cx, the only
// place where the two orders meet (dsx_solver_loop and dsx_solver_step in dsx_exec.cpp fill c1 / c2 by that rule).
struct StepVals { float x0, mean, out; };
__device__ __forceinline__ StepVals step_update(float a, float b, float c1, float c2, float cp, float sigma, bool predict_eps,
                                                bool clip, float x, float net, float x0_prev, float z, bool use_z) {
  StepVals v;
  v.x0 = net;
  if (predict_eps) {
    v.x0 = sub_f(mul_f(a, x), mul_f(b, net));
    if (clip) v.x0 = fminf(fmaxf(v.x0, -1.0f), 1.0f);
  }
  v.mean = add_f(mul_f(c1, v.x0), mul_f(c2, x));
  if (cp != 0.f) v.mean = add_f(v.mean, mul_f(cp, x0_prev));
  v.out = use_z ? add_f(v.mean, mul_f(z, sigma)) : v.mean;
  return v;
}

// The engine's normal stream: element i of the stream (seed, subseq) is component i % 4 of normal4(seed, subseq, i / 4).
// Shared by k_randn (dsx_ops.hip) and the pointwise kernels of dsx_steps.hip, k_update among them, which must agree bitwise.
__device__ __forceinline__ void philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3,
                                              unsigned k0, unsigned k1, unsigned out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
    const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0;
    const unsigned n1 = (unsigned)p1;
    const unsigned n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    const unsigned n3 = (unsigned)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
__device__ __forceinline__ void normal4(unsigned long long seed, unsigned long long subseq,
                                        unsigned long long idx4, float z[4]) {
  unsigned r[4];
  philox4x32_10((unsigned)idx4, (unsigned)(idx4 >> 32), (unsigned)subseq, (unsigned)(subseq >> 32),
                (unsigned)seed, (unsigned)(seed >> 32), r);
  const float u0 = ((float)r[0] + 0.5f) * 2.3283064365386963e-10f;  // (0,1]
  const float u1 = ((float)r[1] + 0.5f) * 2.3283064365386963e-10f;
  const float u2 = ((float)r[2] + 0.5f) * 2.3283064365386963e-10f;
  const float u3 = ((float)r[3] + 0.5f) * 2.3283064365386963e-10f;
  const float ra = sqrtf(-2.0f * logf(u0)), rb = sqrtf(-2.0f * logf(u2));
  float s, c;
  sincosf(6.283185307179586f * u1, &s, &c);
  z[0] = ra * c; z[1] = ra * s;
  sincosf(6.283185307179586f * u3, &s, &c);
  z[2] = rb * c; z[3] = rb * s;
}
// Component k (0..3) of normal4(seed, subseq, idx4), bit for bit: the same operations on the half of the Philox block
// it comes from.  For kernels whose neighbouring elements lie in different blocks (per-sample noise streams).
__device__ __forceinline__ float normal1(unsigned long long seed, unsigned long long subseq,
                                         unsigned long long idx4, int k) {
  unsigned r[4];
  philox4x32_10((unsigned)idx4, (unsigned)(idx4 >> 32), (unsigned)subseq, (unsigned)(subseq >> 32),
                (unsigned)seed, (unsigned)(seed >> 32), r);
  const unsigned ru = (k & 2) ? r[2] : r[0], rv = (k & 2) ? r[3] : r[1];
  const float u = ((float)ru + 0.5f) * 2.3283064365386963e-10f;  // (0,1]
  const float v = ((float)rv + 0.5f) * 2.3283064365386963e-10f;
  const float rad = sqrtf(-2.0f * logf(u));
  float s, c;
  sincosf(6.283185307179586f * v, &s, &c);
  return rad * ((k & 1) ? s : c);
}
#endif

// dsx_steps.hip.  q_sample of the three sampler families in one launch (NCHW fp32):
//   dst[b][coff + c] = c0[b] * x0[b][c] (+ c1[b] * xe[b][c % Ce]) + c2[b] * z[b][c],  each operation rounded on its own.
// xe == nullptr: the two-term (Gaussian) form.  z == nullptr: z is element i of the normal stream (seed, subseq) at
// the flat (B, C, H, W) index i (what launch_randn writes) and is stored to z_out when that is not nullptr.
struct QSampleArgs {
  const float* x0; const float* xe;
  const float* c0; const float* c1; const float* c2;     // device, B values each
  const float* z; unsigned long long seed, subseq; float* z_out;
  float* dst;
  int B, C, Ce, HW, Cdst, coff;
};
hipError_t launch_q_sample(const QSampleArgs& a, hipStream_t st);
// dsx_eval.hip.  per-sample sum |a - b| (squared == 0) or sum (a - b)^2 over n elements, in double: part[B][loss_blocks(n)] partials
// in a fixed partition, out[B] their sums in a fixed order (two launches, no atomics)
int loss_blocks(long long n);
hipError_t launch_loss(const float* a, const float* b, int B, long long n, int squared, double* part, double* out,
                       hipStream_t st);

// dsx_validate.hip.  The validation report of the training loop (split.py:174-241) on NCHW fp32 visuals: uint16 counts
// (x * std + mean in double, every operation rounded on its own, truncated; the prediction clamped to [0, 65535] first),
// exact integer statistics, and -- with the three *_n pointers -- the uint16 numerators of the [0, 1] images.  Two
// launches; the layouts of `part` (B * (C + Cin) * val_blocks(HW) rows of 4 words) and `stats` are stated in include/dsx.h.
constexpr int kValChunk = 4096;        // pixels of one plane per workgroup of the first launch (DSX_VAL_CHUNK)
constexpr int kValMaxC = 16;           // target channels (DSX_VAL_MAX_CHANNELS): their mean / std travel in the kernel arguments
constexpr int kValFinishBlocks = 64;   // workgroups per plane of the second launch at most: each re-reads the plane's partial rows
struct ValArgs {
  const float* input; const float* target; const float* pred;                       // (B, Cin, H, W), (B, C, H, W) x 2
  unsigned short* input_q; unsigned short* target_q; unsigned short* pred_q;
  unsigned short* input_n; unsigned short* target_n; unsigned short* pred_n;        // all three, or all nullptr
  unsigned long long* part; unsigned long long* stats;
  double mean_in, std_in, mean_t[kValMaxC], std_t[kValMaxC];
  int B, Cin, C, nblk;
  long long HW;
};
int val_blocks(long long HW);
hipError_t launch_val_report(const ValArgs& a, hipStream_t st);

// One reverse update with its intermediates (step_update above; NCHW fp32, per-sample coefficients, B values each):
//   out = mean + z*sigma (mean where sigma == 0 or x_out == nullptr: no draw and no sum)
// a / b are read only with predict_eps.  x0_prev == nullptr: every cp counts as 0; else it is read only for the
// samples whose cp != 0.  z == nullptr: element i of the normal stream (seed, subseq); repeat: every sample uses sample
// 0's draw (z then holds C*H*W values).  Outputs that are nullptr are not written; x_out may be x and x_recon_out may
// be x0_prev.
struct StepArgs {
  const float* x; const float* net; const float* x0_prev;
  const float* a; const float* b; const float* c1; const float* c2; const float* cp; const float* sigma;
  const float* z; unsigned long long seed, subseq;
  float* x_recon_out; float* mean_out; float* x_out;
  int B, predict_eps, clip, repeat;
  long long CHW;
};
// ids == nullptr: one launch.  Else (host array of a.B sample ids) z = element (i % CHW) of the stream
// (a.seed, ids[i / CHW] << 24 | draw), kStreamRows samples per launch with every tensor and coefficient pointer moved
// on to the launch's first sample; a.z, a.subseq and a.repeat are not read.
hipError_t launch_step(const StepArgs& a, long long HW, const uint64_t* ids, uint64_t draw, hipStream_t st);
// out = c*(a0[b]*x1 + s0[b]*z1) + d*(a0[b]*x2 + s0[b]*z2); z1 == nullptr: the streams (seed, subseq), (seed, subseq + 1)
struct InterpStartArgs {
  const float* x1; const float* x2; const float* a0; const float* s0;
  const float* z1; const float* z2; unsigned long long seed, subseq;
  float c, d;
  float* out;
  int B;
  long long CHW;
};
hipError_t launch_interp_start(const InterpStartArgs& a, long long HW, hipStream_t st);

// dsx_tiles.hip: tile gather, stitch and pack of tiled prediction (never inside a sampling step).
// the tiles of one launch: ids first, first + stride, ... (count of them); the tables a kernel indexes with an id
// (`starts` [..][3], `regions` [..][8], `off` [..]) live on the device -- the plan's own (dsx_tileplan), or a per-call
// table with first = 0, stride = 1
struct TileSeq { long long first, stride, count; };
constexpr long long kMaxItemsPerLaunch = 65535;   // tiles / items of one launch: they are the grid's y (or z)
// the geometry of a gather: (N, H, W) frames cut into ph x pw patches at starts[id] = (frame, y, x), for the ids of
// seq.  `starts` is a device table; the per-item kernel (launch_tiles_gather_mix_items) carries its starts in its
// records and does not read it.
struct TileGeom { int H, W, ph, pw; const int* starts; TileSeq seq; };
hipError_t launch_tiles_gather(const float* frames, const TileGeom& g, float* tiles, hipStream_t st);
// crop + dataset normalisation fused (SplitDataset.__getitem__): norm = {mean_inp, std_inp, mean_t0, std_t0, mean_t1, std_t1}
hipError_t launch_tiles_gather_norm(const float* f0, const float* f1, const TileGeom& g, float w0, float w1,
                                    const double norm[6], int from_norm_target, float* tin, float* ttar, hipStream_t st);
// the same for frames with colour planes: stacks (N, Cc, H, W), tin (count, Cc, ph, pw), ttar (count, 2 Cc, ph, pw),
// one mean / std per target plane (2 Cc of each); 1 <= Cc <= kPlanesMaxC, the items are the grid's z
constexpr int kPlanesMaxC = 8;
hipError_t launch_tiles_gather_norm_planes(const float* f0, const float* f1, int Cc, const TileGeom& g, float w0, float w1,
                                           double mean_inp, double std_inp, const double* mean_target,
                                           const double* std_target, float* tin, float* ttar, hipStream_t st);
// the network input of an input-only stack: frames (N, H, W) of uint8 / uint16 (pix_bytes 1 / 2) or fp32 (is_float, 4)
// pixels -> out (count, 1, ph, pw) = (float)(((double)min((float)pixel, (float)clip) - mean) / std); clip < 0: none.
// The grid's x grows with ph * pw.
hipError_t launch_tiles_gather_input(const void* frames, int pix_bytes, bool is_float, const TileGeom& g, double mean,
                                     double std, double clip, float* out, hipStream_t st);
// frame-keyed noise: out (count, C, ph, pw), tile k cut at (n, y0, x0) = the crop [c, y0.., x0..] of the (C, H, W) tensor
// of the sample stream (seed, ((id_base + n) << 24) | draw); C * ph * pw fits 32 bits
hipError_t launch_tiles_randn(const TileGeom& g, int C, unsigned long long seed, unsigned long long id_base, unsigned draw,
                              float* out, hipStream_t st);
// crop + target normalisation + the two mixed inputs of the TimePredictor evaluation and their min-max-normalised
// classifier views, fused (op list: include/dsx.h, dsx_tiles_gather_mix).  norm = {mean_t0, std_t0, mean_t1, std_t1};
// w0 = (float)(1 - t), w1 = (float)t; lo / rng = (float)lo, (float)(hi - lo) of the table rows of the two channels.
// Any of ttar / tmix / tcls may be nullptr (not all three); each is (count, 2, ph, pw).
struct MixWeights { float w0, w1, lo0, rng0, lo1, rng1; };
hipError_t launch_tiles_gather_mix(const float* f0, const float* f1, const TileGeom& g, const double norm[4],
                                   const MixWeights& mw, float* ttar, float* tmix, float* tcls, hipStream_t st);
// the same with one record per item (dev table, item k of the launch = items[k]): its (frame, y, x) start and its own
// weights (g.starts is not read, g.seq = {0, 1, count}); the arithmetic per element is launch_tiles_gather_mix's, bit
// for bit.
struct MixItem { int n, y, x; MixWeights w; };
hipError_t launch_tiles_gather_mix_items(const float* f0, const float* f1, const TileGeom& g, const MixItem* items /*dev*/,
                                         const double norm[4], float* ttar, float* tmix, float* tcls, hipStream_t st);
// source of a paste: whole predicted tiles (count, C, ph, pw) of the sequence, or the gathered packed exchange buffer
// [world][rank_stride] (valid regions [C][h][w] of rank q's tiles q, q + world, ... back to back; `off` = pixel offset
// of each tile id inside its rank's run)
struct StitchSrc {
  const float* base; int packed; int ph, pw;
  const long long* off; long long rank_stride; int world;
};
// paste (gt == nullptr) or paste + per-(tile, workgroup, channel) partial sums for RangeInvariantPsnr:
// part[count][gx][C][8] doubles {sum p, sum p^2, sum g, sum g^2, sum g p, min g, max g, 0}, C <= kPsnrMaxC
constexpr int kPsnrMaxC = 4;         // channels of a paste or blend that takes the sums
hipError_t launch_stitch(const StitchSrc& s, int C, const int* regions /*dev*/, TileSeq seq, float* canvas, int H, int W,
                         const float* gt, double* part, int gx, hipStream_t st);
// valid regions of the sequence's tiles -> this rank's flat run (the crop of tile_stitcher.py:38-56 before the collective)
hipError_t launch_tiles_pack(const float* tiles, int C, int ph, int pw, const int* regions, const long long* off,
                             TileSeq seq, float* flat, hipStream_t st);
// Blended stitching: the overlap-add of ALL tiles of a plan into the (N,H,W,C) canvas, as a gather (include/dsx.h,
// dsx_tileplan_blend).  tiles: whole (C, ph, pw) tiles, tile t at  (t % world) * rank_stride + (t / world) * C*ph*pw
// (world == 1: (total, C, ph, pw)).  The plan's tiles are frame-major, ny x nx per frame, tile (iy, ix) of frame n is
// id (n*ny + iy)*nx + ix; rows[y] = (first tile row, count) and cols[x] = (first tile column, count) name the
// contributors of a canvas pixel, wy / wx the separable window.  gt != nullptr: also part[N][blocks][C][8] (C <= kPsnrMaxC).
// step != 0 (dsx_tileplan_blend_step; gt == nullptr): the canvas is a frame state, updated in place with the blended
// value as x0:  X = c_x0*v + c_xt*X (+ z*sigma where sigma != 0), z from the noise field (seed, id_base + n, draw).
struct BlendArgs {
  const float* tiles; int C, world; long long rank_stride;
  int N, H, W, ph, pw, ny, nx;
  const int* starts;                 // dev [total][3]
  const int* rows; const int* cols;  // dev [H][2], [W][2]
  const float* wy; const float* wx;  // dev [ph], [pw]
  float* canvas; const float* gt; double* part;
  int step; float c_x0, c_xt, sigma;
  unsigned long long seed, id_base; unsigned draw;
};
// workgroups per frame of a blend of (H, W) frames: segments of 256 pixels along x times at most 128 row slots
struct BlendGrid { int segs, rows; };
static inline BlendGrid blend_grid(long long H, long long W) {
  return BlendGrid{(int)((W + 255) / 256), (int)(H > 128 ? 128 : H)};
}
hipError_t launch_blend(const BlendArgs& a, hipStream_t st);
// Tile disagreement (include/dsx.h, dsx_tileplan_disagreement): per canvas pixel and channel the unbiased variance among
// the tiles that cover it, in the blend's geometry, tile layouts and contributor tables.  near_y[H] / near_x[W]: the
// near-line masks of the call's band.  map (N,H,W,C) of (float)sqrt(var), or nullptr; part[N][blocks][C][8] =
// {count k >= 2, sum var, band count, band sum var, min var, max var, 0, 0} per (frame, workgroup, channel), C <= kPsnrMaxC.
struct DisagreeArgs {
  const float* tiles; int C, world; long long rank_stride;
  int N, H, W, ph, pw, ny, nx;
  const int* starts;                 // dev [total][3]
  const int* rows; const int* cols;  // dev [H][2], [W][2]
  const unsigned char* near_y; const unsigned char* near_x;   // dev [H], [W]
  float* map; double* part;
};
hipError_t launch_disagreement(const DisagreeArgs& a, hipStream_t st);
// the tiles of the sequence out of a multi-channel frame state: canvas (N,H,W,C) -> tiles (count, C, ph, pw)
hipError_t launch_tiles_gather_canvas(const float* canvas, int C, const TileGeom& g, float* tiles, hipStream_t st);

// dsx_eval.hip: Welford moments, range table, image metrics (the loss reduction is declared with the steps above).
// Welford's recurrence over repeated samples, in double with every operation rounded on its own (include/dsx.h)
hipError_t launch_moments_update(const float* x, double* mean, double* m2, long long count, int r, hipStream_t st);
hipError_t launch_moments_finish(const double* mean, const double* m2, long long count, int n, float* mean_out,
                                 float* std_out /* may be nullptr */, hipStream_t st);
// min / max over all pixels of t * a + (1 - t) * b, t = t_int / n for t_int = 0..n, on the normalised channels
// (compute_input_normalization_dict, data/time_predictor_dataset.py:6-21), fp64 with every operation rounded on its
// own.  part[mix_range_blocks(pixels)][n + 1][2] = {min, max} per pixel workgroup; the caller reduces over the rows.
int mix_range_blocks(long long pixels);
hipError_t launch_mix_range(const float* f0, const float* f1, long long pixels, const double norm[4], int n, double* part,
                            hipStream_t st);
// SSIM (core/metrics.py:72-92) + sum of squared differences of `planes` image pairs (H, W >= 11), optionally quantised
// on the load as tensor2img does (:14-34); part[planes][image_metrics_tiles(H, W)][2] = {sum of the SSIM map over
// the tile, SSD (uint64 bits when quantised, else fp64)}.  win = the 11 taps of cv2.getGaussianKernel(11, 1.5).
struct SsimWindow { double w[11]; };
int image_metrics_tiles(int H, int W);
hipError_t launch_image_metrics(const float* a, const float* b, int planes, int H, int W, int quantize, float lo,
                                float hi, float rng, double c1, double c2, const SsimWindow& win, double* part,
                                hipStream_t st);
// dsx_msssim.hip.  Multi-scale SSIM of `planes` plane pairs (include/dsx.h, dsx_msssim): every launch of a call on `st`,
// nothing synchronised.  ws holds planes * msssim_layout(H, W, scales, ..) doubles; *out_dev (inside ws) receives
// [planes][scales][{mean cs, mean ssim}].  c1, c2 are used when range_invariant == 0, else derived per plane on the device.
struct MsssimLayout { long long off[5]; int tiles[5]; int H[5]; int W[5]; double count[5]; };
size_t msssim_layout(int H, int W, int scales, MsssimLayout* lay);
hipError_t launch_msssim(const float* pred, const float* target, int planes, int H, int W, int scales, int range_invariant,
                         double c1, double c2, const SsimWindow& win, double* ws, double** out_dev, hipStream_t st);

// dsx_refine.hip.  The centred second moments of `planes` plane triples (g, p1, p2) of n pixels each (include/dsx.h,
// dsx_comoments): one pass on data shifted by each plane's first element, two launches on `st`, nothing synchronised.
// stride = {plane, pixel} element strides of g, p1, p2; part[planes][comoments_blocks(n)][kComSlots] = the workgroups'
// {S g', S p1', S p2', S g'g', S p1'p1', S p2'p2', S g'p1', S g'p2', S p1'p2', min g, max g, 0}; out[planes][12].
// vec: 16-byte loads (pixel strides 1, bases and plane strides multiples of four elements, n % 4 == 0: the caller's check).
constexpr int kComSlots = 12;
struct ComArgs {
  const float* g; const float* p1; const float* p2;
  long long n, span;       // span = comoments_span(n): pixels per workgroup
  long long stride[6];
  double* part; double* out;
};
int comoments_blocks(long long n);
long long comoments_span(long long n);
hipError_t launch_comoments(const ComArgs& a, int planes, bool vec, hipStream_t st);

// dsx_calib.hip.  The calibration sums of channel-last canvases (mean, std, target), n pixels of C interleaved fp32
// channels (include/dsx.h, dsx_calibration): one pass, two launches on `st`, nothing synchronised.  A row, of a
// workgroup's partials and of out alike, is [C][3 * nbins + nz] doubles: per channel nbins x {count, Sv, Se}, then nz
// coverage counts; part[calibration_blocks(n)][row].  edges[c * (nbins - 1) + j] and z[] travel in the argument struct.
// vec: 16-byte loads (the three bases 16-byte aligned and n * C % 4 == 0: the caller's check).
constexpr int kCalMaxC = 4, kCalMaxBins = 64, kCalMaxZ = 8;
struct CalArgs {
  const float* mean; const float* sd; const float* target;
  long long elems, span;   // elems = n * C values; span = C * calibration_span(n): values per workgroup, a multiple of 4
  int C, nbins, nz;
  double* part; double* out;
  double edges[kCalMaxC * (kCalMaxBins - 1)];
  double z[kCalMaxZ];
};
inline int calibration_row(int C, int nbins, int nz) { return C * (3 * nbins + nz); }
int calibration_blocks(long long n);
long long calibration_span(long long n);
hipError_t launch_calibration(const CalArgs& a, bool vec, hipStream_t st);

// dsx_quantiles.hip.  Per-element quantiles and ranks across n <= 64 samples (include/dsx.h, dsx_sample_quantiles): one
// launch on `st`, nothing synchronised.  Sample r, element i at x[r * stride + i]; out [nq][count]; target and rank
// [count], both or neither.  lo[k], hi[k], t[k]: the two order statistics of quantile k and the weight between them,
// formed on the host in double.  The network sorts quantiles_wires(n) wires; on the wide path a thread takes
// quantiles_per_thread(wires) neighbouring elements with one load of that width per sample (every base a multiple of
// that many elements, stride and count too: the caller's check), else one element with 4-byte loads.
constexpr int kQuantMaxN = 64, kQuantMaxQ = 8;
struct QuantArgs {
  const float* x; long long stride, count;
  int n, nq;
  float* out; const float* target; float* rank;
  int lo[kQuantMaxQ], hi[kQuantMaxQ];
  double t[kQuantMaxQ];
};
constexpr int quantiles_wires(int n) { return n <= 2 ? 2 : n <= 4 ? 4 : n <= 8 ? 8 : n <= 16 ? 16 : n <= 32 ? 32 : 64; }
constexpr int quantiles_per_thread(int wires) { return wires <= 32 ? 4 : 2; }
hipError_t launch_quantiles(const QuantArgs& a, bool wide, hipStream_t st);

// dsx_consistency.hip.  The residual of a split against its acquisition, x - sum_c w_c p_c, its per-frame report row
// and the Gaussian conditioning of (mean, std) on it (include/dsx.h, dsx_consistency): one pass over `frames` frames
// of `plane` pixels, two launches on `st` (one without a report), nothing synchronised.  in: (frames, plane) of pix
// (DSX_PIX_U8 / U16 / F32); mean, sd, omean, osd: (frames, plane, C) fp32; map: (frames, plane); sd, map, omean, osd,
// out may be null, part only with out.  part[frames][consistency_blocks(plane)][kConSlots]; out[frames][kConSlots].
// vec: four pixels per thread with 16-byte loads and stores of the fp32 operands and one 4 / 8 / 16-byte load of the
// input (every base that aligned and plane % 4 == 0: the caller's check).
constexpr int kConMaxC = 4, kConSlots = 10;
struct ConArgs {
  const void* in; const float* mean; const float* sd;
  float* map; float* omean; float* osd;
  double* part; double* out;
  long long plane, span;   // span = consistency_span(plane): pixels per workgroup, a multiple of 4
  int pix, C;
  double a[kConMaxC], b[kConMaxC], w[kConMaxC];
  double clip, noise_var;
};
int consistency_blocks(long long plane);
long long consistency_span(long long plane);
hipError_t launch_consistency(const ConArgs& a, int frames, bool vec, hipStream_t st);

// dsx_select.hip.  One pass of the radix select behind dsx_order_stats: hist[1 << bits] (64-bit, zeroed by the caller)
// += the digit (u >> shift) & (2^bits - 1) of every element whose key image u has u >> match_shift == prefix
// (match_shift = 64: every element).  b == nullptr: single source.
constexpr int kSelectDigitBits = 11;   // 5 passes of 11 bits and one of 9 cover the 64-bit image
constexpr int kSelectBins = 1 << kSelectDigitBits;
constexpr int kSelectMaxBlocks = 2048;
struct SelectArgs {
  const float* a; const float* b;
  long long count;
  double w0, w1;
  unsigned long long prefix;
  int shift, bits, match_shift;
  unsigned long long* hist;
};
hipError_t launch_select_hist(const SelectArgs& s, hipStream_t st);
// dst = (float)min(src, clip) for count uint8 (src_bytes 1) or uint16 (2) values; clip < 0: none
hipError_t launch_widen(const void* src, int src_bytes, long long count, double clip, float* dst, hipStream_t st);

// LPIPS (AlexNet trunk, v0.1 heads), dsx_lpips.hip: fp32 NHWC, the two images of pair b are images b and B + b of a
// batch of nimg = 2 B.  Weights are packed by dsx_lpips.cpp: conv1 [N block 2][group 46][lane 64] float4 over
// k = (ky * 11 + kx) * 3 + c, conv2 .. conv5 [N block][chunk of 32 channels][tap][group 4][lane 64] float4; in both, row
// i of an N block is output channel 16 ((i >> 2) & 1) + (i & 3) + 4 (i >> 3) and component s of lane (i, h) is
// k = 8 group + 4 h + s.
struct LpipsTaps { long long off[5]; int nblk[5]; int hw[5]; };   // per tap: first partial row, rows per pair, pixels
hipError_t launch_lpips_input_nchw(const float* in0, const float* in1, int B, int H, int W, float* out, hipStream_t st);
hipError_t launch_lpips_input_frames(const float* tgt, const float* prd, int n, int H, int W, int C, int ch, const float* mm,
                                     float* out, hipStream_t st);
int lpips_minmax_blocks(long long pixels);
// min and max of channel `ch` of a channel-last stack -> mm[2]; part holds 2 * lpips_minmax_blocks(pixels) floats
hipError_t launch_lpips_minmax(const float* x, long long pixels, int C, int ch, float* part, float* mm, hipStream_t st);
hipError_t launch_lpips_conv1(const float* in, const float* wpack, const float* bias, float* out, int nimg, int H, int W, int Ho,
                              int Wo, hipStream_t st);
// stride 1, pad ks / 2, ks = 3 or 5, Cin % 32 == 0, Cout % 64 == 0, + bias + ReLU
hipError_t launch_lpips_conv(int ks, const float* in, const float* wpack, const float* bias, float* out, int nimg, int H, int W,
                             int Cin, int Cout, hipStream_t st);
hipError_t launch_lpips_pool(const float* in, float* out, int nimg, int H, int W, int Ho, int Wo, int C, hipStream_t st);
int lpips_dist_blocks(int HW);
// part[B][lpips_dist_blocks(HW)] doubles: sum over the block's pixels of sum_c lin[c] (f0 / |f0| - f1 / |f1|)^2
hipError_t launch_lpips_dist(const float* feat, int B, int HW, int C, const float* lin, double* part, hipStream_t st);
// out[b_off + b] = sum over taps of (partial rows added in order) / pixels; per_tap (may be NULL) [b_off + b][5]
hipError_t launch_lpips_finish(const double* part, const LpipsTaps& taps, int B, int b_off, float* out, float* per_tap,
                               hipStream_t st);

// PIL's 8-bit resampler (libImaging/Resample.c), dsx_resize.hip: one pass over a batch of uint8 images [B][rows][W][C]
// kept as rows of bytes.  Output sample i of the pass uses row t0 + i of the integer tables (xmin, n, k[ksize]) made by
// dsx_resize_coeffs; a workgroup takes S outputs and T units of the other axis and stages their coefficients and the
// source window (lds_pitch bytes per staged row) in LDS.
//   horizontal: n_out columns of n_other rows; src / dst point at the first row, src at byte 0 of it, dst at the first
//               byte written
//   vertical  : n_out rows of n_other bytes; src row 0 is source row `base` of the tables, src / dst point at the
//               first byte column
struct ResizePassArgs {
  const unsigned char* src; unsigned char* dst;
  const int *xmin, *n, *k;
  long long src_img, dst_img;      // bytes from one image to the next
  int src_pitch, dst_pitch;        // bytes per row
  int ksize, t0, C, n_out, n_other, base, S, T, lds_pitch, lds_bytes, B;
};
__host__ __device__ inline int resize_tab_bytes(int S, int ksize) { return (((S * ksize + 2 * S) * 4) + 15) & ~15; }
hipError_t launch_resize_h_u8(const ResizePassArgs& a, hipStream_t st);
hipError_t launch_resize_v_u8(const ResizePassArgs& a, hipStream_t st);
// ToTensor + min_max (data/util.py:74-83): [B][HW][C] uint8 -> [B][C][HW] fp32, (u / 255) * (hi - lo) + lo with every
// operation rounded on its own
hipError_t launch_u8_to_tensor(const unsigned char* src, int B, long long HW, int C, float lo, float hi, float* dst,
                               hipStream_t st);

// dsx_ops.hip.  relu(u) * sigmoid-mask reduction of the TimePredictor head
hipError_t launch_masked_mean(const float* u, const float* mask, int B, long long n, float* out,
                              hipStream_t st);

}  // namespace dsx
