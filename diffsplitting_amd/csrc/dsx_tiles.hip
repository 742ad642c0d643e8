// dsx_tiles.hip — the tile kernels of tiled prediction (gfx950), none of which runs inside a sampling step: gather
// (plain, normalised, colour planes, input-only stack, mixed, mixed per item), stitch with the RangeInvariantPsnr sums
// taken while pasting, and pack.  Their reductions: dsx_reduce.h.  The host side is dsx_tiles.cpp.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

// ---------------------------------------------------------------------------
// tiles: gather (N,H,W) frames -> (count, ph, pw); stitch valid regions of
// (count, C, ph, pw) predictions into the (N,H,W,C) canvas (tile_stitcher.py:26-80).
// The tiles of a launch are the arithmetic sequence  id = first + k * stride  (k = blockIdx.y): a rank's
// shard of a plan (or a batch of it) indexes the plan's device tables directly, nothing is uploaded per call.
// ---------------------------------------------------------------------------
// where tile k of the launch is cut: (frame, y, x) of its id in the geometry's table
struct TileOrigin { int n, y0, x0; };
__device__ __forceinline__ TileOrigin tile_origin(const TileGeom& g, long long k) {
  const long long t = g.seq.first + k * g.seq.stride;
  return TileOrigin{g.starts[t * 3], g.starts[t * 3 + 1], g.starts[t * 3 + 2]};
}
// where pixel i of a ph x pw patch cut at (y0, x0) is read: its element in frames whose rows of this frame (or colour
// plane) begin at row `rows`.  The one-dword-per-lane gathers stride over i, consecutive lanes consecutive x.
__device__ __forceinline__ size_t tile_src(const TileGeom& g, size_t rows, int y0, int x0, int i) {
  const int y = i / g.pw, x = i % g.pw;
  return (rows + (y0 + y)) * g.W + (x0 + x);
}
// workgroups along x of a launch that strides over `elems` elements per tile: one per 256, at most 64
static unsigned tile_grid_x(long long elems) {
  const long long gx = (elems + 255) / 256;
  return (unsigned)(gx > 64 ? 64 : gx);
}

__global__ void k_tiles_gather(const float* __restrict__ frames, int H, int W, int ph, int pw,
                               const int* __restrict__ starts, TileSeq seq, float* __restrict__ tiles) {
  const TileGeom g{H, W, ph, pw, starts, seq};
  const long long k = blockIdx.y;
  const TileOrigin o = tile_origin(g, k);
  const int total = ph * pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x)
    tiles[k * total + i] = frames[tile_src(g, (size_t)o.n * H, o.y0, o.x0, i)];
}
hipError_t launch_tiles_gather(const float* frames, const TileGeom& g, float* tiles, hipStream_t st) {
  hipLaunchKernelGGL(k_tiles_gather, dim3(tile_grid_x((long long)g.ph * g.pw), (unsigned)g.seq.count), dim3(256), 0, st,
                     frames, g.H, g.W, g.ph, g.pw, g.starts, g.seq, tiles);
  return hipGetLastError();
}

// tile crop + the dataset's normalisation in one pass (SplitDataset.__getitem__, data/split_dataset.py:237-278):
//   target_c = (frame_c - mean_target_c) / std_target_c                       (normalize_target, :199-201)
//   input    = w0 * target_0 + w1 * target_1                                   (input_from_normalized_target)
//            | ((w0 * frame_0 + w1 * frame_1) - mean_input) / std_input        (normalize_inp, :195-197)
// in double, rounded to fp32 once, exactly as numpy does with its float64 statistics.
struct GatherNormArgs {
  const float* f0; const float* f1;
  TileGeom g;
  float w0, w1;
  double mean_inp, std_inp, mt0, st0, mt1, st1;
  int from_norm_target;
  float* tin;              // (count, 1, ph, pw)
  float* ttar;             // (count, 2, ph, pw)
};
__global__ void k_tiles_gather_norm(const GatherNormArgs a) {
  const long long k = blockIdx.y;
  const TileOrigin o = tile_origin(a.g, k);
  const int total = a.g.ph * a.g.pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const size_t src = tile_src(a.g, (size_t)o.n * a.g.H, o.y0, o.x0, i);
    const float p0 = a.f0[src], p1 = a.f1[src];
    const float t0 = (float)(((double)p0 - a.mt0) / a.st0), t1 = (float)(((double)p1 - a.mt1) / a.st1);
    float in;
    if (a.from_norm_target) in = __fadd_rn(__fmul_rn(a.w0, t0), __fmul_rn(a.w1, t1));
    else in = (float)(((double)__fadd_rn(__fmul_rn(a.w0, p0), __fmul_rn(a.w1, p1)) - a.mean_inp) / a.std_inp);
    a.tin[k * total + i] = in;
    a.ttar[(k * 2) * total + i] = t0;
    a.ttar[(k * 2 + 1) * total + i] = t1;
  }
}
hipError_t launch_tiles_gather_norm(const float* f0, const float* f1, const TileGeom& g, float w0, float w1,
                                    const double norm[6], int from_norm_target, float* tin, float* ttar, hipStream_t st) {
  GatherNormArgs a{f0, f1, g, w0, w1, norm[0], norm[1], norm[2], norm[3], norm[4], norm[5], from_norm_target, tin, ttar};
  hipLaunchKernelGGL(k_tiles_gather_norm, dim3(tile_grid_x((long long)g.ph * g.pw), (unsigned)g.seq.count), dim3(256), 0, st, a);
  return hipGetLastError();
}

// The same item for frames with colour planes, (N, Cc, H, W) per stack (SplitDataset on data_type 'cifar10',
// data/split_dataset.py:248-272 with patch.ndim == 3): plane c of stack s is target channel s * Cc + c with its own
// statistics, the input keeps the Cc planes.  A streaming kernel: workgroup (x, c, k) owns a strided share of plane c of
// item k, so the plane and its four statistics are uniform in the workgroup and consecutive threads read and write
// consecutive x.  The arithmetic per element is k_tiles_gather_norm's without from_norm_target.
struct GatherPlanesArgs {
  const float* f0; const float* f1;
  int Cc;
  TileGeom g;              // starts = (frame, y, x)
  float w0, w1;
  double mean_inp, std_inp;
  double mt[2 * kPlanesMaxC], st[2 * kPlanesMaxC];
  float* tin;              // (count, Cc, ph, pw)
  float* ttar;             // (count, 2 Cc, ph, pw)
};
__global__ void k_tiles_gather_norm_planes(const GatherPlanesArgs a) {
  const long long k = blockIdx.z;
  const int c = blockIdx.y;
  const TileOrigin o = tile_origin(a.g, k);
  const int total = a.g.ph * a.g.pw;
  const double mt0 = a.mt[c], st0 = a.st[c], mt1 = a.mt[a.Cc + c], st1 = a.st[a.Cc + c];
  float* tin = a.tin + ((size_t)k * a.Cc + c) * total;
  float* tar0 = a.ttar + ((size_t)k * 2 * a.Cc + c) * total;
  float* tar1 = tar0 + (size_t)a.Cc * total;
  const size_t plane = ((size_t)o.n * a.Cc + c) * a.g.H;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const size_t src = tile_src(a.g, plane, o.y0, o.x0, i);
    const float p0 = a.f0[src], p1 = a.f1[src];
    tar0[i] = (float)(((double)p0 - mt0) / st0);
    tar1[i] = (float)(((double)p1 - mt1) / st1);
    tin[i] = (float)(((double)__fadd_rn(__fmul_rn(a.w0, p0), __fmul_rn(a.w1, p1)) - a.mean_inp) / a.std_inp);
  }
}
hipError_t launch_tiles_gather_norm_planes(const float* f0, const float* f1, int Cc, const TileGeom& g, float w0, float w1,
                                           double mean_inp, double std_inp, const double* mean_target,
                                           const double* std_target, float* tin, float* ttar, hipStream_t st) {
  if (Cc < 1 || Cc > kPlanesMaxC) return hipErrorInvalidValue;
  GatherPlanesArgs a{};
  a.f0 = f0; a.f1 = f1; a.Cc = Cc; a.g = g;
  a.w0 = w0; a.w1 = w1; a.mean_inp = mean_inp; a.std_inp = std_inp; a.tin = tin; a.ttar = ttar;
  for (int c = 0; c < 2 * Cc; ++c) { a.mt[c] = mean_target[c]; a.st[c] = std_target[c]; }
  hipLaunchKernelGGL(k_tiles_gather_norm_planes, dim3(tile_grid_x((long long)g.ph * g.pw), (unsigned)Cc, (unsigned)g.seq.count),
                     dim3(256), 0, st, a);
  return hipGetLastError();
}

// The network input of an INPUT-ONLY stack (data/input_stack.py): one (N, H, W) stack in which the two structures are
// already superimposed, resident in its file width (uint8 / uint16 / fp32), cut and normalised in one pass:
//   x = (float)pixel (exact);  x = min(x, clip) with a clip;  out = (float)(((double)x - mean_input) / std_input)
// -- the expression k_tiles_gather_norm applies to w0 * p0 + w1 * p1, so a stack that holds that sum gives its 'input'
// bit for bit.  A streaming kernel: a thread owns four consecutive pixels of one tile row (consecutive lanes,
// consecutive pixels; the grid grows with ph * pw, no workgroup cap), reads them with the widest loads their address
// allows and writes one 16-byte store.  The address of a group is aligned to 4, 2 or 1 pixels (x0, W and the row decide;
// it is the same for every group of a row, so a wave diverges between rows at most):
//   4: one load of four pixels      2: two loads of two      1: a scalar head, the aligned middle pair, a scalar tail
// VEC: pw % 4 == 0 and the output is 16-byte aligned.  Otherwise the last group of a row is ragged and the stores are
// scalar (the loads of the full groups stay wide).  Only pixels of the tile are ever read.
struct GatherInputArgs {
  const void* frames;      // (N, H, W) pixels of the kernel's type
  TileGeom g;
  double mean, std;
  float clip; int has_clip;
  float* out;              // (count, 1, ph, pw)
};
template <class T>
__device__ __forceinline__ void load_pixels4(const T* p, float v[4]) {
  typedef T V2 __attribute__((ext_vector_type(2)));
  typedef T V4 __attribute__((ext_vector_type(4)));
  const uintptr_t a = (uintptr_t)p;
  if ((a & (4 * sizeof(T) - 1)) == 0) {
    const V4 t = *(const V4*)p;
    v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
  } else if ((a & (2 * sizeof(T) - 1)) == 0) {
    const V2 t = *(const V2*)p, u = *(const V2*)(p + 2);
    v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)u.x; v[3] = (float)u.y;
  } else {                                     // p is an odd pixel address: p + 1 is a pair boundary
    const T head = p[0], tail = p[3];
    const V2 t = *(const V2*)(p + 1);
    v[0] = (float)head; v[1] = (float)t.x; v[2] = (float)t.y; v[3] = (float)tail;
  }
}
// uint8: the same three cases on integer words (a vector of four bytes is split into two 16-bit loads by the compiler)
template <>
__device__ __forceinline__ void load_pixels4<unsigned char>(const unsigned char* p, float v[4]) {
  const uintptr_t a = (uintptr_t)p;
  unsigned w;
  if ((a & 3) == 0) w = *(const unsigned*)p;
  else if ((a & 1) == 0) w = (unsigned)*(const unsigned short*)p | ((unsigned)*(const unsigned short*)(p + 2) << 16);
  else w = (unsigned)p[0] | ((unsigned)*(const unsigned short*)(p + 1) << 8) | ((unsigned)p[3] << 24);
  v[0] = (float)(w & 255u); v[1] = (float)((w >> 8) & 255u); v[2] = (float)((w >> 16) & 255u); v[3] = (float)(w >> 24);
}
template <class T, bool VEC>
__global__ __launch_bounds__(256) void k_tiles_gather_input(const GatherInputArgs a) {
  const long long k = blockIdx.y;
  const TileOrigin o = tile_origin(a.g, k);
  const int gpr = (a.g.pw + 3) >> 2;           // groups per tile row
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)a.g.ph * gpr) return;
  const int y = (int)(g / gpr), x = (int)(g - (long long)y * gpr) * 4;
  const int cnt = VEC ? 4 : min(4, a.g.pw - x);
  const T* src = (const T*)a.frames + ((size_t)o.n * a.g.H + (o.y0 + y)) * a.g.W + (o.x0 + x);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (cnt == 4) load_pixels4(src, v);
  else DSX_EACH4(j, cnt) v[j] = (float)src[j];
  DSX_EACH4(j, cnt) {
    const float px = a.has_clip ? fminf(v[j], a.clip) : v[j];
    v[j] = (float)(((double)px - a.mean) / a.std);
  }
  float* dst = a.out + (size_t)k * a.g.ph * a.g.pw + (size_t)y * a.g.pw + x;
  if (VEC) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
  else DSX_EACH4(j, cnt) dst[j] = v[j];
}
template <class T>
static hipError_t launch_gather_input_as(const GatherInputArgs& a, hipStream_t st) {
  const bool vec = (a.g.pw & 3) == 0 && aligned16(a.out);
  const long long groups = (long long)a.g.ph * ((a.g.pw + 3) >> 2);
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)a.g.seq.count);
  if (vec) hipLaunchKernelGGL((k_tiles_gather_input<T, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_tiles_gather_input<T, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_tiles_gather_input(const void* frames, int pix_bytes, bool is_float, const TileGeom& g, double mean,
                                     double std, double clip, float* out, hipStream_t st) {
  const GatherInputArgs a{frames, g, mean, std, (float)clip, clip >= 0 ? 1 : 0, out};
  if (is_float && pix_bytes == 4) return launch_gather_input_as<float>(a, st);
  if (!is_float && pix_bytes == 2) return launch_gather_input_as<unsigned short>(a, st);
  if (!is_float && pix_bytes == 1) return launch_gather_input_as<unsigned char>(a, st);
  return hipErrorInvalidValue;
}

// Frame-keyed noise for tiled prediction (include/dsx.h, dsx_tileplan_randn): the noise field (seed, id, draw) of a
// (C, H, W) frame is the sample stream (seed, (id << 24) | draw) read as that tensor -- element (c, y, x) is stream
// element j = (c*H + y)*W + x, component j % 4 of normal4(seed, subseq, j / 4), what k_randn_samples writes -- and tile k
// of the launch, cut at (n, y0, x0), receives field(seed, id_base + n, draw)[c, y0 + yy, x0 + xx].  Two tiles of a frame
// therefore hold the same bits wherever they overlap.  Tile k is blockIdx.y, as in every tile kernel; grid-stride over the
// groups of the tile: a thread owns four consecutive x of one row of one channel plane (consecutive lanes, consecutive
// groups; 32-bit index arithmetic, the origin and the subsequence are uniform in the workgroup).  r = j0 & 3 of the
// group's first element is the same for every group of a tile row (x advances by 4), so a wave diverges between rows
// at most:
//   r == 0: the group is one Philox block, one normal4
//   r != 0: it straddles two blocks: components r..3 of the first and 0..r-1 of the second, two normal4 (a ragged last
//           group that ends inside the first block takes only that one)
// VEC: pw % 4 == 0 and `out` is 16-byte aligned: one 16-byte store per group; otherwise scalar stores over the group's
// first cnt elements.  No LDS, no atomics.
template <bool VEC>
__global__ __launch_bounds__(256) void k_tiles_randn(float* __restrict__ out, int C, int H, int W, int ph, int pw,
                                                      const int* __restrict__ starts, TileSeq seq, unsigned long long seed,
                                                      unsigned long long id_base, unsigned draw) {
  const TileGeom g{H, W, ph, pw, starts, seq};
  const long long k = blockIdx.y;
  const TileOrigin o = tile_origin(g, k);
  const unsigned long long subseq = ((id_base + (unsigned long long)o.n) << 24) | draw;
  const int gpr = (pw + 3) >> 2;                                   // groups per tile row
  const int groups = C * ph * gpr;                                 // <= C * ph * pw, which fits 32 bits (checked on the host)
  float* __restrict__ tile = out + (size_t)k * C * ph * pw;
  for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < groups; q += gridDim.x * blockDim.x) {
    const int row = q / gpr, x = (q - row * gpr) * 4;              // row = c * ph + yy
    const int c = row / ph, yy = row - c * ph;
    const unsigned long long j0 = ((unsigned long long)c * H + (o.y0 + yy)) * W + (o.x0 + x);
    const int r = (int)(j0 & 3), cnt = VEC ? 4 : min(4, pw - x);
    float a[4], b[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
    normal4(seed, subseq, j0 >> 2, a);
    if (r + cnt > 4) normal4(seed, subseq, (j0 >> 2) + 1, b);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr)                                 // constant indices: the blocks stay in registers
      if (r == rr) DSX_EACH4(j, 4) v[j] = rr + j < 4 ? a[rr + j] : b[rr + j - 4];
    float* dst = tile + (size_t)row * pw + x;
    if (VEC) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    else DSX_EACH4(j, cnt) dst[j] = v[j];
  }
}
hipError_t launch_tiles_randn(const TileGeom& g, int C, unsigned long long seed, unsigned long long id_base, unsigned draw,
                              float* out, hipStream_t st) {
  const bool vec = (g.pw & 3) == 0 && aligned16(out);
  const long long groups = (long long)C * g.ph * ((g.pw + 3) >> 2);
  hipLaunchKernelGGL(vec ? k_tiles_randn<true> : k_tiles_randn<false>, dim3(grid_for(groups), (unsigned)g.seq.count), dim3(256),
                     0, st, out, C, g.H, g.W, g.ph, g.pw, g.starts, g.seq, seed, id_base, draw);
  return hipGetLastError();
}

// (mul_f / add_f / mul_d / add_d, one IEEE operation each, live in dsx_kernels.h)
// The mixed inputs of the TimePredictor evaluation (notebooks/EvaluateJointIndiIterative.ipynb cells 40/43,
// time_prediction_evaluation.ipynb cell 4) cut, normalised, mixed and min-max-normalised in one pass; the op list is
// in include/dsx.h (dsx_tiles_gather_mix).  Channel 0 is indi1's input, channel 1 indi2's.
struct GatherMixArgs {
  const float* f0; const float* f1;
  TileGeom g;
  double mt0, st0, mt1, st1;
  MixWeights mw;
  float* ttar; float* tmix; float* tcls;   // (count, 2, ph, pw) each, or nullptr
};
// item k of a launch, cut at (n, y0, x0) with the weights w: the one body of both mixed gathers, so that an item of
// k_tiles_gather_mix_items is bitwise the item k_tiles_gather_mix writes for the same location, t and table rows
__device__ __forceinline__ void mix_item(const GatherMixArgs& a, long long k, int n, int y0, int x0, const MixWeights w) {
  const int total = a.g.ph * a.g.pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const size_t src = tile_src(a.g, (size_t)n * a.g.H, y0, x0, i);
    const float t0 = (float)(((double)a.f0[src] - a.mt0) / a.st0), t1 = (float)(((double)a.f1[src] - a.mt1) / a.st1);
    const size_t d0 = (size_t)(k * 2) * total + i, d1 = d0 + total;
    if (a.ttar) { a.ttar[d0] = t0; a.ttar[d1] = t1; }
    if (a.tmix || a.tcls) {
      const float m0 = add_f(mul_f(t0, w.w0), mul_f(t1, w.w1));
      const float m1 = add_f(mul_f(t1, w.w0), mul_f(t0, w.w1));
      if (a.tmix) { a.tmix[d0] = m0; a.tmix[d1] = m1; }
      if (a.tcls) {
        a.tcls[d0] = add_f(mul_f(2.0f, add_f(m0, -w.lo0)) / w.rng0, -1.0f);
        a.tcls[d1] = add_f(mul_f(2.0f, add_f(m1, -w.lo1)) / w.rng1, -1.0f);
      }
    }
  }
}
__global__ void k_tiles_gather_mix(const GatherMixArgs a) {
  const long long k = blockIdx.y;
  const TileOrigin o = tile_origin(a.g, k);
  mix_item(a, k, o.n, o.y0, o.x0, a.mw);
}
// the same with one (location, weights) record per item: a batch whose items each carry their own t and table rows
// (TimePredictorDataset.batch).  The record is uniform in the workgroup (indexed by blockIdx.y); pixels are read and
// written one dword per lane, consecutive lanes consecutive x: patch starts are arbitrary and ph * pw need not be a
// multiple of 4, so neither the source rows nor the items of the outputs are 16-byte aligned in general.
__global__ void k_tiles_gather_mix_items(const GatherMixArgs a, const MixItem* __restrict__ items) {
  const long long k = blockIdx.y;
  const MixItem it = items[k];
  mix_item(a, k, it.n, it.y, it.x, it.w);
}
hipError_t launch_tiles_gather_mix_items(const float* f0, const float* f1, const TileGeom& g, const MixItem* items,
                                         const double norm[4], float* ttar, float* tmix, float* tcls, hipStream_t st) {
  GatherMixArgs a{f0, f1, g, norm[0], norm[1], norm[2], norm[3], MixWeights{}, ttar, tmix, tcls};
  hipLaunchKernelGGL(k_tiles_gather_mix_items, dim3(tile_grid_x((long long)g.ph * g.pw), (unsigned)g.seq.count), dim3(256), 0,
                     st, a, items);
  return hipGetLastError();
}
hipError_t launch_tiles_gather_mix(const float* f0, const float* f1, const TileGeom& g, const double norm[4],
                                   const MixWeights& mw, float* ttar, float* tmix, float* tcls, hipStream_t st) {
  GatherMixArgs a{f0, f1, g, norm[0], norm[1], norm[2], norm[3], mw, ttar, tmix, tcls};
  hipLaunchKernelGGL(k_tiles_gather_mix, dim3(tile_grid_x((long long)g.ph * g.pw), (unsigned)g.seq.count), dim3(256), 0, st, a);
  return hipGetLastError();
}

// Where the pixels of tile `t` (the k-th of the launch) come from: whole predicted tiles (count, C, ph, pw), or the
// packed exchange buffer of tiled multi-GPU prediction -- per rank one flat run of valid regions [C][h][w], tile after
// tile in id order (rank q owns the ids q, q + world, ...); `off` = pixel offset of every tile inside its rank's run.
struct TileSrc {
  const float* base;       // tiles, or the gathered flat buffer [world][rank_stride]
  int packed;              // 0: whole tiles, 1: packed valid regions
  int ph, pw;              // whole tiles
  const long long* off;    // packed: dev [total] pixel offsets
  long long rank_stride;   // packed: elements between two ranks' runs
  int world;
};
struct TileView { const float* p; int pitch; long long plane; };
__device__ __forceinline__ TileView tile_view(const TileSrc& s, long long k, long long t, int C, const int* r) {
  TileView v;
  if (s.packed) {
    v.p = s.base + (t % s.world) * s.rank_stride + s.off[t] * C;
    v.pitch = r[4]; v.plane = (long long)r[3] * r[4];
  } else {
    v.p = s.base + (size_t)k * C * s.ph * s.pw + (size_t)r[5] * s.pw + r[6];
    v.pitch = s.pw; v.plane = (long long)s.ph * s.pw;
  }
  return v;
}

__global__ void k_stitch(const TileSrc src, int C, const int* __restrict__ regions, TileSeq seq,
                         float* __restrict__ canvas, int H, int W) {
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int* r = regions + t * 8;
  const int n = r[0], y0 = r[1], x0 = r[2], h = r[3], w = r[4];
  const int total = h * w * C;
  const TileView v = tile_view(src, k, t, C, r);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i % C;
    const int p = i / C;
    const int x = p % w, y = p / w;
    canvas[(((size_t)n * H + (y0 + y)) * W + (x0 + x)) * C + c] = v.p[c * v.plane + (size_t)y * v.pitch + x];
  }
}

// The valid region of every tile of the sequence, [C][h][w], to its place in this rank's flat run: the crop of
// tile_stitcher.py:38-56 applied BEFORE the collective (a 512^2 tile of a 256 grid ships 256^2 .. 384^2 pixels).
__global__ void k_tiles_pack(const float* __restrict__ tiles, int C, int ph, int pw, const int* __restrict__ regions,
                             const long long* __restrict__ off, TileSeq seq, float* __restrict__ flat) {
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int* r = regions + t * 8;
  const int h = r[3], w = r[4], ry = r[5], rx = r[6];
  const int total = C * h * w;
  const float* tile = tiles + (size_t)k * C * ph * pw;
  float* dst = flat + off[t] * C;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int x = i % w, q = i / w, y = q % h, c = q / h;
    dst[i] = tile[((size_t)c * ph + (ry + y)) * pw + (rx + x)];
  }
}
hipError_t launch_tiles_pack(const float* tiles, int C, int ph, int pw, const int* regions, const long long* off,
                             TileSeq seq, float* flat, hipStream_t st) {
  hipLaunchKernelGGL(k_tiles_pack, dim3(tile_grid_x((long long)ph * pw * C), (unsigned)seq.count), dim3(256), 0, st, tiles,
                     C, ph, pw, regions, off, seq, flat);
  return hipGetLastError();
}

// Stitch + the sums RangeInvariantPsnr needs (core/psnr.py:70-82), in the same pass: while a tile's valid region
// is pasted, every (tile, workgroup) also reduces, per channel, sum(p), sum(p^2), sum(g), sum(g^2), sum(g p),
// min(g), max(g) of prediction p against the ground truth g at the same canvas pixels (every canvas pixel is pasted
// exactly once).  Fixed reduction order (thread -> wave shuffles -> 4 waves): bitwise reproducible.
// part[k][blockIdx.x][c][8] doubles (PsnrSums, dsx_reduce.h); the per-frame combination (a few hundred values) is the
// caller's.
__global__ __launch_bounds__(256) void k_stitch_psnr(const TileSrc src, int C, const int* __restrict__ regions, TileSeq seq,
                                                      float* __restrict__ canvas, const float* __restrict__ gt, int H, int W,
                                                      double* __restrict__ part) {
  __shared__ double red[kPsnrRed];
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int* r = regions + t * 8;
  const int n = r[0], y0 = r[1], x0 = r[2], h = r[3], w = r[4];
  const TileView v = tile_view(src, k, t, C, r);
  PsnrSums acc[kPsnrMaxC];
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < h * w; i += gridDim.x * blockDim.x) {
    const int x = i % w, y = i / w;
    const size_t cpix = (((size_t)n * H + (y0 + y)) * W + (x0 + x)) * C;
#pragma unroll
    for (int c = 0; c < kPsnrMaxC; ++c) {
      if (c < C) {
        const float p = v.p[c * v.plane + (size_t)y * v.pitch + x];
        const float g = gt[cpix + c];
        canvas[cpix + c] = p;
        acc[c].add(p, g);
      }
    }
  }
  psnr_sums_write(acc, C, red, part + ((size_t)k * gridDim.x + blockIdx.x) * C * 8);
}
// gt == nullptr: plain paste; else also the RangeInvariantPsnr partial sums (C <= kPsnrMaxC, gx workgroups per tile)
hipError_t launch_stitch(const StitchSrc& s, int C, const int* regions, TileSeq seq, float* canvas, int H, int W,
                         const float* gt, double* part, int gx, hipStream_t st) {
  const TileSrc src{s.base, s.packed, s.ph, s.pw, s.off, s.rank_stride, s.world < 1 ? 1 : s.world};
  if (gt != nullptr) {
    if (C < 1 || C > kPsnrMaxC || gx < 1 || part == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stitch_psnr, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, src, C, regions, seq,
                       canvas, gt, H, W, part);
  } else {
    hipLaunchKernelGGL(k_stitch, dim3(tile_grid_x((long long)s.ph * s.pw * C), (unsigned)seq.count), dim3(256), 0, st, src,
                       C, regions, seq, canvas, H, W);
  }
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Blended stitching (include/dsx.h, dsx_tileplan_blend): the overlap-add of all tiles of a plan as a GATHER.  A thread
// owns canvas pixels and loops over the tiles that cover them, in ascending tile id; nothing is accumulated across
// threads or launches, so the canvas is a function of the tiles alone.  Per pixel and channel, every operation rounded
// on its own:
//   one contributor: out = v (a copy)      else: num = num + w * v, den = den + w with w = wy[yy] * wx[xx]; out = num / den
// Workgroup (sx, sy, n) owns the 256 pixels from x = 256 * sx of the rows y = sy, sy + gridDim.y, ... of frame n.  A
// thread keeps its x: the tile columns that cover it, its offset xx into each and wx[xx] are read once, before the
// rows (the first four columns stay in registers; a plan with more than four per pixel reads the rest per row).  The
// contributing tile rows, yy and wy[yy] are uniform in the workgroup.  The contributors are the outer loops and the
// channels the inner one, so a tile's address and weight are formed once for its C values; den is the same sum for
// every channel.  Consecutive lanes read consecutive x of a tile row, one dword each (a shifted tile's rows are not
// 16-byte aligned).  The C values of a pixel are contiguous in the canvas: WIDE writes them as one 8- / 16-byte store
// (C = 2 / 4 and the canvas aligned to it), otherwise one dword per channel.  CT = C for C <= 4; CT = 0 is any C, one
// channel after the other.  PSNR: the seven RangeInvariantPsnr sums of k_stitch_psnr per (frame, workgroup, channel),
// through the same fixed-order block reduction (C <= kPsnrMaxC).  No LDS beyond those slots, no atomics.
// STEP (include/dsx.h, dsx_tileplan_blend_step): the canvas is a frame state X, updated in place by the thread that
// owns the pixel -- read once, written once -- with the blended value v as the x0 of one reverse step without an eps
// form (step_update, dsx_kernels.h):  mean = c_x0*v + c_xt*X;  out = sigma != 0 ? mean + z*sigma : mean,  z = element
// j = (c*H + y)*W + x of the stream (seed, ((id_base + n) << 24) | draw): the frame's noise field, what k_randn_samples
// writes and k_tiles_randn crops.  The canvas is NHWC and the field CHW, so the C values of a pixel lie in C different
// Philox blocks and the four elements of a block in four neighbouring lanes: every lane computes the block of its
// element and keeps its component (normal1: one log and one sincos, not two).  Nothing is drawn where sigma == 0.
// ---------------------------------------------------------------------------
constexpr int kBlendCols = 4;                  // tile columns of a pixel kept in registers
template <class Args>                          // BlendArgs or DisagreeArgs: the two layouts of whole tiles
__device__ __forceinline__ const float* blend_tile(const Args& a, unsigned t, unsigned tile_elems) {
  return a.world == 1 ? a.tiles + (size_t)t * tile_elems
                      : a.tiles + (size_t)(t % (unsigned)a.world) * a.rank_stride + (size_t)(t / (unsigned)a.world) * tile_elems;
}
// any C: channel c of the pixel, the contributors in the same order
__device__ __forceinline__ float blend_pixel(const BlendArgs& a, unsigned tile0, int ty0, int tyn, int tx0, int txn, int c,
                                             int y, int x) {
  const int plane = a.ph * a.pw;
  float num = 0.f, den = 0.f, v = 0.f;
  for (int iy = ty0; iy < ty0 + tyn; ++iy)
    for (int ix = tx0; ix < tx0 + txn; ++ix) {
      const unsigned t = tile0 + (unsigned)iy * a.nx + ix;
      const int yy = y - a.starts[(size_t)t * 3 + 1], xx = x - a.starts[(size_t)t * 3 + 2];
      v = blend_tile(a, t, (unsigned)plane * a.C)[c * plane + yy * a.pw + xx];
      const float w = mul_f(a.wy[yy], a.wx[xx]);
      num = add_f(num, mul_f(w, v));
      den = add_f(den, w);
    }
  return tyn * txn == 1 ? v : __fdiv_rn(num, den);
}
template <int CT>
__device__ __forceinline__ void blend_add(const BlendArgs& a, unsigned t, int plane, int off, float w, float v[CT], float num[CT],
                                          float& den) {
  const float* p = blend_tile(a, t, (unsigned)plane * CT) + off;
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    v[c] = p[c * plane];
    num[c] = add_f(num[c], mul_f(w, v[c]));
  }
  den = add_f(den, w);
}
// STEP: channel c of pixel (y, x) of a frame whose field is the stream `subseq`: blended value v and state xs -> new state
__device__ __forceinline__ float blend_step(const BlendArgs& a, unsigned long long subseq, int c, int y, int x, float v,
                                            float xs) {
  const bool use_z = a.sigma != 0.f;
  float z = 0.f;
  if (use_z) {
    const unsigned long long j = ((unsigned long long)c * a.H + y) * a.W + x;
    z = normal1(a.seed, subseq, j >> 2, (int)(j & 3));
  }
  return step_update(0.f, 0.f, a.c_x0, a.c_xt, 0.f, a.sigma, false, false, xs, v, 0.f, z, use_z).out;
}
template <int CT, bool WIDE, bool PSNR, bool STEP>
__global__ __launch_bounds__(256) void k_blend(const BlendArgs a) {
  constexpr int NC = CT > 0 ? CT : 1;
  __shared__ double red[PSNR ? kPsnrRed : 1];
  const int n = blockIdx.z, x = blockIdx.x * 256 + threadIdx.x;
  const bool live = x < a.W;
  const unsigned tile0 = (unsigned)n * a.ny * a.nx;
  const int plane = a.ph * a.pw;
  const unsigned long long subseq = ((a.id_base + (unsigned long long)n) << 24) | a.draw;   // STEP: the frame's field
  int tx0 = 0, txn = 0, xo[kBlendCols];
  float wxc[kBlendCols];
  if (live) { tx0 = a.cols[2 * x]; txn = a.cols[2 * x + 1]; }
#pragma unroll
  for (int j = 0; j < kBlendCols; ++j) {       // tile (0, ix) of frame 0 starts at the x every tile of column ix starts at
    xo[j] = 0; wxc[j] = 0.f;
    if (CT > 0 && j < txn) { xo[j] = x - a.starts[(size_t)(tx0 + j) * 3 + 2]; wxc[j] = a.wx[xo[j]]; }
  }
  PsnrSums acc[kPsnrMaxC];
  for (int y = blockIdx.y; y < a.H; y += gridDim.y) {
    if (!live) continue;
    const int ty0 = a.rows[2 * y], tyn = a.rows[2 * y + 1];
    const size_t cpix = (((size_t)n * a.H + y) * a.W + x) * a.C;
    if (CT == 0) {
      for (int c = 0; c < a.C; ++c) {
        const float v = blend_pixel(a, tile0, ty0, tyn, tx0, txn, c, y, x);
        a.canvas[cpix + c] = STEP ? blend_step(a, subseq, c, y, x, v, a.canvas[cpix + c]) : v;
      }
      continue;
    }
    float num[NC], v[NC], xs[NC], den = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) num[c] = v[c] = xs[c] = 0.f;
    if (STEP) {                                  // the state's C values, read as they are written below; asked for before
      if (WIDE && NC == 2) {                     // the tiles, so that the load is in flight under theirs
        const float2 t = *(const float2*)(a.canvas + cpix);
        xs[0] = t.x; xs[NC > 1 ? 1 : 0] = t.y;
      } else if (WIDE && NC == 4) {
        const float4 t = *(const float4*)(a.canvas + cpix);
        xs[0] = t.x; xs[NC > 1 ? 1 : 0] = t.y; xs[NC > 2 ? 2 : 0] = t.z; xs[NC > 3 ? 3 : 0] = t.w;
      } else {
#pragma unroll
        for (int c = 0; c < NC; ++c) xs[c] = a.canvas[cpix + c];
      }
    }
    for (int iy = ty0; iy < ty0 + tyn; ++iy) {
      const unsigned trow = tile0 + (unsigned)iy * a.nx;       // tile (iy, 0): every tile of row iy starts at its y
      const int yy = y - a.starts[(size_t)trow * 3 + 1];
      const float wyv = a.wy[yy];
#pragma unroll
      for (int j = 0; j < kBlendCols; ++j)
        if (j < txn) blend_add<NC>(a, trow + tx0 + j, plane, yy * a.pw + xo[j], mul_f(wyv, wxc[j]), v, num, den);
      for (int j = kBlendCols; j < txn; ++j) {
        const int xx = x - a.starts[(size_t)(tx0 + j) * 3 + 2];
        blend_add<NC>(a, trow + tx0 + j, plane, yy * a.pw + xx, mul_f(wyv, a.wx[xx]), v, num, den);
      }
    }
    float o[NC];
    const bool one = tyn * txn == 1;
#pragma unroll
    for (int c = 0; c < NC; ++c) o[c] = one ? v[c] : __fdiv_rn(num[c], den);
    if (STEP) {
#pragma unroll
      for (int c = 0; c < NC; ++c) o[c] = blend_step(a, subseq, c, y, x, o[c], xs[c]);
    }
    if (WIDE && NC == 2) *(float2*)(a.canvas + cpix) = make_float2(o[0], o[NC > 1 ? 1 : 0]);
    else if (WIDE && NC == 4) *(float4*)(a.canvas + cpix) = make_float4(o[0], o[NC > 1 ? 1 : 0], o[NC > 2 ? 2 : 0], o[NC > 3 ? 3 : 0]);
    else {
#pragma unroll
      for (int c = 0; c < NC; ++c) a.canvas[cpix + c] = o[c];
    }
    if (PSNR) {
#pragma unroll
      for (int c = 0; c < NC && c < kPsnrMaxC; ++c) acc[c].add(o[c], a.gt[cpix + c]);
    }
  }
  if (PSNR) {
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x, blocks = (size_t)gridDim.x * gridDim.y;
    psnr_sums_write(acc, a.C, red, a.part + ((size_t)n * blocks + b) * a.C * 8);
  }
}
template <int CT, bool WIDE>
static void launch_blend_as(const BlendArgs& a, const dim3 grid, hipStream_t st) {
  if (a.step) hipLaunchKernelGGL((k_blend<CT, WIDE, false, true>), grid, dim3(256), 0, st, a);
  else if (a.gt != nullptr) hipLaunchKernelGGL((k_blend<CT, WIDE, true, false>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_blend<CT, WIDE, false, false>), grid, dim3(256), 0, st, a);
}
hipError_t launch_blend(const BlendArgs& a, hipStream_t st) {
  if (a.gt != nullptr && (a.C < 1 || a.C > kPsnrMaxC || a.part == nullptr)) return hipErrorInvalidValue;
  if (a.step && a.gt != nullptr) return hipErrorInvalidValue;          // a step takes no PSNR sums
  if (a.N < 1 || a.N > 65535 || a.C < 1) return hipErrorInvalidValue;
  const BlendGrid bg = blend_grid(a.H, a.W);
  const dim3 grid((unsigned)bg.segs, (unsigned)bg.rows, (unsigned)a.N);
  const uintptr_t at = (uintptr_t)a.canvas;
  if (a.C == 1) launch_blend_as<1, false>(a, grid, st);
  else if (a.C == 2 && (at & 7u) == 0) launch_blend_as<2, true>(a, grid, st);
  else if (a.C == 2) launch_blend_as<2, false>(a, grid, st);
  else if (a.C == 3) launch_blend_as<3, false>(a, grid, st);
  else if (a.C == 4 && (at & 15u) == 0) launch_blend_as<4, true>(a, grid, st);
  else if (a.C == 4) launch_blend_as<4, false>(a, grid, st);
  else if (a.step) hipLaunchKernelGGL((k_blend<0, false, false, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_blend<0, false, false, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Tile disagreement (include/dsx.h, dsx_tileplan_disagreement): the sibling of the blend that reports how far the
// contributors of a canvas pixel differ instead of averaging them.  The geometry is k_blend's: workgroup (sx, sy, n)
// owns the 256 pixels from x = 256 * sx of the rows y = sy, sy + gridDim.y, ...; a thread keeps its x, the tile columns
// that cover it (the first kBlendCols offsets in registers) and whether its column is near a crop line; the tile rows
// and the row's near-line flag are uniform in the workgroup.  One dword per tile row and lane.  Per pixel and channel
// Welford's recurrence over the contributors in ascending tile id, in double, every operation rounded on its own (the
// update of k_moments_update); var = M2 / (k - 1), s = (float)sqrt(var).  MAP: s goes to map (N,H,W,C), WIDE as one 8- /
// 16-byte store for C = 2 / 4.  Every thread keeps, per channel, sum and min / max of var over its pixels with k >= 2
// and the sum over those in the band, and once the two pixel counts (they are the same for every channel); the rows go
// through RedRow<4, 1>: row[c][8] = {count, sum var, band count, band sum var, min var, max var, 0, 0}.  No atomics.
// ---------------------------------------------------------------------------
using DisRow = RedRow<4, 1>;
constexpr int kDisRed = 4 * kPsnrMaxC * DisRow::kSlots;           // doubles of LDS, [wave][channel][slot]
template <int CT>
__device__ __forceinline__ void disagree_add(const DisagreeArgs& a, unsigned t, int plane, int off, int r, double mean[CT],
                                             double m2[CT]) {
  const float* p = blend_tile(a, t, (unsigned)plane * CT) + off;
  const double rn = (double)(r + 1);
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const double v = (double)p[c * plane];
    if (r == 0) { mean[c] = v; m2[c] = 0.0; continue; }
    const double d = sub_d(v, mean[c]);
    const double m1 = add_d(mean[c], d / rn);
    m2[c] = add_d(m2[c], mul_d(d, sub_d(v, m1)));
    mean[c] = m1;
  }
}
template <int CT, bool WIDE, bool MAP>
__global__ __launch_bounds__(256) void k_tile_disagreement(const DisagreeArgs a) {
  constexpr int kS = DisRow::kSlots;
  __shared__ double red[kDisRed];
  const int n = blockIdx.z, x = blockIdx.x * 256 + threadIdx.x;
  const bool live = x < a.W;
  const unsigned tile0 = (unsigned)n * a.ny * a.nx;
  const int plane = a.ph * a.pw;
  int tx0 = 0, txn = 0, xo[kBlendCols];
  bool near_x = false;
  if (live) { tx0 = a.cols[2 * x]; txn = a.cols[2 * x + 1]; near_x = a.near_x[x] != 0; }
#pragma unroll
  for (int j = 0; j < kBlendCols; ++j) xo[j] = j < txn ? x - a.starts[(size_t)(tx0 + j) * 3 + 2] : 0;
  double cnt = 0.0, cnt_band = 0.0, sum[CT], sum_band[CT], mn[CT], mx[CT];
#pragma unroll
  for (int c = 0; c < CT; ++c) { sum[c] = sum_band[c] = 0.0; mn[c] = INFINITY; mx[c] = -INFINITY; }
  for (int y = blockIdx.y; y < a.H; y += gridDim.y) {
    if (!live) continue;
    const int ty0 = a.rows[2 * y], tyn = a.rows[2 * y + 1];
    const int k = tyn * txn;
    const bool band = k >= 2 && (near_x || a.near_y[y] != 0);
    double mean[CT], m2[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) mean[c] = m2[c] = 0.0;
    int r = 0;
    for (int iy = ty0; iy < ty0 + tyn; ++iy) {
      const unsigned trow = tile0 + (unsigned)iy * a.nx;       // tile (iy, 0): every tile of row iy starts at its y
      const int yy = y - a.starts[(size_t)trow * 3 + 1];
#pragma unroll
      for (int j = 0; j < kBlendCols; ++j)
        if (j < txn) disagree_add<CT>(a, trow + tx0 + j, plane, yy * a.pw + xo[j], r++, mean, m2);
      for (int j = kBlendCols; j < txn; ++j) {
        const int xx = x - a.starts[(size_t)(tx0 + j) * 3 + 2];
        disagree_add<CT>(a, trow + tx0 + j, plane, yy * a.pw + xx, r++, mean, m2);
      }
    }
    float s[CT];
    const double km1 = (double)(k - 1);
#pragma unroll
    for (int c = 0; c < CT; ++c) {
      const double var = k > 1 ? m2[c] / km1 : 0.0;
      s[c] = (float)sqrt(var);
      if (k > 1) {
        sum[c] += var; mn[c] = fmin(mn[c], var); mx[c] = fmax(mx[c], var);
        if (band) sum_band[c] += var;
      }
    }
    if (k > 1) { cnt += 1.0; if (band) cnt_band += 1.0; }
    if (MAP) {
      float* dst = a.map + (((size_t)n * a.H + y) * a.W + x) * CT;
      if (WIDE && CT == 2) *(float2*)dst = make_float2(s[0], s[CT > 1 ? 1 : 0]);
      else if (WIDE && CT == 4) *(float4*)dst = make_float4(s[0], s[CT > 1 ? 1 : 0], s[CT > 2 ? 2 : 0], s[CT > 3 ? 3 : 0]);
      else {
#pragma unroll
        for (int c = 0; c < CT; ++c) dst[c] = s[c];
      }
    }
  }
#pragma unroll
  for (int c = 0; c < CT; ++c) {
    const double v[kS] = {cnt, sum[c], cnt_band, sum_band[c], mn[c], mx[c]};
    DisRow::park(v, red, kPsnrMaxC * kS, c * kS);
  }
  __syncthreads();
  if (threadIdx.x < CT * 8) {
    const int c = threadIdx.x >> 3, j = threadIdx.x & 7;
    const size_t b = (size_t)blockIdx.y * gridDim.x + blockIdx.x, blocks = (size_t)gridDim.x * gridDim.y;
    a.part[(((size_t)n * blocks + b) * CT + c) * 8 + j] = j < kS ? DisRow::combine(red, j, kPsnrMaxC * kS, c * kS) : 0.0;
  }
}
template <int CT, bool WIDE>
static void launch_disagreement_as(const DisagreeArgs& a, const dim3 grid, hipStream_t st) {
  if (a.map != nullptr) hipLaunchKernelGGL((k_tile_disagreement<CT, WIDE, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_tile_disagreement<CT, false, false>), grid, dim3(256), 0, st, a);
}
hipError_t launch_disagreement(const DisagreeArgs& a, hipStream_t st) {
  if (a.N < 1 || a.N > 65535 || a.C < 1 || a.C > kPsnrMaxC || a.part == nullptr) return hipErrorInvalidValue;
  const BlendGrid bg = blend_grid(a.H, a.W);
  const dim3 grid((unsigned)bg.segs, (unsigned)bg.rows, (unsigned)a.N);
  const uintptr_t at = (uintptr_t)a.map;                       // a null map is aligned: its form has no stores
  if (a.C == 1) launch_disagreement_as<1, false>(a, grid, st);
  else if (a.C == 2 && (at & 7u) == 0) launch_disagreement_as<2, true>(a, grid, st);
  else if (a.C == 2) launch_disagreement_as<2, false>(a, grid, st);
  else if (a.C == 3) launch_disagreement_as<3, false>(a, grid, st);
  else if ((at & 15u) == 0) launch_disagreement_as<4, true>(a, grid, st);
  else launch_disagreement_as<4, false>(a, grid, st);
  return hipGetLastError();
}

// Tiles out of a multi-channel frame state: canvas (N,H,W,C) -> tiles (count, C, ph, pw), tile k of the launch cut at
// its plan start.  A thread owns a pixel of the tile (consecutive lanes, consecutive x): it reads the C values of the
// pixel, which are contiguous in the canvas, and writes one dword into each of the C planes.
__global__ void k_tiles_gather_canvas(const float* __restrict__ canvas, int C, int H, int W, int ph, int pw,
                                      const int* __restrict__ starts, TileSeq seq, float* __restrict__ tiles) {
  const TileGeom g{H, W, ph, pw, starts, seq};
  const long long k = blockIdx.y;
  const TileOrigin o = tile_origin(g, k);
  const int total = ph * pw;
  float* __restrict__ tile = tiles + (size_t)k * C * total;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const float* src = canvas + tile_src(g, (size_t)o.n * H, o.y0, o.x0, i) * C;
    for (int c = 0; c < C; ++c) tile[(size_t)c * total + i] = src[c];
  }
}
hipError_t launch_tiles_gather_canvas(const float* canvas, int C, const TileGeom& g, float* tiles, hipStream_t st) {
  hipLaunchKernelGGL(k_tiles_gather_canvas, dim3(tile_grid_x((long long)g.ph * g.pw), (unsigned)g.seq.count), dim3(256), 0,
                     st, canvas, C, g.H, g.W, g.ph, g.pw, g.starts, g.seq, tiles);
  return hipGetLastError();
}

}  // namespace dsx
