// dsx_eval.hip — the evaluation kernels (gfx950), none of which runs inside a sampling step: tile gather / mix /
// stitch / pack of tiled prediction, the TimePredictor's range table, the RangeInvariantPsnr sums taken while
// stitching, SSIM + PSNR of image pairs, and the per-sample L1 / L2 reduction of the training objective (the noising
// step in front of the UNet forward is k_q_sample, dsx_steps.hip).  Their reductions: dsx_reduce.h.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

namespace dsx {

// ---------------------------------------------------------------------------
// tiles: gather (N,H,W) frames -> (count, ph, pw); stitch valid regions of
// (count, C, ph, pw) predictions into the (N,H,W,C) canvas (tile_stitcher.py:26-80).
// The tiles of a launch are the arithmetic sequence  id = first + k * stride  (k = blockIdx.y): a rank's
// shard of a plan (or a batch of it) indexes the plan's device tables directly, nothing is uploaded per call.
// ---------------------------------------------------------------------------
__global__ void k_tiles_gather(const float* __restrict__ frames, int H, int W, int ph, int pw,
                               const int* __restrict__ starts, TileSeq seq, float* __restrict__ tiles) {
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int n = starts[t * 3], y0 = starts[t * 3 + 1], x0 = starts[t * 3 + 2];
  const int total = ph * pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / pw, x = i % pw;
    tiles[k * total + i] = frames[((size_t)n * H + (y0 + y)) * W + (x0 + x)];
  }
}
hipError_t launch_tiles_gather(const float* frames, int H, int W, int ph, int pw, const int* starts, TileSeq seq,
                               float* tiles, hipStream_t st) {
  int gx = (ph * pw + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, frames, H, W,
                     ph, pw, starts, seq, tiles);
  return hipGetLastError();
}

// tile crop + the dataset's normalisation in one pass (SplitDataset.__getitem__, data/split_dataset.py:237-278):
//   target_c = (frame_c - mean_target_c) / std_target_c                       (normalize_target, :199-201)
//   input    = w0 * target_0 + w1 * target_1                                   (input_from_normalized_target)
//            | ((w0 * frame_0 + w1 * frame_1) - mean_input) / std_input        (normalize_inp, :195-197)
// in double, rounded to fp32 once, exactly as numpy does with its float64 statistics.
struct GatherNormArgs {
  const float* f0; const float* f1;
  int H, W, ph, pw;
  const int* starts;       // dev [..][3], indexed by tile id
  TileSeq seq;
  float w0, w1;
  double mean_inp, std_inp, mt0, st0, mt1, st1;
  int from_norm_target;
  float* tin;              // (count, 1, ph, pw)
  float* ttar;             // (count, 2, ph, pw)
};
__global__ void k_tiles_gather_norm(const GatherNormArgs a) {
  const long long k = blockIdx.y, t = a.seq.first + k * a.seq.stride;
  const int n = a.starts[t * 3], y0 = a.starts[t * 3 + 1], x0 = a.starts[t * 3 + 2];
  const int total = a.ph * a.pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / a.pw, x = i % a.pw;
    const size_t src = ((size_t)n * a.H + (y0 + y)) * a.W + (x0 + x);
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
hipError_t launch_tiles_gather_norm(const float* f0, const float* f1, int H, int W, int ph, int pw, const int* starts,
                                    TileSeq seq, float w0, float w1, const double norm[6], int from_norm_target,
                                    float* tin, float* ttar, hipStream_t st) {
  GatherNormArgs a{f0, f1, H, W, ph, pw, starts, seq, w0, w1, norm[0], norm[1], norm[2], norm[3], norm[4], norm[5],
                   from_norm_target, tin, ttar};
  int gx = (ph * pw + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather_norm, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, a);
  return hipGetLastError();
}

// The same item for frames with colour planes, (N, Cc, H, W) per stack (SplitDataset on data_type 'cifar10',
// data/split_dataset.py:248-272 with patch.ndim == 3): plane c of stack s is target channel s * Cc + c with its own
// statistics, the input keeps the Cc planes.  A streaming kernel: workgroup (x, c, k) owns a strided share of plane c of
// item k, so the plane and its four statistics are uniform in the workgroup and consecutive threads read and write
// consecutive x.  The arithmetic per element is k_tiles_gather_norm's without from_norm_target.
struct GatherPlanesArgs {
  const float* f0; const float* f1;
  int Cc, H, W, ph, pw;
  const int* starts;       // dev [..][3] = (frame, y, x), indexed by tile id
  TileSeq seq;
  float w0, w1;
  double mean_inp, std_inp;
  double mt[2 * kPlanesMaxC], st[2 * kPlanesMaxC];
  float* tin;              // (count, Cc, ph, pw)
  float* ttar;             // (count, 2 Cc, ph, pw)
};
__global__ void k_tiles_gather_norm_planes(const GatherPlanesArgs a) {
  const long long k = blockIdx.z, t = a.seq.first + k * a.seq.stride;
  const int c = blockIdx.y;
  const int n = a.starts[t * 3], y0 = a.starts[t * 3 + 1], x0 = a.starts[t * 3 + 2];
  const int total = a.ph * a.pw;
  const double mt0 = a.mt[c], st0 = a.st[c], mt1 = a.mt[a.Cc + c], st1 = a.st[a.Cc + c];
  const size_t plane = ((size_t)n * a.Cc + c) * a.H;
  float* tin = a.tin + ((size_t)k * a.Cc + c) * total;
  float* tar0 = a.ttar + ((size_t)k * 2 * a.Cc + c) * total;
  float* tar1 = tar0 + (size_t)a.Cc * total;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / a.pw, x = i % a.pw;
    const size_t src = (plane + (y0 + y)) * a.W + (x0 + x);
    const float p0 = a.f0[src], p1 = a.f1[src];
    tar0[i] = (float)(((double)p0 - mt0) / st0);
    tar1[i] = (float)(((double)p1 - mt1) / st1);
    tin[i] = (float)(((double)__fadd_rn(__fmul_rn(a.w0, p0), __fmul_rn(a.w1, p1)) - a.mean_inp) / a.std_inp);
  }
}
hipError_t launch_tiles_gather_norm_planes(const float* f0, const float* f1, int Cc, int H, int W, int ph, int pw,
                                           const int* starts, TileSeq seq, float w0, float w1, double mean_inp,
                                           double std_inp, const double* mean_target, const double* std_target,
                                           float* tin, float* ttar, hipStream_t st) {
  if (Cc < 1 || Cc > kPlanesMaxC || seq.count < 1 || seq.count > 65535) return hipErrorInvalidValue;
  GatherPlanesArgs a{};
  a.f0 = f0; a.f1 = f1; a.Cc = Cc; a.H = H; a.W = W; a.ph = ph; a.pw = pw; a.starts = starts; a.seq = seq;
  a.w0 = w0; a.w1 = w1; a.mean_inp = mean_inp; a.std_inp = std_inp; a.tin = tin; a.ttar = ttar;
  for (int c = 0; c < 2 * Cc; ++c) { a.mt[c] = mean_target[c]; a.st[c] = std_target[c]; }
  int gx = (int)(((long long)ph * pw + 255) / 256);
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather_norm_planes, dim3((unsigned)gx, (unsigned)Cc, (unsigned)seq.count), dim3(256), 0, st, a);
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
  int H, W, ph, pw;
  const int* starts;       // dev [..][3], indexed by tile id
  TileSeq seq;
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
  const long long k = blockIdx.y, t = a.seq.first + k * a.seq.stride;
  const int n = a.starts[t * 3], y0 = a.starts[t * 3 + 1], x0 = a.starts[t * 3 + 2];
  const int gpr = (a.pw + 3) >> 2;             // groups per tile row
  const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long long)a.ph * gpr) return;
  const int y = (int)(g / gpr), x = (int)(g - (long long)y * gpr) * 4;
  const int cnt = VEC ? 4 : min(4, a.pw - x);
  const T* src = (const T*)a.frames + ((size_t)n * a.H + (y0 + y)) * a.W + (x0 + x);
  float v[4] = {0.f, 0.f, 0.f, 0.f};
  if (cnt == 4) load_pixels4(src, v);
  else DSX_EACH4(j, cnt) v[j] = (float)src[j];
  DSX_EACH4(j, cnt) {
    const float px = a.has_clip ? fminf(v[j], a.clip) : v[j];
    v[j] = (float)(((double)px - a.mean) / a.std);
  }
  float* dst = a.out + (size_t)k * a.ph * a.pw + (size_t)y * a.pw + x;
  if (VEC) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
  else DSX_EACH4(j, cnt) dst[j] = v[j];
}
template <class T>
static hipError_t launch_gather_input_as(const GatherInputArgs& a, hipStream_t st) {
  const bool vec = (a.pw & 3) == 0 && aligned16(a.out);
  const long long groups = (long long)a.ph * ((a.pw + 3) >> 2);
  const dim3 grid((unsigned)((groups + 255) / 256), (unsigned)a.seq.count);
  if (vec) hipLaunchKernelGGL((k_tiles_gather_input<T, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_tiles_gather_input<T, false>), grid, dim3(256), 0, st, a);
  return hipGetLastError();
}
hipError_t launch_tiles_gather_input(const void* frames, int pix_bytes, bool is_float, int H, int W, int ph, int pw,
                                     const int* starts, TileSeq seq, double mean, double std, double clip, float* out,
                                     hipStream_t st) {
  if (seq.count < 1 || seq.count > 65535 || ph < 1 || pw < 1) return hipErrorInvalidValue;
  const GatherInputArgs a{frames, H, W, ph, pw, starts, seq, mean, std, (float)clip, clip >= 0 ? 1 : 0, out};
  if (is_float && pix_bytes == 4) return launch_gather_input_as<float>(a, st);
  if (!is_float && pix_bytes == 2) return launch_gather_input_as<unsigned short>(a, st);
  if (!is_float && pix_bytes == 1) return launch_gather_input_as<unsigned char>(a, st);
  return hipErrorInvalidValue;
}

// Mean and spread over N posterior samples, Welford's recurrence in double, one launch per sample and one to finish:
//   r == 0: mean = x, M2 = 0;   else d = x - mean;  mean' = mean + d / (r + 1);  M2' = M2 + d * (x - mean')
//   finish: mean_out = (float)mean;  std_out = n > 1 ? (float)sqrt(M2 / (n - 1)) : 0
// Every operation is rounded on its own, so a numpy float64 restatement of these lines gives the same bits.  The
// __d*_rn forms are plain operators in the toolchain's headers and may be contracted once inlined: the product and the
// sums go through mul_d / add_d / sub_d, which take the `contract` flag off their own instruction.
__device__ __forceinline__ double sub_d(double a, double b) {
#pragma clang fp contract(off)
  return a - b;
}
__global__ __launch_bounds__(256) void k_moments_update(const float* __restrict__ x, double* __restrict__ mean,
                                                        double* __restrict__ m2, long long count, int r) {
  const double rn = (double)(r + 1);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    const double xv = (double)x[i];
    if (r == 0) { mean[i] = xv; m2[i] = 0.0; continue; }
    const double m = mean[i], d = sub_d(xv, m);
    const double m1 = add_d(m, d / rn);
    mean[i] = m1;
    m2[i] = add_d(m2[i], mul_d(d, sub_d(xv, m1)));
  }
}
__global__ __launch_bounds__(256) void k_moments_finish(const double* __restrict__ mean, const double* __restrict__ m2,
                                                        long long count, int n, float* __restrict__ mean_out,
                                                        float* __restrict__ std_out) {
  const double nm1 = (double)(n - 1);
  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
    mean_out[i] = (float)mean[i];
    if (std_out) std_out[i] = n > 1 ? (float)sqrt(m2[i] / nm1) : 0.0f;
  }
}
hipError_t launch_moments_update(const float* x, double* mean, double* m2, long long count, int r, hipStream_t st) {
  hipLaunchKernelGGL(k_moments_update, dim3(grid_for(count)), dim3(256), 0, st, x, mean, m2, count, r);
  return hipGetLastError();
}
hipError_t launch_moments_finish(const double* mean, const double* m2, long long count, int n, float* mean_out,
                                 float* std_out, hipStream_t st) {
  hipLaunchKernelGGL(k_moments_finish, dim3(grid_for(count)), dim3(256), 0, st, mean, m2, count, n, mean_out, std_out);
  return hipGetLastError();
}

// (mul_f / add_f / mul_d / add_d, one IEEE operation each, live in dsx_kernels.h)
// The mixed inputs of the TimePredictor evaluation (notebooks/EvaluateJointIndiIterative.ipynb cells 40/43,
// time_prediction_evaluation.ipynb cell 4) cut, normalised, mixed and min-max-normalised in one pass; the op list is
// in include/dsx.h (dsx_tiles_gather_mix).  Channel 0 is indi1's input, channel 1 indi2's.
struct GatherMixArgs {
  const float* f0; const float* f1;
  int H, W, ph, pw;
  const int* starts;       // dev [..][3], indexed by tile id
  TileSeq seq;
  double mt0, st0, mt1, st1;
  MixWeights mw;
  float* ttar; float* tmix; float* tcls;   // (count, 2, ph, pw) each, or nullptr
};
// item k of a launch, cut at (n, y0, x0) with the weights w: the one body of both mixed gathers, so that an item of
// k_tiles_gather_mix_items is bitwise the item k_tiles_gather_mix writes for the same location, t and table rows
__device__ __forceinline__ void mix_item(const GatherMixArgs& a, long long k, int n, int y0, int x0, const MixWeights w) {
  const int total = a.ph * a.pw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int y = i / a.pw, x = i % a.pw;
    const size_t src = ((size_t)n * a.H + (y0 + y)) * a.W + (x0 + x);
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
  const long long k = blockIdx.y, t = a.seq.first + k * a.seq.stride;
  mix_item(a, k, a.starts[t * 3], a.starts[t * 3 + 1], a.starts[t * 3 + 2], a.mw);
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
hipError_t launch_tiles_gather_mix_items(const float* f0, const float* f1, int H, int W, int ph, int pw,
                                         const MixItem* items, long long count, const double norm[4], float* ttar,
                                         float* tmix, float* tcls, hipStream_t st) {
  if (count < 1 || count > 65535) return hipErrorInvalidValue;
  GatherMixArgs a{f0, f1, H, W, ph, pw, nullptr, TileSeq{0, 1, count}, norm[0], norm[1], norm[2], norm[3], MixWeights{},
                  ttar, tmix, tcls};
  int gx = (ph * pw + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather_mix_items, dim3((unsigned)gx, (unsigned)count), dim3(256), 0, st, a, items);
  return hipGetLastError();
}
hipError_t launch_tiles_gather_mix(const float* f0, const float* f1, int H, int W, int ph, int pw, const int* starts,
                                   TileSeq seq, const double norm[4], const MixWeights& mw, float* ttar, float* tmix,
                                   float* tcls, hipStream_t st) {
  GatherMixArgs a{f0, f1, H, W, ph, pw, starts, seq, norm[0], norm[1], norm[2], norm[3], mw, ttar, tmix, tcls};
  int gx = (ph * pw + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_gather_mix, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, a);
  return hipGetLastError();
}

// The TimePredictor's input range table (compute_input_normalization_dict, data/time_predictor_dataset.py:6-21): for
// every t_int in 0..n the min and max over all pixels of  t * a + (1 - t) * b,  t = t_int / n,  a, b = the normalised
// channels -- n + 1 numpy passes over the frame set in the reference, one launch here.  All of it in fp64 with every
// operation rounded on its own (numpy has no fma), so the table is bitwise numpy's; min / max are exact, the result
// does not depend on the reduction tree.  fp64-VALU-bound, not HBM-bound: a thread keeps the running min / max of
// kMixTB values of t in registers (and their weights) while it strides over its workgroup's pixel chunk; the t blocks
// are blockIdx.x, so the workgroups that re-read a chunk are dispatched together and find it in L2 / MALL.  Wave
// reduction by shuffles, the four waves through LDS, one partial row per workgroup: part[chunk][t_int][{min, max}].
constexpr int kMixTB = 8;
constexpr int kMixMaxChunks = 512;
__global__ __launch_bounds__(256) void k_mix_range(const float* __restrict__ f0, const float* __restrict__ f1,
                                                   long long pixels, long long chunk, double m0, double s0, double m1,
                                                   double s1, int n, double* __restrict__ part) {
  __shared__ double red[4 * kMixTB * 2];       // [wave][t][{min, max}]
  const int tb = blockIdx.x * kMixTB;
  double tw[kMixTB], uw[kMixTB], mn[kMixTB], mx[kMixTB];
#pragma unroll
  for (int j = 0; j < kMixTB; ++j) {
    const int ti = min(tb + j, n);             // the rows past n of the last block repeat row n and are not written
    tw[j] = (double)ti / (double)n;            // IEEE division, as numpy's t_int / n_timesteps
    uw[j] = 1.0 - tw[j];
    mn[j] = INFINITY; mx[j] = -INFINITY;
  }
  const long long p0 = blockIdx.y * chunk, p1 = min(pixels, p0 + chunk);
  for (long long p = p0 + threadIdx.x; p < p1; p += 256) {
    const double a = ((double)f0[p] - m0) / s0, b = ((double)f1[p] - m1) / s1;
#pragma unroll
    for (int j = 0; j < kMixTB; ++j) {
      const double v = add_d(mul_d(tw[j], a), mul_d(uw[j], b));
      mn[j] = fmin(mn[j], v); mx[j] = fmax(mx[j], v);
    }
  }
#pragma unroll
  for (int j = 0; j < kMixTB; ++j) {
    block_park<RedMin>(mn[j], red, kMixTB * 2, 2 * j);
    block_park<RedMax>(mx[j], red, kMixTB * 2, 2 * j + 1);
  }
  __syncthreads();
  if (threadIdx.x < kMixTB * 2) {
    const int j = threadIdx.x >> 1, kk = threadIdx.x & 1;
    if (tb + j <= n)
      part[((size_t)blockIdx.y * (n + 1) + (tb + j)) * 2 + kk] =
          kk ? block_combine<RedMax, Pairwise>(red, kMixTB * 2, threadIdx.x)
             : block_combine<RedMin, Pairwise>(red, kMixTB * 2, threadIdx.x);
  }
}
// pixel workgroups (= rows of partials) of a call: about a thousand pixels per workgroup at least, 512 chunks at most
int mix_range_blocks(long long pixels) {
  const long long g = (pixels + 1023) / 1024;
  return (int)(g > kMixMaxChunks ? kMixMaxChunks : (g < 1 ? 1 : g));
}
hipError_t launch_mix_range(const float* f0, const float* f1, long long pixels, const double norm[4], int n, double* part,
                            hipStream_t st) {
  const int gy = mix_range_blocks(pixels);
  const long long chunk = (pixels + gy - 1) / gy;
  hipLaunchKernelGGL(k_mix_range, dim3((unsigned)((n + kMixTB) / kMixTB), (unsigned)gy), dim3(256), 0, st, f0, f1, pixels,
                     chunk, norm[0], norm[1], norm[2], norm[3], n, part);
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
  int gx = (ph * pw * C + 255) / 256;
  if (gx > 64) gx = 64;
  hipLaunchKernelGGL(k_tiles_pack, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, tiles, C, ph, pw, regions,
                     off, seq, flat);
  return hipGetLastError();
}

// Stitch + the sums RangeInvariantPsnr needs (core/psnr.py:70-82), in the same pass: while a tile's valid region
// is pasted, every (tile, workgroup) also reduces, per channel, sum(p), sum(p^2), sum(g), sum(g^2), sum(g p),
// min(g), max(g) of prediction p against the ground truth g at the same canvas pixels (every canvas pixel is pasted
// exactly once).  Fixed reduction order (thread -> wave shuffles -> 4 waves): bitwise reproducible.
// part[k][blockIdx.x][c][8] doubles; the per-frame combination (a few hundred values) is the caller's.
constexpr int kPsnrMaxC = 4;
__global__ __launch_bounds__(256) void k_stitch_psnr(const TileSrc src, int C, const int* __restrict__ regions, TileSeq seq,
                                                      float* __restrict__ canvas, const float* __restrict__ gt, int H, int W,
                                                      double* __restrict__ part) {
  __shared__ double red[4 * kPsnrMaxC * 7];    // [wave][channel][7 values]
  const long long k = blockIdx.y, t = seq.first + k * seq.stride;
  const int* r = regions + t * 8;
  const int n = r[0], y0 = r[1], x0 = r[2], h = r[3], w = r[4];
  const TileView v = tile_view(src, k, t, C, r);
  double sp[kPsnrMaxC], spp[kPsnrMaxC], sg[kPsnrMaxC], sgg[kPsnrMaxC], sgp[kPsnrMaxC], mn[kPsnrMaxC], mx[kPsnrMaxC];
#pragma unroll
  for (int c = 0; c < kPsnrMaxC; ++c) { sp[c] = spp[c] = sg[c] = sgg[c] = sgp[c] = 0; mn[c] = INFINITY; mx[c] = -INFINITY; }
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < h * w; i += gridDim.x * blockDim.x) {
    const int x = i % w, y = i / w;
    const size_t cpix = (((size_t)n * H + (y0 + y)) * W + (x0 + x)) * C;
#pragma unroll
    for (int c = 0; c < kPsnrMaxC; ++c) {
      if (c < C) {
        const float p = v.p[c * v.plane + (size_t)y * v.pitch + x];
        const float g = gt[cpix + c];
        canvas[cpix + c] = p;
        sp[c] += p; spp[c] += (double)p * p; sg[c] += g; sgg[c] += (double)g * g; sgp[c] += (double)g * p;
        mn[c] = fmin(mn[c], (double)g); mx[c] = fmax(mx[c], (double)g);
      }
    }
  }
  constexpr int kSlots = kPsnrMaxC * 7;
#pragma unroll
  for (int c = 0; c < kPsnrMaxC; ++c) {
    block_park<RedSum>(sp[c], red, kSlots, c * 7);
    block_park<RedSum>(spp[c], red, kSlots, c * 7 + 1);
    block_park<RedSum>(sg[c], red, kSlots, c * 7 + 2);
    block_park<RedSum>(sgg[c], red, kSlots, c * 7 + 3);
    block_park<RedSum>(sgp[c], red, kSlots, c * 7 + 4);
    block_park<RedMin>(mn[c], red, kSlots, c * 7 + 5);
    block_park<RedMax>(mx[c], red, kSlots, c * 7 + 6);
  }
  __syncthreads();
  if (threadIdx.x < C * 8) {
    const int c = threadIdx.x >> 3, kk = threadIdx.x & 7;
    double o = 0;
    if (kk < 5) o = block_combine<RedSum, Pairwise>(red, kSlots, c * 7 + kk);
    else if (kk == 5) o = block_combine<RedMin, Pairwise>(red, kSlots, c * 7 + 5);
    else if (kk == 6) o = block_combine<RedMax, Pairwise>(red, kSlots, c * 7 + 6);
    part[(((size_t)k * gridDim.x + blockIdx.x) * C + c) * 8 + kk] = o;
  }
}
// gt == nullptr: plain paste; else also the RangeInvariantPsnr partial sums (C <= 4, gx workgroups per tile)
hipError_t launch_stitch(const StitchSrc& s, int C, const int* regions, TileSeq seq, float* canvas, int H, int W,
                         const float* gt, double* part, int gx, hipStream_t st) {
  const TileSrc src{s.base, s.packed, s.ph, s.pw, s.off, s.rank_stride, s.world < 1 ? 1 : s.world};
  if (gt != nullptr) {
    if (C < 1 || C > kPsnrMaxC || gx < 1 || part == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_stitch_psnr, dim3((unsigned)gx, (unsigned)seq.count), dim3(256), 0, st, src, C, regions, seq,
                       canvas, gt, H, W, part);
  } else {
    int g = (s.ph * s.pw * C + 255) / 256;
    if (g > 64) g = 64;
    hipLaunchKernelGGL(k_stitch, dim3((unsigned)g, (unsigned)seq.count), dim3(256), 0, st, src, C, regions, seq, canvas,
                       H, W);
  }
  return hipGetLastError();
}

// SSIM (core/metrics.py:72-92) + sum of squared differences (calculate_psnr, :62-69) of image pairs in one pass.
// One workgroup per (32 x 32 tile of the valid region [5:-5, 5:-5], image plane): the 42 x 42 input tile (10-pixel
// halo, re-read by the neighbours through L2) is staged in LDS, quantised on the load when asked (tensor2img,
// :14-34: clamp, (x - lo) / (hi - lo) with IEEE division, * 255, round half to even); then the 11-tap Gaussian is
// applied horizontally to the five moments x, y, x^2, y^2, x y of all 42 rows (fp64, to LDS) and vertically to the
// 32 output rows.  Each plane's pixels are partitioned among its tiles (edge tiles also own the 5-pixel border) for
// the SSD: exact uint64 of integers when quantised, fp64 otherwise.  Fixed reduction order (thread -> wave shuffles
// -> 4 waves), no atomics: part[plane][tile] = {sum of the SSIM map over the tile, SSD}, bitwise reproducible.
constexpr int kSsimT = 32, kSsimIn = kSsimT + 10;
__device__ __forceinline__ float metrics_load(const float* p, bool quantize, float lo, float hi, float rng) {
  float x = *p;
  if (quantize) x = rintf((fminf(fmaxf(x, lo), hi) - lo) / rng * 255.0f);
  return x;
}
__global__ __launch_bounds__(256) void k_image_metrics(const float* __restrict__ a, const float* __restrict__ b, int H,
                                                       int W, int quantize, float lo, float hi, float rng, double c1,
                                                       double c2, SsimWindow win, int tiles_x, double* __restrict__ part) {
  __shared__ float sa[kSsimIn][kSsimIn], sb[kSsimIn][kSsimIn];
  __shared__ double hm[5][kSsimIn][kSsimT];
  __shared__ double red[4 * 2];                // [wave][{SSIM sum, fp64 SSD}]
  __shared__ unsigned long long redq[4];       // [wave] integer SSD
  const int tile = blockIdx.x, plane = blockIdx.y;
  const int y0 = (tile / tiles_x) * kSsimT, x0 = (tile % tiles_x) * kSsimT;    // output tile = input rows/cols + 5
  const int ty_last = (H - 10 + kSsimT - 1) / kSsimT - 1, tx_last = tiles_x - 1;
  // pixels of this tile's SSD share: its output rows/cols, widened to the image edge on the edge tiles
  const int oy0 = y0 == 0 ? 0 : y0 + 5, oy1 = y0 / kSsimT == ty_last ? H : y0 + 5 + kSsimT;
  const int ox0 = x0 == 0 ? 0 : x0 + 5, ox1 = x0 / kSsimT == tx_last ? W : x0 + 5 + kSsimT;
  const size_t pl = (size_t)plane * H * W;
  const bool q = quantize != 0;
  double ssd = 0;
  unsigned long long ssdq = 0;
  for (int i = threadIdx.x; i < kSsimIn * kSsimIn; i += 256) {
    const int r = i / kSsimIn, c = i % kSsimIn, y = y0 + r, x = x0 + c;
    float va = 0.f, vb = 0.f;
    if (y < H && x < W) {
      va = metrics_load(a + pl + (size_t)y * W + x, q, lo, hi, rng);
      vb = metrics_load(b + pl + (size_t)y * W + x, q, lo, hi, rng);
      if (y >= oy0 && y < oy1 && x >= ox0 && x < ox1) {
        if (q) { const int d = (int)va - (int)vb; ssdq += (unsigned long long)(d * d); }
        else { const double d = (double)va - (double)vb; ssd += d * d; }
      }
    }
    sa[r][c] = va; sb[r][c] = vb;
  }
  __syncthreads();
  const int col = threadIdx.x & (kSsimT - 1), r8 = threadIdx.x / kSsimT;
  for (int r = r8; r < kSsimIn; r += 256 / kSsimT) {
    double m0 = 0, m1 = 0, m2 = 0, m3 = 0, m4 = 0;
#pragma unroll
    for (int k = 0; k < 11; ++k) {
      const double u = sa[r][col + k], v = sb[r][col + k], w = win.w[k];
      m0 += w * u; m1 += w * v; m2 += w * (u * u); m3 += w * (v * v); m4 += w * (u * v);
    }
    hm[0][r][col] = m0; hm[1][r][col] = m1; hm[2][r][col] = m2; hm[3][r][col] = m3; hm[4][r][col] = m4;
  }
  __syncthreads();
  // vertical: 4 consecutive output rows per thread share their 14 rows of horizontal sums (taps in ascending order)
  constexpr int kRows = kSsimT / (256 / kSsimT);
  const int rv = r8 * kRows;
  double acc = 0;
  if (x0 + col < W - 10) {
    double mu1[kRows] = {}, mu2[kRows] = {}, e11[kRows] = {}, e22[kRows] = {}, e12[kRows] = {};
#pragma unroll
    for (int k = 0; k < kRows + 10; ++k) {
      const double h0 = hm[0][rv + k][col], h1 = hm[1][rv + k][col], h2 = hm[2][rv + k][col],
                   h3 = hm[3][rv + k][col], h4 = hm[4][rv + k][col];
#pragma unroll
      for (int j = 0; j < kRows; ++j) {
        if (k - j >= 0 && k - j < 11) {
          const double w = win.w[k - j];
          mu1[j] += w * h0; mu2[j] += w * h1; e11[j] += w * h2; e22[j] += w * h3; e12[j] += w * h4;
        }
      }
    }
#pragma unroll
    for (int j = 0; j < kRows; ++j) {
      if (y0 + rv + j < H - 10) {
        const double mu11 = mu1[j] * mu1[j], mu22 = mu2[j] * mu2[j], mu12 = mu1[j] * mu2[j];
        const double s11 = e11[j] - mu11, s22 = e22[j] - mu22, s12 = e12[j] - mu12;
        acc += ((2 * mu12 + c1) * (2 * s12 + c2)) / ((mu11 + mu22 + c1) * (s11 + s22 + c2));
      }
    }
  }
  block_park<RedSum>(acc, red, 2, 0);
  if (q) block_park<RedSum>(ssdq, redq);       // q is the same in every thread
  else block_park<RedSum>(ssd, red, 2, 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = part + ((size_t)plane * gridDim.x + tile) * 2;
    o[0] = block_combine<RedSum, Pairwise>(red, 2, 0);
    o[1] = q ? __longlong_as_double((long long)block_combine<RedSum, Pairwise>(redq))
             : block_combine<RedSum, Pairwise>(red, 2, 1);
  }
}
int image_metrics_tiles(int H, int W) {
  return ((H - 10 + kSsimT - 1) / kSsimT) * ((W - 10 + kSsimT - 1) / kSsimT);
}
hipError_t launch_image_metrics(const float* a, const float* b, int planes, int H, int W, int quantize, float lo,
                                float hi, float rng, double c1, double c2, const SsimWindow& win, double* part,
                                hipStream_t st) {
  if (H < 11 || W < 11 || planes < 1 || planes > 65535) return hipErrorInvalidValue;
  const int tiles_x = (W - 10 + kSsimT - 1) / kSsimT;
  hipLaunchKernelGGL(k_image_metrics, dim3((unsigned)image_metrics_tiles(H, W), (unsigned)planes), dim3(256), 0, st,
                     a, b, H, W, quantize, lo, hi, rng, c1, c2, win, tiles_x, part);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// Per-sample sum |a - b| (L1Loss) or sum (a - b)^2 (MSELoss) over (C, H, W): difference, square and accumulation in
// double.  Workgroup (x, b) owns elements [x * kLossChunk, (x + 1) * kLossChunk) of sample b -- loss_blocks(n) of them,
// a function of the shape alone -- and reduces thread -> wave shuffles -> 4 waves in a fixed order; k_loss_finish adds a
// sample's partials front to back.  No atomics: equal inputs give bitwise-equal outputs.
// ---------------------------------------------------------------------------
constexpr int kLossChunk = 4096;   // 16 elements per thread
__global__ __launch_bounds__(256) void k_loss_partial(const float* __restrict__ a, const float* __restrict__ b,
                                                      long long n, int squared, double* __restrict__ part) {
  __shared__ double red[4];
  const long long base = (long long)blockIdx.y * n;
  const long long i0 = (long long)blockIdx.x * kLossChunk, i1 = min(n, i0 + kLossChunk);
  double s = 0;
  for (long long i = i0 + threadIdx.x; i < i1; i += 256) {
    const double d = (double)a[base + i] - (double)b[base + i];   // exact: both are fp32 values
    s = add_d(s, squared ? mul_d(d, d) : fabs(d));                 // the square rounded on its own, never an fma
  }
  s = block_reduce<RedSum, Pairwise>(s, red);
  if (threadIdx.x == 0) part[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}
__global__ __launch_bounds__(64) void k_loss_finish(const double* __restrict__ part, int B, int nblk,
                                                    double* __restrict__ out) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double s = 0;
  for (int k = 0; k < nblk; ++k) s += part[(size_t)b * nblk + k];
  out[b] = s;
}
int loss_blocks(long long n) { return (int)((n + kLossChunk - 1) / kLossChunk); }
hipError_t launch_loss(const float* a, const float* b, int B, long long n, int squared, double* part, double* out,
                       hipStream_t st) {
  const int nblk = loss_blocks(n);
  hipLaunchKernelGGL(k_loss_partial, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, st, a, b, n, squared, part);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_loss_finish, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, st, part, B, nblk, out);
  return hipGetLastError();
}

}  // namespace dsx
