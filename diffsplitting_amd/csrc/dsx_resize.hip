// dsx_resize.hip — PIL's 8-bit antialiased resampler (Image.resize, BILINEAR / BICUBIC: libImaging/Resample.c,
// ImagingResampleHorizontal_8bpc / ImagingResampleVertical_8bpc) and ToTensor on gfx950, for the SR3 image path
// (data/prepare_data.py:17-40 resize_multiple, data/util.py:74-83 transform_augment).
//
// The resampler is integer arithmetic: per output sample ss = 1 << 21, ss += pixel * k[t] over the n taps from xmin
// (int32 coefficients scaled by 2^22, dsx_resize_coeffs), output clip(ss >> 22, 0, 255).  The two passes keep PIL's
// order (horizontal first) and its uint8 intermediate, so the result is equal to PIL's byte for byte.
//
//   k_resize_h_u8   one workgroup = (image, S output columns, T rows): the S coefficient rows and the source span of the
//                   T rows in LDS; a thread makes 4 consecutive output bytes of a row
//   k_resize_v_u8   one workgroup = (image, S output rows, T byte columns): the S coefficient rows and the source rows
//                   they cover in LDS; a thread makes 4 consecutive bytes of an output row, tap loop outermost
//   k_u8_to_tensor  NHWC uint8 -> NCHW fp32, (u / 255) * (hi - lo) + lo
//
// Tap counts are not bounded (1024 -> 16 bicubic: 257): the tap loops run over n, nothing is unrolled to a maximum.
// Rows of 3-byte pixels start at any byte address, so a row is staged from its 16-byte-aligned groups: whole groups
// inside the wanted bytes move as 16-byte vectors, the edge groups byte by byte, and the row keeps its misalignment
// inside its LDS row (nothing outside the wanted bytes is ever read).  Only the window the caller asks for (the centre
// crop of resize_and_convert) is computed and stored.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "dsx_kernels.h"

namespace dsx {

namespace {

constexpr int kThreads = 256;
constexpr int kHalf = 1 << 21;      // 1 << (PRECISION_BITS - 1), PRECISION_BITS = 32 - 8 - 2

__device__ __forceinline__ int misalign(const unsigned char* p) { return (int)((uintptr_t)p & 15); }

// rows x nbytes from g0 (row r at g0 + r * gpitch) -> lds[r * pitch + misalign(row) + i]
__device__ __forceinline__ void stage_rows(unsigned char* lds, int pitch, const unsigned char* g0, long long gpitch, int rows,
                                           int nbytes) {
  const int groups = pitch >> 4;
  for (int idx = threadIdx.x; idx < rows * groups; idx += kThreads) {
    const int r = idx / groups, g = idx - r * groups;
    const unsigned char* p = g0 + r * gpitch;
    const int lo = g * 16 - misalign(p);      // index, relative to p, of the group's first byte
    if (lo >= nbytes || lo + 16 <= 0) continue;
    unsigned char* d = lds + r * pitch + g * 16;
    if (lo >= 0 && lo + 16 <= nbytes) {
      *(uint4*)d = *(const uint4*)(p + lo);
    } else {
      for (int i = 0; i < 16; ++i)
        if (lo + i >= 0 && lo + i < nbytes) d[i] = p[lo + i];
    }
  }
}

__device__ __forceinline__ void stage_tables(const ResizePassArgs& a, int first, int ns, int* s_k, int* s_xmin, int* s_n) {
  const int* gk = a.k + (size_t)first * a.ksize;
  for (int i = threadIdx.x; i < ns * a.ksize; i += kThreads) s_k[i] = gk[i];
  for (int i = threadIdx.x; i < ns; i += kThreads) {
    s_xmin[i] = a.xmin[first + i];
    s_n[i] = a.n[first + i];
  }
}

__device__ __forceinline__ int clip8(int ss) { return min(max(ss >> 22, 0), 255); }   // arithmetic shift

__device__ __forceinline__ void store4(unsigned char* d, const int (&v)[4], int valid) {
  if (valid == 4 && ((uintptr_t)d & 3) == 0) {
    *(uchar4*)d = make_uchar4((unsigned char)v[0], (unsigned char)v[1], (unsigned char)v[2], (unsigned char)v[3]);
  } else {
    for (int e = 0; e < valid; ++e) d[e] = (unsigned char)v[e];
  }
}

}  // namespace

__global__ __launch_bounds__(kThreads) void k_resize_h_u8(ResizePassArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* s_k = (int*)smem;
  int* s_xmin = s_k + a.S * a.ksize;
  int* s_n = s_xmin + a.S;
  unsigned char* s_src = smem + resize_tab_bytes(a.S, a.ksize);
  const int x0 = blockIdx.x * a.S, ns = min(a.S, a.n_out - x0);
  const int r0 = blockIdx.y * a.T, nr = min(a.T, a.n_other - r0);
  const int first = a.t0 + x0;
  stage_tables(a, first, ns, s_k, s_xmin, s_n);
  // xmin and xmin + n never decrease along the outputs: the strip's span is [xmin of the first, end of the last)
  const int smin = a.xmin[first], smax = a.xmin[first + ns - 1] + a.n[first + ns - 1];
  const unsigned char* g0 = a.src + blockIdx.z * a.src_img + (long long)r0 * a.src_pitch + smin * a.C;
  stage_rows(s_src, a.lds_pitch, g0, a.src_pitch, nr, (smax - smin) * a.C);
  __syncthreads();
  const int strip_bytes = ns * a.C, q = (strip_bytes + 3) >> 2;
  unsigned char* d0 = a.dst + blockIdx.z * a.dst_img + (long long)r0 * a.dst_pitch + x0 * a.C;
  for (int it = threadIdx.x; it < nr * q; it += kThreads) {
    const int r = it / q, j4 = (it - r * q) * 4;
    const unsigned char* row = s_src + r * a.lds_pitch + misalign(g0 + (long long)r * a.src_pitch);
    const int valid = min(4, strip_bytes - j4);
    int v[4] = {0, 0, 0, 0};
    for (int e = 0; e < valid; ++e) {
      const int j = j4 + e, x = j / a.C, c = j - x * a.C;
      const int* kk = s_k + x * a.ksize;
      const unsigned char* sp = row + (s_xmin[x] - smin) * a.C + c;
      const int nn = s_n[x];
      int ss = kHalf;
      for (int t = 0; t < nn; ++t) ss += (int)sp[t * a.C] * kk[t];
      v[e] = clip8(ss);
    }
    store4(d0 + (long long)r * a.dst_pitch + j4, v, valid);
  }
}

__global__ __launch_bounds__(kThreads) void k_resize_v_u8(ResizePassArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  int* s_k = (int*)smem;
  int* s_xmin = s_k + a.S * a.ksize;
  int* s_n = s_xmin + a.S;
  unsigned char* s_src = smem + resize_tab_bytes(a.S, a.ksize);
  const int c0 = blockIdx.x * a.T, nb = min(a.T, a.n_other - c0);
  const int y0 = blockIdx.y * a.S, ns = min(a.S, a.n_out - y0);
  const int first = a.t0 + y0;
  stage_tables(a, first, ns, s_k, s_xmin, s_n);
  const int rmin = a.xmin[first] - a.base, rmax = a.xmin[first + ns - 1] + a.n[first + ns - 1] - a.base;
  const unsigned char* g0 = a.src + blockIdx.z * a.src_img + (long long)rmin * a.src_pitch + c0;
  stage_rows(s_src, a.lds_pitch, g0, a.src_pitch, rmax - rmin, nb);
  __syncthreads();
  const int q = (nb + 3) >> 2;
  unsigned char* d0 = a.dst + blockIdx.z * a.dst_img + (long long)y0 * a.dst_pitch + c0;
  for (int it = threadIdx.x; it < ns * q; it += kThreads) {
    const int y = it / q, j4 = (it - y * q) * 4;
    const int* kk = s_k + y * a.ksize;
    const int rm = s_xmin[y] - a.base - rmin, nn = s_n[y];
    int ss[4] = {kHalf, kHalf, kHalf, kHalf};
    for (int t = 0; t < nn; ++t) {
      // bytes past nb (the last group of a chunk) lie inside the row's padding: read, never stored
      const unsigned char* p = s_src + (rm + t) * a.lds_pitch + misalign(g0 + (long long)(rm + t) * a.src_pitch) + j4;
      const int kv = kk[t];
#pragma unroll
      for (int e = 0; e < 4; ++e) ss[e] += (int)p[e] * kv;
    }
    int v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = clip8(ss[e]);
    store4(d0 + (long long)y * a.dst_pitch + j4, v, min(4, nb - j4));
  }
}

// a thread converts 4 consecutive pixels of one image: C 4-byte loads and C 16-byte stores when `vec` (HW % 4 == 0,
// src 4-byte and dst 16-byte aligned), bytes and single floats otherwise
__global__ __launch_bounds__(kThreads) void k_u8_to_tensor(const unsigned char* __restrict__ src, float* __restrict__ dst,
                                                          long long HW, int C, long long groups, long long total, float lo,
                                                          float hi, int vec) {
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= total) return;
  const long long b = i / groups, p = (i - b * groups) * 4;
  const int npix = (int)min(4ll, HW - p);
  const unsigned char* s = src + (b * HW + p) * C;
  unsigned char u[12];
  if (vec) {
    for (int w = 0; w < C; ++w) {
      const uchar4 q = ((const uchar4*)s)[w];
      u[4 * w] = q.x; u[4 * w + 1] = q.y; u[4 * w + 2] = q.z; u[4 * w + 3] = q.w;
    }
  } else {
    for (int e = 0; e < npix * C; ++e) u[e] = s[e];
  }
  const float scale = __fsub_rn(hi, lo);
  for (int c = 0; c < C; ++c) {
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int e = 0; e < npix; ++e)
      o[e] = __fadd_rn(__fmul_rn(__fdiv_rn((float)u[e * C + c], 255.0f), scale), lo);
    float* d = dst + (b * C + c) * HW + p;
    if (vec) {
      *(float4*)d = make_float4(o[0], o[1], o[2], o[3]);
    } else {
      for (int e = 0; e < npix; ++e) d[e] = o[e];
    }
  }
}

hipError_t launch_resize_h_u8(const ResizePassArgs& a, hipStream_t st) {
  const dim3 grid((a.n_out + a.S - 1) / a.S, (a.n_other + a.T - 1) / a.T, a.B);
  hipLaunchKernelGGL(k_resize_h_u8, grid, dim3(kThreads), a.lds_bytes, st, a);
  return hipGetLastError();
}

hipError_t launch_resize_v_u8(const ResizePassArgs& a, hipStream_t st) {
  const dim3 grid((a.n_other + a.T - 1) / a.T, (a.n_out + a.S - 1) / a.S, a.B);
  hipLaunchKernelGGL(k_resize_v_u8, grid, dim3(kThreads), a.lds_bytes, st, a);
  return hipGetLastError();
}

hipError_t launch_u8_to_tensor(const unsigned char* src, int B, long long HW, int C, float lo, float hi, float* dst,
                               hipStream_t st) {
  const long long groups = (HW + 3) / 4, total = groups * B;
  const int vec = HW % 4 == 0 && ((uintptr_t)src & 3) == 0 && ((uintptr_t)dst & 15) == 0;
  hipLaunchKernelGGL(k_u8_to_tensor, dim3((unsigned)((total + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, src, dst, HW,
                     C, groups, total, lo, hi, vec);
  return hipGetLastError();
}

}  // namespace dsx
