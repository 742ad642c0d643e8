// dsx_consistency.hip — the residual of a split against its acquisition, r = x - sum_c w_c p_c, the report row of every
// frame and the prediction conditioned on the observation (gfx950; include/dsx.h, dsx_consistency), in ONE pass over
// the acquisition and the canvases.  Host side: dsx_consistency.cpp.
//
// Arithmetic: double, every operation rounded on its own.  The whole file is compiled with contraction off (the pragma
// below), so that a product and the addition behind it never fuse: map, out_mean and out_std are the bits of a numpy
// float64 restatement.  Division and sqrt in double are correctly rounded on this target.
//
// Partition, a function of plane alone: consistency_blocks(plane) workgroups per frame, each owns
// consistency_span(plane) consecutive pixels (a multiple of 4); inside it thread t takes the groups of four pixels
// t, t + 256, .. in ascending order, one pixel after the other, whether the four arrive by 16-byte accesses (kVec) or
// one element at a time.  So a frame's numbers do not depend on the load path, on its position in the call or on the
// number of frames.  Reduction: dsx_reduce.h, RedRow<8, 1> (kDown butterfly, Pairwise combine) into
// part[frame][block][kConSlots]; k_consistency_finish folds the rows of a frame with one wave: row r on lane r % 64,
// ascending, then the kDown butterfly.  No atomics.
//
// In place: a thread loads the operands of its four pixels before it stores any of them and no other thread touches
// them, so out_mean == mean and out_std == std are safe; the pointers carry no __restrict__ for that reason.
#include "dsx_kernels.h"
#include "dsx_reduce.h"

#pragma clang fp contract(off)

namespace dsx {

constexpr int kConChunk = 4096;      // pixels per workgroup up to kConMaxBlocks workgroups: 4 groups of four per thread
constexpr int kConMaxBlocks = 1024;  // per frame (grid x); frames are grid y

int consistency_blocks(long long plane) {
  const long long b = (plane + kConChunk - 1) / kConChunk;
  return (int)(b > kConMaxBlocks ? kConMaxBlocks : (b < 1 ? 1 : b));
}
long long consistency_span(long long plane) {
  const long long b = consistency_blocks(plane);
  return ((plane + b - 1) / b + 3) / 4 * 4;
}

using ConRow = RedRow<8, 1>;
static_assert(ConRow::kSlots == kConSlots, "a report row is eight sums and one (min, max) pair");

template <class T> struct alignas(4 * sizeof(T)) ConIn4 { T v[4]; };

// one pixel: the residual, the conditioned channels (when `project`) and the pixel's terms of the row (when `report`)
template <int C>
__device__ __forceinline__ void con_pixel(const ConArgs& a, double x, const float (&mf)[C], const float (&sf)[C], bool has_sd,
                                          bool project, bool report, float& mapv, float (&om)[C], float (&os)[C],
                                          double (&acc)[kConSlots]) {
  const bool sat = a.clip >= 0 && x >= a.clip;
  double p[C], v[C], m = 0.0, den = 0.0;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    p[c] = (double)mf[c] * a.a[c] + a.b[c];
    m = m + a.w[c] * p[c];
  }
  const double r = x - m;
  mapv = (float)r;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    if (has_sd) { const double t = (double)sf[c] * a.a[c]; v[c] = t * t; }
    else v[c] = 1.0;
    den = den + (a.w[c] * a.w[c]) * v[c];
  }
  den = den + a.noise_var;
  const bool upd = !sat && den > 0;
  if (project) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      if (upd) {
        const double vw = v[c] * a.w[c];
        const double pc = p[c] + (vw * r) / den;
        om[c] = (float)((pc - a.b[c]) / a.a[c]);
        const double vp = v[c] - (vw * vw) / den;
        os[c] = (float)(sqrt(fmax(vp, 0.0)) / a.a[c]);
      } else {
        om[c] = mf[c];
        os[c] = has_sd ? sf[c] : 0.f;
      }
    }
  }
  if (report) {
    if (!sat) {
      const double rr = r * r;
      acc[0] = acc[0] + 1.0; acc[2] = acc[2] + r; acc[3] = acc[3] + rr; acc[4] = acc[4] + x; acc[5] = acc[5] + x * x;
      if (den > 0) { acc[6] = acc[6] + 1.0; acc[7] = acc[7] + rr / den; }
      acc[8] = fmin(acc[8], r); acc[9] = fmax(acc[9], r);
    } else {
      acc[1] = acc[1] + 1.0;
    }
  }
}

template <class T, int C, bool kVec>
__global__ __launch_bounds__(256) void k_consistency_partial(ConArgs a) {
  __shared__ double red[4 * kConSlots];
  const long long frame = blockIdx.y, f0 = frame * a.plane;
  const T* in = (const T*)a.in + f0;
  const float* mean = a.mean + f0 * C;
  const float* sd = a.sd ? a.sd + f0 * C : nullptr;
  float* map = a.map ? a.map + f0 : nullptr;
  float* omean = a.omean ? a.omean + f0 * C : nullptr;
  float* osd = a.osd ? a.osd + f0 * C : nullptr;
  const bool has_sd = sd != nullptr, project = omean != nullptr || osd != nullptr, report = a.out != nullptr;
  const long long i0 = (long long)blockIdx.x * a.span, i1 = min(a.plane, i0 + a.span);
  double acc[kConSlots];
  ConRow::init(acc);
  for (long long i = i0 + 4 * (long long)threadIdx.x; i < i1; i += 4 * 256) {
    const int n = kVec ? 4 : (int)min((long long)4, i1 - i);      // kVec: plane % 4 == 0 and span % 4 == 0, the group is whole
    T xin[4];
    float mf[4][C], sf[4][C], om[4][C], os[4][C], mapv[4];
    // every load of the group first
    if (kVec) {
      const ConIn4<T> q = *(const ConIn4<T>*)(in + i);
#pragma unroll
      for (int j = 0; j < 4; ++j) xin[j] = q.v[j];
#pragma unroll
      for (int k = 0; k < C; ++k) {                                 // C 16-byte loads: floats 4 k .. 4 k + 3 of the group's 4 C
        const float4 t = ((const float4*)(mean + i * C))[k];
        const float e[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) mf[(4 * k + q4) / C][(4 * k + q4) % C] = e[q4];
      }
      if (has_sd) {
#pragma unroll
        for (int k = 0; k < C; ++k) {
          const float4 t = ((const float4*)(sd + i * C))[k];
          const float e[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) sf[(4 * k + q4) / C][(4 * k + q4) % C] = e[q4];
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          xin[j] = in[i + j];
#pragma unroll
          for (int c = 0; c < C; ++c) mf[j][c] = mean[(i + j) * C + c];
          if (has_sd) {
#pragma unroll
            for (int c = 0; c < C; ++c) sf[j][c] = sd[(i + j) * C + c];
          }
        }
      }
    }
    if (!has_sd) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int c = 0; c < C; ++c) sf[j][c] = 0.f;
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < n) con_pixel<C>(a, (double)xin[j], mf[j], sf[j], has_sd, project, report, mapv[j], om[j], os[j], acc);
    // then the stores
    if (kVec) {
      if (map) *(float4*)(map + i) = make_float4(mapv[0], mapv[1], mapv[2], mapv[3]);
#pragma unroll
      for (int k = 0; k < C; ++k) {
        if (omean) {
          float e[4];
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) e[q4] = om[(4 * k + q4) / C][(4 * k + q4) % C];
          ((float4*)(omean + i * C))[k] = make_float4(e[0], e[1], e[2], e[3]);
        }
        if (osd) {
          float e[4];
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) e[q4] = os[(4 * k + q4) / C][(4 * k + q4) % C];
          ((float4*)(osd + i * C))[k] = make_float4(e[0], e[1], e[2], e[3]);
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (j < n) {
          if (map) map[i + j] = mapv[j];
#pragma unroll
          for (int c = 0; c < C; ++c) {
            if (omean) omean[(i + j) * C + c] = om[j][c];
            if (osd) osd[(i + j) * C + c] = os[j][c];
          }
        }
      }
    }
  }
  if (!report) return;                              // uniform: a.out is a kernel argument
  ConRow::park(acc, red);
  __syncthreads();
  if (threadIdx.x < kConSlots)
    a.part[((size_t)frame * gridDim.x + blockIdx.x) * kConSlots + threadIdx.x] = ConRow::combine(red, threadIdx.x);
}

// one wave per frame: lane l folds the rows l, l + 64, .. in ascending order, the kDown butterfly folds the 64 lanes
__global__ __launch_bounds__(64) void k_consistency_finish(ConArgs a, int nblk) {
  const long long frame = blockIdx.x;
  const double* p = a.part + (size_t)frame * nblk * kConSlots;
  double tot[kConSlots];
  ConRow::init(tot);
  for (int k = threadIdx.x; k < nblk; k += 64) ConRow::fold(tot, p + (size_t)k * kConSlots);
#pragma unroll
  for (int j = 0; j < kConSlots; ++j)
    tot[j] = ConRow::is_sum(j) ? wave_reduce<RedSum>(tot[j])
                               : (ConRow::is_min(j) ? wave_reduce<RedMin>(tot[j]) : wave_reduce<RedMax>(tot[j]));
  if (threadIdx.x == 0) {
#pragma unroll
    for (int j = 0; j < kConSlots; ++j) a.out[frame * kConSlots + j] = tot[j];
  }
}

template <class T, int C>
static void con_launch(const ConArgs& a, dim3 grid, bool vec, hipStream_t st) {
  if (vec) hipLaunchKernelGGL((k_consistency_partial<T, C, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((k_consistency_partial<T, C, false>), grid, dim3(256), 0, st, a);
}
template <class T>
static void con_launch_c(const ConArgs& a, dim3 grid, bool vec, hipStream_t st) {
  switch (a.C) {
    case 1: con_launch<T, 1>(a, grid, vec, st); break;
    case 2: con_launch<T, 2>(a, grid, vec, st); break;
    case 3: con_launch<T, 3>(a, grid, vec, st); break;
    default: con_launch<T, 4>(a, grid, vec, st); break;
  }
}

// a.pix: 0 = uint8, 1 = uint16, 3 = fp32 (DSX_PIX_U8 / U16 / F32; the caller has refused everything else)
hipError_t launch_consistency(const ConArgs& a, int frames, bool vec, hipStream_t st) {
  const int nblk = consistency_blocks(a.plane);
  const dim3 grid((unsigned)nblk, (unsigned)frames);
  if (a.pix == 0) con_launch_c<unsigned char>(a, grid, vec, st);
  else if (a.pix == 1) con_launch_c<unsigned short>(a, grid, vec, st);
  else con_launch_c<float>(a, grid, vec, st);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || !a.out) return e;
  hipLaunchKernelGGL(k_consistency_finish, dim3((unsigned)frames), dim3(64), 0, st, a, nblk);
  return hipGetLastError();
}

}  // namespace dsx
