// dsx_conv_direct.hip — the two direct conv kernels outside the variant table: k_conv_first (the UNet's first conv) and
// k_conv_naive (one thread per output element).
#include "dsx_conv_common.h"

namespace dsx {

// ===========================================================================================
// First conv of the UNet (downs.0: 3 x 3, 1..7 input channels -> 16..64 output channels, no GroupNorm in front).
//
// With so few input channels the per-tap channel chunk of the implicit-GEMM kernels is almost all padding
// (6 of 32 channels x 9 taps) and their staging falls back to per-element loads.  Here the whole receptive
// field is ONE K dimension, k = tap * Cin + c (K = 9 Cin <= 63, padded to 64): a 16 x 16 pixel tile's halo
// patch sits in LDS as [y][x][Cin], a lane gathers its 8 consecutive k's of a step with 2-byte LDS reads through
// a per-lane table of k -> patch offsets that is the same for every pixel, weights (packed [N block][k step] in
// fragment order) live in registers.  The layer is HBM-bound: it writes B * H * W * Cout activations and reads
// almost nothing.  Epilogue + fused GroupNorm statistics as in the other kernels (one partial row per (tile, wave)).
// ===========================================================================================
template <typename DT>
__global__ __launch_bounds__(256) void k_conv_first(const ConvArgs a) {
  constexpr bool F32 = sizeof(DT) == 4;
  constexpr int ES = (int)sizeof(DT);
  constexpr int KSTEP = F32 ? 2 : 16;            // k per MFMA
  constexpr int NS16 = 4;                        // 16-bit: K padded to 64
  __shared__ __attribute__((aligned(16))) unsigned char sm[18 * 18 * 7 * 4 + 64 * 4];
  DT* patch = (DT*)sm;
  int* kofft = (int*)(sm + 18 * 18 * 7 * 4);     // fp32 path: k -> element offset inside the patch

  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 31, lh = lane >> 5;
  const int Cin = a.C0 + a.C1, K = 9 * Cin;
  const int tiles_x = a.Wo >> 4, tiles_y = a.Ho >> 4;
  const int t = blockIdx.x % (tiles_x * tiles_y), b = blockIdx.x / (tiles_x * tiles_y);
  const int ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oy0 = ty * 16, ox0 = tx * 16;
  const int NBLK = (a.Cout + 31) >> 5;           // 1 or 2

  // ---- halo patch -> LDS [18][18][Cin] (zero outside the image)
  for (int e = tid; e < 18 * 18 * Cin; e += 256) {
    const int c = e % Cin, pp = e / Cin, px = pp % 18, py = pp / 18;
    const int iy = oy0 + py - 1, ix = ox0 + px - 1;
    DT v = (DT)0.f;
    if (iy >= 0 && iy < a.Hs && ix >= 0 && ix < a.Ws) {
      const size_t pix = ((size_t)b * a.Hs + iy) * a.Ws + ix;
      v = c < a.C0 ? ((const DT*)a.src0)[pix * a.C0 + c] : ((const DT*)a.src1)[pix * a.C1 + (c - a.C0)];
    }
    patch[e] = v;
  }
  if (F32 && tid < 64) {
    const int k = tid < K ? tid : 0;             // padded k: weight 0, any finite element
    const int tap = k / Cin, c = k - tap * Cin;
    kofft[tid] = ((tap / 3) * 18 + (tap % 3)) * Cin + c;
  }
  // 16-bit path: this lane's k's (the same for every pixel): k = 16 s + 8 lh + j
  int koff[F32 ? 1 : NS16 * 8];
  if constexpr (!F32) {
#pragma unroll
    for (int s = 0; s < NS16; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        int k = 16 * s + 8 * lh + j;
        if (k >= K) k = 0;
        const int tap = k / Cin, c = k - tap * Cin;
        koff[s * 8 + j] = (((tap / 3) * 18 + (tap % 3)) * Cin + c) * 2;
      }
  }
  // weights: [N block][k step][lane][16 B] (16-bit) or [N block][k step][lane] floats (fp32), rows permuted as in pack_conv
  uint4 wf[F32 ? 1 : 2 * NS16];
  if constexpr (!F32) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int s = 0; s < NS16; ++s)
        wf[nb * NS16 + s] = nb < NBLK ? ((const uint4*)a.wpack)[(nb * NS16 + s) * 64 + lane] : make_uint4(0u, 0u, 0u, 0u);
  }
  __syncthreads();

  f32x16 acc[2][2];
#pragma unroll
  for (int mb = 0; mb < 2; ++mb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.f;

#pragma unroll
  for (int mb = 0; mb < 2; ++mb) {
    const int m = (wave * 2 + mb) * 32 + li;     // pixel of the 16 x 16 tile
    const int base = ((m >> 4) * 18 + (m & 15)) * Cin;
    if constexpr (F32) {
      const int nsteps = (K + 1) >> 1;
      const float* wp = (const float*)a.wpack;
      for (int s = 0; s < nsteps; ++s) {
        const float pv = ((const float*)patch)[base + kofft[2 * s + lh]];
#pragma unroll
        for (int nb = 0; nb < 2; ++nb) {
          if (nb < NBLK) acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wp[(nb * 32 + s) * 64 + lane], pv, acc[mb][nb], 0, 0, 0);
        }
      }
    } else {
      const unsigned char* pb = (const unsigned char*)patch + base * 2;
#pragma unroll
      for (int s = 0; s < NS16; ++s) {
        unsigned w4[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const unsigned lo = *(const unsigned short*)(pb + koff[s * 8 + 2 * q]);
          const unsigned hi = *(const unsigned short*)(pb + koff[s * 8 + 2 * q + 1]);
          w4[q] = lo | (hi << 16);
        }
        const f32x4_t px = __builtin_bit_cast(f32x4_t, make_uint4(w4[0], w4[1], w4[2], w4[3]));
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          if (nb < NBLK) acc[mb][nb] = mfma_step<DT>(wf[nb * NS16 + s], px, acc[mb][nb]);
      }
    }
  }
  (void)KSTEP; (void)ES;

  // ---- epilogue: + bias, store (16 consecutive channels per lane), GroupNorm partial sums per (tile, wave)
  const int okind = a.out_bf16;
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const int nbase = nb * 32 + 16 * lh;
    if (nb >= NBLK) continue;
    float s1[16], s2[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) { s1[r] = 0.f; s2[r] = 0.f; }
    const bool live = nbase < a.Cout;            // Cout is a multiple of 16
#pragma unroll
    for (int mb = 0; mb < 2; ++mb) {
      const int m = (wave * 2 + mb) * 32 + li;
      const size_t opix = ((size_t)b * a.Ho + (oy0 + (m >> 4))) * a.Wo + (ox0 + (m & 15));
      float x[16], pv[16];
#pragma unroll
      for (int r = 0; r < 16; ++r) { x[r] = acc[mb][nb][r]; pv[r] = 0.f; }
      if (live) {
        if (a.bias) {
#pragma unroll
          for (int j = 0; j < 4; ++j) { const float4 tt = *(const float4*)(a.bias + nbase + 4 * j); pv[4 * j] = tt.x; pv[4 * j + 1] = tt.y; pv[4 * j + 2] = tt.z; pv[4 * j + 3] = tt.w; }
#pragma unroll
          for (int r = 0; r < 16; ++r) x[r] += pv[r];
        }
        store16<true>(a.out, opix * a.out_ld + nbase, x, okind, 16);
        // statistics shifted by the bias (StatPivot): a uniform input region gives x ~ bias, whose raw sums would cancel
#pragma unroll
        for (int r = 0; r < 16; ++r) { const float d = x[r] - pv[r]; s1[r] += d; s2[r] += d * d; }
      }
    }
    if (a.stat_part != nullptr) {
      float w1 = row16_fold(s1, lane), w2 = row16_fold(s2, lane);
      w1 += __shfl_xor(w1, 16, 64);
      w2 += __shfl_xor(w2, 16, 64);
      const int nch = tiles_x * tiles_y * 4, chunk = t * 4 + wave;
      const int n = nbase + row16_fold_reg(li);
      if (li < 16 && n < a.Cout) {
        float* pp = a.stat_part + (((size_t)b * nch + chunk) * a.Cout + n) * 2;
        pp[0] = w1; pp[1] = w2;
      }
    }
  }
}

bool conv_first_applicable(int ks, int stride, const ConvArgs& a, bool gn) {
  const int C = a.C0 + a.C1;
  return ks == 3 && stride == 1 && !a.up && !gn && !a.swish && C >= 1 && C <= 7 && a.Cout >= 16 && a.Cout <= 64 &&
         (a.Cout & 15) == 0 && (a.Ho & 15) == 0 && (a.Wo & 15) == 0 && a.Ho == a.Hs && a.Wo == a.Ws && a.out_ld == a.Cout;
}
hipError_t launch_conv_first(int dtype, const ConvArgs& a, hipStream_t st) {
  const unsigned grid = (unsigned)(a.B * (a.Ho >> 4) * (a.Wo >> 4));
  if (dtype == 1) hipLaunchKernelGGL(k_conv_first<__bf16>, dim3(grid), dim3(256), 0, st, a);
  else if (dtype == 2) hipLaunchKernelGGL(k_conv_first<_Float16>, dim3(grid), dim3(256), 0, st, a);
  else hipLaunchKernelGGL(k_conv_first<float>, dim3(grid), dim3(256), 0, st, a);
  return hipGetLastError();
}

// ------------------------------------------------------------ naive direct conv
__global__ void k_conv_naive(const NaiveConvArgs na) {
  const ConvArgs& a = na.c;
  const long long total = (long long)a.B * a.Ho * a.Wo * a.Cout;
  const int C = a.C0 + a.C1;
  const int pad = na.ks / 2;
  const int Hi = a.up ? a.Hs * 2 : a.Hs, Wi = a.up ? a.Ws * 2 : a.Ws;
  for (long long idx = blockIdx.x * (long long)blockDim.x + threadIdx.x; idx < total;
       idx += (long long)gridDim.x * blockDim.x) {
    const int n = (int)(idx % a.Cout);
    long long p = idx / a.Cout;
    const int ox = (int)(p % a.Wo); p /= a.Wo;
    const int oy = (int)(p % a.Ho);
    const int b = (int)(p / a.Ho);
    float acc = 0.f;
    for (int dy = 0; dy < na.ks; ++dy) {
      const int iy = oy * na.stride + dy - pad;
      if (iy < 0 || iy >= Hi) continue;
      for (int dx = 0; dx < na.ks; ++dx) {
        const int ix = ox * na.stride + dx - pad;
        if (ix < 0 || ix >= Wi) continue;
        const int sy = a.up ? iy >> 1 : iy, sx = a.up ? ix >> 1 : ix;
        const size_t so = ((size_t)b * a.Hs + sy) * a.Ws + sx;
        const float* w = na.w + (((size_t)n * na.ks + dy) * na.ks + dx) * C;
        for (int c = 0; c < C; ++c) {
          float v = c < a.C0 ? act_load_kind(a.src0, so * a.C0 + c, a.act_bf16)
                             : act_load_kind(a.src1, so * a.C1 + (c - a.C0), a.act_bf16);
          if (a.gn_scale) v = v * a.gn_scale[(size_t)b * C + c] + a.gn_shift[(size_t)b * C + c];
          if (a.swish) v = swish_f(v);
          acc = fmaf(v, w[c], acc);
        }
      }
    }
    const size_t opix = ((size_t)b * a.Ho + oy) * a.Wo + ox;
    float v = acc + (a.bias ? a.bias[n] : 0.f);
    if (a.film) v += a.film[(size_t)b * a.film_bs + n];
    if (a.resid) v += act_load_kind(a.resid, opix * a.resid_ld + n, a.act_bf16);
    if (na.sigmoid_out) v = 1.0f / (1.0f + __expf(-v));
    act_store(a.out, opix * a.out_ld + n, v, a.out_bf16);
  }
}

hipError_t launch_conv_naive(const NaiveConvArgs& a, hipStream_t st) {
  const long long total = (long long)a.c.B * a.c.Ho * a.c.Wo * a.c.Cout;
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(k_conv_naive, dim3((unsigned)blocks), dim3(256), 0, st, a);
  return hipGetLastError();
}

}  // namespace dsx
