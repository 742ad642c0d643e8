// dsx_conv_common.h — what more than one conv kernel family uses on the device (dsx_conv_mfma.hip, dsx_conv_ws.hip,
// dsx_conv_img.hip, dsx_conv_direct.hip): GroupNorm affine + Swish arithmetic, the DPP row folds, conversions and
// packing, the activation storage types (Chunk / Kind / Unit, act_load / act_store, store16 / store8), the inline-asm
// LDS helpers and counted waits, the MFMA steps of both shapes, and the diagnostic builds' stamps and ablation switch.
#pragma once
#include "dsx_kernels.h"
#include <type_traits>
#include <utility>

// DSX_ABLATE (phase-skipping timing experiments, results wrong) exists only in the diagnostic build
// (DSX_EXTRA_FLAGS=-DDSX_DIAG ./build.sh); the product binary has no such switch.
#ifdef DSX_DIAG
#define DSX_ABLATED(bit) ((a.ablate & (bit)) != 0)
#else
#define DSX_ABLATED(bit) false
#endif

namespace dsx {

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(16))) float f32x16;


// x * sigmoid(x).  v_exp + v_rcp (1 ulp each) instead of an IEEE division sequence (10 more VALU
// instructions per element on the loaders' critical path); far inside the 1e-3 parity budget.
__device__ __forceinline__ float swish_f(float v) {
  return v * __builtin_amdgcn_rcpf(1.0f + __expf(-v));
}
// The same arithmetic on element pairs, written with two-element vectors so that hipcc selects the packed fp32
// instructions (v_pk_mul_f32 / v_pk_add_f32 / v_pk_fma_f32: one issue slot for two elements; the scalar spelling gets
// one v_mul / v_add per element).  Results are bit-identical to swish_f / x * s + h: the same operations in the same
// order (v_exp_f32 is 2^x: __expf(-v) is the product with -log2(e), then v_exp_f32).
typedef __attribute__((ext_vector_type(2))) float f32x2_t;
template <int N> __device__ __forceinline__ void swish_vec(float (&v)[N]) {
  static_assert(N % 2 == 0, "pairs");
#pragma unroll
  for (int j = 0; j < N; j += 2) {
    f32x2_t x = {v[j], v[j + 1]};
    const f32x2_t k = {-1.44269504088896340736f, -1.44269504088896340736f};
    const f32x2_t t = x * k;
    f32x2_t e = {__builtin_amdgcn_exp2f(t.x), __builtin_amdgcn_exp2f(t.y)};
    e = e + 1.0f;
    const f32x2_t r = {__builtin_amdgcn_rcpf(e.x), __builtin_amdgcn_rcpf(e.y)};
    x = x * r;
    v[j] = x.x; v[j + 1] = x.y;
  }
}
template <int N> __device__ __forceinline__ void affine_vec(float (&v)[N], const float (&sc)[N], const float (&sh)[N]) {
  static_assert(N % 2 == 0, "pairs");
#pragma unroll
  for (int j = 0; j < N; j += 2) {
    const f32x2_t x = {v[j], v[j + 1]}, s = {sc[j], sc[j + 1]}, h = {sh[j], sh[j + 1]};
    const f32x2_t y = x * s + h;               // contracted to v_pk_fma_f32 (as the scalar form is to v_fma_f32)
    v[j] = y.x; v[j + 1] = y.y;
  }
}

// 16 per-lane registers -> one total per lane: lane i of a DPP row ends up with the row's sum of register
// r = 8*bit0(i) + 4*bit1(i) + 2*bit2(i) + bit3(i).  Each butterfly stage halves the register count (the
// lane keeps the half its bit selects and receives the partner's copy of that half): 15 adds instead of
// the 64 of sixteen full 16-lane reductions.
template <int CTRL, int BANKS>
__device__ __forceinline__ float dpp_take(float old, float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(__builtin_bit_cast(int, old), __builtin_bit_cast(int, v),
                                                               CTRL, 0xF, BANKS, false));
}
__device__ __forceinline__ float row16_fold(const float (&s)[16], int lane) {
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4, b3 = lane & 8;
  float a8[8], a4[4], a2[2];
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float keep = b0 ? s[k + 8] : s[k], send = b0 ? s[k] : s[k + 8];
    a8[k] = keep + dpp_take<0xB1, 0xF>(0.f, send);                       // lane ^ 1
  }
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float keep = b1 ? a8[k + 4] : a8[k], send = b1 ? a8[k] : a8[k + 4];
    a4[k] = keep + dpp_take<0x4E, 0xF>(0.f, send);                       // lane ^ 2
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float keep = b2 ? a4[k + 2] : a4[k], send = b2 ? a4[k] : a4[k + 2];
    float t = dpp_take<0x104, 0x5>(0.f, send);                           // banks 0,2 <- lane + 4
    t = dpp_take<0x114, 0xA>(t, send);                                   // banks 1,3 <- lane - 4
    a2[k] = keep + t;
  }
  const float keep = b3 ? a2[1] : a2[0], send = b3 ? a2[0] : a2[1];
  return keep + dpp_take<0x128, 0xF>(0.f, send);                         // lane ^ 8 (row_ror:8)
}
__device__ __forceinline__ int row16_fold_reg(int lane) {
  return 8 * (lane & 1) + 4 * ((lane >> 1) & 1) + 2 * ((lane >> 2) & 1) + ((lane >> 3) & 1);
}

// (vector conversions: one v_cvt_pk_* per pair; converted one by one each element costs a convert, and the pair a shift and an or)
typedef __attribute__((ext_vector_type(2))) float f32x2_cvt;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_cvt;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_cvt;
__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) {
  const f32x2_cvt v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, f16x2_cvt));   // RNE
}
__device__ __forceinline__ float f16_lo(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w & 0xffffu)); }
__device__ __forceinline__ float f16_hi(unsigned w) { return (float)__builtin_bit_cast(_Float16, (unsigned short)(w >> 16)); }
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  const f32x2_cvt v = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2_cvt));  // RNE (v_cvt_pk_bf16_f32)
}

// diagnostic stamps (DSX_STAMP_OP): wave 0 of one chosen workgroup records s_memtime at phase
// boundaries into a debug buffer that nothing else reads; off (nullptr) in normal runs
#ifdef DSX_STAMPS   // diagnostic build (DSX_EXTRA_FLAGS=-DDSX_STAMPS ./build.sh): the checks cost scalar work in hot loops
#define DSX_STAMP(i)                                                                        \
  do {                                                                                      \
    if (a.stamp != nullptr && blockIdx.x == (unsigned)a.stamp_block && tid == 0 && (i) < 120) \
      a.stamp[(i)] = __builtin_amdgcn_s_memtime();                                          \
  } while (0)

#define DSX_STAMP_T(i, cond)                                                               \
  do {                                                                                      \
    if (a.stamp != nullptr && blockIdx.x == (unsigned)a.stamp_block && (cond) && (i) < 128)  \
      a.stamp[(i)] = __builtin_amdgcn_s_memtime();                                          \
  } while (0)
#else
#define DSX_STAMP(i) do { } while (0)
#define DSX_STAMP_T(i, cond) do { } while (0)
#endif

template <typename DT> struct Chunk;
template <> struct Chunk<float> { static constexpr int KC = 16; };
template <> struct Chunk<__bf16> { static constexpr int KC = 32; };
template <> struct Chunk<_Float16> { static constexpr int KC = 32; };
// storage kind of an activation tensor as the host passes it (ConvArgs::act_bf16 / out_bf16): 0 fp32, 1 bf16, 2 fp16
template <typename DT> struct Kind;
template <> struct Kind<float> { static constexpr int value = 0; };
template <> struct Kind<__bf16> { static constexpr int value = 1; };
template <> struct Kind<_Float16> { static constexpr int value = 2; };

// Activations live in HBM in the MFMA operand type (fp32 or bf16); everything is staged in 16-byte units:
// Unit<DT>::N consecutive channels of one pixel (4 fp32 / 8 bf16), which is also 16 bytes of the LDS image.
template <typename DT> struct Unit;
template <> struct Unit<float> {
  static constexpr int N = 4;
  static __device__ __forceinline__ void unpack(const uint4 r, float (&v)[4]) {
    v[0] = __builtin_bit_cast(float, r.x); v[1] = __builtin_bit_cast(float, r.y);
    v[2] = __builtin_bit_cast(float, r.z); v[3] = __builtin_bit_cast(float, r.w);
  }
  static __device__ __forceinline__ uint4 pack(const float (&v)[4]) {
    return make_uint4(__builtin_bit_cast(unsigned, v[0]), __builtin_bit_cast(unsigned, v[1]),
                      __builtin_bit_cast(unsigned, v[2]), __builtin_bit_cast(unsigned, v[3]));
  }
};
template <> struct Unit<__bf16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const uint4 r, float (&v)[8]) {
    v[0] = __builtin_bit_cast(float, r.x << 16); v[1] = __builtin_bit_cast(float, r.x & 0xffff0000u);
    v[2] = __builtin_bit_cast(float, r.y << 16); v[3] = __builtin_bit_cast(float, r.y & 0xffff0000u);
    v[4] = __builtin_bit_cast(float, r.z << 16); v[5] = __builtin_bit_cast(float, r.z & 0xffff0000u);
    v[6] = __builtin_bit_cast(float, r.w << 16); v[7] = __builtin_bit_cast(float, r.w & 0xffff0000u);
  }
  static __device__ __forceinline__ uint4 pack(const float (&v)[8]) {
    return make_uint4(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]), pack_bf16x2(v[4], v[5]),
                      pack_bf16x2(v[6], v[7]));
  }
};
template <> struct Unit<_Float16> {
  static constexpr int N = 8;
  static __device__ __forceinline__ void unpack(const uint4 r, float (&v)[8]) {
    v[0] = f16_lo(r.x); v[1] = f16_hi(r.x); v[2] = f16_lo(r.y); v[3] = f16_hi(r.y);
    v[4] = f16_lo(r.z); v[5] = f16_hi(r.z); v[6] = f16_lo(r.w); v[7] = f16_hi(r.w);
  }
  static __device__ __forceinline__ uint4 pack(const float (&v)[8]) {
    return make_uint4(pack_f16x2(v[0], v[1]), pack_f16x2(v[2], v[3]), pack_f16x2(v[4], v[5]), pack_f16x2(v[6], v[7]));
  }
};
// one activation element -> float (scalar fallback paths)
template <typename DT> __device__ __forceinline__ float act_load(const void* p, size_t i) {
  if constexpr (Kind<DT>::value == 1) return __builtin_bit_cast(float, (unsigned)((const unsigned short*)p)[i] << 16);
  else if constexpr (Kind<DT>::value == 2) return (float)((const _Float16*)p)[i];
  else return ((const float*)p)[i];
}
__device__ __forceinline__ float act_load_kind(const void* p, size_t i, int kind) {
  return kind == 1 ? act_load<__bf16>(p, i) : (kind == 2 ? act_load<_Float16>(p, i) : act_load<float>(p, i));
}
// kind: 0 fp32, 1 bf16, 2 fp16
__device__ __forceinline__ void act_store(void* p, size_t i, float v, int kind) {
  if (kind == 1) {
    const __bf16 h = (__bf16)v;
    ((unsigned short*)p)[i] = __builtin_bit_cast(unsigned short, h);
  } else if (kind == 2) {
    ((_Float16*)p)[i] = (_Float16)v;
  } else {
    ((float*)p)[i] = v;
  }
}
// Accumulator layout of every conv kernel here (weights are the MFMA A operand, packed with permuted
// rows, see pack_conv): lane (li = lane & 31, lh = lane >> 5) holds pixel li of its row block, register r
// holds channel 16*lh + r of the wave's 32-channel block -> 16 consecutive channels per lane.
// x[16] -> out (+ optional 16-B vector stores); `n0` = first channel, `valid` = channels that exist
template <bool VEC>
__device__ __forceinline__ void store16(void* out, size_t elem, const float (&x)[16], int kind, int valid) {
  if (VEC) {
    if (kind == 1) {
      uint4* q = (uint4*)((unsigned short*)out + elem);
      q[0] = make_uint4(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7]));
      q[1] = make_uint4(pack_bf16x2(x[8], x[9]), pack_bf16x2(x[10], x[11]), pack_bf16x2(x[12], x[13]), pack_bf16x2(x[14], x[15]));
    } else if (kind == 2) {
      uint4* q = (uint4*)((unsigned short*)out + elem);
      q[0] = make_uint4(pack_f16x2(x[0], x[1]), pack_f16x2(x[2], x[3]), pack_f16x2(x[4], x[5]), pack_f16x2(x[6], x[7]));
      q[1] = make_uint4(pack_f16x2(x[8], x[9]), pack_f16x2(x[10], x[11]), pack_f16x2(x[12], x[13]), pack_f16x2(x[14], x[15]));
    } else {
      float4* q = (float4*)((float*)out + elem);
#pragma unroll
      for (int j = 0; j < 4; ++j) q[j] = make_float4(x[4 * j], x[4 * j + 1], x[4 * j + 2], x[4 * j + 3]);
    }
  } else {
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (r < valid) act_store(out, elem + r, x[r], kind);
  }
}

// LDS accesses of the loader waves go through inline asm: for a ds_read that may alias an LDS-DMA
// destination hipcc would insert s_waitcnt vmcnt(0) and drain the whole DMA ring; ordering is done by
// the counted vmcnt waits (wait_young) instead.
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
static __device__ __forceinline__ void lds_write_b128_asm(unsigned addr, f32x4_t w) {
  asm volatile("ds_write_b128 %0, %1" ::"v"(addr), "v"(w) : "memory");
}

static __device__ __forceinline__ void ws_barrier() {
  __builtin_amdgcn_s_waitcnt(0xC07F);  // lgkmcnt(0) only: own LDS writes visible, DMAs stay in flight
  __builtin_amdgcn_s_barrier();
}
template <int N> static __device__ __forceinline__ void wait_vmcnt() {
  static_assert(N >= 0 && N < 64, "vmcnt is 6 bits");
  __builtin_amdgcn_s_waitcnt((N & 0xF) | ((N >> 4) << 14) | 0x0F70);  // vmcnt(N) only
}


// compile-time loop: f(std::integral_constant<int, 0>) ... f(std::integral_constant<int, N-1>)
template <class F, int... I>
static __device__ __forceinline__ void static_for_impl(F&& f, std::integer_sequence<int, I...>) {
  (f(std::integral_constant<int, I>{}), ...);
}
template <int N, class F> static __device__ __forceinline__ void static_for(F&& f) {
  static_for_impl(f, std::make_integer_sequence<int, N>{});
}
// MFMA operand fragments of the compute waves are read with explicit ds_read_b128 + counted lgkmcnt waits,
// PF steps ahead of their MFMAs: left to itself the register-starved scheduler puts every read right before
// its use ("ds_read; s_waitcnt lgkmcnt(0); v_mfma"), which exposes the LDS latency on every MFMA.
template <int OFF> static __device__ __forceinline__ void lds_read_frag(f32x4_t& d, unsigned addr) {
  asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(d) : "v"(addr), "n"(OFF) : "memory");
}
static __device__ __forceinline__ void touch_frag(f32x4_t& d, unsigned addr) { asm volatile("" : "+v"(d) : "v"(addr)); }
template <int N> static __device__ __forceinline__ void wait_frags(f32x4_t& a) {
  asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(a) : "n"(N) : "memory");
}
template <int N> static __device__ __forceinline__ void wait_frags(f32x4_t& a, f32x4_t& b) {
  asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(a), "+v"(b) : "n"(N) : "memory");
}
template <int N> static __device__ __forceinline__ void wait_frags(f32x4_t& a, f32x4_t& b, f32x4_t& c, f32x4_t& d) {
  asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(a), "+v"(b), "+v"(c), "+v"(d) : "n"(N) : "memory");
}


// one 16-byte fragment pair on the matrix core in the operand type DT (weights = A, pixels = B)
template <typename DT>
__device__ __forceinline__ f32x16 mfma_step(const uint4 w, const f32x4_t px, f32x16 acc) {
  if constexpr (Kind<DT>::value == 1) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, px), acc, 0, 0, 0);
  } else if constexpr (Kind<DT>::value == 2) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, px), acc, 0, 0, 0);
  } else {
    const float4 af = __builtin_bit_cast(float4, px);
    const float4 bf = __builtin_bit_cast(float4, w);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.x, af.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.y, af.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(bf.z, af.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_32x32x2f32(bf.w, af.w, acc, 0, 0, 0);
  }
}

// k_conv_ws multiplies with the 16 x 16 MFMA shapes (v_mfma_f32_16x16x32_bf16 / _f16, 16x16x4 f32): the same FLOP per
// cycle, operand bytes and accumulator registers as 32x32x16, but the chip holds a higher clock under them
// (MI355X_MICROARCH.md, DVFS give-back 7; measured here with a probe build before the re-layout: every 3 x 3 launch
// -3.6 .. -4.2 %, the 2000-step loop -4.1 %, profiles/r03_ab_experiments.md).
//   A (weights): lane (i = lane & 15, kq = lane >> 4) = output channel row i, K slice kq (16 bytes);
//   B (pixels):  lane (c, kq) = pixel column c, K slice kq;   D: lane (c, kq), register j = row 4 kq + j of column c.
// The 16-byte K slice of a 64-byte chunk that lane group kq multiplies is slice ws16_slice(kq) = {0, 2, 1, 3}[kq] and
// column c is pixel ws16_pixel(c) of a 16-pixel block -- the b128 read groups of the LDS ({0-3,12-15,20-27}, ...) then
// pair 8 even pixels at one slice with the 8 odd pixels two slices on: 16 distinct 16-byte bank groups for the pixel
// pitches used here (80 / 144 bytes; the row pitches of conv_lds_row keep the parity).
// One fragment per lane pair (ch = 0, 1) covers a 32-channel N block: row i of fragment ch is channel
// 8 (i / 4) + 4 ch + i % 4, so a lane ends up with 8 consecutive channels 8 kq .. 8 kq + 7 of ONE pixel per 16-pixel
// block (registers 8 ph + 4 ch + j of the f32x16: ph = which half of the 32-pixel row block).
__host__ __device__ constexpr int ws16_slice(int kq) { return ((kq & 1) << 1) | (kq >> 1); }
__device__ __forceinline__ int ws16_pixel(int c) { return c < 4 ? 2 * c : (c < 12 ? 2 * (c - 4) + 1 : 2 * (c - 8)); }
// byte offset of lane (i, kq)'s 16 bytes of fragment ch inside the 2 KiB (tap, chunk) pair of pack_conv's stream
// ([half fs][lane (i_old, h)][16 B]: K slice s is half s / 2, lane half s % 2; channel 16 hh + 4 jj + q is row q + 8 jj + 4 hh)
__device__ __forceinline__ int ws16_woff(int lane, int ch) {
  const int i = lane & 15, sl = ws16_slice(lane >> 4);
  const int i_old = (i & 3) + 16 * ((i >> 2) & 1) + 8 * ch + 4 * (i >> 3);
  return (sl >> 1) * 1024 + ((sl & 1) * 32 + i_old) * 16;
}
template <typename DT>
__device__ __forceinline__ f32x4_t mfma16_step(const uint4 w, const f32x4_t px, f32x4_t acc) {
  if constexpr (Kind<DT>::value == 1) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, w), __builtin_bit_cast(bf16x8, px), acc, 0, 0, 0);
  } else if constexpr (Kind<DT>::value == 2) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, w), __builtin_bit_cast(f16x8, px), acc, 0, 0, 0);
  } else {
    const float4 af = __builtin_bit_cast(float4, px);
    const float4 bf = __builtin_bit_cast(float4, w);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bf.x, af.x, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bf.y, af.y, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(bf.z, af.z, acc, 0, 0, 0);
    return __builtin_amdgcn_mfma_f32_16x16x4f32(bf.w, af.w, acc, 0, 0, 0);
  }
}
// 8 per-lane registers -> the 16-lane DPP row's total of ONE register per lane: lane i ends up with register
// row8_fold_reg(i) summed over the row (three halving butterfly stages, then lane ^ 8): 7 + 1 adds
__device__ __forceinline__ float row8_fold(const float (&s)[8], int lane) {
  const bool b0 = lane & 1, b1 = lane & 2, b2 = lane & 4;
  float a4[4], a2[2];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const float keep = b0 ? s[k + 4] : s[k], send = b0 ? s[k] : s[k + 4];
    a4[k] = keep + dpp_take<0xB1, 0xF>(0.f, send);                       // lane ^ 1
  }
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const float keep = b1 ? a4[k + 2] : a4[k], send = b1 ? a4[k] : a4[k + 2];
    a2[k] = keep + dpp_take<0x4E, 0xF>(0.f, send);                       // lane ^ 2
  }
  const float keep = b2 ? a2[1] : a2[0], send = b2 ? a2[0] : a2[1];
  float t = dpp_take<0x104, 0x5>(0.f, send);                             // banks 0,2 <- lane + 4
  t = dpp_take<0x114, 0xA>(t, send);                                     // banks 1,3 <- lane - 4
  const float a1 = keep + t;
  return a1 + dpp_take<0x128, 0xF>(0.f, a1);                             // lane ^ 8 (row_ror:8)
}
__device__ __forceinline__ int row8_fold_reg(int lane) { return 4 * (lane & 1) + 2 * ((lane >> 1) & 1) + ((lane >> 2) & 1); }
// x[8] = 8 consecutive channels of one pixel -> out in the storage type (16-byte vector stores)
__device__ __forceinline__ void store8(void* out, size_t elem, const float (&x)[8], int kind) {
  if (kind == 1) {
    *(uint4*)((unsigned short*)out + elem) =
        make_uint4(pack_bf16x2(x[0], x[1]), pack_bf16x2(x[2], x[3]), pack_bf16x2(x[4], x[5]), pack_bf16x2(x[6], x[7]));
  } else if (kind == 2) {
    *(uint4*)((unsigned short*)out + elem) =
        make_uint4(pack_f16x2(x[0], x[1]), pack_f16x2(x[2], x[3]), pack_f16x2(x[4], x[5]), pack_f16x2(x[6], x[7]));
  } else {
    float4* q = (float4*)((float*)out + elem);
    q[0] = make_float4(x[0], x[1], x[2], x[3]);
    q[1] = make_float4(x[4], x[5], x[6], x[7]);
  }
}

}  // namespace dsx
