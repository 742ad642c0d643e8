// dsx_select.hip — what the frame statistics of compute_normalization_dict (data/split_dataset.py:29-74) need on
// gfx950 without a sort: k_select_hist, one pass of a most-significant-digit radix select over the order-preserving
// integer image of a float64 key, and k_widen, the integer frame stacks of the .tif files widened to fp32.
#include "dsx_kernels.h"

namespace dsx {

// ---------------------------------------------------------------------------
// The key of element i: (double)a[i], or with a second source (double)a[i] * w0 + (double)b[i] * w1 with both products
// and the sum rounded on their own (numpy's t1 * w0 + t2 * w1 on float64 arrays; never an fma).  Its image
// u = bits ^ (sign ? ~0 : 1 << 63) orders as the keys do (-0.0 directly below +0.0; NaN is not defined).
// One pass counts, over the elements whose image agrees with `prefix` above bit `shift + bits`, the digit
// (u >> shift) & (2^bits - 1): per-workgroup LDS counters, merged into the 64-bit global counters with one atomic per
// non-empty bin.  A wave whose active lanes all hold one digit -- ties: the background value, the clip value, and in
// the upper passes nearly everything -- adds its lane count once.  The LDS counters are 32 bits wide and are flushed
// after kSelFlushIters iterations of at most 1024 elements each, so they cannot wrap for any count.
// ---------------------------------------------------------------------------
constexpr int kSelFlushIters = 1 << 21;   // * 256 threads * 4 elements = 2^31 increments per counter at most

__device__ __forceinline__ unsigned long long sel_image(double key) {
  const unsigned long long bits = (unsigned long long)__double_as_longlong(key);
  return bits ^ ((bits >> 63) ? ~0ull : 0x8000000000000000ull);
}
template <bool PAIR>
__device__ __forceinline__ unsigned long long sel_key(float a, float b, double w0, double w1) {
  if (!PAIR) return sel_image((double)a);
  return sel_image(add_d(mul_d((double)a, w0), mul_d((double)b, w1)));
}
__device__ __forceinline__ void sel_count(unsigned* hist, bool valid, unsigned digit) {
  const unsigned long long act = __ballot(valid);
  if (act == 0) return;
  const int first = __ffsll((long long)act) - 1;
  const unsigned d0 = (unsigned)__shfl((int)digit, first);
  const unsigned long long same = __ballot(valid && digit == d0);
  if (same == act) {
    if ((int)(threadIdx.x & 63) == first) atomicAdd(&hist[d0], (unsigned)__popcll(act));
  } else if (valid) {
    atomicAdd(&hist[digit], 1u);
  }
}
__device__ __forceinline__ void sel_flush(unsigned* hist, unsigned long long* out, int bins) {
  __syncthreads();
  for (int i = threadIdx.x; i < bins; i += 256) {
    const unsigned c = hist[i];
    if (c) atomicAdd(&out[i], (unsigned long long)c);
    hist[i] = 0;
  }
  __syncthreads();
}

template <bool PAIR, bool VEC>
__global__ __launch_bounds__(256) void k_select_hist(const SelectArgs s) {
  __shared__ unsigned hist[kSelectBins];
  const int bins = 1 << s.bits;
  for (int i = threadIdx.x; i < bins; i += 256) hist[i] = 0;
  __syncthreads();
  const unsigned mask = (unsigned)bins - 1u;
  const bool all = s.match_shift >= 64;                    // first pass: no prefix yet
  // groups of 4 elements under VEC (16-byte loads from aligned bases), single elements otherwise
  const long long per = VEC ? 4 : 1;
  const long long groups = VEC ? s.count / 4 : s.count;
  const long long stride = (long long)gridDim.x * 256;
  const long long rounds = (groups + stride - 1) / stride;  // the same for every thread: the ballots stay whole
  int since = 0;
  for (long long r = 0; r < rounds; ++r) {
    const long long g = r * stride + (long long)blockIdx.x * 256 + threadIdx.x;
    const bool valid = g < groups;
    float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f};
    if (valid) {
      if (VEC) {
        const float4 va = *reinterpret_cast<const float4*>(s.a + g * 4);
        a[0] = va.x; a[1] = va.y; a[2] = va.z; a[3] = va.w;
        if (PAIR) {
          const float4 vb = *reinterpret_cast<const float4*>(s.b + g * 4);
          b[0] = vb.x; b[1] = vb.y; b[2] = vb.z; b[3] = vb.w;
        }
      } else {
        a[0] = s.a[g];
        if (PAIR) b[0] = s.b[g];
      }
    }
#pragma unroll
    for (int j = 0; j < (VEC ? 4 : 1); ++j) {
      const unsigned long long u = sel_key<PAIR>(a[j], b[j], s.w0, s.w1);
      const bool hit = valid && (all || (u >> s.match_shift) == s.prefix);
      sel_count(hist, hit, (unsigned)(u >> s.shift) & mask);
    }
    if (++since == kSelFlushIters) { sel_flush(hist, s.hist, bins); since = 0; }
  }
  // the ragged tail of the vector form: the last count % 4 elements, by the first threads of workgroup 0
  if (VEC && blockIdx.x == 0) {
    const long long i = groups * per + threadIdx.x;
    const bool valid = threadIdx.x < 4 && i < s.count;
    const float ta = valid ? s.a[i] : 0.f;
    const float tb = valid && PAIR ? s.b[i] : 0.f;
    const unsigned long long u = sel_key<PAIR>(ta, tb, s.w0, s.w1);
    const bool hit = valid && (all || (u >> s.match_shift) == s.prefix);
    sel_count(hist, hit, (unsigned)(u >> s.shift) & mask);
  }
  sel_flush(hist, s.hist, bins);
}

int select_blocks(long long count) {
  const long long want = (count + 4095) / 4096;             // ~16 elements per thread before the grid stops growing
  return (int)(want < 1 ? 1 : want > kSelectMaxBlocks ? kSelectMaxBlocks : want);
}
hipError_t launch_select_hist(const SelectArgs& s, hipStream_t st) {
  const bool pair = s.b != nullptr;
  const bool vec = aligned16(s.a, s.b);
  const dim3 grid((unsigned)select_blocks(s.count)), block(256);
  void (*kernel)(const SelectArgs) = pair ? (vec ? k_select_hist<true, true> : k_select_hist<true, false>)
                                          : (vec ? k_select_hist<false, true> : k_select_hist<false, false>);
  hipLaunchKernelGGL(kernel, grid, block, 0, st, s);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------
// k_widen: dst[i] = (float)min((double)src[i], clip) for uint8 / uint16 sources (clip < 0: none) -- the reference's
// data[data > 1993.0] = 1993.0 (data/split_dataset.py:80-82) and the cast to fp32, on the stack in its file width.
// A thread takes 8 consecutive elements: one 16-byte (uint16) or 8-byte (uint8) load, two 16-byte stores; the last
// count % 8 elements go one by one.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float widen_one(unsigned v, double clip) {
  const double d = (double)v;
  return (float)(clip >= 0.0 && d > clip ? clip : d);
}
template <class T, bool VEC>
__global__ __launch_bounds__(256) void k_widen(const T* __restrict__ src, long long count, double clip, float* __restrict__ dst) {
  const long long stride = (long long)gridDim.x * 256;
  const long long t0 = (long long)blockIdx.x * 256 + threadIdx.x;
  if (VEC) {
    const long long groups = count / 8;
    for (long long g = t0; g < groups; g += stride) {
      alignas(16) T v[8];
      if constexpr (sizeof(T) == 2) *reinterpret_cast<uint4*>(v) = *reinterpret_cast<const uint4*>(src + g * 8);
      else *reinterpret_cast<uint2*>(v) = *reinterpret_cast<const uint2*>(src + g * 8);
      float4 lo, hi;
      lo.x = widen_one(v[0], clip); lo.y = widen_one(v[1], clip); lo.z = widen_one(v[2], clip); lo.w = widen_one(v[3], clip);
      hi.x = widen_one(v[4], clip); hi.y = widen_one(v[5], clip); hi.z = widen_one(v[6], clip); hi.w = widen_one(v[7], clip);
      *reinterpret_cast<float4*>(dst + g * 8) = lo;
      *reinterpret_cast<float4*>(dst + g * 8 + 4) = hi;
    }
    for (long long i = groups * 8 + t0; i < count; i += stride) dst[i] = widen_one(src[i], clip);
  } else {
    for (long long i = t0; i < count; i += stride) dst[i] = widen_one(src[i], clip);
  }
}

hipError_t launch_widen(const void* src, int src_bytes, long long count, double clip, float* dst, hipStream_t st) {
  const long long want = (count / 8 + 255) / 256;
  const dim3 grid((unsigned)(want < 1 ? 1 : want > 8192 ? 8192 : want)), block(256);
  const bool vec = (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0;
  if (src_bytes == 2) {
    const unsigned short* p = (const unsigned short*)src;
    void (*kernel)(const unsigned short*, long long, double, float*) = vec ? k_widen<unsigned short, true> : k_widen<unsigned short, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, p, count, clip, dst);
  } else {
    const unsigned char* p = (const unsigned char*)src;
    void (*kernel)(const unsigned char*, long long, double, float*) = vec ? k_widen<unsigned char, true> : k_widen<unsigned char, false>;
    hipLaunchKernelGGL(kernel, grid, block, 0, st, p, count, clip, dst);
  }
  return hipGetLastError();
}

}  // namespace dsx
