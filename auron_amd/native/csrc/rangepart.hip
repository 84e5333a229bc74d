// Auron-AMD native engine — range-bucket kernels, gfx950 (MI355X, CDNA4) only.
//
// "Which range bucket does this row fall in" for keys torch.searchsorted
// cannot compare: UTF-8 strings (Arrow bytes + int64 offsets) and
// decimal128 (two int64 limbs). One row per thread, grid-stride; each row
// binary-searches the B sorted bounds. The bounds are a few KB read by
// every lane, so they stay cache-resident and are read straight from
// global memory.
//
// Semantics are torch.searchsorted(bounds, key, right=...):
//   right == 0 -> number of bounds strictly less than the row
//   right != 0 -> number of bounds <= the row
//
// C ABI only — loaded via ctypes from auron_amd/native/__init__.py.
// All pointers are device pointers owned by torch; `stream` is the torch
// current stream. No allocation happens here.

#include <hip/hip_runtime.h>
#include <stdint.h>

#define AU_EXPORT extern "C" __attribute__((visibility("default")))

// same cap as au_grid in kernels.hip
static inline int rp_grid(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CU x 8 — grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// Unsigned-byte lexicographic compare (UTF-8 binary collation); a proper
// prefix sorts before the longer string. Returns <0, 0, >0.
// Eight bytes at a time over the common length: load, and on the first
// differing word byte-swap to big-endian so the uint64 compare orders by
// the first differing byte. The word loop runs only while a full 8 bytes
// remain in BOTH operands; the tail is a byte loop, so no byte outside
// [a, a+la) or [b, b+lb) is ever touched.
__device__ __forceinline__ int rp_cmp_bytes(const uint8_t* __restrict__ a,
                                            int64_t la,
                                            const uint8_t* __restrict__ b,
                                            int64_t lb) {
  const int64_t m = la < lb ? la : lb;
  int64_t j = 0;
  for (; j + 8 <= m; j += 8) {
    uint64_t x, y;
    __builtin_memcpy(&x, a + j, 8);
    __builtin_memcpy(&y, b + j, 8);
    if (x != y) {
      x = __builtin_bswap64(x);
      y = __builtin_bswap64(y);
      return x < y ? -1 : 1;
    }
  }
  for (; j < m; j++) {
    const uint8_t x = a[j], y = b[j];
    if (x != y) return x < y ? -1 : 1;
  }
  return la < lb ? -1 : (la > lb ? 1 : 0);
}

__global__ void k_range_bucket_str(const uint8_t* __restrict__ bytes,
                                   const int64_t* __restrict__ offsets,
                                   int64_t n,
                                   const uint8_t* __restrict__ b_bytes,
                                   const int64_t* __restrict__ b_offsets,
                                   int32_t B, int right,
                                   int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r0 = offsets[i];
    const int64_t rl = offsets[i + 1] - r0;
    const uint8_t* row = bytes + r0;
    int32_t lo = 0, hi = B;
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      const int64_t b0 = b_offsets[mid];
      const int c = rp_cmp_bytes(b_bytes + b0, b_offsets[mid + 1] - b0,
                                 row, rl);
      // bound < row (left) / bound <= row (right): the answer is past mid
      if (right ? (c <= 0) : (c < 0)) lo = mid + 1;
      else hi = mid;
    }
    out[i] = lo;
  }
}

// decimal128 layout: [:,0] low limb (bit pattern, unsigned order),
// [:,1] high limb (signed).
__global__ void k_range_bucket_i128(const int64_t* __restrict__ data,
                                    int64_t n,
                                    const int64_t* __restrict__ bounds,
                                    int32_t B, int right,
                                    int32_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    const uint64_t rlo = (uint64_t)data[2 * i];
    const int64_t rhi = data[2 * i + 1];
    int32_t lo = 0, hi = B;
    while (lo < hi) {
      const int32_t mid = lo + ((hi - lo) >> 1);
      const uint64_t blo = (uint64_t)bounds[2 * (int64_t)mid];
      const int64_t bhi = bounds[2 * (int64_t)mid + 1];
      const bool lt = bhi < rhi || (bhi == rhi && blo < rlo);
      const bool eq = bhi == rhi && blo == rlo;
      if (lt || (right && eq)) lo = mid + 1;
      else hi = mid;
    }
    out[i] = lo;
  }
}

AU_EXPORT int au_range_bucket_str(const uint8_t* bytes, const int64_t* offsets,
                                  int64_t n, const uint8_t* b_bytes,
                                  const int64_t* b_offsets, int32_t B,
                                  int right, int32_t* out, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_range_bucket_str, dim3(rp_grid(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, bytes, offsets, n, b_bytes,
                     b_offsets, B, right, out);
  return (int)hipGetLastError();
}

AU_EXPORT int au_range_bucket_i128(const int64_t* data, int64_t n,
                                   const int64_t* bounds, int32_t B, int right,
                                   int32_t* out, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_range_bucket_i128, dim3(rp_grid(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, data, n, bounds, B, right, out);
  return (int)hipGetLastError();
}
