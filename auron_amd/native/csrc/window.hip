// Auron-AMD native engine — window frame kernels, gfx950 (MI355X, CDNA4) only.
//
// Two primitives behind "aggregate over an arbitrary per-row frame [a, b]":
//
//   au_window_range_bounds_{i64,f64}
//     RANGE frames with value offsets. One row per thread, grid-stride.
//     Row i owns an inclusive index window [slo[i], shi[i]] holding the
//     ordinary (non-null, non-NaN) keys of its partition; inside it the
//     keys are monotone (non-decreasing for ASC, non-increasing for DESC).
//     Two binary searches give
//       a[i] = first index whose key is inside the lower bound
//       b[i] = last  index whose key is inside the upper bound
//     with a[i] = shi+1 / b[i] = slo-1 when no key qualifies, so a > b
//     marks an empty frame. int64 key+offset saturates, float64 is IEEE.
//     Null/NaN rows and unbounded bounds are patched by the caller.
//
//   au_window_frame_minmax_{i64,f64}
//     Per-row min/max of x[a[i] .. b[i]] in O(126 * levels) loads whatever
//     the frame width, from a 64-ary aggregate pyramid: level 1 holds the
//     min/max of each aligned 64-element tile of x, level 2 of each 64
//     level-1 entries, ... until a level has <= 64 entries. A level with m
//     entries is followed by one with ceil(m/64); levels are stored back to
//     back in one caller-provided buffer (au_window_pyramid_size entries).
//     One wave64 reduces one tile with __shfl_xor. Floating NaN propagates
//     (torch.minimum / torch.maximum semantics).
//
// C ABI only — loaded via ctypes from auron_amd/native/__init__.py.
// All pointers are device pointers owned by torch; `stream` is the torch
// current stream. No allocation happens here.

#include <hip/hip_runtime.h>
#include <stdint.h>

#define AU_EXPORT extern "C" __attribute__((visibility("default")))

#define WN_TILE 64
#define WN_MAX_LEVELS 12  // ceil(63 / 6) + 1: enough for any int64 n

// same cap as rp_grid in rangepart.hip
static inline int wn_grid(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CU x 8 — grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// ------------------------------------------------------------ range bounds
#define WN_LO_UNBOUNDED 1
#define WN_HI_UNBOUNDED 2
#define WN_DESC 4

__device__ __forceinline__ int64_t wn_add(int64_t k, int64_t d) {
  int64_t r;
  if (__builtin_add_overflow(k, d, &r)) return d > 0 ? INT64_MAX : INT64_MIN;
  return r;
}
__device__ __forceinline__ int64_t wn_sub(int64_t k, int64_t d) {
  int64_t r;
  if (__builtin_sub_overflow(k, d, &r)) return d > 0 ? INT64_MIN : INT64_MAX;
  return r;
}
__device__ __forceinline__ double wn_add(double k, double d) { return k + d; }
__device__ __forceinline__ double wn_sub(double k, double d) { return k - d; }

template <typename T>
__global__ void k_window_range_bounds(const T* __restrict__ key,
                                      const int64_t* __restrict__ slo,
                                      const int64_t* __restrict__ shi,
                                      int64_t n, T lo_off, T hi_off, int flags,
                                      int64_t* __restrict__ a,
                                      int64_t* __restrict__ b) {
  const bool desc = (flags & WN_DESC) != 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t w0 = slo[i], w1 = shi[i];
    // never index outside the key array, whatever the caller passed
    if (w0 < 0) w0 = 0;
    if (w1 > n - 1) w1 = n - 1;
    const T k = key[i];
    int64_t ai = w0, bi = w1;
    if (!(flags & WN_LO_UNBOUNDED)) {
      // first j in [w0, w1] with key[j] >= k+lo (ASC) / key[j] <= k-lo (DESC)
      const T t = desc ? wn_sub(k, lo_off) : wn_add(k, lo_off);
      int64_t l = w0, h = w1 + 1;
      while (l < h) {
        const int64_t mid = l + ((h - l) >> 1);
        const T v = key[mid];
        const bool inside = desc ? (v <= t) : (v >= t);
        if (inside) h = mid;
        else l = mid + 1;
      }
      ai = l;
    }
    if (!(flags & WN_HI_UNBOUNDED)) {
      // last j in [w0, w1] with key[j] <= k+hi (ASC) / key[j] >= k-hi (DESC)
      const T t = desc ? wn_sub(k, hi_off) : wn_add(k, hi_off);
      int64_t l = w0, h = w1 + 1;
      while (l < h) {
        const int64_t mid = l + ((h - l) >> 1);
        const T v = key[mid];
        const bool inside = desc ? (v >= t) : (v <= t);
        if (inside) l = mid + 1;
        else h = mid;
      }
      bi = l - 1;
    }
    a[i] = ai;
    b[i] = bi;
  }
}

template <typename T>
static int wn_launch_bounds(const T* key, const int64_t* slo,
                            const int64_t* shi, int64_t n, T lo_off, T hi_off,
                            int flags, int64_t* a, int64_t* b, void* stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_window_range_bounds<T>, dim3(wn_grid(n, 256)),
                     dim3(256), 0, (hipStream_t)stream, key, slo, shi, n,
                     lo_off, hi_off, flags, a, b);
  return (int)hipGetLastError();
}

AU_EXPORT int au_window_range_bounds_i64(const int64_t* key,
                                         const int64_t* slo,
                                         const int64_t* shi, int64_t n,
                                         int64_t lo_off, int64_t hi_off,
                                         int flags, int64_t* a, int64_t* b,
                                         void* stream) {
  return wn_launch_bounds<int64_t>(key, slo, shi, n, lo_off, hi_off, flags, a,
                                   b, stream);
}

AU_EXPORT int au_window_range_bounds_f64(const double* key, const int64_t* slo,
                                         const int64_t* shi, int64_t n,
                                         double lo_off, double hi_off,
                                         int flags, int64_t* a, int64_t* b,
                                         void* stream) {
  return wn_launch_bounds<double>(key, slo, shi, n, lo_off, hi_off, flags, a,
                                  b, stream);
}

// ----------------------------------------------------------- frame min/max
template <typename T, bool IS_MAX>
struct WnOp;
template <bool IS_MAX>
struct WnOp<int64_t, IS_MAX> {
  static __host__ __device__ __forceinline__ int64_t identity() {
    return IS_MAX ? INT64_MIN : INT64_MAX;
  }
  static __device__ __forceinline__ int64_t combine(int64_t x, int64_t y) {
    return IS_MAX ? (x > y ? x : y) : (x < y ? x : y);
  }
  static __device__ __forceinline__ int64_t shfl_xor(int64_t v, int m) {
    return (int64_t)__shfl_xor((long long)v, m, WN_TILE);
  }
};
template <bool IS_MAX>
struct WnOp<double, IS_MAX> {
  static __host__ __device__ __forceinline__ double identity() {
    return IS_MAX ? -__builtin_huge_val() : __builtin_huge_val();
  }
  // NaN on either side wins, like torch.minimum / torch.maximum
  static __device__ __forceinline__ double combine(double x, double y) {
    if (x != x) return x;
    if (y != y) return y;
    return IS_MAX ? (x > y ? x : y) : (x < y ? x : y);
  }
  static __device__ __forceinline__ double shfl_xor(double v, int m) {
    return __shfl_xor(v, m, WN_TILE);
  }
};

// Number of pyramid entries above an n-element base (levels >= 1).
static inline int64_t wn_pyramid_size(int64_t n) {
  int64_t total = 0;
  while (n > WN_TILE) {
    n = (n + WN_TILE - 1) / WN_TILE;
    total += n;
  }
  return total;
}

AU_EXPORT int64_t au_window_pyramid_size(int64_t n) {
  return wn_pyramid_size(n);
}

// One wave64 per tile of the level below: dst[t] = op(src[64t .. 64t+63]),
// entries past m read as the identity. The tile loop is wave-uniform, so
// all 64 lanes reach every shuffle.
template <typename T, bool IS_MAX>
__global__ void k_window_pyramid_level(const T* __restrict__ src, int64_t m,
                                       T* __restrict__ dst, int64_t tiles) {
  typedef WnOp<T, IS_MAX> Op;
  const int lane = threadIdx.x & (WN_TILE - 1);
  const int64_t waves_per_block = blockDim.x / WN_TILE;
  const int64_t wave = (int64_t)blockIdx.x * waves_per_block +
                       threadIdx.x / WN_TILE;
  const int64_t nwaves = (int64_t)gridDim.x * waves_per_block;
  for (int64_t t = wave; t < tiles; t += nwaves) {
    const int64_t j = t * WN_TILE + lane;
    T v = j < m ? src[j] : Op::identity();
#pragma unroll
    for (int s = WN_TILE / 2; s >= 1; s >>= 1)
      v = Op::combine(v, Op::shfl_xor(v, s));
    if (lane == 0) dst[t] = v;
  }
}

template <typename T, bool IS_MAX>
static int wn_build(const T* x, int64_t n, T* pyr, void* stream) {
  const T* src = x;
  int64_t m = n;
  T* dst = pyr;
  while (m > WN_TILE) {
    const int64_t tiles = (m + WN_TILE - 1) / WN_TILE;
    // 4 waves (tiles) per 256-thread block
    hipLaunchKernelGGL((k_window_pyramid_level<T, IS_MAX>),
                       dim3(wn_grid(tiles * WN_TILE, 256)), dim3(256), 0,
                       (hipStream_t)stream, src, m, dst, tiles);
    const int rc = (int)hipGetLastError();
    if (rc) return rc;
    src = dst;
    dst += tiles;
    m = tiles;
  }
  return 0;
}

// Level table passed by value: level 0 is x itself, level l >= 1 starts at
// pyr + off[l].
struct WnLevels {
  int nlevels;
  int64_t off[WN_MAX_LEVELS];
};

template <typename T, bool IS_MAX>
__global__ void k_window_frame_minmax(const T* __restrict__ x,
                                      const T* __restrict__ pyr, WnLevels lv,
                                      const int64_t* __restrict__ a,
                                      const int64_t* __restrict__ b, int64_t n,
                                      int64_t rows, T* __restrict__ out) {
  typedef WnOp<T, IS_MAX> Op;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = a[i], hi = b[i];
    // never index outside x, whatever the caller passed
    if (lo < 0) lo = 0;
    if (hi > n - 1) hi = n - 1;
    T acc = Op::identity();
    const T* cur = x;
    int l = 0;
    while (lo <= hi) {
      if (hi - lo < 2 * WN_TILE || l + 1 >= lv.nlevels) {
        // narrow (or top level, <= 64 entries above level 0): scan
        for (int64_t j = lo; j <= hi; j++) acc = Op::combine(acc, cur[j]);
        break;
      }
      // <= 63 leading entries up to the next tile edge
      const int64_t lo_al = (lo + WN_TILE - 1) & ~(int64_t)(WN_TILE - 1);
      for (int64_t j = lo; j < lo_al; j++) acc = Op::combine(acc, cur[j]);
      // <= 63 trailing entries after the last whole tile
      const int64_t hi_al = (hi + 1) & ~(int64_t)(WN_TILE - 1);
      for (int64_t j = hi_al; j <= hi; j++) acc = Op::combine(acc, cur[j]);
      // whole aligned tiles [lo_al, hi_al) continue one level up
      lo = lo_al / WN_TILE;
      hi = hi_al / WN_TILE - 1;
      l++;
      cur = pyr + lv.off[l];
    }
    out[i] = acc;
  }
}

template <typename T, bool IS_MAX>
static int wn_query(const T* x, int64_t n, const T* pyr, const int64_t* a,
                    const int64_t* b, int64_t rows, T* out, void* stream) {
  WnLevels lv;
  lv.nlevels = 1;
  lv.off[0] = 0;
  int64_t m = n, off = 0;
  while (m > WN_TILE && lv.nlevels < WN_MAX_LEVELS) {
    m = (m + WN_TILE - 1) / WN_TILE;
    lv.off[lv.nlevels] = off;
    off += m;
    lv.nlevels++;
  }
  hipLaunchKernelGGL((k_window_frame_minmax<T, IS_MAX>),
                     dim3(wn_grid(rows, 256)), dim3(256), 0,
                     (hipStream_t)stream, x, pyr, lv, a, b, n, rows, out);
  return (int)hipGetLastError();
}

template <typename T>
static int wn_frame_minmax(const T* x, int64_t n, T* pyr, int64_t pyr_len,
                           const int64_t* a, const int64_t* b, int64_t rows,
                           int is_max, T* out, void* stream) {
  if (rows <= 0) return 0;
  if (n <= 0) return (int)hipErrorInvalidValue;
  if (pyr_len < wn_pyramid_size(n)) return (int)hipErrorInvalidValue;
  int rc = is_max ? wn_build<T, true>(x, n, pyr, stream)
                  : wn_build<T, false>(x, n, pyr, stream);
  if (rc) return rc;
  return is_max ? wn_query<T, true>(x, n, pyr, a, b, rows, out, stream)
                : wn_query<T, false>(x, n, pyr, a, b, rows, out, stream);
}

// out[i] = min|max of x[a[i] .. b[i]] for i < rows; a[i] > b[i] gives the
// identity. `pyr` is scratch of at least au_window_pyramid_size(n) entries,
// built here and then queried on the same stream.
AU_EXPORT int au_window_frame_minmax_i64(const int64_t* x, int64_t n,
                                         int64_t* pyr, int64_t pyr_len,
                                         const int64_t* a, const int64_t* b,
                                         int64_t rows, int is_max,
                                         int64_t* out, void* stream) {
  return wn_frame_minmax<int64_t>(x, n, pyr, pyr_len, a, b, rows, is_max, out,
                                  stream);
}

AU_EXPORT int au_window_frame_minmax_f64(const double* x, int64_t n,
                                         double* pyr, int64_t pyr_len,
                                         const int64_t* a, const int64_t* b,
                                         int64_t rows, int is_max, double* out,
                                         void* stream) {
  return wn_frame_minmax<double>(x, n, pyr, pyr_len, a, b, rows, is_max, out,
                                 stream);
}
