// Auron-AMD native engine — window frame kernels, gfx950 (MI355X, CDNA4) only.
//
// The primitives behind "aggregate over an arbitrary per-row frame [a, b]":
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
//   au_prefix_sum_i128 / au_window_frame_sum_i128 / au_window_frame_minmax_i128
//     The same frame aggregates over 128-bit integers (decimal128 backing:
//     [lo bit pattern, hi signed] int64 pairs, row-major [n,2]). Sums are a
//     difference of two entries of one unsegmented inclusive prefix sum
//     modulo 2^128 — wrapped prefixes cancel in the difference — built in
//     three launches (tile totals, one-block scan of the totals, per-tile
//     rescan) so no workgroup ever waits on another. Min/max instantiate
//     the pyramid above for the limb pair.
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

// ===================================================== 128-bit frame kernels
// One decimal128 value. 16-byte aligned so a load/store is one dwordx4.
struct alignas(16) WnI128 {
  uint64_t lo;  // low 64 bits, bit pattern
  int64_t hi;   // high 64 bits, signed
};

__device__ __forceinline__ WnI128 wn_add128(WnI128 x, WnI128 y) {
  WnI128 r;
  r.lo = x.lo + y.lo;
  r.hi = (int64_t)((uint64_t)x.hi + (uint64_t)y.hi + (r.lo < x.lo ? 1u : 0u));
  return r;
}
__device__ __forceinline__ WnI128 wn_sub128(WnI128 x, WnI128 y) {
  WnI128 r;
  r.lo = x.lo - y.lo;
  r.hi = (int64_t)((uint64_t)x.hi - (uint64_t)y.hi - (x.lo < y.lo ? 1u : 0u));
  return r;
}
__device__ __forceinline__ WnI128 wn_zero128() {
  WnI128 r;
  r.lo = 0;
  r.hi = 0;
  return r;
}
__device__ __forceinline__ WnI128 wn_shfl_up128(WnI128 v, int d) {
  WnI128 r;
  r.lo = (uint64_t)__shfl_up((unsigned long long)v.lo, d, WN_TILE);
  r.hi = (int64_t)__shfl_up((long long)v.hi, d, WN_TILE);
  return r;
}

// ------------------------------------------------------------- prefix sum
#define WN_SCAN_BLOCK 256
#define WN_SCAN_ITEMS 4  // consecutive elements per thread
#define WN_SCAN_TILE (WN_SCAN_BLOCK * WN_SCAN_ITEMS)
#define WN_SCAN_WAVES (WN_SCAN_BLOCK / WN_TILE)

AU_EXPORT int64_t au_i128_scan_tile() { return WN_SCAN_TILE; }

// Inclusive scan of one value per thread over a 256-thread block: wave64
// scan with __shfl_up (every lane reaches every shuffle; only the add is
// predicated), wave totals through LDS. Returns the inclusive prefix and
// the block total. Every thread of the block must call it; `wtot` may be
// reused after the call (barrier at both ends).
__device__ __forceinline__ WnI128 wn_block_scan128(WnI128 v, WnI128* wtot,
                                                   WnI128* block_total) {
  const int lane = threadIdx.x & (WN_TILE - 1);
  const int wave = threadIdx.x / WN_TILE;
#pragma unroll
  for (int d = 1; d < WN_TILE; d <<= 1) {
    const WnI128 up = wn_shfl_up128(v, d);
    const WnI128 s = wn_add128(v, up);
    if (lane >= d) v = s;
  }
  __syncthreads();  // earlier readers of wtot are done
  if (lane == WN_TILE - 1) wtot[wave] = v;
  __syncthreads();
  WnI128 off = wn_zero128(), tot = wn_zero128();
#pragma unroll
  for (int w = 0; w < WN_SCAN_WAVES; w++) {
    const WnI128 t = wtot[w];
    if (w < wave) off = wn_add128(off, t);
    tot = wn_add128(tot, t);
  }
  *block_total = tot;
  return wn_add128(v, off);
}

// Loads the thread's WN_SCAN_ITEMS consecutive elements of tile `t`; rows
// past n or with valid[i] == 0 read as zero.
__device__ __forceinline__ void wn_scan_load(const WnI128* __restrict__ x,
                                             const uint8_t* __restrict__ valid,
                                             int64_t n, int64_t t,
                                             WnI128 v[WN_SCAN_ITEMS]) {
  const int64_t base = t * WN_SCAN_TILE + (int64_t)threadIdx.x * WN_SCAN_ITEMS;
#pragma unroll
  for (int k = 0; k < WN_SCAN_ITEMS; k++) {
    const int64_t i = base + k;
    v[k] = wn_zero128();
    if (i < n && (valid == nullptr || valid[i] != 0)) v[k] = x[i];
  }
}

// pass 1: totals[t] = sum of tile t
__global__ void __launch_bounds__(WN_SCAN_BLOCK)
k_i128_tile_totals(const WnI128* __restrict__ x,
                   const uint8_t* __restrict__ valid, int64_t n,
                   int64_t tiles, WnI128* __restrict__ totals) {
  __shared__ WnI128 wtot[WN_SCAN_WAVES];
  const int lane = threadIdx.x & (WN_TILE - 1);
  const int wave = threadIdx.x / WN_TILE;
  // block-uniform loop: all 256 threads reach every shuffle and barrier
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
    WnI128 v[WN_SCAN_ITEMS];
    wn_scan_load(x, valid, n, t, v);
    WnI128 s = v[0];
#pragma unroll
    for (int k = 1; k < WN_SCAN_ITEMS; k++) s = wn_add128(s, v[k]);
#pragma unroll
    for (int d = WN_TILE / 2; d >= 1; d >>= 1) {
      WnI128 o;
      o.lo = (uint64_t)__shfl_xor((unsigned long long)s.lo, d, WN_TILE);
      o.hi = (int64_t)__shfl_xor((long long)s.hi, d, WN_TILE);
      s = wn_add128(s, o);
    }
    __syncthreads();  // the previous tile's reader is done
    if (lane == 0) wtot[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      WnI128 tot = wtot[0];
#pragma unroll
      for (int w = 1; w < WN_SCAN_WAVES; w++) tot = wn_add128(tot, wtot[w]);
      totals[t] = tot;
    }
  }
}

// pass 2 (one block): totals[t] <- sum of totals[0 .. t-1], in place,
// 256 tiles per round with a running carry
__global__ void __launch_bounds__(WN_SCAN_BLOCK)
k_i128_scan_totals(WnI128* __restrict__ totals, int64_t tiles) {
  __shared__ WnI128 wtot[WN_SCAN_WAVES];
  WnI128 carry = wn_zero128();
  for (int64_t c = 0; c < tiles; c += WN_SCAN_BLOCK) {  // block-uniform
    const int64_t t = c + threadIdx.x;
    const WnI128 own = t < tiles ? totals[t] : wn_zero128();
    WnI128 round_total;
    const WnI128 incl = wn_block_scan128(own, wtot, &round_total);
    if (t < tiles) totals[t] = wn_add128(carry, wn_sub128(incl, own));
    carry = wn_add128(carry, round_total);
  }
}

// pass 3: out[i] = offsets[tile(i)] + inclusive prefix inside the tile
__global__ void __launch_bounds__(WN_SCAN_BLOCK)
k_i128_tile_rescan(const WnI128* __restrict__ x,
                   const uint8_t* __restrict__ valid, int64_t n,
                   int64_t tiles, const WnI128* __restrict__ offsets,
                   WnI128* __restrict__ out) {
  __shared__ WnI128 wtot[WN_SCAN_WAVES];
  for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {  // block-uniform
    WnI128 v[WN_SCAN_ITEMS];
    wn_scan_load(x, valid, n, t, v);
#pragma unroll
    for (int k = 1; k < WN_SCAN_ITEMS; k++) v[k] = wn_add128(v[k], v[k - 1]);
    const WnI128 own = v[WN_SCAN_ITEMS - 1];
    WnI128 tile_total;
    const WnI128 incl = wn_block_scan128(own, wtot, &tile_total);
    const WnI128 excl = wn_add128(offsets[t], wn_sub128(incl, own));
    const int64_t base =
        t * WN_SCAN_TILE + (int64_t)threadIdx.x * WN_SCAN_ITEMS;
#pragma unroll
    for (int k = 0; k < WN_SCAN_ITEMS; k++)
      if (base + k < n) out[base + k] = wn_add128(excl, v[k]);
  }
}

static inline int wn_tile_grid(int64_t tiles) {
  return (int)(tiles > 2048 ? 2048 : tiles);
}

// out[i] = (x[0] + ... + x[i]) mod 2^128 over [n,2] limb pairs; a row with
// valid[i] == 0 adds zero (valid == NULL: every row counts). tile_scratch
// holds ceil(n / au_i128_scan_tile()) limb pairs. out may not alias x.
AU_EXPORT int au_prefix_sum_i128(const int64_t* x, const uint8_t* valid,
                                 int64_t n, int64_t* out,
                                 int64_t* tile_scratch, void* stream) {
  if (n <= 0) return 0;
  if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)tile_scratch) & 15)
    return (int)hipErrorInvalidValue;
  const int64_t tiles = (n + WN_SCAN_TILE - 1) / WN_SCAN_TILE;
  const WnI128* xv = (const WnI128*)x;
  WnI128* tot = (WnI128*)tile_scratch;
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(k_i128_tile_totals, dim3(wn_tile_grid(tiles)),
                     dim3(WN_SCAN_BLOCK), 0, s, xv, valid, n, tiles, tot);
  int rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(k_i128_scan_totals, dim3(1), dim3(WN_SCAN_BLOCK), 0, s,
                     tot, tiles);
  rc = (int)hipGetLastError();
  if (rc) return rc;
  hipLaunchKernelGGL(k_i128_tile_rescan, dim3(wn_tile_grid(tiles)),
                     dim3(WN_SCAN_BLOCK), 0, s, xv, valid, n, tiles,
                     (const WnI128*)tot, (WnI128*)out);
  return (int)hipGetLastError();
}

// --------------------------------------------------------------- frame sum
__global__ void k_window_frame_sum_i128(const WnI128* __restrict__ P,
                                        int64_t n,
                                        const int64_t* __restrict__ a,
                                        const int64_t* __restrict__ b,
                                        int64_t rows,
                                        WnI128* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < rows;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t lo = a[i], hi = b[i];
    // never index outside P, whatever the caller passed
    if (lo < 0) lo = 0;
    if (hi > n - 1) hi = n - 1;
    WnI128 r = wn_zero128();
    if (lo <= hi) {
      r = P[hi];
      if (lo > 0) r = wn_sub128(r, P[lo - 1]);
    }
    out[i] = r;
  }
}

// out[i] = P[b[i]] - (a[i] > 0 ? P[a[i]-1] : 0) mod 2^128 for i < rows, zero
// when a[i] > b[i]; P is the [n,2] inclusive prefix sum. Frames are clamped
// to [0, n-1] like au_window_frame_minmax.
AU_EXPORT int au_window_frame_sum_i128(const int64_t* P, int64_t n,
                                       const int64_t* a, const int64_t* b,
                                       int64_t rows, int64_t* out,
                                       void* stream) {
  if (rows <= 0) return 0;
  if (((uintptr_t)P | (uintptr_t)out) & 15) return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_window_frame_sum_i128, dim3(wn_grid(rows, 256)),
                     dim3(256), 0, (hipStream_t)stream, (const WnI128*)P, n,
                     a, b, rows, (WnI128*)out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------ frame min/max
// Order: signed hi first, then unsigned lo.
template <bool IS_MAX>
struct WnOp<WnI128, IS_MAX> {
  static __host__ __device__ __forceinline__ WnI128 identity() {
    WnI128 r;  // min: 2^127 - 1, max: -2^127
    r.lo = IS_MAX ? 0 : ~(uint64_t)0;
    r.hi = IS_MAX ? INT64_MIN : INT64_MAX;
    return r;
  }
  static __device__ __forceinline__ bool less(WnI128 x, WnI128 y) {
    return x.hi < y.hi || (x.hi == y.hi && x.lo < y.lo);
  }
  static __device__ __forceinline__ WnI128 combine(WnI128 x, WnI128 y) {
    return (IS_MAX ? less(x, y) : less(y, x)) ? y : x;
  }
  static __device__ __forceinline__ WnI128 shfl_xor(WnI128 v, int m) {
    WnI128 r;
    r.lo = (uint64_t)__shfl_xor((unsigned long long)v.lo, m, WN_TILE);
    r.hi = (int64_t)__shfl_xor((long long)v.hi, m, WN_TILE);
    return r;
  }
};

// As au_window_frame_minmax_i64 over [n,2] limb pairs; `pyr` is scratch of
// at least au_window_pyramid_size(n) pairs, out is [rows,2].
AU_EXPORT int au_window_frame_minmax_i128(const int64_t* x, int64_t n,
                                          int64_t* pyr, int64_t pyr_len,
                                          const int64_t* a, const int64_t* b,
                                          int64_t rows, int is_max,
                                          int64_t* out, void* stream) {
  if (((uintptr_t)x | (uintptr_t)pyr | (uintptr_t)out) & 15)
    return (int)hipErrorInvalidValue;
  return wn_frame_minmax<WnI128>((const WnI128*)x, n, (WnI128*)pyr, pyr_len,
                                 a, b, rows, is_max, (WnI128*)out, stream);
}
