// Auron-AMD native engine kernels — gfx950 (MI355X, CDNA4) only.
//
// Role parity (reference, for capability mapping — no code is ported):
//  - Spark-compatible murmur3 row hash:   /root/reference/native-engine/datafusion-ext-commons/src/spark_hash.rs
//  - group-by hash table:                 .../datafusion-ext-plans/src/agg/agg_hash_map.rs
//  - join hash table build/probe:         .../datafusion-ext-plans/src/joins/join_hash_map.rs
//
// Design: MI355X-first. 64-wide wavefronts, grid-stride loops capped at
// ~2048 workgroups (256 CUs x 8 blocks — fills all 8 XCDs), device-scope
// atomics for cross-XCD correctness (per-XCD L2s are not coherent).
// Tables live in HBM3E; LDS-staged variants are layered on top where
// profiling shows payoff.
//
// C ABI only — loaded via ctypes from auron_amd/native/__init__.py.
// All pointers are device pointers owned by torch; `stream` is the torch
// current stream. No allocation happens here.

#include <hip/hip_runtime.h>
#include <stdint.h>

#define AU_EXPORT extern "C" __attribute__((visibility("default")))

// dtype codes — keep in sync with auron_amd/dtypes.py
enum AuDType : int32_t {
  AU_BOOL = 0,
  AU_INT8 = 1,
  AU_INT16 = 2,
  AU_INT32 = 3,
  AU_INT64 = 4,
  AU_FLOAT32 = 5,
  AU_FLOAT64 = 6,
  AU_DATE32 = 7,
  AU_STRING = 8,
  AU_DECIMAL64 = 9,
  AU_LIST = 10,
  AU_TIMESTAMP = 11,  // int64 microseconds since epoch
  AU_DECIMAL128 = 12, // [n,2] int64 per row: low 64 bits, signed high limb
};

struct AuColDesc {
  const void* data;        // typed buffer; for STRING: uint8 bytes
  const int64_t* offsets;  // STRING only, n+1 (LargeString: 64-bit)
  const uint8_t* validity; // bool bytes (1 = valid) or nullptr
  int32_t dtype;
  int32_t scale;
};

static inline int au_grid(int64_t n, int block) {
  int64_t g = (n + block - 1) / block;
  if (g > 2048) g = 2048;  // 256 CU x 8 — grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// ----------------------------------------------------------------- murmur3
// Spark Murmur3_x86_32 (seed-chained across columns, null-skipping).
__device__ __forceinline__ uint32_t rotl32(uint32_t x, int r) {
  return (x << r) | (x >> (32 - r));
}
__device__ __forceinline__ uint32_t mixK1(uint32_t k1) {
  k1 *= 0xcc9e2d51u;
  k1 = rotl32(k1, 15);
  k1 *= 0x1b873593u;
  return k1;
}
__device__ __forceinline__ uint32_t mixH1(uint32_t h1, uint32_t k1) {
  h1 ^= k1;
  h1 = rotl32(h1, 13);
  h1 = h1 * 5u + 0xe6546b64u;
  return h1;
}
__device__ __forceinline__ uint32_t fmix(uint32_t h1, uint32_t len) {
  h1 ^= len;
  h1 ^= h1 >> 16;
  h1 *= 0x85ebca6bu;
  h1 ^= h1 >> 13;
  h1 *= 0xc2b2ae35u;
  h1 ^= h1 >> 16;
  return h1;
}
__device__ __forceinline__ uint32_t hash_int(uint32_t v, uint32_t seed) {
  return fmix(mixH1(seed, mixK1(v)), 4);
}
__device__ __forceinline__ uint32_t hash_long(uint64_t v, uint32_t seed) {
  uint32_t h1 = mixH1(seed, mixK1((uint32_t)v));
  h1 = mixH1(h1, mixK1((uint32_t)(v >> 32)));
  return fmix(h1, 8);
}
__device__ uint32_t hash_bytes(const uint8_t* p, int32_t len, uint32_t seed) {
  int32_t aligned = len & ~3;
  uint32_t h1 = seed;
  for (int32_t i = 0; i < aligned; i += 4) {
    uint32_t w = (uint32_t)p[i] | ((uint32_t)p[i + 1] << 8) |
                 ((uint32_t)p[i + 2] << 16) | ((uint32_t)p[i + 3] << 24);
    h1 = mixH1(h1, mixK1(w));
  }
  for (int32_t i = aligned; i < len; i++) {
    // Spark sign-extends each tail byte to int
    int32_t b = (int8_t)p[i];
    h1 = mixH1(h1, mixK1((uint32_t)b));
  }
  return fmix(h1, (uint32_t)len);
}

// Spark hashes a decimal of precision > 18 as
// hashUnsafeBytes(BigInteger.toByteArray(unscaled)): the minimal big-endian
// two's-complement bytes, bitLength/8 + 1 of them (1..16). Same mixing as
// hash_bytes, with the bytes shifted out of the two limbs: the value is
// moved up so that its first byte is the top byte of the 128 bits, a whole
// word is then the byte-swapped top 32 bits, a tail byte the top 8.
__device__ __forceinline__ uint32_t hash_dec128(uint64_t lo, int64_t hi,
                                                uint32_t seed) {
  const uint64_t sign = (uint64_t)(hi >> 63);  // 0 or all ones
  const uint64_t xh = (uint64_t)hi ^ sign, xl = lo ^ sign;
  const int lz = xh ? __clzll((long long)xh)
                    : 64 + (xl ? __clzll((long long)xl) : 64);
  const int len = ((128 - lz) >> 3) + 1;  // bitLength / 8 + 1
  const int sh = 8 * (16 - len);          // 0, 8, .. 120
  uint64_t th = (uint64_t)hi, tl = lo;
  if (sh >= 64) {
    th = lo << (sh - 64);
    tl = 0;
  } else if (sh > 0) {
    th = (th << sh) | (lo >> (64 - sh));
    tl = lo << sh;
  }
  uint32_t h1 = seed;
  for (int w = len >> 2; w > 0; w--) {
    h1 = mixH1(h1, mixK1(__builtin_bswap32((uint32_t)(th >> 32))));
    th = (th << 32) | (tl >> 32);
    tl <<= 32;
  }
  for (int t = len & 3; t > 0; t--) {
    // Spark sign-extends each tail byte to int
    h1 = mixH1(h1, mixK1((uint32_t)(int32_t)(int8_t)(th >> 56)));
    th <<= 8;
  }
  return fmix(h1, (uint32_t)len);
}

__device__ __forceinline__ bool row_valid(const AuColDesc& c, int64_t i) {
  return c.validity == nullptr || c.validity[i] != 0;
}

__device__ uint32_t hash_one(const AuColDesc& c, int64_t i, uint32_t seed) {
  switch (c.dtype) {
    case AU_BOOL:
      return hash_int(((const uint8_t*)c.data)[i] ? 1u : 0u, seed);
    case AU_INT8:
      return hash_int((uint32_t)(int32_t)((const int8_t*)c.data)[i], seed);
    case AU_INT16:
      return hash_int((uint32_t)(int32_t)((const int16_t*)c.data)[i], seed);
    case AU_INT32:
    case AU_DATE32:
      return hash_int((uint32_t)((const int32_t*)c.data)[i], seed);
    case AU_INT64:
    case AU_DECIMAL64:
    case AU_TIMESTAMP:
      return hash_long((uint64_t)((const int64_t*)c.data)[i], seed);
    // floats as Spark's floatToIntBits / doubleToLongBits see them: -0.0 as
    // 0.0 and every NaN (either sign, any payload) as the one canonical NaN,
    // so keys that compare equal in keys_equal hash alike
    case AU_FLOAT32: {
      float f = ((const float*)c.data)[i];
      if (f == 0.0f) f = 0.0f;  // normalize -0.0
      return hash_int(f != f ? 0x7fc00000u : __float_as_uint(f), seed);
    }
    case AU_FLOAT64: {
      double d = ((const double*)c.data)[i];
      if (d == 0.0) d = 0.0;
      return hash_long(d != d ? 0x7ff8000000000000ull
                              : (uint64_t)__double_as_longlong(d), seed);
    }
    case AU_STRING: {
      int64_t s = c.offsets[i];
      int64_t e = c.offsets[i + 1];
      return hash_bytes((const uint8_t*)c.data + s, (int32_t)(e - s), seed);
    }
    case AU_DECIMAL128: {
      // one 16-byte load; the host keeps these columns 16-byte aligned
      const ulonglong2 v = ((const ulonglong2*)c.data)[i];
      return hash_dec128(v.x, (int64_t)v.y, seed);
    }
  }
  return seed;
}

__global__ void k_murmur3(const AuColDesc* cols, int ncols, int64_t n,
                          uint32_t seed, int32_t* out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t h = seed;
    for (int c = 0; c < ncols; c++) {
      if (row_valid(cols[c], i)) h = hash_one(cols[c], i, h);
    }
    out[i] = (int32_t)h;
  }
}

AU_EXPORT int au_murmur3(const void* cols_dev, int ncols, int64_t n,
                         int32_t seed, int32_t* out, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_murmur3, dim3(au_grid(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, (const AuColDesc*)cols_dev, ncols, n,
                     (uint32_t)seed, out);
  return (int)hipGetLastError();
}

// -------------------------------------------------------------- key equality
// Rows may come from two different batches (probe vs build).
__device__ bool keys_equal(const AuColDesc* a_cols, int64_t ai,
                           const AuColDesc* b_cols, int64_t bi, int ncols) {
  for (int c = 0; c < ncols; c++) {
    const AuColDesc& a = a_cols[c];
    const AuColDesc& b = b_cols[c];
    bool av = row_valid(a, ai);
    bool bv = row_valid(b, bi);
    if (av != bv) return false;
    if (!av) continue;  // both null: equal for GROUP BY grouping
    switch (a.dtype) {
      case AU_BOOL:
      case AU_INT8:
        if (((const int8_t*)a.data)[ai] != ((const int8_t*)b.data)[bi]) return false;
        break;
      case AU_INT16:
        if (((const int16_t*)a.data)[ai] != ((const int16_t*)b.data)[bi]) return false;
        break;
      case AU_INT32:
      case AU_DATE32:
        if (((const int32_t*)a.data)[ai] != ((const int32_t*)b.data)[bi]) return false;
        break;
      case AU_INT64:
      case AU_DECIMAL64:
      case AU_TIMESTAMP:
        if (((const int64_t*)a.data)[ai] != ((const int64_t*)b.data)[bi]) return false;
        break;
      // float keys: -0.0 == 0.0 and NaN == NaN (Spark's grouping and join
      // rule; IEEE != alone makes every NaN row a group of its own)
      case AU_FLOAT32: {
        const float x = ((const float*)a.data)[ai], y = ((const float*)b.data)[bi];
        if (x != y && !(x != x && y != y)) return false;
        break;
      }
      case AU_FLOAT64: {
        const double x = ((const double*)a.data)[ai], y = ((const double*)b.data)[bi];
        if (x != y && !(x != x && y != y)) return false;
        break;
      }
      case AU_STRING: {
        int64_t as = a.offsets[ai], ae = a.offsets[ai + 1];
        int64_t bs = b.offsets[bi], be = b.offsets[bi + 1];
        if (ae - as != be - bs) return false;
        const uint8_t* ap = (const uint8_t*)a.data + as;
        const uint8_t* bp = (const uint8_t*)b.data + bs;
        int32_t len = (int32_t)(ae - as);
        int32_t k = 0;
        for (; k + 8 <= len; k += 8) {
          uint64_t wa, wb;
          __builtin_memcpy(&wa, ap + k, 8);
          __builtin_memcpy(&wb, bp + k, 8);
          if (wa != wb) return false;
        }
        for (; k < len; k++)
          if (ap[k] != bp[k]) return false;
        break;
      }
      case AU_DECIMAL128: {
        // exact: the two's-complement value has one representation
        const ulonglong2 va = ((const ulonglong2*)a.data)[ai];
        const ulonglong2 vb = ((const ulonglong2*)b.data)[bi];
        if (va.x != vb.x || va.y != vb.y) return false;
        break;
      }
    }
  }
  return true;
}

// ------------------------------------------------------------ group-by table
// Open-addressing, linear probing. slots[cap] holds representative row idx
// (-1 empty). cap is a power of two >= 2*n_distinct-safe (caller sizes 2n).
__global__ void k_group_insert(const AuColDesc* cols, int ncols, int64_t n,
                               int32_t* slots, uint32_t cap_mask,
                               const int32_t* hashes, int32_t* rep) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t p = ((uint32_t)hashes[i]) & cap_mask;
    int32_t me = (int32_t)i;
    while (true) {
      int32_t cur = slots[p];
      if (cur == -1) {
        int32_t prev = atomicCAS(&slots[p], -1, me);
        if (prev == -1) {
          rep[i] = me;
          break;
        }
        cur = prev;
      }
      if (keys_equal(cols, cur, cols, i, ncols)) {
        rep[i] = cur;
        break;
      }
      p = (p + 1) & cap_mask;
    }
  }
}

__global__ void k_group_assign(const int32_t* rep, int64_t n, int32_t* gid_of_row,
                               int64_t* rep_rows, int32_t* counter) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (rep[i] == (int32_t)i) {
      int32_t g = atomicAdd(counter, 1);
      gid_of_row[i] = g;
      rep_rows[g] = i;
    }
  }
}

__global__ void k_group_gather(const int32_t* rep, int64_t n, int32_t* gid_of_row) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    gid_of_row[i] = gid_of_row[rep[i]];
  }
}

AU_EXPORT int au_group_ids(const void* cols_dev, int ncols, int64_t n,
                           int32_t* slots, int64_t cap, const int32_t* hashes,
                           int32_t* rep, int32_t* gids, int64_t* rep_rows,
                           int32_t* counter, void* stream) {
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  uint32_t mask = (uint32_t)(cap - 1);
  int g = au_grid(n, 256);
  hipLaunchKernelGGL(k_group_insert, dim3(g), dim3(256), 0, s,
                     (const AuColDesc*)cols_dev, ncols, n, slots, mask, hashes, rep);
  hipLaunchKernelGGL(k_group_assign, dim3(g), dim3(256), 0, s, rep, n, gids,
                     rep_rows, counter);
  hipLaunchKernelGGL(k_group_gather, dim3(g), dim3(256), 0, s, rep, n, gids);
  return (int)hipGetLastError();
}

// --------------------------------------------------------------- join table
// Chained buckets: heads[cap] (-1 empty) + next[n_build].
__global__ void k_join_build(int64_t n, int32_t* heads, uint32_t cap_mask,
                             int32_t* next, const int32_t* hashes) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint32_t p = ((uint32_t)hashes[i]) & cap_mask;
    next[i] = atomicExch(&heads[p], (int32_t)i);
  }
}

// has_null_key: rows whose key contains a SQL NULL never match (unlike
// GROUP BY where nulls group together).
__device__ __forceinline__ bool join_row_has_null(const AuColDesc* cols,
                                                  int ncols, int64_t i) {
  for (int c = 0; c < ncols; c++)
    if (!row_valid(cols[c], i)) return true;
  return false;
}

__global__ void k_join_count(const AuColDesc* bcols, const AuColDesc* pcols,
                             int ncols, int64_t n_probe, const int32_t* heads,
                             uint32_t cap_mask, const int32_t* next,
                             const int32_t* phashes, int32_t* counts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_probe;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t cnt = 0;
    if (!join_row_has_null(pcols, ncols, i)) {
      int32_t j = heads[((uint32_t)phashes[i]) & cap_mask];
      while (j != -1) {
        if (keys_equal(bcols, j, pcols, i, ncols) &&
            !join_row_has_null(bcols, ncols, j))
          cnt++;
        j = next[j];
      }
    }
    counts[i] = cnt;
  }
}

__global__ void k_join_fill(const AuColDesc* bcols, const AuColDesc* pcols,
                            int ncols, int64_t n_probe, const int32_t* heads,
                            uint32_t cap_mask, const int32_t* next,
                            const int32_t* phashes, const int64_t* offsets,
                            int64_t* build_out, int64_t* probe_out,
                            uint8_t* build_matched, int emit_unmatched_probe) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_probe;
       i += (int64_t)gridDim.x * blockDim.x) {
    int64_t o = offsets[i];
    int64_t start = o;
    if (!join_row_has_null(pcols, ncols, i)) {
      int32_t j = heads[((uint32_t)phashes[i]) & cap_mask];
      while (j != -1) {
        if (keys_equal(bcols, j, pcols, i, ncols) &&
            !join_row_has_null(bcols, ncols, j)) {
          build_out[o] = j;
          probe_out[o] = i;
          if (build_matched) build_matched[j] = 1;
          o++;
        }
        j = next[j];
      }
    }
    if (emit_unmatched_probe && o == start) {
      build_out[o] = -1;
      probe_out[o] = i;
    }
  }
}

AU_EXPORT int au_join_build(int64_t n, int32_t* heads, int64_t cap,
                            int32_t* next, const int32_t* hashes, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_join_build, dim3(au_grid(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, n, heads, (uint32_t)(cap - 1), next,
                     hashes);
  return (int)hipGetLastError();
}

AU_EXPORT int au_join_count(const void* bcols, const void* pcols, int ncols,
                            int64_t n_probe, const int32_t* heads, int64_t cap,
                            const int32_t* next, const int32_t* phashes,
                            int32_t* counts, void* stream) {
  if (n_probe == 0) return 0;
  hipLaunchKernelGGL(k_join_count, dim3(au_grid(n_probe, 256)), dim3(256), 0,
                     (hipStream_t)stream, (const AuColDesc*)bcols,
                     (const AuColDesc*)pcols, ncols, n_probe, heads,
                     (uint32_t)(cap - 1), next, phashes, counts);
  return (int)hipGetLastError();
}

AU_EXPORT int au_join_fill(const void* bcols, const void* pcols, int ncols,
                           int64_t n_probe, const int32_t* heads, int64_t cap,
                           const int32_t* next, const int32_t* phashes,
                           const int64_t* offsets, int64_t* build_out,
                           int64_t* probe_out, uint8_t* build_matched,
                           int emit_unmatched_probe, void* stream) {
  if (n_probe == 0) return 0;
  hipLaunchKernelGGL(k_join_fill, dim3(au_grid(n_probe, 256)), dim3(256), 0,
                     (hipStream_t)stream, (const AuColDesc*)bcols,
                     (const AuColDesc*)pcols, ncols, n_probe, heads,
                     (uint32_t)(cap - 1), next, phashes, offsets, build_out,
                     probe_out, build_matched, emit_unmatched_probe);
  return (int)hipGetLastError();
}

// ---------------------------------------------------------- fused join probe
// count -> torch glue -> fill, folded into two kernels: the probe hash is
// computed in-kernel (same seed chaining as k_murmur3), the chain is walked
// once, and output offsets come from a per-tile sum plus an in-block scan
// instead of N-sized int64 temporaries. Key descriptors travel by value in
// the kernel-argument struct (as MgParams does), so no descriptor upload and
// no per-row descriptor load from global memory.
//
// Rows are handled in fixed tiles: tile t covers [t*JP_TILE, (t+1)*JP_TILE),
// row = tile_base + slab*256 + tid. Everything is indexed by tile, never by
// block, so the row -> output mapping does not depend on the grid.
#define JP_MAX_KEYS 8
#define JP_BLOCK 256
#define JP_SLABS 4
#define JP_TILE (JP_BLOCK * JP_SLABS)

struct JpKeys {
  AuColDesc build[JP_MAX_KEYS];
  AuColDesc probe[JP_MAX_KEYS];
};

// MODE 0: any key shape (hash_one / keys_equal per column)
// MODE 1: exactly one int64 / decimal64 / timestamp key
// MODE 2: exactly one int32 / date32 key
// pkey carries the probe key of the integer modes; MODE 0 ignores it.
template <int MODE>
__device__ __forceinline__ bool jp_probe_key(const JpKeys& k, int ncols,
                                             int64_t i, int64_t* pkey) {
  if (MODE == 0) return !join_row_has_null(k.probe, ncols, i);
  const uint8_t* v = k.probe[0].validity;
  if (v != nullptr && v[i] == 0) return false;
  if (MODE == 1) *pkey = ((const int64_t*)k.probe[0].data)[i];
  else *pkey = ((const int32_t*)k.probe[0].data)[i];
  return true;
}

template <int MODE>
__device__ __forceinline__ uint32_t jp_hash(const JpKeys& k, int ncols,
                                            int64_t i, int64_t pkey,
                                            uint32_t seed) {
  if (MODE == 1) return hash_long((uint64_t)pkey, seed);
  if (MODE == 2) return hash_int((uint32_t)(int32_t)pkey, seed);
  uint32_t h = seed;
  for (int c = 0; c < ncols; c++) h = hash_one(k.probe[c], i, h);  // no NULLs here
  return h;
}

template <int MODE>
__device__ __forceinline__ bool jp_match(const JpKeys& k, int ncols, int32_t j,
                                         int64_t i, int64_t pkey) {
  if (MODE == 0)
    return keys_equal(k.build, j, k.probe, i, ncols) &&
           !join_row_has_null(k.build, ncols, j);
  const uint8_t* v = k.build[0].validity;
  if (MODE == 1) {
    if (((const int64_t*)k.build[0].data)[j] != pkey) return false;
  } else {
    if (((const int32_t*)k.build[0].data)[j] != (int32_t)pkey) return false;
  }
  return v == nullptr || v[j] != 0;
}

template <int MODE>
__global__ void __launch_bounds__(JP_BLOCK) k_join_probe_count(
    JpKeys k, int ncols, int64_t n_probe, int64_t n_tiles,
    const int32_t* __restrict__ heads, uint32_t cap_mask,
    const int32_t* __restrict__ next, uint32_t seed, int emit_unmatched_probe,
    int32_t* __restrict__ counts, int32_t* __restrict__ first,
    int64_t* __restrict__ tile_sums, uint8_t* build_matched) {
  __shared__ int64_t wsum[JP_BLOCK / 64];
  const int tid = threadIdx.x;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t base = t * JP_TILE;
    // heads of all slabs first: the loads are independent, so they overlap
    int32_t j0[JP_SLABS];
    int64_t pk[JP_SLABS];
#pragma unroll
    for (int s = 0; s < JP_SLABS; s++) {
      const int64_t i = base + s * JP_BLOCK + tid;
      j0[s] = -1;
      pk[s] = 0;
      if (i < n_probe && jp_probe_key<MODE>(k, ncols, i, &pk[s]))
        j0[s] = heads[jp_hash<MODE>(k, ncols, i, pk[s], seed) & cap_mask];
    }
    int64_t acc = 0;
#pragma unroll
    for (int s = 0; s < JP_SLABS; s++) {
      const int64_t i = base + s * JP_BLOCK + tid;
      if (i >= n_probe) continue;
      int32_t cnt = 0, f = -1;
      for (int32_t j = j0[s]; j != -1; j = next[j]) {
        if (jp_match<MODE>(k, ncols, j, i, pk[s])) {
          if (cnt == 0) f = j;
          cnt++;
          if (build_matched) build_matched[j] = 1;
        }
      }
      counts[i] = cnt;
      first[i] = f;
      acc += (emit_unmatched_probe && cnt == 0) ? 1 : cnt;
    }
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_down(acc, d, 64);
    if ((tid & 63) == 0) wsum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
      int64_t sum = 0;
      for (int w = 0; w < JP_BLOCK / 64; w++) sum += wsum[w];
      tile_sums[t] = sum;
    }
    __syncthreads();
  }
}

// tile_ends = inclusive prefix sum of tile_sums (host: one cumsum over
// n_tiles elements). Offsets inside a tile come from a block-exclusive scan
// per slab (wave scan + LDS across the four waves) with the running base
// carried from slab to slab. cnt == 1 rows never touch the table or a key.
template <int MODE>
__global__ void __launch_bounds__(JP_BLOCK) k_join_probe_fill(
    JpKeys k, int ncols, int64_t n_probe, int64_t n_tiles,
    const int32_t* __restrict__ next, const int32_t* __restrict__ counts,
    const int32_t* __restrict__ first, const int64_t* __restrict__ tile_ends,
    int emit_unmatched_probe, int64_t* __restrict__ build_out,
    int64_t* __restrict__ probe_out) {
  // two buffers, alternating per slab: one barrier per slab is enough
  __shared__ int64_t wtot[2][JP_BLOCK / 64];
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  for (int64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    const int64_t base = t * JP_TILE;
    int64_t running = t == 0 ? 0 : tile_ends[t - 1];
    for (int s = 0; s < JP_SLABS; s++) {
      const int64_t i = base + s * JP_BLOCK + tid;
      const bool in = i < n_probe;
      const int32_t cnt = in ? counts[i] : 0;
      const int64_t eff = !in ? 0 : (emit_unmatched_probe && cnt == 0) ? 1 : cnt;
      int64_t incl = eff;
      for (int d = 1; d < 64; d <<= 1) {
        int64_t up = __shfl_up(incl, d, 64);
        if (lane >= d) incl += up;
      }
      if (lane == 63) wtot[s & 1][wave] = incl;
      __syncthreads();
      int64_t before = 0, total = 0;
      for (int w = 0; w < JP_BLOCK / 64; w++) {
        const int64_t x = wtot[s & 1][w];
        if (w < wave) before += x;
        total += x;
      }
      int64_t o = running + before + incl - eff;
      running += total;
      if (!in) continue;
      if (cnt == 0) {
        if (emit_unmatched_probe) {
          build_out[o] = -1;
          probe_out[o] = i;
        }
      } else if (cnt == 1) {
        build_out[o] = first[i];
        probe_out[o] = i;
      } else {
        int64_t pkey = 0;
        jp_probe_key<MODE>(k, ncols, i, &pkey);
        int32_t left = cnt;
        for (int32_t j = first[i]; j != -1 && left > 0; j = next[j]) {
          if (jp_match<MODE>(k, ncols, j, i, pkey)) {
            build_out[o] = j;
            probe_out[o] = i;
            o++;
            left--;
          }
        }
      }
    }
  }
}

// semi / anti / existence: stop at the first match, one byte per probe row
template <int MODE>
__global__ void __launch_bounds__(JP_BLOCK) k_join_exists(
    JpKeys k, int ncols, int64_t n_probe, const int32_t* __restrict__ heads,
    uint32_t cap_mask, const int32_t* __restrict__ next, uint32_t seed,
    uint8_t* __restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_probe;
       i += (int64_t)gridDim.x * blockDim.x) {
    uint8_t found = 0;
    int64_t pkey = 0;
    if (jp_probe_key<MODE>(k, ncols, i, &pkey)) {
      int32_t j = heads[jp_hash<MODE>(k, ncols, i, pkey, seed) & cap_mask];
      while (j != -1) {
        if (jp_match<MODE>(k, ncols, j, i, pkey)) {
          found = 1;
          break;
        }
        j = next[j];
      }
    }
    out[i] = found;
  }
}

static inline bool jp_int64_family(int32_t d) {
  return d == AU_INT64 || d == AU_DECIMAL64 || d == AU_TIMESTAMP;
}
static inline bool jp_int32_family(int32_t d) {
  return d == AU_INT32 || d == AU_DATE32;
}

// host_descs: AuColDesc[2 * ncols] in host memory, build keys then probe keys
static int jp_pack(const void* host_descs, int ncols, JpKeys* k) {
  const AuColDesc* d = (const AuColDesc*)host_descs;
  for (int c = 0; c < ncols; c++) {
    k->build[c] = d[c];
    k->probe[c] = d[ncols + c];
  }
  if (ncols == 1) {
    if (jp_int64_family(d[0].dtype) && jp_int64_family(d[1].dtype)) return 1;
    if (jp_int32_family(d[0].dtype) && jp_int32_family(d[1].dtype)) return 2;
  }
  return 0;
}

static inline int jp_grid(int64_t n_tiles) {
  return (int)(n_tiles > 2048 ? 2048 : n_tiles);
}

AU_EXPORT int64_t au_join_probe_tile() { return JP_TILE; }
AU_EXPORT int au_join_probe_max_keys() { return JP_MAX_KEYS; }

AU_EXPORT int au_join_probe_count(const void* host_descs, int ncols,
                                  int64_t n_probe, const int32_t* heads,
                                  int64_t cap, const int32_t* next,
                                  int32_t seed, int emit_unmatched_probe,
                                  int32_t* counts, int32_t* first,
                                  int64_t* tile_sums, uint8_t* build_matched,
                                  void* stream) {
  if (n_probe == 0) return 0;
  if (ncols < 1 || ncols > JP_MAX_KEYS) return 1002;
  JpKeys k{};
  const int mode = jp_pack(host_descs, ncols, &k);
  const int64_t n_tiles = (n_probe + JP_TILE - 1) / JP_TILE;
#define JP_LAUNCH_COUNT(M)                                                     \
  hipLaunchKernelGGL(k_join_probe_count<M>, dim3(jp_grid(n_tiles)),            \
                     dim3(JP_BLOCK), 0, (hipStream_t)stream, k, ncols, n_probe, \
                     n_tiles, heads, (uint32_t)(cap - 1), next, (uint32_t)seed, \
                     emit_unmatched_probe, counts, first, tile_sums,           \
                     build_matched)
  if (mode == 1) JP_LAUNCH_COUNT(1);
  else if (mode == 2) JP_LAUNCH_COUNT(2);
  else JP_LAUNCH_COUNT(0);
#undef JP_LAUNCH_COUNT
  return (int)hipGetLastError();
}

AU_EXPORT int au_join_probe_fill(const void* host_descs, int ncols,
                                 int64_t n_probe, const int32_t* next,
                                 const int32_t* counts, const int32_t* first,
                                 const int64_t* tile_ends,
                                 int emit_unmatched_probe, int64_t* build_out,
                                 int64_t* probe_out, void* stream) {
  if (n_probe == 0) return 0;
  if (ncols < 1 || ncols > JP_MAX_KEYS) return 1002;
  JpKeys k{};
  const int mode = jp_pack(host_descs, ncols, &k);
  const int64_t n_tiles = (n_probe + JP_TILE - 1) / JP_TILE;
#define JP_LAUNCH_FILL(M)                                                      \
  hipLaunchKernelGGL(k_join_probe_fill<M>, dim3(jp_grid(n_tiles)),             \
                     dim3(JP_BLOCK), 0, (hipStream_t)stream, k, ncols, n_probe, \
                     n_tiles, next, counts, first, tile_ends,                  \
                     emit_unmatched_probe, build_out, probe_out)
  if (mode == 1) JP_LAUNCH_FILL(1);
  else if (mode == 2) JP_LAUNCH_FILL(2);
  else JP_LAUNCH_FILL(0);
#undef JP_LAUNCH_FILL
  return (int)hipGetLastError();
}

AU_EXPORT int au_join_exists(const void* host_descs, int ncols, int64_t n_probe,
                             const int32_t* heads, int64_t cap,
                             const int32_t* next, int32_t seed, uint8_t* out,
                             void* stream) {
  if (n_probe == 0) return 0;
  if (ncols < 1 || ncols > JP_MAX_KEYS) return 1002;
  JpKeys k{};
  const int mode = jp_pack(host_descs, ncols, &k);
#define JP_LAUNCH_EXISTS(M)                                                    \
  hipLaunchKernelGGL(k_join_exists<M>, dim3(au_grid(n_probe, JP_BLOCK)),       \
                     dim3(JP_BLOCK), 0, (hipStream_t)stream, k, ncols, n_probe, \
                     heads, (uint32_t)(cap - 1), next, (uint32_t)seed, out)
  if (mode == 1) JP_LAUNCH_EXISTS(1);
  else if (mode == 2) JP_LAUNCH_EXISTS(2);
  else JP_LAUNCH_EXISTS(0);
#undef JP_LAUNCH_EXISTS
  return (int)hipGetLastError();
}

// ------------------------------------------------------------- partitioning
// part_id = pmod(murmur3_hash, nparts)  (Spark HashPartitioning semantics)
__global__ void k_pmod(const int32_t* hashes, int64_t n, int32_t nparts,
                       int32_t* part_ids) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t m = hashes[i] % nparts;
    part_ids[i] = m < 0 ? m + nparts : m;
  }
}

AU_EXPORT int au_pmod(const int32_t* hashes, int64_t n, int32_t nparts,
                      int32_t* part_ids, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_pmod, dim3(au_grid(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, hashes, n, nparts, part_ids);
  return (int)hipGetLastError();
}

// Stable counting-sort scatter by partition id.
// Pass 1: histogram (atomics). Host computes exclusive prefix (torch cumsum).
// Pass 2: stable scatter — each row's final slot = base[part] + rank of row
// within its partition. Rank computed via one atomicAdd per row gives an
// arbitrary intra-partition order; stability is not required by the shuffle
// contract (Spark shuffle reader order is unspecified).
__global__ void k_part_hist(const int32_t* part_ids, int64_t n, int32_t nparts,
                            int32_t* counts) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    atomicAdd(&counts[part_ids[i]], 1);
  }
}

__global__ void k_part_scatter(const int32_t* part_ids, int64_t n,
                               const int64_t* base, int32_t* cursors,
                               int64_t* order) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    int32_t p = part_ids[i];
    int64_t slot = base[p] + atomicAdd(&cursors[p], 1);
    order[slot] = i;
  }
}

AU_EXPORT int au_part_hist(const int32_t* part_ids, int64_t n, int32_t nparts,
                           int32_t* counts, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_part_hist, dim3(au_grid(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, part_ids, n, nparts, counts);
  return (int)hipGetLastError();
}

AU_EXPORT int au_part_scatter(const int32_t* part_ids, int64_t n,
                              const int64_t* base, int32_t* cursors,
                              int64_t* order, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_part_scatter, dim3(au_grid(n, 256)), dim3(256), 0,
                     (hipStream_t)stream, part_ids, n, base, cursors, order);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------- byte gather
// Variable-length row gather for string columns (arrow/selection.rs take()
// analogue): one wavefront per output row copies its bytes, replacing the
// arange/repeat_interleave/fancy-index chain (5 torch kernels) the r2
// profile showed on every string gather.
__global__ void k_bytes_gather(const uint8_t* __restrict__ src,
                               const int64_t* __restrict__ src_start,
                               const int64_t* __restrict__ out_off,
                               uint8_t* __restrict__ out, int64_t nrows) {
  // thread-per-row: TPC-DS strings average 10-30 bytes, so row-level
  // parallelism beats wavefront-per-row lane masking; long rows chunk
  // through an 8-byte loop
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
       row < nrows; row += (int64_t)gridDim.x * blockDim.x) {
    const int64_t dst0 = out_off[row];
    const int64_t len = out_off[row + 1] - dst0;
    const int64_t s0 = src_start[row];
    int64_t j = 0;
    for (; j + 8 <= len; j += 8) {
      uint64_t w;
      __builtin_memcpy(&w, src + s0 + j, 8);
      __builtin_memcpy(out + dst0 + j, &w, 8);
    }
    for (; j < len; j++) out[dst0 + j] = src[s0 + j];
  }
}

AU_EXPORT int au_bytes_gather(const uint8_t* src, const int64_t* src_start,
                              const int64_t* out_off, uint8_t* out,
                              int64_t nrows, void* stream) {
  if (nrows == 0) return 0;
  int64_t blocks = (nrows + 255) / 256;
  if (blocks > 16384) blocks = 16384;
  if (blocks < 1) blocks = 1;
  hipLaunchKernelGGL(k_bytes_gather, dim3((uint32_t)blocks), dim3(256), 0,
                     (hipStream_t)stream, src, src_start, out_off, out, nrows);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ version
AU_EXPORT int au_abi_version() { return 1; }

// ------------------------------------------------------- fused gather
// One launch gathers ALL fixed-width columns of a batch (join/window/
// sort/partition row gathers were one at::native index_select launch per
// column — the top at::native entry of the final SF=10 profile).
// Negative row index => null output (outer-join semantics).
#define MG_MAX_COLS 24

struct MgCol {
  const void* src;
  const uint8_t* src_valid;  // nullptr = all valid
  void* dst;
  uint8_t* dst_valid;        // nullptr = caller wants no validity
  int64_t esize;             // 1/2/4/8/16
  int64_t pad;
};

struct MgParams { MgCol cols[MG_MAX_COLS]; };

__global__ void __launch_bounds__(256) k_multi_gather(
    const int64_t* __restrict__ idx, int64_t n, MgParams p, int ncols) {
  // blocks tile (col, row-chunk): consecutive blocks cover the same col
  int64_t chunks_per_col = (n + 255) / 256;
  for (int64_t b = blockIdx.x; b < chunks_per_col * ncols; b += gridDim.x) {
    int c = (int)(b / chunks_per_col);
    int64_t row = (b % chunks_per_col) * 256 + threadIdx.x;
    if (row >= n) continue;
    const MgCol col = p.cols[c];
    int64_t i = idx[row];
    bool ok = i >= 0;
    int64_t src_i = ok ? i : 0;
    bool v = ok && (!col.src_valid || col.src_valid[src_i]);
    if (col.dst_valid) col.dst_valid[row] = v;
    switch (col.esize) {
      case 1: ((uint8_t*)col.dst)[row] = ok ? ((const uint8_t*)col.src)[src_i] : 0; break;
      case 2: ((uint16_t*)col.dst)[row] = ok ? ((const uint16_t*)col.src)[src_i] : 0; break;
      case 4: ((uint32_t*)col.dst)[row] = ok ? ((const uint32_t*)col.src)[src_i] : 0; break;
      case 8: ((uint64_t*)col.dst)[row] = ok ? ((const uint64_t*)col.src)[src_i] : 0; break;
      case 16: {
        ulonglong2 z; z.x = 0; z.y = 0;
        ((ulonglong2*)col.dst)[row] = ok ? ((const ulonglong2*)col.src)[src_i] : z;
        break;
      }
      default: break;
    }
  }
}

AU_EXPORT int au_multi_gather(const void* idx, int64_t n,
                              const void* host_cols, int ncols,
                              void* stream) {
  if (n <= 0 || ncols <= 0) return 0;
  if (ncols > MG_MAX_COLS) return 1002;
  MgParams p{};
  const MgCol* hc = (const MgCol*)host_cols;
  for (int i = 0; i < ncols; i++) p.cols[i] = hc[i];
  int64_t chunks = ((n + 255) / 256) * ncols;
  int64_t g = chunks > 4096 ? 4096 : chunks;
  hipLaunchKernelGGL(k_multi_gather, dim3((uint32_t)g), dim3(256), 0,
                     (hipStream_t)stream, (const int64_t*)idx, n, p, ncols);
  return (int)hipGetLastError();
}
