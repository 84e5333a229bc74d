// GPU Parquet page decode — gfx950.
//
// Role parity: the reference's CPU parquet decode (parquet_exec.rs via
// arrow-rs). Here the host ships raw uncompressed column-chunk bytes to
// HBM and these kernels do the decode work:
//  - k_pq_rle1:      RLE/bit-packed-hybrid definition levels (bit width 1)
//                    -> validity bytes, one workgroup per page
//  - k_pq_scatter:   PLAIN non-null values scattered to row slots using a
//                    precomputed validity prefix sum
//  - k_pq_copy:      PLAIN values for required (no-null) chunks, segmented
//                    vectorized copy
//  - k_pq_delta_*:   DELTA_BINARY_PACKED values and DELTA_LENGTH_BYTE_ARRAY
//                    lengths, one wave per miniblock (host-indexed headers)
//  - k_pq_dba_bytes: DELTA_BYTE_ARRAY strings rebuilt from the prefix and
//                    suffix lengths the delta kernels decoded, one wave
//                    per segment of values, seeded from source bytes only
//
// Page descriptor layout (int64 x 6, packed by parquet_native.py):
//   [0]=def_off [1]=def_len [2]=values_off [3]=n_values [4]=row_start [5]=pad

#include <hip/hip_runtime.h>
#include <stdint.h>

#define AU_EXPORT extern "C" __attribute__((visibility("default")))

struct PqPage {
  int64_t def_off;
  int64_t def_len;
  int64_t values_off;
  int64_t n_values;
  int64_t row_start;
  int64_t pad;
};

// ------------------------------------------------------------------- RLE1
// Two-phase per block: lane 0 parses run headers into an LDS window, then
// all 256 threads expand the window in parallel. Runs are (value,count) or
// bit-packed literal groups.
struct Run {
  int32_t out_start;  // relative to page
  int32_t count;
  int32_t src_off;    // for literal runs: byte offset of packed bits
  int32_t rep_val;    // for repeat runs: value; -1 => literal
};

#define RLE_WINDOW 512

// Split factor: each page gets RLE1_SPLIT workgroups. Writers (pyarrow,
// parquet-mr) emit definition levels as ONE hybrid run per page in the
// common case; that run is sliced across the page's workgroups so the
// whole chip fills even for a handful of pages. Multi-run pages fall back
// to the windowed serial-parse path in workgroup 0.
#define RLE1_SPLIT 16

#define RLE1_LDS_BYTES 16384

__global__ void k_pq_rle1(const PqPage* pages, const uint8_t* buf, uint8_t* out) {
  const PqPage p = pages[blockIdx.x / RLE1_SPLIT];
  const int slice = blockIdx.x % RLE1_SPLIT;
  const uint8_t* src = buf + p.def_off;
  int64_t src_len = p.def_len;
  uint8_t* dst = out + p.row_start;
  const int64_t n = p.n_values;

  // Stage the page's level bytes through LDS: the run-header parse is a
  // serial chain of dependent byte loads, and HBM-latency per byte is
  // what made this kernel the r2 profile's #1 entry. A bit-width-1 page
  // of 8k values is ~1-3 KB, far under the 160 KB LDS per CU.
  __shared__ uint8_t sbuf[RLE1_LDS_BYTES];
  if (src_len <= RLE1_LDS_BYTES) {
    for (int64_t i = threadIdx.x; i < src_len; i += blockDim.x)
      sbuf[i] = src[i];
    __syncthreads();
    src = sbuf;
  }

  // ---- fast path: single run spans the page ----
  {
    int64_t pos = 0;
    uint64_t header = 0;
    int shift = 0;
    while (pos < src_len) {
      uint8_t b = src[pos++];
      header |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    int64_t covered = (header & 1) ? (int64_t)(header >> 1) * 8
                                   : (int64_t)(header >> 1);
    if (covered >= n) {
      const int64_t per = (n + RLE1_SPLIT - 1) / RLE1_SPLIT;
      const int64_t lo = slice * per;
      const int64_t hi = min(lo + per, n);
      if (lo >= hi) return;
      if (header & 1) {
        const uint8_t* bits = src + pos;
        for (int64_t j = lo + threadIdx.x; j < hi; j += blockDim.x)
          dst[j] = (bits[j >> 3] >> (j & 7)) & 1;
      } else {
        const uint8_t v = src[pos] & 1;
        for (int64_t j = lo + threadIdx.x; j < hi; j += blockDim.x)
          dst[j] = v;
      }
      return;
    }
  }
  if (slice != 0) return;  // general path: one workgroup per page

  __shared__ Run runs[RLE_WINDOW];
  __shared__ int nruns;
  __shared__ int64_t s_pos, s_i;

  if (threadIdx.x == 0) {
    s_pos = 0;
    s_i = 0;
  }
  __syncthreads();

  while (true) {
    if (threadIdx.x == 0) {
      int64_t pos = s_pos;
      int64_t i = s_i;
      int r = 0;
      while (r < RLE_WINDOW && i < n && pos < src_len) {
        // uvarint
        uint64_t header = 0;
        int shift = 0;
        while (true) {
          uint8_t b = src[pos++];
          header |= (uint64_t)(b & 0x7F) << shift;
          if (!(b & 0x80)) break;
          shift += 7;
        }
        if (header & 1) {  // literal: (header>>1) groups of 8 bit-packed
          int64_t ngroups = header >> 1;
          int64_t nvals = ngroups * 8;
          if (nvals > n - i) nvals = n - i;
          runs[r].out_start = (int32_t)i;
          runs[r].count = (int32_t)nvals;
          runs[r].src_off = (int32_t)pos;
          runs[r].rep_val = -1;
          pos += ngroups;
          i += nvals;
        } else {
          int64_t cnt = header >> 1;
          if (cnt > n - i) cnt = n - i;
          runs[r].out_start = (int32_t)i;
          runs[r].count = (int32_t)cnt;
          runs[r].rep_val = src[pos] & 1;
          pos += 1;
          i += cnt;
        }
        r++;
      }
      nruns = r;
      s_pos = pos;
      s_i = i;
    }
    __syncthreads();
    int count = nruns;
    if (count == 0) break;
    // expand: threads stride over runs
    for (int r = threadIdx.x / 64; r < count; r += blockDim.x / 64) {
      const Run run = runs[r];
      int lane = threadIdx.x & 63;
      if (run.rep_val >= 0) {
        for (int j = lane; j < run.count; j += 64) dst[run.out_start + j] = (uint8_t)run.rep_val;
      } else {
        for (int j = lane; j < run.count; j += 64) {
          dst[run.out_start + j] = (src[run.src_off + (j >> 3)] >> (j & 7)) & 1;
        }
      }
    }
    __syncthreads();
    if (count < RLE_WINDOW) break;
  }
}

// --------------------------------------------------- host-parsed RLE1 path
// The run-header walk is inherently serial PER PAGE and, at ~2-3k runs per
// page for a few-percent-null column, dominates decode time if done on one
// device thread. Pages are static per file, so the HOST parses headers once
// (this plain-C routine, cached in the reader's file metadata) and the
// device only runs the embarrassingly-parallel expansion kernel below.
// Run encoding: out_start/count are chunk-absolute rows; src_off is an
// absolute byte offset into the staged buffer; rep_val -1 = literal run.
AU_EXPORT int64_t au_host_rle1_parse(const uint8_t* src, int64_t src_len,
                                     int64_t n, int64_t out_base,
                                     int64_t src_base, int32_t* runs,
                                     int64_t cap) {
  int64_t pos = 0, i = 0, r = 0;
  while (i < n && pos < src_len) {
    uint64_t header = 0;
    int shift = 0;
    while (pos < src_len) {
      uint8_t b = src[pos++];
      header |= (uint64_t)(b & 0x7F) << shift;
      if (!(b & 0x80)) break;
      shift += 7;
    }
    if (r >= cap) return -1;
    if (header & 1) {
      int64_t ngroups = (int64_t)(header >> 1);
      int64_t nvals = ngroups * 8;
      if (nvals > n - i) nvals = n - i;
      runs[4 * r + 0] = (int32_t)(out_base + i);
      runs[4 * r + 1] = (int32_t)nvals;
      runs[4 * r + 2] = (int32_t)(src_base + pos);
      runs[4 * r + 3] = -1;
      pos += ngroups;
      i += nvals;
    } else {
      int64_t cnt = (int64_t)(header >> 1);
      if (cnt > n - i) cnt = n - i;
      runs[4 * r + 0] = (int32_t)(out_base + i);
      runs[4 * r + 1] = (int32_t)cnt;
      runs[4 * r + 2] = 0;
      runs[4 * r + 3] = src[pos] & 1;
      pos += 1;
      i += cnt;
    }
    r++;
  }
  return i == n ? r : -1;
}

__global__ void k_rle1_expand(const int32_t* __restrict__ runs, int64_t nruns,
                              const uint8_t* __restrict__ buf,
                              uint8_t* __restrict__ out) {
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t r = wave; r < nruns; r += nwaves) {
    const int32_t out_start = runs[4 * r + 0];
    const int32_t count = runs[4 * r + 1];
    const int32_t src_off = runs[4 * r + 2];
    const int32_t rep = runs[4 * r + 3];
    if (rep >= 0) {
      const uint8_t v = (uint8_t)rep;
      for (int32_t j = lane; j < count; j += 64) out[out_start + j] = v;
    } else {
      const uint8_t* bits = buf + src_off;
      for (int32_t j = lane; j < count; j += 64)
        out[out_start + j] = (bits[j >> 3] >> (j & 7)) & 1;
    }
  }
}

AU_EXPORT int au_rle1_expand(const int32_t* runs_dev, int64_t nruns,
                             const void* buf, uint8_t* out, void* stream) {
  if (nruns == 0) return 0;
  int64_t blocks = (nruns * 64 + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(k_rle1_expand, dim3((uint32_t)blocks), dim3(256), 0,
                     (hipStream_t)stream, runs_dev, nruns,
                     (const uint8_t*)buf, out);
  return (int)hipGetLastError();
}

AU_EXPORT int au_pq_rle1(const void* pages_dev, int npages, const void* buf,
                         uint8_t* out, void* stream) {
  if (npages == 0) return 0;
  hipLaunchKernelGGL(k_pq_rle1, dim3(npages * RLE1_SPLIT), dim3(256), 0,
                     (hipStream_t)stream,
                     (const PqPage*)pages_dev, (const uint8_t*)buf, out);
  return (int)hipGetLastError();
}

// ------------------------------------------------------------------ RLE idx
// Generalized RLE/bit-packed hybrid decode for DICTIONARY indices
// (bit width 1..32). One workgroup per page; same two-phase structure as
// k_pq_rle1. Descriptor reuses PqPage with repurposed fields:
//   def_off=idx_off  def_len=idx_len  values_off=unused
//   n_values=page rows  row_start=chunk-relative row  pad=bit_width
// `prefix` is the chunk-wide inclusive cumsum of validity (or null for
// no-null chunks): the kernel derives each page's valid count and its
// compact output base on-device, so the host never syncs.
// The staged buffer is padded by 8 bytes so the unaligned 8-byte loads at
// a literal run's tail never read out of bounds.
__global__ void k_pq_rle_idx(const PqPage* pages, const uint8_t* buf, int32_t* out,
                             const int64_t* prefix) {
  const PqPage p = pages[blockIdx.x];
  const uint8_t* src = buf + p.def_off;
  const int64_t src_len = p.def_len;
  int64_t base, n;
  if (prefix) {
    base = p.row_start == 0 ? 0 : prefix[p.row_start - 1];
    n = prefix[p.row_start + p.n_values - 1] - base;
  } else {
    base = p.row_start;
    n = p.n_values;
  }
  int32_t* dst = out + base;
  const int bw = (int)p.pad;
  const uint64_t mask = bw >= 64 ? ~0ull : ((1ull << bw) - 1);
  const int vbytes = (bw + 7) >> 3;

  __shared__ Run runs[RLE_WINDOW];
  __shared__ int nruns;
  __shared__ int64_t s_pos, s_i;

  if (threadIdx.x == 0) {
    s_pos = 0;
    s_i = 0;
  }
  __syncthreads();

  while (true) {
    if (threadIdx.x == 0) {
      int64_t pos = s_pos;
      int64_t i = s_i;
      int r = 0;
      while (r < RLE_WINDOW && i < n && pos < src_len) {
        uint64_t header = 0;
        int shift = 0;
        while (true) {
          uint8_t b = src[pos++];
          header |= (uint64_t)(b & 0x7F) << shift;
          if (!(b & 0x80)) break;
          shift += 7;
        }
        if (header & 1) {  // literal: (header>>1) groups of 8, bw bits each
          int64_t ngroups = header >> 1;
          int64_t nvals = ngroups * 8;
          if (nvals > n - i) nvals = n - i;
          runs[r].out_start = (int32_t)i;
          runs[r].count = (int32_t)nvals;
          runs[r].src_off = (int32_t)pos;
          runs[r].rep_val = -1;
          pos += ngroups * bw;  // bw bytes per group of 8
          i += nvals;
        } else {
          int64_t cnt = header >> 1;
          if (cnt > n - i) cnt = n - i;
          uint32_t v = 0;
          for (int b2 = 0; b2 < vbytes; b2++) v |= (uint32_t)src[pos + b2] << (8 * b2);
          runs[r].out_start = (int32_t)i;
          runs[r].count = (int32_t)cnt;
          runs[r].rep_val = (int32_t)(v & mask);
          pos += vbytes;
          i += cnt;
        }
        r++;
      }
      nruns = r;
      s_pos = pos;
      s_i = i;
    }
    __syncthreads();
    int count = nruns;
    if (count == 0) break;
    for (int r = threadIdx.x / 64; r < count; r += blockDim.x / 64) {
      const Run run = runs[r];
      int lane = threadIdx.x & 63;
      if (run.rep_val >= 0) {
        for (int j = lane; j < run.count; j += 64) dst[run.out_start + j] = run.rep_val;
      } else {
        for (int j = lane; j < run.count; j += 64) {
          int64_t bitpos = (int64_t)j * bw;
          uint64_t w;
          __builtin_memcpy(&w, src + run.src_off + (bitpos >> 3), 8);
          dst[run.out_start + j] = (int32_t)((w >> (bitpos & 7)) & mask);
        }
      }
    }
    __syncthreads();
    if (count < RLE_WINDOW) break;
  }
}

AU_EXPORT int au_pq_rle_idx(const void* pages_dev, int npages, const void* buf,
                            int32_t* out, const int64_t* prefix, void* stream) {
  if (npages == 0) return 0;
  hipLaunchKernelGGL(k_pq_rle_idx, dim3(npages), dim3(256), 0, (hipStream_t)stream,
                     (const PqPage*)pages_dev, (const uint8_t*)buf, out, prefix);
  return (int)hipGetLastError();
}

// ----------------------------------------------------------------- scatter
// out[row] = valid(row) ? values[prefix[row]-1 - page_base] : 0
// prefix = inclusive cumsum of validity over the whole chunk (int64).
template <typename T>
__global__ void k_pq_scatter(const PqPage* pages, int npages, const uint8_t* buf,
                             const uint8_t* validity, const int64_t* prefix,
                             T* out, int64_t total) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < total;
       row += (int64_t)gridDim.x * blockDim.x) {
    // binary search the page containing `row`
    int lo = 0, hi = npages - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (pages[mid].row_start <= row) lo = mid; else hi = mid - 1;
    }
    const PqPage p = pages[lo];
    if (!validity[row]) {
      out[row] = (T)0;
      continue;
    }
    int64_t page_base = p.row_start == 0 ? 0 : prefix[p.row_start - 1];
    int64_t k = prefix[row] - 1 - page_base;
    T v;
    __builtin_memcpy(&v, buf + p.values_off + k * (int64_t)sizeof(T), sizeof(T));
    out[row] = v;
  }
}

// ---------------------------------------------------------------- copy (no nulls)
template <typename T>
__global__ void k_pq_copy(const PqPage* pages, int npages, const uint8_t* buf,
                          T* out, int64_t total) {
  for (int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; row < total;
       row += (int64_t)gridDim.x * blockDim.x) {
    int lo = 0, hi = npages - 1;
    while (lo < hi) {
      int mid = (lo + hi + 1) >> 1;
      if (pages[mid].row_start <= row) lo = mid; else hi = mid - 1;
    }
    const PqPage p = pages[lo];
    int64_t k = row - p.row_start;
    T v;
    __builtin_memcpy(&v, buf + p.values_off + k * (int64_t)sizeof(T), sizeof(T));
    out[row] = v;
  }
}

static inline int pq_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

AU_EXPORT int au_pq_scatter(const void* pages_dev, int npages, const void* buf,
                            const uint8_t* validity, const int64_t* prefix,
                            void* out, int esize, int64_t total, void* stream) {
  if (total == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  dim3 g(pq_grid(total)), b(256);
  if (esize == 4)
    hipLaunchKernelGGL((k_pq_scatter<uint32_t>), g, b, 0, s, (const PqPage*)pages_dev,
                       npages, (const uint8_t*)buf, validity, prefix, (uint32_t*)out, total);
  else
    hipLaunchKernelGGL((k_pq_scatter<uint64_t>), g, b, 0, s, (const PqPage*)pages_dev,
                       npages, (const uint8_t*)buf, validity, prefix, (uint64_t*)out, total);
  return (int)hipGetLastError();
}

AU_EXPORT int au_pq_copy_plain(const void* pages_dev, int npages, const void* buf,
                               void* out, int esize, int64_t total, void* stream) {
  if (total == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  dim3 g(pq_grid(total)), b(256);
  if (esize == 4)
    hipLaunchKernelGGL((k_pq_copy<uint32_t>), g, b, 0, s, (const PqPage*)pages_dev,
                       npages, (const uint8_t*)buf, (uint32_t*)out, total);
  else
    hipLaunchKernelGGL((k_pq_copy<uint64_t>), g, b, 0, s, (const PqPage*)pages_dev,
                       npages, (const uint8_t*)buf, (uint64_t*)out, total);
  return (int)hipGetLastError();
}

// Host-side walk of a PLAIN BYTE_ARRAY data-page payload:
// [u32 len][bytes][u32 len][bytes]... -> per-value (absolute offset, length).
// Returns the number of values parsed, or -1 on overflow/corruption.
// (arrow-rs does the equivalent offset materialization host-side too;
// the variable-length walk is inherently serial.)
AU_EXPORT int64_t au_host_plainba_parse(const uint8_t* buf, int64_t off,
                                        int64_t len, int64_t* offs,
                                        int32_t* lens, int64_t cap) {
  int64_t pos = off, end = off + len, n = 0;
  while (pos + 4 <= end) {
    uint32_t l = (uint32_t)buf[pos] | ((uint32_t)buf[pos + 1] << 8) |
                 ((uint32_t)buf[pos + 2] << 16) | ((uint32_t)buf[pos + 3] << 24);
    pos += 4;
    if ((int64_t)l > end - pos || n >= cap) return -1;
    offs[n] = pos;
    lens[n] = (int32_t)l;
    pos += l;
    n++;
  }
  return n;
}

// Host-side DELTA_BINARY_PACKED decode (parquet encoding 5) into PLAIN
// little-endian values (esize 4 or 8). Serial reference decoder: it is
// the scan path only when spark.auron.scan.deltaNative.enable is off
// (one "delta" host job per page, expanded bytes uploaded as PLAIN).
// With the switch on, au_host_delta_index below walks just the headers
// and the k_pq_delta_* kernels decode the values on the device.
// Returns values written, -1 on corruption.
static inline int64_t du_uvarint(const uint8_t* b, int64_t end, int64_t* pos,
                                 uint64_t* out) {
  uint64_t v = 0; int shift = 0;
  while (*pos < end) {
    uint8_t x = b[(*pos)++];
    v |= (uint64_t)(x & 0x7F) << shift;
    if (!(x & 0x80)) { *out = v; return 0; }
    shift += 7;
    if (shift > 63) return -1;
  }
  return -1;
}

AU_EXPORT int64_t au_host_delta_unpack(const uint8_t* buf, int64_t off,
                                       int64_t len, int64_t n, int esize,
                                       uint8_t* out) {
  int64_t pos = off, end = off + len;
  uint64_t block_size, nmini, total, ufirst;
  if (du_uvarint(buf, end, &pos, &block_size)) return -1;
  if (du_uvarint(buf, end, &pos, &nmini)) return -1;
  if (du_uvarint(buf, end, &pos, &total)) return -1;
  if (du_uvarint(buf, end, &pos, &ufirst)) return -1;
  if (nmini == 0 || block_size % nmini) return -1;
  // `n` is the output CAPACITY (page row count); the page encodes
  // `total` values (= present values when the column has nulls)
  if ((int64_t)total < n) n = (int64_t)total;
  if (n <= 0) return 0;
  int64_t per_mini = (int64_t)(block_size / nmini);
  int64_t value = (int64_t)((ufirst >> 1) ^ -(int64_t)(ufirst & 1));
  int64_t count = 0;
  #define EMIT(v) do { \
    if (esize == 4) { int32_t t = (int32_t)(v); __builtin_memcpy(out + 4 * count, &t, 4); } \
    else { int64_t t = (v); __builtin_memcpy(out + 8 * count, &t, 8); } \
    count++; } while (0)
  EMIT(value);
  while (count < n) {
    uint64_t umin;
    if (du_uvarint(buf, end, &pos, &umin)) return -1;
    int64_t min_delta = (int64_t)((umin >> 1) ^ -(int64_t)(umin & 1));
    if (pos + (int64_t)nmini > end) return -1;
    const uint8_t* bws = buf + pos;
    pos += nmini;
    for (uint64_t mb = 0; mb < nmini && count < n; mb++) {
      int bw = bws[mb];
      if (bw > 64) return -1;
      int64_t nbytes = (per_mini * bw + 7) / 8;
      if (pos + nbytes > end) return -1;
      // LSB-first bit unpack
      int64_t bit = 0;
      for (int64_t i = 0; i < per_mini && count < n; i++) {
        uint64_t d = 0;
        for (int got = 0; got < bw; ) {
          int64_t byte_i = pos + (bit >> 3);
          int within = (int)(bit & 7);
          int take = 8 - within;
          if (take > bw - got) take = bw - got;
          uint64_t bits = ((uint64_t)buf[byte_i] >> within) & ((1ULL << take) - 1);
          d |= bits << got;
          got += take;
          bit += take;
        }
        value += min_delta + (int64_t)d;
        EMIT(value);
      }
      pos += nbytes;
    }
  }
  #undef EMIT
  return count;
}

// ------------------------------------------------- DELTA_BINARY_PACKED
// Device decode of parquet encoding 5 (and of the length stream of
// encoding 6, DELTA_LENGTH_BYTE_ARRAY). Only the header walk is serial:
// one varint plus a few bit-width bytes per block. The host does that
// walk once per file (au_host_delta_index) and emits descriptors; the
// values are a bit-unpack plus a prefix sum and run here, one wave per
// miniblock:
//   k_pq_delta_sums   sums[m]  = sum of (min_delta + packed delta) of m
//   k_pq_delta_scan   sums[m] <- exclusive scan over the whole chunk
//   k_pq_delta_emit   value    = page first + (scan[m] - scan[page's
//                     first miniblock]) + inclusive wave scan inside m
// All arithmetic is unsigned 64-bit, i.e. exact under two's-complement
// wrap; INT32 columns keep the low 32 bits. No delta array is written
// to HBM: the emit kernel unpacks a second time instead.
//
// Page descriptor (int64 x 5):
//   [0]=first value  [1]=total values in the stream header
//   [2]=absolute byte offset of the stream's end
//   [3]=compact output index of the first value
//   [4]=index of the page's first miniblock descriptor
// Miniblock descriptor (int64 x 4), only miniblocks that hold values:
//   [0]=absolute byte offset of the bit data  [1]=min_delta
//   [2]=compact output index of its first value
//   [3]=bit width | values held << 8 | page index << 32
struct DlPage {
  int64_t first;
  int64_t total;
  int64_t end;
  int64_t out_base;
  int64_t mb_begin;
};

struct DlMini {
  int64_t byte_off;
  int64_t min_delta;
  int64_t out_idx;
  int64_t packed;
};

#define DL_MAX_BLOCK (1 << 24)  // values held must fit the 24-bit field

// Walks one page's stream; writes pg[5] and up to `cap` miniblock
// descriptors at `mb`. Returns the number of miniblocks, -1 on a corrupt
// or unsupported stream. Trailing miniblocks of the last block that hold
// no value are skipped without looking at their bit-width byte.
AU_EXPORT int64_t au_host_delta_index(const uint8_t* buf, int64_t off,
                                      int64_t len, int64_t n_rows,
                                      int64_t out_base, int64_t page_id,
                                      int64_t mb_begin, int64_t* pg,
                                      int64_t* mb, int64_t cap) {
  int64_t pos = off;
  const int64_t end = off + len;
  uint64_t block_size, nmini, total, ufirst;
  if (len < 0 || n_rows < 0) return -1;
  if (du_uvarint(buf, end, &pos, &block_size)) return -1;
  if (du_uvarint(buf, end, &pos, &nmini)) return -1;
  if (du_uvarint(buf, end, &pos, &total)) return -1;
  if (du_uvarint(buf, end, &pos, &ufirst)) return -1;
  if (nmini == 0 || block_size == 0 || block_size >= DL_MAX_BLOCK ||
      block_size % nmini)
    return -1;
  const int64_t per_mini = (int64_t)(block_size / nmini);
  if (per_mini % 32) return -1;
  if (total > (uint64_t)n_rows) return -1;
  pg[0] = (int64_t)((ufirst >> 1) ^ (~(ufirst & 1) + 1));
  pg[1] = (int64_t)total;
  pg[3] = out_base;
  pg[4] = mb_begin;
  int64_t remaining = total ? (int64_t)total - 1 : 0;
  int64_t o = out_base + 1;
  int64_t r = 0;
  while (remaining > 0) {
    uint64_t umin;
    if (du_uvarint(buf, end, &pos, &umin)) return -1;
    const int64_t min_delta = (int64_t)((umin >> 1) ^ (~(umin & 1) + 1));
    if (pos + (int64_t)nmini > end) return -1;
    const uint8_t* bws = buf + pos;
    pos += (int64_t)nmini;
    for (uint64_t i = 0; i < nmini && remaining > 0; i++) {
      const int64_t bw = bws[i];
      if (bw > 64) return -1;
      const int64_t cnt = remaining < per_mini ? remaining : per_mini;
      const int64_t need = (cnt * bw + 7) / 8;
      if (pos + need > end) return -1;
      if (r >= cap) return -1;
      mb[4 * r + 0] = pos;
      mb[4 * r + 1] = min_delta;
      mb[4 * r + 2] = o;
      mb[4 * r + 3] = bw | (cnt << 8) | (page_id << 32);
      // a short last miniblock is padded to its nominal size; tolerate a
      // writer that did not pad
      pos += per_mini * bw / 8;
      if (pos > end) pos = end;
      o += cnt;
      remaining -= cnt;
      r++;
    }
  }
  pg[2] = pos;
  return r;
}

// LSB-first unpack of value j of a miniblock, as in k_pq_rle_idx: one
// unaligned 8-byte word at bit>>3. The second word is read only when the
// value straddles the first one; those bytes belong to the miniblock, so
// no load goes beyond the staged buffer's 8-byte tail pad.
__device__ __forceinline__ uint64_t dl_unpack(const uint8_t* __restrict__ p,
                                              int64_t j, int bw,
                                              uint64_t mask) {
  if (bw == 0) return 0;
  const int64_t bit = j * bw;
  const uint8_t* q = p + (bit >> 3);
  const int sh = (int)(bit & 7);
  uint64_t w;
  __builtin_memcpy(&w, q, 8);
  uint64_t v = w >> sh;
  if (sh + bw > 64) {  // implies sh >= 1
    uint64_t w2;
    __builtin_memcpy(&w2, q + 8, 8);
    v |= w2 << (64 - sh);
  }
  return v & mask;
}

__global__ void k_pq_delta_sums(const DlMini* __restrict__ mb, int64_t nmb,
                                const uint8_t* __restrict__ buf,
                                uint64_t* __restrict__ sums) {
  const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int lane = threadIdx.x & 63;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t m = wave; m < nmb; m += nwaves) {  // wave-uniform
    const DlMini d = mb[m];
    const int bw = (int)(d.packed & 0xFF);
    const int64_t count = (d.packed >> 8) & 0xFFFFFF;
    const uint64_t mask = bw >= 64 ? ~0ull : ((1ull << bw) - 1);
    const uint8_t* src = buf + d.byte_off;
    unsigned long long s = 0;
    for (int64_t j = lane; j < count; j += 64)
      s += (uint64_t)d.min_delta + dl_unpack(src, j, bw, mask);
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) sums[m] = s;
  }
}

// In-place exclusive scan of the per-miniblock sums, one 256-thread block,
// 8 entries per thread and round (the input is n/32 to n/64 entries).
#define DL_SCAN_ITEMS 8
__global__ void __launch_bounds__(256)
k_pq_delta_scan(uint64_t* __restrict__ x, int64_t n) {
  __shared__ uint64_t wtot[4];
  const int lane = threadIdx.x & 63;
  const int wv = threadIdx.x >> 6;
  uint64_t carry = 0;
  for (int64_t c = 0; c < n; c += 256 * DL_SCAN_ITEMS) {  // block-uniform
    const int64_t b = c + (int64_t)threadIdx.x * DL_SCAN_ITEMS;
    uint64_t v[DL_SCAN_ITEMS];
    unsigned long long tsum = 0;
#pragma unroll
    for (int k = 0; k < DL_SCAN_ITEMS; k++) {
      v[k] = b + k < n ? x[b + k] : 0;
      tsum += v[k];
    }
    unsigned long long incl = tsum;
    for (int d = 1; d < 64; d <<= 1) {
      const unsigned long long t = __shfl_up(incl, d, 64);
      if (lane >= d) incl += t;
    }
    if (lane == 63) wtot[wv] = incl;
    __syncthreads();
    uint64_t woff = 0, round = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
      if (w < wv) woff += wtot[w];
      round += wtot[w];
    }
    uint64_t excl = carry + woff + (incl - tsum);
#pragma unroll
    for (int k = 0; k < DL_SCAN_ITEMS; k++) {
      if (b + k < n) x[b + k] = excl;
      excl += v[k];
    }
    carry += round;
    __syncthreads();  // wtot is rewritten next round
  }
}

template <typename T>
__global__ void k_pq_delta_emit(const DlMini* __restrict__ mb, int64_t nmb,
                                const DlPage* __restrict__ pg, int64_t npages,
                                const uint8_t* __restrict__ buf,
                                const uint64_t* __restrict__ excl,
                                T* __restrict__ out) {
  const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t nthreads = (int64_t)gridDim.x * blockDim.x;
  const int lane = threadIdx.x & 63;
  for (int64_t m = tid >> 6; m < nmb; m += nthreads >> 6) {  // wave-uniform
    const DlMini d = mb[m];
    const int bw = (int)(d.packed & 0xFF);
    const int64_t count = (d.packed >> 8) & 0xFFFFFF;
    const DlPage p = pg[d.packed >> 32];
    const uint64_t mask = bw >= 64 ? ~0ull : ((1ull << bw) - 1);
    const uint8_t* src = buf + d.byte_off;
    uint64_t carry = (uint64_t)p.first + (excl[m] - excl[p.mb_begin]);
    for (int64_t s = 0; s < count; s += 64) {  // 64-lane strips
      const int64_t j = s + lane;
      unsigned long long incl =
          j < count ? (uint64_t)d.min_delta + dl_unpack(src, j, bw, mask) : 0;
      for (int k = 1; k < 64; k <<= 1) {
        const unsigned long long t = __shfl_up(incl, k, 64);
        if (lane >= k) incl += t;
      }
      if (j < count) out[d.out_idx + j] = (T)(carry + incl);
      carry += __shfl(incl, 63, 64);
    }
  }
  // every page's first value, pages without any miniblock included
  for (int64_t i = tid; i < npages; i += nthreads) {
    const DlPage p = pg[i];
    if (p.total > 0) out[p.out_base] = (T)(uint64_t)p.first;
  }
}

static inline int dl_grid(int64_t nmb) {
  int64_t g = (nmb * 64 + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

AU_EXPORT int au_pq_delta_sums(const void* mb_dev, int64_t nmb,
                               const void* buf, void* sums, void* stream) {
  if (nmb <= 0) return 0;
  hipLaunchKernelGGL(k_pq_delta_sums, dim3(dl_grid(nmb)), dim3(256), 0,
                     (hipStream_t)stream, (const DlMini*)mb_dev, nmb,
                     (const uint8_t*)buf, (uint64_t*)sums);
  return (int)hipGetLastError();
}

AU_EXPORT int au_pq_delta_scan(void* sums, int64_t nmb, void* stream) {
  if (nmb <= 0) return 0;
  hipLaunchKernelGGL(k_pq_delta_scan, dim3(1), dim3(256), 0,
                     (hipStream_t)stream, (uint64_t*)sums, nmb);
  return (int)hipGetLastError();
}

// `out` holds the compact per-present-value array: int32 (esize 4, low 32
// bits of each value) or int64 (esize 8).
AU_EXPORT int au_pq_delta_emit(const void* mb_dev, int64_t nmb,
                               const void* pg_dev, int64_t npages,
                               const void* buf, const void* excl, void* out,
                               int esize, void* stream) {
  if (npages <= 0) return 0;
  if (esize != 4 && esize != 8) return (int)hipErrorInvalidValue;
  hipStream_t s = (hipStream_t)stream;
  dim3 g(dl_grid(nmb)), b(256);
  if (esize == 4)
    hipLaunchKernelGGL((k_pq_delta_emit<uint32_t>), g, b, 0, s,
                       (const DlMini*)mb_dev, nmb, (const DlPage*)pg_dev,
                       npages, (const uint8_t*)buf, (const uint64_t*)excl,
                       (uint32_t*)out);
  else
    hipLaunchKernelGGL((k_pq_delta_emit<uint64_t>), g, b, 0, s,
                       (const DlMini*)mb_dev, nmb, (const DlPage*)pg_dev,
                       npages, (const uint8_t*)buf, (const uint64_t*)excl,
                       (uint64_t*)out);
  return (int)hipGetLastError();
}

// ---------------------------------------------------- DELTA_BYTE_ARRAY
// Parquet encoding 7: a page is two DELTA_BINARY_PACKED streams (prefix
// lengths, suffix lengths) and the suffix bytes. String i is the first
// P[i] bytes of string i-1 followed by suffix i. The lengths come from the
// k_pq_delta_* kernels; what is left is the byte reconstruction, which
// looks serial because every string leans on the one before.
//
// Serial host reference, bounds-checked: the oracle for k_pq_dba_bytes
// and the CPU read path. P/S = prefix/suffix lengths, so = absolute
// offset of each suffix in buf, O = output offset of each string.
// Returns 0, or -1 when an entry points outside buf/out or a prefix is
// longer than the string before.
AU_EXPORT int64_t au_host_dba_decode(const uint8_t* buf, int64_t buf_len,
                                     const int64_t* P, const int64_t* S,
                                     const int64_t* so, const int64_t* O,
                                     int64_t n, uint8_t* out,
                                     int64_t out_len) {
  int64_t prev_o = 0, prev_l = 0;
  for (int64_t i = 0; i < n; i++) {
    const int64_t p = P[i], s = S[i], o = O[i], src = so[i];
    if (p < 0 || s < 0 || p > prev_l) return -1;
    if (o < 0 || o > out_len || p > out_len - o || s > out_len - o - p)
      return -1;
    if (src < 0 || src > buf_len || s > buf_len - src) return -1;
    for (int64_t j = 0; j < p; j++) out[o + j] = out[prev_o + j];
    for (int64_t j = 0; j < s; j++) out[o + p + j] = buf[src + j];
    prev_o = o;
    prev_l = p + s;
  }
  return 0;
}

// Device reconstruction without any store->load dependency through
// memory. One wave owns a segment of `seg` consecutive values of the
// chunk's compact stream (pages are nothing special: so[] is absolute)
// and keeps the "current string" position-striped in registers: lane l
// holds byte positions t0 + l + 64*r of the tile [t0, t0 + DBA_TILE).
// For string i, positions P[i] <= j < L[i] are loaded from suffix i and
// overwrite the tile, positions j < L[i] are stored to out[O[i] + j], and
// positions j < P[i] are simply what the string before left there. A lane
// only ever touches its own positions: no barrier, no cross-lane bytes.
//
// Seed: before its first string s0 the tile must hold positions
// j < P[s0] of string s0-1. Walking back k = s0-1, s0-2, ... with
// need = min(P[s0], t0 + DBA_TILE): whenever P[k] < need, positions
// [max(P[k], t0), need) are bytes of suffix k, and need = P[k]; done when
// need <= t0. The walk takes 64 P[k] per step (running minimum by wave
// scan) and reads source bytes only, never another wave's output.
// P[0] == 0 ends every walk at the latest.
//
// Strings longer than the tile repeat seed and forward pass per tile;
// strings that end before t0 contribute nothing to that tile (the next
// string's prefix cannot reach into it either).
//
// The kernel trusts its inputs like k_pq_delta_emit: the caller has
// checked P, S >= 0, P[0] == 0, P[i] <= L[i-1], and that every suffix
// lies inside its page. Metadata loads in the forward pass are
// wave-uniform; all stores are per-lane byte stores.
#define DBA_TILE 256
#define DBA_REGS (DBA_TILE / 64)

__device__ __forceinline__ int64_t dba_lane64(int64_t v, int lane) {
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)(uint64_t)v, lane);
  const uint32_t hi =
      __builtin_amdgcn_readlane((uint32_t)((uint64_t)v >> 32), lane);
  return (int64_t)(((uint64_t)hi << 32) | lo);
}

__global__ void __launch_bounds__(256)
k_pq_dba_bytes(const int64_t* __restrict__ P, const int64_t* __restrict__ S,
               const int64_t* __restrict__ so, const int64_t* __restrict__ O,
               int64_t n, int64_t seg, const uint8_t* __restrict__ buf,
               uint8_t* __restrict__ out) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * 4 +
                       __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t nwaves = (int64_t)gridDim.x * 4;
  const int64_t nseg = (n + seg - 1) / seg;
  for (int64_t g = wave; g < nseg; g += nwaves) {  // wave-uniform
    const int64_t s0 = g * seg;
    const int64_t s1 = s0 + seg < n ? s0 + seg : n;
    // longest string of the segment: how many tiles it takes
    int64_t maxl = 0;
    for (int64_t i = s0 + lane; i < s1; i += 64) {
      const int64_t l = P[i] + S[i];
      maxl = l > maxl ? l : maxl;
    }
    for (int off = 32; off > 0; off >>= 1) {
      const int64_t t = __shfl_xor((long long)maxl, off, 64);
      maxl = t > maxl ? t : maxl;
    }
    maxl = dba_lane64(maxl, 0);
    const int64_t p0 = P[s0];
    for (int64_t t0 = 0; t0 < maxl; t0 += DBA_TILE) {
      uint8_t tile[DBA_REGS];
#pragma unroll
      for (int r = 0; r < DBA_REGS; r++) tile[r] = 0;

      // ---- seed: positions [t0, need) of string s0-1
      int64_t need = p0 < t0 + DBA_TILE ? p0 : t0 + DBA_TILE;
      for (int64_t kb = s0 - 1; need > t0; kb -= 64) {
        const int64_t k = kb - lane;
        const int64_t pk = k >= 0 ? P[k] : 0;
        // inclusive running minimum over need, P[kb], P[kb-1], ...
        int64_t incl = pk < need ? pk : need;
        for (int d = 1; d < 64; d <<= 1) {
          const int64_t t = __shfl_up((long long)incl, d, 64);
          if (lane >= d && t < incl) incl = t;
        }
        int64_t before = __shfl_up((long long)incl, 1, 64);
        if (lane == 0) before = need;
        // strings whose suffix supplies positions [max(pk, t0), before)
        unsigned long long m = __ballot(pk < before && before > t0);
        while (m) {  // wave-uniform
          const int b = __ffsll(m) - 1;
          m &= m - 1;
          const int64_t pb = dba_lane64(pk, b);
          const int64_t hi = dba_lane64(before, b);
          const int64_t lo = pb > t0 ? pb : t0;
          const uint8_t* src = buf + (so[kb - b] - pb);
#pragma unroll
          for (int r = 0; r < DBA_REGS; r++) {
            const int64_t j = t0 + lane + 64 * r;
            if (j >= lo && j < hi) tile[r] = src[j];
          }
        }
        need = dba_lane64(incl, 63);
      }

      // ---- forward pass over the segment's strings
      for (int64_t i = s0; i < s1; i++) {
        const int64_t p = P[i];
        const int64_t l = p + S[i];
        if (l <= t0) continue;
        const uint8_t* src = buf + (so[i] - p);
        uint8_t* dst = out + O[i];
#pragma unroll
        for (int r = 0; r < DBA_REGS; r++) {
          if (t0 + 64 * r >= l) break;  // wave-uniform
          const int64_t j = t0 + lane + 64 * r;
          if (j >= p && j < l) tile[r] = src[j];
          if (j < l) dst[j] = tile[r];
        }
      }
    }
  }
}

AU_EXPORT int64_t au_pq_dba_tile() { return DBA_TILE; }

// P, S, so, O: int64[n] device arrays of the chunk's compact stream;
// `seg` values per wave; out holds sum(P + S) bytes.
AU_EXPORT int au_pq_dba_bytes(const void* P, const void* S, const void* so,
                              const void* O, int64_t n, int64_t seg,
                              const void* buf, void* out, void* stream) {
  if (n <= 0) return 0;
  if (seg <= 0) return (int)hipErrorInvalidValue;
  const int64_t nseg = (n + seg - 1) / seg;
  int64_t g = (nseg + 3) / 4;
  if (g > 2048) g = 2048;
  hipLaunchKernelGGL(k_pq_dba_bytes, dim3((uint32_t)g), dim3(256), 0,
                     (hipStream_t)stream, (const int64_t*)P,
                     (const int64_t*)S, (const int64_t*)so,
                     (const int64_t*)O, n, seg, (const uint8_t*)buf,
                     (uint8_t*)out);
  return (int)hipGetLastError();
}
