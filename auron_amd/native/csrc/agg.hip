// Aggregate accumulation kernels — gfx950.
//
// Role parity: the reference's per-function accumulators
// (datafusion-ext-plans/src/agg/acc.rs + sum/maxmin/count). On MI355X
// the accumulate is a scatter with device-scope atomics over the
// group-id array produced by k_group_insert (kernels.hip). Replaces
// torch's scatter_add_ path, which measured ~400x slower than the
// atomic scatter on fp64 (rocprof: 5.5s per 14M-row scatter).
//
// value dtypes: f64 (code 0), i64 (code 1), i32 (code 2), f32 (code 3).
// ops: sum=0, min=1, max=2. Sums accumulate in f64 or i64 (widened); MIN
// and MAX always in i64, floats as their order keys (f64_order_key).
// count (valid-row count per group) accumulates alongside when
// `counts` is non-null.

#include <hip/hip_runtime.h>
#include <stdint.h>

#define AU_EXPORT extern "C" __attribute__((visibility("default")))

static inline int agg_grid(int64_t n) {
  int64_t g = (n + 255) / 256;
  if (g > 2048) g = 2048;
  if (g < 1) g = 1;
  return (int)g;
}

// Float MIN/MAX run on int64 order keys, not on the doubles: the key of a
// double is its bit pattern with the low 63 bits flipped when the sign is
// set, every NaN first replaced by the canonical 0x7ff8000000000000. Signed
// integer order on the keys is then the aggregate order
//   -inf < ... < -0.0 < 0.0 < ... < +inf < NaN
// (NaN the greatest value: MAX is NaN if any input is, MIN only if all
// are), the result no longer depends on lane position or on which atomic
// lands first, and the int64 identities INT64_MAX / INT64_MIN lie outside
// the keys of all doubles, so a group of NaNs alone still leaves the
// identity. The host decodes the accumulator (ops._f64_from_order_keys).
__device__ __forceinline__ int64_t f64_order_key(double v) {
  int64_t b = (v != v) ? (int64_t)0x7ff8000000000000ll : __double_as_longlong(v);
  return b ^ ((b >> 63) & INT64_MAX);
}

__device__ __forceinline__ void atomic_min_i64(int64_t* addr, int64_t v) {
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a, assumed;
  do {
    assumed = old;
    if (v >= (int64_t)assumed) return;
    old = atomicCAS(a, assumed, (unsigned long long)v);
  } while (old != assumed);
}

__device__ __forceinline__ void atomic_max_i64(int64_t* addr, int64_t v) {
  unsigned long long* a = (unsigned long long*)addr;
  unsigned long long old = *a, assumed;
  do {
    assumed = old;
    if (v <= (int64_t)assumed) return;
    old = atomicCAS(a, assumed, (unsigned long long)v);
  } while (old != assumed);
}

// Wave-segmented scatter: lanes load 64 consecutive rows (coalesced),
// then a shfl-based segmented reduction combines lanes sharing a group
// id BEFORE touching global atomics. Group-by outputs are usually
// correlated with input order (rollups over sorted-ish facts produce
// long equal-gid runs), so this collapses most atomics; for random gids
// it degrades gracefully to one atomic per lane plus 6 shfl rounds.
template <typename VT, bool ACC_F64>
__global__ void k_agg_scatter(const int64_t* gids, int64_t n, const uint8_t* validity,
                              const VT* values, int op, void* acc, int64_t* counts) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_global = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = wave_global * 64; base < n; base += nwaves * 64) {
    int64_t i = base + lane;
    bool live = i < n && (!validity || validity[i]);
    int64_t g = (i < n) ? gids[i] : (int64_t)-1;
    if (ACC_F64 && op == 0) {
      double v = live ? (double)values[i] : 0.0;
      int64_t c = live ? 1 : 0;
      // head-flag segmented inclusive scan (a gid may recur in separate
      // runs within the wave; plain gid-equality folding would double
      // count across the intervening segment)
      int64_t pg1 = __shfl_up(g, 1, 64);
      int flag = (lane == 0) || (pg1 != g);
      for (int d = 1; d < 64; d <<= 1) {
        double pv = __shfl_up(v, d, 64);
        int64_t pc = __shfl_up(c, d, 64);
        int pf = __shfl_up(flag, d, 64);
        if (lane >= d) {
          if (!flag) {
            v += pv;
            c += pc;
          }
          flag = flag || pf;
        }
      }
      int64_t ng = __shfl_down(g, 1, 64);
      bool seg_last = (lane == 63) || (ng != g);
      if (seg_last && g >= 0 && c > 0) {
        if (counts) atomicAdd((unsigned long long*)&counts[g], (unsigned long long)c);
        atomicAdd(&((double*)acc)[g], v);
      }
    } else {
      // integer values, and float MIN/MAX on order keys
      int64_t ident = op == 0 ? 0 : (op == 1 ? INT64_MAX : INT64_MIN);
      int64_t v = !live ? ident
                  : ACC_F64 ? f64_order_key((double)values[i]) : (int64_t)values[i];
      int64_t c = live ? 1 : 0;
      int64_t pg1 = __shfl_up(g, 1, 64);
      int flag = (lane == 0) || (pg1 != g);
      for (int d = 1; d < 64; d <<= 1) {
        int64_t pv = __shfl_up(v, d, 64);
        int64_t pc = __shfl_up(c, d, 64);
        int pf = __shfl_up(flag, d, 64);
        if (lane >= d) {
          if (!flag) {
            if (op == 0) v += pv;
            else if (op == 1) v = v < pv ? v : pv;
            else v = v > pv ? v : pv;
            c += pc;
          }
          flag = flag || pf;
        }
      }
      int64_t ng = __shfl_down(g, 1, 64);
      bool seg_last = (lane == 63) || (ng != g);
      if (seg_last && g >= 0 && c > 0) {
        int64_t* a = (int64_t*)acc;
        if (counts) atomicAdd((unsigned long long*)&counts[g], (unsigned long long)c);
        if (op == 0) atomicAdd((unsigned long long*)&a[g], (unsigned long long)v);
        else if (op == 1) atomic_min_i64(&a[g], v);
        else atomic_max_i64(&a[g], v);
      }
    }
  }
}

// ------------------------------------------------------- LDS-staged path
// For small group counts the global-atomic scatter serializes on hot
// accumulator addresses (every lane of every CU hits the same few
// cachelines). Stage per-workgroup partial accumulators in LDS (shared
// atomics are per-CU, no cross-XCD traffic), then flush once per group
// per block. Selected by the host when ngroups fits in 64 KB of LDS and
// n is large enough to amortize the flush.
__device__ __forceinline__ void lds_min_i64(unsigned long long* a, int64_t v) {
  unsigned long long old = *a, assumed;
  do {
    assumed = old;
    if (v >= (int64_t)assumed) return;
    old = atomicCAS(a, assumed, (unsigned long long)v);
  } while (old != assumed);
}

__device__ __forceinline__ void lds_max_i64(unsigned long long* a, int64_t v) {
  unsigned long long old = *a, assumed;
  do {
    assumed = old;
    if (v <= (int64_t)assumed) return;
    old = atomicCAS(a, assumed, (unsigned long long)v);
  } while (old != assumed);
}

template <typename VT, bool ACC_F64>
__global__ void k_agg_scatter_lds(const int64_t* gids, int64_t n,
                                  const uint8_t* validity, const VT* values,
                                  int op, void* acc, int64_t* counts,
                                  int ngroups, unsigned long long init_bits) {
  extern __shared__ unsigned long long smem[];
  unsigned long long* sacc = smem;
  unsigned long long* scnt = counts ? smem + ngroups : nullptr;
  for (int i = threadIdx.x; i < ngroups; i += blockDim.x) {
    sacc[i] = init_bits;
    if (scnt) scnt[i] = 0;
  }
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    if (validity && !validity[i]) continue;
    int g = (int)gids[i];
    if (scnt) atomicAdd(&scnt[g], 1ull);
    if (ACC_F64 && op == 0) {
      atomicAdd((double*)&sacc[g], (double)values[i]);
    } else {
      int64_t v = ACC_F64 ? f64_order_key((double)values[i]) : (int64_t)values[i];
      if (op == 0) atomicAdd(&sacc[g], (unsigned long long)v);
      else if (op == 1) lds_min_i64(&sacc[g], v);
      else lds_max_i64(&sacc[g], v);
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < ngroups; i += blockDim.x) {
    if (scnt && scnt[i]) atomicAdd((unsigned long long*)&counts[i], scnt[i]);
    if (sacc[i] == init_bits) continue;  // untouched (or identity: no-op)
    if (ACC_F64 && op == 0) {
      atomicAdd(&((double*)acc)[i], __longlong_as_double((long long)sacc[i]));
    } else {
      int64_t v = (int64_t)sacc[i];
      int64_t* a = (int64_t*)acc;
      if (op == 0) atomicAdd((unsigned long long*)&a[i], (unsigned long long)v);
      else if (op == 1) atomic_min_i64(&a[i], v);
      else atomic_max_i64(&a[i], v);
    }
  }
}

// ----------------------------------------------------------- fused multi
// All aggregates of one HashAgg in a single pass: gids are read once and
// the wave head-flags are computed once; each aggregate folds through
// the same segmented scan and flushes its own accumulator.
// AggDesc layout (int64 x 6, packed host-side):
//   [0]=values ptr [1]=validity ptr(0=none) [2]=vtype(0 f64,1 i64,2 i32,3 f32)
//   [3]=op(0 sum,1 min,2 max) [4]=acc ptr [5]=counts ptr(0=none)
// acc is f64 for a float sum and i64 for everything else (see f64_order_key)
struct AggDesc {
  const void* values;
  const uint8_t* validity;
  int64_t vtype;
  int64_t op;
  void* acc;
  int64_t* counts;
};

__device__ __forceinline__ double agg_load_f64(const void* v, int64_t vt, int64_t i) {
  switch (vt) {
    case 0: return ((const double*)v)[i];
    case 3: return (double)((const float*)v)[i];
    case 2: return (double)((const int32_t*)v)[i];
    default: return (double)((const int64_t*)v)[i];
  }
}

__device__ __forceinline__ int64_t agg_load_i64(const void* v, int64_t vt, int64_t i) {
  return vt == 2 ? (int64_t)((const int32_t*)v)[i] : ((const int64_t*)v)[i];
}

__global__ void k_agg_multi(const int64_t* gids, int64_t n, const AggDesc* descs,
                            int ndescs) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_global = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = wave_global * 64; base < n; base += nwaves * 64) {
    int64_t i = base + lane;
    int64_t g = (i < n) ? gids[i] : (int64_t)-1;
    int64_t pg1 = __shfl_up(g, 1, 64);
    int head = (lane == 0) || (pg1 != g);
    int64_t ng = __shfl_down(g, 1, 64);
    bool seg_last = (lane == 63) || (ng != g);
    for (int a = 0; a < ndescs; a++) {
      const AggDesc d = descs[a];
      bool live = i < n && (!d.validity || d.validity[i]);
      bool f64p = d.vtype == 0 || d.vtype == 3;
      int64_t c = live ? 1 : 0;
      int flag = head;
      if (f64p && d.op == 0) {
        double v = live ? agg_load_f64(d.values, d.vtype, i) : 0.0;
        for (int dd = 1; dd < 64; dd <<= 1) {
          double pv = __shfl_up(v, dd, 64);
          int64_t pc = __shfl_up(c, dd, 64);
          int pf = __shfl_up(flag, dd, 64);
          if (lane >= dd) {
            if (!flag) {
              v += pv;
              c += pc;
            }
            flag = flag || pf;
          }
        }
        if (seg_last && g >= 0 && c > 0) {
          if (d.counts) atomicAdd((unsigned long long*)&d.counts[g], (unsigned long long)c);
          atomicAdd(&((double*)d.acc)[g], v);
        }
      } else {
        // integer values, and float MIN/MAX on order keys
        int64_t ident = d.op == 0 ? 0 : (d.op == 1 ? INT64_MAX : INT64_MIN);
        int64_t v = !live ? ident
                    : f64p ? f64_order_key(agg_load_f64(d.values, d.vtype, i))
                           : agg_load_i64(d.values, d.vtype, i);
        for (int dd = 1; dd < 64; dd <<= 1) {
          int64_t pv = __shfl_up(v, dd, 64);
          int64_t pc = __shfl_up(c, dd, 64);
          int pf = __shfl_up(flag, dd, 64);
          if (lane >= dd) {
            if (!flag) {
              if (d.op == 0) v += pv;
              else if (d.op == 1) v = v < pv ? v : pv;
              else v = v > pv ? v : pv;
              c += pc;
            }
            flag = flag || pf;
          }
        }
        if (seg_last && g >= 0 && c > 0) {
          int64_t* acc = (int64_t*)d.acc;
          if (d.counts) atomicAdd((unsigned long long*)&d.counts[g], (unsigned long long)c);
          if (d.op == 0) atomicAdd((unsigned long long*)&acc[g], (unsigned long long)v);
          else if (d.op == 1) atomic_min_i64(&acc[g], v);
          else atomic_max_i64(&acc[g], v);
        }
      }
    }
  }
}

AU_EXPORT int au_agg_multi(const int64_t* gids, int64_t n, const void* descs_dev,
                           int ndescs, void* stream) {
  if (n == 0 || ndescs == 0) return 0;
  hipLaunchKernelGGL(k_agg_multi, dim3(agg_grid(n)), dim3(256), 0,
                     (hipStream_t)stream, gids, n, (const AggDesc*)descs_dev,
                     ndescs);
  return (int)hipGetLastError();
}

// count-only (count_star / count of a validity-masked column);
// wave-segmented like k_agg_scatter
__global__ void k_agg_count(const int64_t* gids, int64_t n, const uint8_t* validity,
                            int64_t* counts) {
  const int lane = threadIdx.x & 63;
  const int64_t wave_global = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int64_t nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
  for (int64_t base = wave_global * 64; base < n; base += nwaves * 64) {
    int64_t i = base + lane;
    bool live = i < n && (!validity || validity[i]);
    int64_t g = (i < n) ? gids[i] : (int64_t)-1;
    int64_t c = live ? 1 : 0;
    int64_t pg1 = __shfl_up(g, 1, 64);
    int flag = (lane == 0) || (pg1 != g);
    for (int d = 1; d < 64; d <<= 1) {
      int64_t pc = __shfl_up(c, d, 64);
      int pf = __shfl_up(flag, d, 64);
      if (lane >= d) {
        if (!flag) c += pc;
        flag = flag || pf;
      }
    }
    int64_t ng = __shfl_down(g, 1, 64);
    bool seg_last = (lane == 63) || (ng != g);
    if (seg_last && g >= 0 && c > 0)
      atomicAdd((unsigned long long*)&counts[g], (unsigned long long)c);
  }
}

AU_EXPORT int au_agg_scatter(const int64_t* gids, int64_t n, const uint8_t* validity,
                             const void* values, int vtype, int op, int acc_f64,
                             void* acc, int64_t* counts, int64_t ngroups,
                             void* stream) {
  if (n == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  // LDS staging: accumulators (+counts) must fit in 64 KB and the row
  // count must amortize the per-block flush (grid*ngroups global atomics)
  int slots = counts ? 2 : 1;
  bool use_lds = ngroups > 0 && ngroups * slots * 8 <= (64 << 10) &&
                 n >= 16 * ngroups;
  if (use_lds) {
    unsigned long long init;
    if (op == 0) init = 0ull;  // sum identity (0.0 and 0 share the bit pattern)
    else init = (unsigned long long)(op == 1 ? INT64_MAX : INT64_MIN);  // keys too
    int64_t g64 = (n + 255) / 256;
    int64_t cap = n / (16 * ngroups) + 1;  // keep flush << accumulate
    if (g64 > cap) g64 = cap;
    if (g64 > 2048) g64 = 2048;
    if (g64 < 1) g64 = 1;
    dim3 g((int)g64), b(256);
    size_t smem = (size_t)ngroups * slots * 8;
#define CASE_LDS(VT)                                                              \
    if (acc_f64)                                                                  \
      hipLaunchKernelGGL((k_agg_scatter_lds<VT, true>), g, b, smem, s, gids, n,   \
                         validity, (const VT*)values, op, acc, counts,            \
                         (int)ngroups, init);                                     \
    else                                                                          \
      hipLaunchKernelGGL((k_agg_scatter_lds<VT, false>), g, b, smem, s, gids, n,  \
                         validity, (const VT*)values, op, acc, counts,            \
                         (int)ngroups, init);
    if (vtype == 0) { CASE_LDS(double) }
    else if (vtype == 1) { CASE_LDS(int64_t) }
    else if (vtype == 2) { CASE_LDS(int32_t) }
    else { CASE_LDS(float) }
#undef CASE_LDS
    return (int)hipGetLastError();
  }
  dim3 g(agg_grid(n)), b(256);
#define CASE(VT)                                                                  \
  if (acc_f64)                                                                    \
    hipLaunchKernelGGL((k_agg_scatter<VT, true>), g, b, 0, s, gids, n, validity,  \
                       (const VT*)values, op, acc, counts);                       \
  else                                                                            \
    hipLaunchKernelGGL((k_agg_scatter<VT, false>), g, b, 0, s, gids, n, validity, \
                       (const VT*)values, op, acc, counts);
  if (vtype == 0) { CASE(double) }
  else if (vtype == 1) { CASE(int64_t) }
  else if (vtype == 2) { CASE(int32_t) }
  else { CASE(float) }
#undef CASE
  return (int)hipGetLastError();
}

AU_EXPORT int au_agg_count(const int64_t* gids, int64_t n, const uint8_t* validity,
                           int64_t* counts, void* stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(k_agg_count, dim3(agg_grid(n)), dim3(256), 0,
                     (hipStream_t)stream, gids, n, validity, counts);
  return (int)hipGetLastError();
}
