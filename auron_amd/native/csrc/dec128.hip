// Auron-AMD native engine — exact decimal128 arithmetic, comparison and
// rescale kernels, gfx950 (MI355X, CDNA4) only.
//
// A decimal128 value is a scaled 128-bit integer: two int64 limbs
// [lo bit pattern, hi signed], row-major [n,2] (the Column layout). Every
// operand here is either such a limb array (16-byte loads) or a plain int64
// [n] array (decimal64 / integer backing) that the kernel sign-extends on
// load; no widened temporary exists anywhere.
//
// Every operation has one shape: split sign and magnitude, build an exact
// magnitude of up to 256 bits, divide it by a 128-bit divisor (a power of
// ten, or |b| for the division) rounding HALF_UP on the magnitude (ties away
// from zero), and null the row when the rounded magnitude reaches `bound`
// (10^p of the result type). Overflow and division by zero only ever clear
// the row's validity byte: nothing is reported to the host.
//
//   au_dec128_addsub   (a*10^ka +- b*10^kb) / 10^d
//   au_dec128_mul      (a*b) / 10^d
//   au_dec128_div      round_half_up(a*10^k / b), null when b == 0
//   au_dec128_cmp      a*10^ka <op> b*10^kb, aligned in 256 bits
//   au_dec128_rescale  x*10^k or x/10^k, optional abs / negate / truncation,
//                      limb or int64 output (casts, CheckOverflow, abs)
//
// The arithmetic kernels take the operands' validity bytes (nullable) and
// write the final validity; a null row stores zero limbs. Powers of ten come
// from a host table (10^0 .. 10^38) and travel as kernel arguments, so they
// sit in scalar registers. The 256-bit state is two `unsigned __int128`
// scalars, never an indexed array.
//
// One row per thread, grid-stride, grid capped like wn_grid / rp_grid.
// C ABI only — loaded via ctypes from auron_amd/native/__init__.py. All
// pointers are device pointers owned by torch; `stream` is the torch current
// stream. No allocation happens here.

#include <hip/hip_runtime.h>
#include <stdint.h>

#define AU_EXPORT extern "C" __attribute__((visibility("default")))

typedef unsigned __int128 dx_u128;

#define DX_BLOCK 256
#define DX_MAX_GRID 2048  // 256 CU x 8, same cap as wn_grid / rp_grid
#define DX_MAX_POW10 38

// rescale flags
#define DX_ABS 1       // result takes the magnitude
#define DX_NEGATE 2    // result changes sign
#define DX_TRUNCATE 4  // divide truncating toward zero instead of HALF_UP
#define DX_ASYM 8      // two's-complement range: -bound itself is kept

// comparison operators
#define DX_EQ 0
#define DX_NE 1
#define DX_LT 2
#define DX_LE 3
#define DX_GT 4
#define DX_GE 5

static inline int dx_grid(int64_t n) {
  int64_t g = (n + DX_BLOCK - 1) / DX_BLOCK;
  if (g > DX_MAX_GRID) g = DX_MAX_GRID;  // grid-stride the rest
  if (g < 1) g = 1;
  return (int)g;
}

// Threads of the largest grid: one more row than this wraps the grid-stride
// loop.
AU_EXPORT int64_t au_dec128_grid_threads() {
  return (int64_t)DX_MAX_GRID * DX_BLOCK;
}

struct alignas(16) DxI128 {
  uint64_t lo;  // low 64 bits, bit pattern
  int64_t hi;   // high 64 bits, signed
};

struct DxU256 {
  dx_u128 lo, hi;
};

// a 128-bit unsigned kernel argument
struct DxArg128 {
  uint64_t lo, hi;
};

__host__ __device__ __forceinline__ dx_u128 dx_arg(DxArg128 a) {
  return ((dx_u128)a.hi << 64) | a.lo;
}

// 10^k as a kernel argument; k in [0, 38]
static DxArg128 dx_pow10(int k) {
  dx_u128 v = 1;
  for (int i = 0; i < k; i++) v *= 10;
  DxArg128 a;
  a.lo = (uint64_t)v;
  a.hi = (uint64_t)(v >> 64);
  return a;
}

// Sign/magnitude split of row i. `narrow` selects the int64 [n] form.
__host__ __device__ __forceinline__ dx_u128
dx_load_mag(const void* __restrict__ p, int narrow, int64_t i, bool* neg) {
  dx_u128 bits;
  if (narrow) {
    const int64_t v = ((const int64_t*)p)[i];
    *neg = v < 0;
    bits = (dx_u128)(__int128)v;
  } else {
    const DxI128 v = ((const DxI128*)p)[i];
    *neg = v.hi < 0;
    bits = ((dx_u128)(uint64_t)v.hi << 64) | v.lo;
  }
  return *neg ? (dx_u128)0 - bits : bits;
}

__host__ __device__ __forceinline__ DxU256
dx_mul128(dx_u128 x, dx_u128 y) {
  const uint64_t x0 = (uint64_t)x, x1 = (uint64_t)(x >> 64);
  const uint64_t y0 = (uint64_t)y, y1 = (uint64_t)(y >> 64);
  const dx_u128 p00 = (dx_u128)x0 * y0, p01 = (dx_u128)x0 * y1;
  const dx_u128 p10 = (dx_u128)x1 * y0, p11 = (dx_u128)x1 * y1;
  // three 64-bit terms: below 3 * 2^64
  const dx_u128 mid = (p00 >> 64) + (uint64_t)p01 + (uint64_t)p10;
  DxU256 r;
  r.lo = (mid << 64) | (uint64_t)p00;
  r.hi = p11 + (p01 >> 64) + (p10 >> 64) + (mid >> 64);
  return r;
}

// magnitude * 10^k; `pw` == 1 skips the multiply (uniform branch)
__host__ __device__ __forceinline__ DxU256
dx_scale_up(dx_u128 mag, dx_u128 pw) {
  if (pw == 1) {
    DxU256 r;
    r.lo = mag;
    r.hi = 0;
    return r;
  }
  return dx_mul128(mag, pw);
}

__host__ __device__ __forceinline__ DxU256
dx_add256(DxU256 x, DxU256 y) {
  DxU256 r;
  r.lo = x.lo + y.lo;
  r.hi = x.hi + y.hi + (r.lo < x.lo ? 1 : 0);
  return r;
}

// x - y, for x >= y
__host__ __device__ __forceinline__ DxU256
dx_sub256(DxU256 x, DxU256 y) {
  DxU256 r;
  r.lo = x.lo - y.lo;
  r.hi = x.hi - y.hi - (x.lo < y.lo ? 1 : 0);
  return r;
}

__host__ __device__ __forceinline__ bool
dx_less256(DxU256 x, DxU256 y) {
  return x.hi < y.hi || (x.hi == y.hi && x.lo < y.lo);
}

// floor(n / d) and the remainder, for d != 0 and n.hi < d (the quotient then
// fits 128 bits). A divisor below 2^32 takes four 64-by-32-bit steps; else a
// numerator below 2^128 divides natively, and a wider one runs 128
// shift-subtract steps in which `q` hands its top bit to the remainder and
// collects quotient bits at the bottom.
__host__ __device__ dx_u128 dx_div256(DxU256 n, dx_u128 d, dx_u128* rem) {
  if ((d >> 32) == 0) {
    // schoolbook division over base-2^32 digits: n.hi < d is the first
    // partial remainder, and every step is a 64-bit by 32-bit division
    // (10^1 .. 10^9 land here, the usual scale differences)
    const uint32_t d32 = (uint32_t)d;
    const uint64_t hi = (uint64_t)(n.lo >> 64), lo = (uint64_t)n.lo;
    uint64_t cur = ((uint64_t)n.hi << 32) | (hi >> 32);
    const uint64_t q3 = cur / d32;
    cur = ((cur % d32) << 32) | (hi & 0xffffffffu);
    const uint64_t q2 = cur / d32;
    cur = ((cur % d32) << 32) | (lo >> 32);
    const uint64_t q1 = cur / d32;
    cur = ((cur % d32) << 32) | (lo & 0xffffffffu);
    const uint64_t q0 = cur / d32;
    *rem = cur % d32;
    return ((dx_u128)((q3 << 32) | q2) << 64) | ((q1 << 32) | q0);
  }
  if (n.hi == 0) {
    if ((n.lo >> 64) == 0 && (d >> 64) == 0) {
      const uint64_t n64 = (uint64_t)n.lo, d64 = (uint64_t)d;
      *rem = n64 % d64;
      return n64 / d64;
    }
    *rem = n.lo % d;
    return n.lo / d;
  }
  dx_u128 r = n.hi, q = n.lo;
#pragma nounroll
  for (int i = 0; i < 128; i++) {
    const bool carry = (r >> 127) != 0;
    r = (r << 1) | (q >> 127);
    q <<= 1;
    if (carry || r >= d) {
      r -= d;
      q |= 1;
    }
  }
  *rem = r;
  return q;
}

// Shared tail: q = m / div (HALF_UP on the magnitude unless DX_TRUNCATE),
// then the bound check. Returns false when the row overflows; otherwise
// *bits holds the two's-complement result.
__host__ __device__ __forceinline__ bool
dx_finish(DxU256 m, bool neg, dx_u128 div, dx_u128 bound, int flags,
          dx_u128* bits) {
  dx_u128 q;
  if (div == 1) {
    if (m.hi != 0) return false;
    q = m.lo;
  } else {
    if (m.hi >= div) return false;  // quotient >= 2^128 > any bound
    dx_u128 r;
    q = dx_div256(m, div, &r);
    if (q > bound) return false;  // bound < 2^127: q + 1 cannot wrap
    if (!(flags & DX_TRUNCATE) && r >= div - r) q += 1;
  }
  if (q == 0) neg = false;
  if (q >= bound && !((flags & DX_ASYM) && neg && q == bound)) return false;
  *bits = neg ? (dx_u128)0 - q : q;
  return true;
}

__host__ __device__ __forceinline__ void
dx_store(DxI128* __restrict__ out, int64_t i, dx_u128 bits) {
  DxI128 r;
  r.lo = (uint64_t)bits;
  r.hi = (int64_t)(uint64_t)(bits >> 64);
  out[i] = r;
}

__host__ __device__ __forceinline__ bool
dx_row_valid(const uint8_t* __restrict__ va, const uint8_t* __restrict__ vb,
             int64_t i) {
  return (va == nullptr || va[i] != 0) && (vb == nullptr || vb[i] != 0);
}

// Per-row bodies, shared by the kernels and by host-side checks. Each returns
// the row's validity and leaves the two's-complement result in *bits.

// ----------------------------------------------------------------- add/sub
__host__ __device__ __forceinline__ bool
dx_row_addsub(const void* __restrict__ a, int a_narrow,
              const void* __restrict__ b, int b_narrow, int64_t i, dx_u128 pa,
              dx_u128 pb, dx_u128 pd, dx_u128 bound, int is_sub,
              dx_u128* bits) {
  bool na, nb;
  const DxU256 ma = dx_scale_up(dx_load_mag(a, a_narrow, i, &na), pa);
  const DxU256 mb = dx_scale_up(dx_load_mag(b, b_narrow, i, &nb), pb);
  if (is_sub) nb = !nb;
  DxU256 m;
  bool neg;
  if (na == nb) {  // each side is below 2^254: the sum cannot wrap
    m = dx_add256(ma, mb);
    neg = na;
  } else if (dx_less256(ma, mb)) {
    m = dx_sub256(mb, ma);
    neg = nb;
  } else {
    m = dx_sub256(ma, mb);
    neg = na;
  }
  return dx_finish(m, neg, pd, bound, 0, bits);
}

__global__ void __launch_bounds__(DX_BLOCK)
k_dec128_addsub(const void* __restrict__ a, int a_narrow,
                const uint8_t* __restrict__ va, const void* __restrict__ b,
                int b_narrow, const uint8_t* __restrict__ vb, int64_t n,
                DxArg128 pa_, DxArg128 pb_, DxArg128 pd_, DxArg128 bound_,
                int is_sub, DxI128* __restrict__ out,
                uint8_t* __restrict__ valid) {
  const dx_u128 pa = dx_arg(pa_), pb = dx_arg(pb_), pd = dx_arg(pd_);
  const dx_u128 bound = dx_arg(bound_);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    dx_u128 bits = 0;
    const bool ok = dx_row_valid(va, vb, i) &&
                    dx_row_addsub(a, a_narrow, b, b_narrow, i, pa, pb, pd,
                                  bound, is_sub, &bits);
    dx_store(out, i, ok ? bits : (dx_u128)0);
    valid[i] = ok ? 1 : 0;
  }
}

// ---------------------------------------------------------------- multiply
__host__ __device__ __forceinline__ bool
dx_row_mul(const void* __restrict__ a, int a_narrow,
           const void* __restrict__ b, int b_narrow, int64_t i, dx_u128 pd,
           dx_u128 bound, dx_u128* bits) {
  bool na, nb;
  const dx_u128 ma = dx_load_mag(a, a_narrow, i, &na);
  const dx_u128 mb = dx_load_mag(b, b_narrow, i, &nb);
  return dx_finish(dx_mul128(ma, mb), na != nb, pd, bound, 0, bits);
}

__global__ void __launch_bounds__(DX_BLOCK)
k_dec128_mul(const void* __restrict__ a, int a_narrow,
             const uint8_t* __restrict__ va, const void* __restrict__ b,
             int b_narrow, const uint8_t* __restrict__ vb, int64_t n,
             DxArg128 pd_, DxArg128 bound_, DxI128* __restrict__ out,
             uint8_t* __restrict__ valid) {
  const dx_u128 pd = dx_arg(pd_), bound = dx_arg(bound_);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    dx_u128 bits = 0;
    const bool ok = dx_row_valid(va, vb, i) &&
                    dx_row_mul(a, a_narrow, b, b_narrow, i, pd, bound, &bits);
    dx_store(out, i, ok ? bits : (dx_u128)0);
    valid[i] = ok ? 1 : 0;
  }
}

// ------------------------------------------------------------------ divide
__host__ __device__ __forceinline__ bool
dx_row_div(const void* __restrict__ a, int a_narrow,
           const void* __restrict__ b, int b_narrow, int64_t i, dx_u128 pk,
           dx_u128 bound, dx_u128* bits) {
  bool na, nb;
  const dx_u128 ma = dx_load_mag(a, a_narrow, i, &na);
  const dx_u128 mb = dx_load_mag(b, b_narrow, i, &nb);
  if (mb == 0) return false;  // x / 0 is null
  return dx_finish(dx_scale_up(ma, pk), na != nb, mb, bound, 0, bits);
}

__global__ void __launch_bounds__(DX_BLOCK)
k_dec128_div(const void* __restrict__ a, int a_narrow,
             const uint8_t* __restrict__ va, const void* __restrict__ b,
             int b_narrow, const uint8_t* __restrict__ vb, int64_t n,
             DxArg128 pk_, DxArg128 bound_, DxI128* __restrict__ out,
             uint8_t* __restrict__ valid) {
  const dx_u128 pk = dx_arg(pk_), bound = dx_arg(bound_);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    dx_u128 bits = 0;
    const bool ok = dx_row_valid(va, vb, i) &&
                    dx_row_div(a, a_narrow, b, b_narrow, i, pk, bound, &bits);
    dx_store(out, i, ok ? bits : (dx_u128)0);
    valid[i] = ok ? 1 : 0;
  }
}

// ----------------------------------------------------------------- compare
__host__ __device__ __forceinline__ bool
dx_row_cmp(const void* __restrict__ a, int a_narrow,
           const void* __restrict__ b, int b_narrow, int64_t i, dx_u128 pa,
           dx_u128 pb, int op) {
  bool na, nb;
  const DxU256 ma = dx_scale_up(dx_load_mag(a, a_narrow, i, &na), pa);
  const DxU256 mb = dx_scale_up(dx_load_mag(b, b_narrow, i, &nb), pb);
  // a negative sign always comes with a non-zero magnitude
  bool lt, gt;
  if (na != nb) {
    lt = na;
    gt = nb;
  } else {
    const bool ml = dx_less256(ma, mb), mg = dx_less256(mb, ma);
    lt = na ? mg : ml;
    gt = na ? ml : mg;
  }
  switch (op) {
    case DX_EQ: return !lt && !gt;
    case DX_NE: return lt || gt;
    case DX_LT: return lt;
    case DX_LE: return !gt;
    case DX_GT: return gt;
    default: return !lt;
  }
}

__global__ void __launch_bounds__(DX_BLOCK)
k_dec128_cmp(const void* __restrict__ a, int a_narrow,
             const void* __restrict__ b, int b_narrow, int64_t n,
             DxArg128 pa_, DxArg128 pb_, int op, uint8_t* __restrict__ out) {
  const dx_u128 pa = dx_arg(pa_), pb = dx_arg(pb_);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x)
    out[i] = dx_row_cmp(a, a_narrow, b, b_narrow, i, pa, pb, op) ? 1 : 0;
}

// ----------------------------------------------------------------- rescale
__host__ __device__ __forceinline__ bool
dx_row_rescale(const void* __restrict__ x, int x_narrow, int64_t i,
               dx_u128 pk, int scale_up, int flags, dx_u128 bound,
               dx_u128* bits) {
  bool neg;
  const dx_u128 mag = dx_load_mag(x, x_narrow, i, &neg);
  if (flags & DX_ABS) neg = false;
  if (flags & DX_NEGATE) neg = !neg;
  DxU256 m;
  m.lo = mag;
  m.hi = 0;
  if (scale_up) m = dx_scale_up(mag, pk);
  return dx_finish(m, neg, scale_up ? (dx_u128)1 : pk, bound, flags, bits);
}

__global__ void __launch_bounds__(DX_BLOCK)
k_dec128_rescale(const void* __restrict__ x, int x_narrow,
                 const uint8_t* __restrict__ vx, int64_t n, DxArg128 pk_,
                 int scale_up, int flags, DxArg128 bound_,
                 void* __restrict__ out, int out_narrow,
                 uint8_t* __restrict__ valid) {
  const dx_u128 pk = dx_arg(pk_), bound = dx_arg(bound_);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
       i += (int64_t)gridDim.x * blockDim.x) {
    dx_u128 bits = 0;
    const bool ok = dx_row_valid(vx, nullptr, i) &&
                    dx_row_rescale(x, x_narrow, i, pk, scale_up, flags, bound,
                                   &bits);
    if (!ok) bits = 0;
    if (out_narrow)
      ((int64_t*)out)[i] = (int64_t)(uint64_t)bits;
    else
      dx_store((DxI128*)out, i, bits);
    valid[i] = ok ? 1 : 0;
  }
}

// -------------------------------------------------------------- entry points
static inline bool dx_misaligned(const void* p, int narrow) {
  return !narrow && (((uintptr_t)p) & 15) != 0;
}

static inline bool dx_bad_pow(int k) { return k < 0 || k > DX_MAX_POW10; }

// out[i] = (a[i]*10^ka +- b[i]*10^kb) / 10^d, HALF_UP; valid[i] = va[i] &&
// vb[i] && |out[i]| < 10^p. a/b: [n,2] limbs (16-byte aligned) or, with
// *_narrow, int64 [n]. va/vb may be null. out: [n,2] limbs; valid: n bytes.
AU_EXPORT int au_dec128_addsub(const void* a, int a_narrow, const uint8_t* va,
                               const void* b, int b_narrow, const uint8_t* vb,
                               int64_t n, int ka, int kb, int d, int p,
                               int is_sub, int64_t* out, uint8_t* valid,
                               void* stream) {
  if (n <= 0) return 0;
  if (dx_bad_pow(ka) || dx_bad_pow(kb) || dx_bad_pow(d) || dx_bad_pow(p) ||
      dx_misaligned(a, a_narrow) || dx_misaligned(b, b_narrow) ||
      dx_misaligned(out, 0))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dec128_addsub, dim3(dx_grid(n)), dim3(DX_BLOCK), 0,
                     (hipStream_t)stream, a, a_narrow, va, b, b_narrow, vb, n,
                     dx_pow10(ka), dx_pow10(kb), dx_pow10(d), dx_pow10(p),
                     is_sub, (DxI128*)out, valid);
  return (int)hipGetLastError();
}

// out[i] = (a[i]*b[i]) / 10^d, HALF_UP; operands and outputs as above.
AU_EXPORT int au_dec128_mul(const void* a, int a_narrow, const uint8_t* va,
                            const void* b, int b_narrow, const uint8_t* vb,
                            int64_t n, int d, int p, int64_t* out,
                            uint8_t* valid, void* stream) {
  if (n <= 0) return 0;
  if (dx_bad_pow(d) || dx_bad_pow(p) || dx_misaligned(a, a_narrow) ||
      dx_misaligned(b, b_narrow) || dx_misaligned(out, 0))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dec128_mul, dim3(dx_grid(n)), dim3(DX_BLOCK), 0,
                     (hipStream_t)stream, a, a_narrow, va, b, b_narrow, vb, n,
                     dx_pow10(d), dx_pow10(p), (DxI128*)out, valid);
  return (int)hipGetLastError();
}

// out[i] = round_half_up(a[i]*10^k / b[i]); b[i] == 0 clears valid[i].
AU_EXPORT int au_dec128_div(const void* a, int a_narrow, const uint8_t* va,
                            const void* b, int b_narrow, const uint8_t* vb,
                            int64_t n, int k, int p, int64_t* out,
                            uint8_t* valid, void* stream) {
  if (n <= 0) return 0;
  if (dx_bad_pow(k) || dx_bad_pow(p) || dx_misaligned(a, a_narrow) ||
      dx_misaligned(b, b_narrow) || dx_misaligned(out, 0))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dec128_div, dim3(dx_grid(n)), dim3(DX_BLOCK), 0,
                     (hipStream_t)stream, a, a_narrow, va, b, b_narrow, vb, n,
                     dx_pow10(k), dx_pow10(p), (DxI128*)out, valid);
  return (int)hipGetLastError();
}

// out[i] = a[i]*10^ka <op> b[i]*10^kb (DX_EQ .. DX_GE), one byte per row.
AU_EXPORT int au_dec128_cmp(const void* a, int a_narrow, const void* b,
                            int b_narrow, int64_t n, int ka, int kb, int op,
                            uint8_t* out, void* stream) {
  if (n <= 0) return 0;
  if (dx_bad_pow(ka) || dx_bad_pow(kb) || op < DX_EQ || op > DX_GE ||
      dx_misaligned(a, a_narrow) || dx_misaligned(b, b_narrow))
    return (int)hipErrorInvalidValue;
  hipLaunchKernelGGL(k_dec128_cmp, dim3(dx_grid(n)), dim3(DX_BLOCK), 0,
                     (hipStream_t)stream, a, a_narrow, b, b_narrow, n,
                     dx_pow10(ka), dx_pow10(kb), op, out);
  return (int)hipGetLastError();
}

// out[i] = x[i]*10^k (k >= 0) or x[i]/10^-k (k < 0; HALF_UP, or toward zero
// with DX_TRUNCATE), after DX_ABS / DX_NEGATE; valid[i] = vx[i] && |out[i]| <
// bound, where bound = bound_hi*2^64 + bound_lo (DX_ASYM also keeps -bound).
// out is [n,2] limbs, or int64 [n] with out_narrow (bound <= 2^63 then).
AU_EXPORT int au_dec128_rescale(const void* x, int x_narrow,
                                const uint8_t* vx, int64_t n, int k,
                                int flags, uint64_t bound_lo,
                                uint64_t bound_hi, void* out, int out_narrow,
                                uint8_t* valid, void* stream) {
  if (n <= 0) return 0;
  const int ak = k < 0 ? -k : k;
  if (dx_bad_pow(ak) || dx_misaligned(x, x_narrow) ||
      dx_misaligned(out, out_narrow) || (bound_hi >> 63) != 0 ||
      (out_narrow && (bound_hi != 0 || bound_lo > ((uint64_t)1 << 63))))
    return (int)hipErrorInvalidValue;
  DxArg128 bound;
  bound.lo = bound_lo;
  bound.hi = bound_hi;
  hipLaunchKernelGGL(k_dec128_rescale, dim3(dx_grid(n)), dim3(DX_BLOCK), 0,
                     (hipStream_t)stream, x, x_narrow, vx, n, dx_pow10(ak),
                     k > 0 ? 1 : 0, flags, bound, out, out_narrow, valid);
  return (int)hipGetLastError();
}
