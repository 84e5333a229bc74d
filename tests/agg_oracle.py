"""Independent oracle for GROUP BY ids, aggregates, Spark's row hash and
hash joins: pure Python and numpy, nothing from auron_amd.ops.

Values are plain Python objects. A column is a list whose entries are
None (SQL NULL) or a value: int, bool, float (float32 columns hold floats
that are exactly representable in float32) or bytes (strings).

The rules it encodes (Spark's, unless noted):
  keys        NaN == NaN, -0.0 == 0.0, NULL is a value of its own
  hash        every NaN hashes as the canonical NaN, -0.0 as 0.0, NULL
              columns are skipped (the running seed passes through)
  MIN / MAX   NaN is greater than every float, +inf included
  float SUM   IEEE: NaN and +-inf propagate, +inf with -inf is NaN
  int SUM     wraps modulo 2**64
"""
import math
import struct
from fractions import Fraction

M32 = 0xFFFFFFFF
M64 = (1 << 64) - 1
I64_MIN = -(1 << 63)
I64_MAX = (1 << 63) - 1

F64_NAN_BITS = 0x7FF8000000000000
F32_NAN_BITS = 0x7FC00000

INT_KINDS = ("bool", "int8", "int16", "int32", "date32")
LONG_KINDS = ("int64", "timestamp", "decimal64")


# ------------------------------------------------------------------ murmur3
def _rotl(x, r):
    return ((x << r) | (x >> (32 - r))) & M32


def _mix_k1(k):
    k = (k * 0xCC9E2D51) & M32
    k = _rotl(k, 15)
    return (k * 0x1B873593) & M32


def _mix_h1(h, k):
    h = _rotl(h ^ k, 13)
    return (h * 5 + 0xE6546B64) & M32


def _fmix(h, length):
    h ^= length & M32
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M32
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M32
    h ^= h >> 16
    return h


def signed32(h):
    h &= M32
    return h - (1 << 32) if h >= (1 << 31) else h


def hash_int(v, seed):
    """Murmur3_x86_32.hashInt: `v` any int, taken modulo 2**32."""
    return signed32(_fmix(_mix_h1(seed & M32, _mix_k1(v & M32)), 4))


def hash_long(v, seed):
    """hashLong: low word, then high word."""
    v &= M64
    h = _mix_h1(seed & M32, _mix_k1(v & M32))
    h = _mix_h1(h, _mix_k1(v >> 32))
    return signed32(_fmix(h, 8))


def hash_bytes(b, seed):
    """hashUnsafeBytes: little-endian words, then each tail byte
    sign-extended to an int and mixed on its own."""
    h = seed & M32
    n = len(b)
    for i in range(0, n - n % 4, 4):
        h = _mix_h1(h, _mix_k1(int.from_bytes(b[i:i + 4], "little")))
    for i in range(n - n % 4, n):
        byte = b[i] - 256 if b[i] >= 128 else b[i]
        h = _mix_h1(h, _mix_k1(byte & M32))
    return signed32(_fmix(h, n))


def f64_bits(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f32_bits(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def f64_from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def hash_double(x, seed):
    """doubleToLongBits (one NaN), -0.0 normalised to 0.0."""
    bits = F64_NAN_BITS if x != x else (0 if x == 0 else f64_bits(x))
    return hash_long(bits, seed)


def hash_float(x, seed):
    bits = F32_NAN_BITS if x != x else (0 if x == 0 else f32_bits(x))
    return hash_int(bits, seed)


def hash_value(kind, v, seed):
    if kind in INT_KINDS:
        return hash_int(int(v), seed)
    if kind in LONG_KINDS:
        return hash_long(int(v), seed)
    if kind == "float32":
        return hash_float(v, seed)
    if kind == "float64":
        return hash_double(v, seed)
    if kind == "string":
        return hash_bytes(v, seed)
    raise TypeError(kind)


def hash_rows(kinds, cols, seed=42):
    """Row hash over several columns: seed-chained, NULLs skipped."""
    n = len(cols[0]) if cols else 0
    out = []
    for i in range(n):
        h = seed
        for kind, col in zip(kinds, cols):
            if col[i] is not None:
                h = hash_value(kind, col[i], h)
        out.append(signed32(h))
    return out


def pmod(h, nparts):
    return h % nparts  # Python's % is already non-negative


# -------------------------------------------------------------------- keys
_NAN = ("nan",)
_NULL = ("null",)


def norm_key(v):
    if v is None:
        return _NULL
    if isinstance(v, float):
        if v != v:
            return _NAN
        if v == 0.0:
            return 0.0
    return v


def key_tuples(cols):
    return [tuple(norm_key(c[i]) for c in cols) for i in range(len(cols[0]))]


def group_ids(cols):
    """-> (gid per row, number of groups), gids in order of appearance."""
    seen = {}
    gids = []
    for k in key_tuples(cols):
        gids.append(seen.setdefault(k, len(seen)))
    return gids, len(seen)


def check_group_ids(got_gids, got_reps, cols):
    """Assert that (gids, reps) of a GROUP BY id assignment describe the
    oracle's partition of the rows."""
    want, G = group_ids(cols)
    got_gids = [int(g) for g in got_gids]
    got_reps = [int(r) for r in got_reps]
    n = len(want)
    assert len(got_gids) == n
    assert len(got_reps) == G, f"{len(got_reps)} groups, oracle has {G}"
    assert all(0 <= g < G for g in got_gids), "gids not dense in [0, G)"
    fwd, back = {}, {}
    for g, w in zip(got_gids, want):
        assert fwd.setdefault(g, w) == w, f"gid {g} spans oracle groups"
        assert back.setdefault(w, g) == g, f"oracle group {w} split"
    assert len(fwd) == G and len(back) == G
    assert len(set(got_reps)) == G, "reps are not distinct rows"
    for g, r in enumerate(got_reps):
        assert 0 <= r < n and got_gids[r] == g, f"gids[reps[{g}]] != {g}"


def join_pairs(build_cols, probe_cols, emit_unmatched_probe):
    """-> (set of (build row | -1, probe row), build_matched list). A row
    with a NULL in any key column never matches."""
    table = {}
    bkeys = key_tuples(build_cols)
    for j, k in enumerate(bkeys):
        if _NULL not in k:
            table.setdefault(k, []).append(j)
    matched = [False] * len(bkeys)
    pairs = set()
    for i, k in enumerate(key_tuples(probe_cols)):
        rows = [] if _NULL in k else table.get(k, [])
        for j in rows:
            pairs.add((j, i))
            matched[j] = True
        if not rows and emit_unmatched_probe:
            pairs.add((-1, i))
    return pairs, matched


# -------------------------------------------------------------- aggregates
def _wrap64(x):
    x &= M64
    return x - (1 << 64) if x > I64_MAX else x


def float_sum(vals):
    """-> (IEEE sum of `vals` in the best case, error bound of a sum taken
    in any order). Special values by hand, the rest by math.fsum; the
    bound is the recursive-summation one, 1.01 (m-1) 2**-53 sum|v|."""
    if any(v != v for v in vals):
        return math.nan, 0.0
    pinf = any(v == math.inf for v in vals)
    ninf = any(v == -math.inf for v in vals)
    if pinf and ninf:
        return math.nan, 0.0
    if pinf or ninf:
        return (math.inf if pinf else -math.inf), 0.0
    mag = sum(Fraction(abs(v)) for v in vals)
    # every partial sum stays within a small part of half an ulp above
    # DBL_MAX (2**970), so none rounds to infinity in any order
    assert mag < Fraction(1.7976931348623157e308) + 2 ** 960, \
        "test data: a partial sum could overflow, the result is order-dependent"
    bound = 1.01 * max(len(vals) - 1, 0) * 2.0 ** -53 * float(mag)
    return math.fsum(vals), bound


def float_min(vals):
    """NaN is the greatest value: NaN only when every input is NaN."""
    real = [v for v in vals if v == v]
    return min(real) if real else math.nan


def float_max(vals):
    if any(v != v for v in vals):
        return math.nan
    return max(vals)


def aggregate(gids, ngroups, values, fn, is_float):
    """Per-group aggregate over the non-NULL entries of `values`.
    -> (acc, counts, bounds): acc[g] is None for a group with no valid
    row; bounds[g] is the float-sum error bound (0.0 elsewhere)."""
    rows = [[] for _ in range(ngroups)]
    for g, v in zip(gids, values):
        if v is not None:
            rows[g].append(v)
    acc, bounds = [], []
    for vs in rows:
        b = 0.0
        if not vs:
            a = None
        elif fn == "count":
            a = len(vs)
        elif fn == "sum":
            if is_float:
                a, b = float_sum(vs)
            else:
                a = _wrap64(sum(int(v) for v in vs))
        elif fn == "min":
            a = float_min(vs) if is_float else min(vs)
        elif fn == "max":
            a = float_max(vs) if is_float else max(vs)
        else:
            raise ValueError(fn)
        acc.append(a)
        bounds.append(b)
    return acc, [len(vs) for vs in rows], bounds


def check_agg(got_acc, got_cnt, want, what="", exact=False):
    """Compare one aggregate's output with aggregate()'s. Groups with no
    valid row are compared on count only; nothing else is masked.
    exact=True drops the float-sum bound (for inputs that sum exactly)."""
    acc, cnt, bounds = want
    got_cnt = [int(c) for c in got_cnt]
    assert got_cnt == cnt, f"{what}: counts {got_cnt} != {cnt}"
    assert len(got_acc) == len(acc)
    for g, (a, w, b) in enumerate(zip(got_acc, acc, bounds)):
        if w is None:
            continue
        where = f"{what}: group {g}: got {a!r}, want {w!r}"
        if isinstance(w, float) and w != w:
            assert a != a, where
        elif isinstance(w, float) and b > 0.0 and not exact:
            assert abs(a - w) <= b, f"{where} (bound {b!r})"
        else:
            assert a == w, where  # 0.0 == -0.0, inf == inf
