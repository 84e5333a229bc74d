"""Input builders shared by test_agg_semantics.py (CPU paths) and the GPU
files test_gpu_agg_edges.py / test_gpu_group_keys.py. A helper module like
agg_oracle.py, not a conftest: it builds well-formed inputs (gids inside
[0, ngroups)) as plain Python lists and converts them to Columns."""
import math

import numpy as np
import torch

from auron_amd import dtypes
from auron_amd.column import Column

import agg_oracle as O

FLOAT_KINDS = ("float64", "float32")
VALUE_KINDS = ("float64", "float32", "int64", "int32", "int16", "int8", "bool")

DTYPES = {
    "bool": dtypes.bool_, "int8": dtypes.int8, "int16": dtypes.int16,
    "int32": dtypes.int32, "int64": dtypes.int64, "date32": dtypes.date32,
    "timestamp": dtypes.timestamp, "decimal64": dtypes.decimal64(18, 2),
    "float32": dtypes.float32, "float64": dtypes.float64,
    "string": dtypes.string,
}
_NP = {"bool": np.bool_, "int8": np.int8, "int16": np.int16,
       "int32": np.int32, "date32": np.int32, "int64": np.int64,
       "timestamp": np.int64, "decimal64": np.int64,
       "float32": np.float32, "float64": np.float64}

F32_MAX = float(np.finfo(np.float32).max)
F32_TINY = float(np.float32(1.401298464324817e-45))  # smallest subnormal
F64_MAX = float(np.finfo(np.float64).max)
F64_TINY = 5e-324
NEG_NAN = O.f64_from_bits(0xFFF8000000000000)


def ops_for(kind):
    """Every value dtype takes all three: SUM over bool counts the Trues
    (int64, as the executor's state dtype for sum(bool) says)."""
    return ("sum", "min", "max")


def poison(kind):
    """What the data buffer holds under an invalid row: it must never
    reach a result."""
    if kind in FLOAT_KINDS:
        return math.nan
    if kind == "bool":
        return True
    return int(np.iinfo(_NP[kind]).min)


def column(kind, values, device="cpu", validity=None):
    """Column over `values` (None = NULL, its slot filled with poison).
    A validity tensor is attached when a value is None or validity=True."""
    if kind == "string":
        return string_column(values, device)
    fill = poison(kind)
    data = np.array([fill if v is None else v for v in values], dtype=_NP[kind])
    valid = None
    if validity or any(v is None for v in values):
        valid = torch.tensor([v is not None for v in values], dtype=torch.bool)
    return Column(DTYPES[kind], torch.from_numpy(data), valid).to(device)


def string_column(values, device="cpu"):
    """String column over bytes objects (any bytes, not only UTF-8). A NULL
    slot keeps the bytes b"null" so that its data is not empty."""
    bufs = [b"null" if v is None else v for v in values]
    offs = np.zeros(len(bufs) + 1, dtype=np.int64)
    np.cumsum([len(b) for b in bufs], out=offs[1:])
    raw = b"".join(bufs)
    data = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else \
        torch.empty(0, dtype=torch.uint8)
    valid = None
    if any(v is None for v in values):
        valid = torch.tensor([v is not None for v in values], dtype=torch.bool)
    return Column(dtypes.string, data, valid, torch.from_numpy(offs)).to(device)


def bits_column(kind, bits, device="cpu"):
    """float column from raw bit patterns (NaN payloads survive)."""
    if kind == "float64":
        data = np.array(bits, dtype=np.uint64).view(np.float64)
    else:
        data = np.array(bits, dtype=np.uint32).view(np.float32)
    return Column(DTYPES[kind], torch.from_numpy(data.copy())).to(device)


class AggCase:
    def __init__(self, name, kind, gids, ngroups, values, with_validity):
        self.name, self.kind = name, kind
        self.gids, self.ngroups, self.values = gids, ngroups, values
        self.with_validity = with_validity
        self._want = {}

    @property
    def is_float(self):
        return self.kind in FLOAT_KINDS

    def gids_t(self, device="cpu"):
        return torch.tensor(self.gids, dtype=torch.int64).to(device)

    def column(self, device="cpu"):
        return column(self.kind, self.values, device,
                      validity=self.with_validity)

    def want(self, fn):
        """The oracle's result, computed once per case and op."""
        if fn not in self._want:
            self._want[fn] = O.aggregate(self.gids, self.ngroups, self.values,
                                         fn, self.is_float)
        return self._want[fn]

    def row_counts(self):
        return np.bincount(self.gids, minlength=self.ngroups).tolist()


def make_gids(n, ngroups, pattern, rng, unused=()):
    """Every gid outside `unused` occurs at least once. "random": no
    structure; "runs": runs of equal gids, a gid recurring in several
    runs (A A B A)."""
    used = [g for g in range(ngroups) if g not in unused]
    assert n >= len(used)
    if pattern == "random":
        g = np.concatenate([np.array(used), rng.choice(used, n - len(used))])
        rng.shuffle(g)
        return g.tolist()
    avg = max(1, n // (2 * len(used)))
    out = []
    first = list(used)
    rng.shuffle(first)
    budget = n - len(first)  # rows beyond one per guaranteed run
    for g in first:
        extra = min(budget, int(rng.integers(0, 2 * avg - 1))) if avg > 1 else 0
        budget -= extra
        out += [g] * (1 + extra)
    while len(out) < n:
        run = int(rng.integers(1, 2 * avg + 1))
        out += [int(rng.choice(used))] * min(run, n - len(out))
    return out


def _base_value(kind, flavour, rng):
    if kind in FLOAT_KINDS:
        if flavour == "exact":  # k/8, |k| <= 2**20: sums are exact in any order
            return int(rng.integers(-2 ** 20, 2 ** 20 + 1)) / 8.0
        v = float(rng.normal(0.0, 1e3))
        return float(np.float32(v)) if kind == "float32" else v
    if kind == "bool":
        return bool(rng.integers(0, 2))
    if kind == "int64":
        return int(rng.integers(-2 ** 40, 2 ** 40))
    ii = np.iinfo(_NP[kind])
    return int(rng.integers(ii.min, ii.max + 1))


def _place_specials(kind, flavour, values, rows_of):
    """Overwrite valid rows of chosen groups with the special values of the
    dtype. rows_of: per usable group, its valid rows in row order."""
    groups = [r for r in rows_of if r]
    if not groups:
        return

    def role(k):
        # nine roles: distinct groups once there are nine to choose from
        return groups[(k * max(1, len(groups) // 9)) % len(groups)]

    if kind in FLOAT_KINDS:
        fmax, tiny = (F64_MAX, F64_TINY) if kind == "float64" else (F32_MAX, F32_TINY)
        if len(groups) < 8:  # a reduced set that cannot overflow a sum
            r = role(0)
            values[r[-1]] = math.nan
            values[r[0]] = -math.inf
            if len(r) > 3:
                values[r[1]], values[r[2]] = -0.0, 0.0
            if len(groups) >= 3:
                for j, i in enumerate(groups[1]):   # the whole group
                    values[i] = math.nan if j % 2 else NEG_NAN
                values[groups[2][0]] = math.inf     # NaN above +inf
                values[groups[2][-1]] = math.nan
            return
        values[role(0)[0]] = math.nan               # first of its group
        values[role(1)[-1]] = NEG_NAN               # last, sign bit set
        for j, i in enumerate(role(2)):             # the whole group
            values[i] = math.nan if j % 2 else NEG_NAN
        r = role(3)
        values[r[0]] = math.inf
        values[r[-1]] = -math.inf if len(r) > 1 else math.inf
        for j, i in enumerate(role(4)):
            values[i] = -0.0 if j % 2 == 0 else 0.0
        r = role(5)                                 # NaN above +inf
        values[r[0]] = math.inf
        if len(r) > 1:
            values[r[-1]] = math.nan
        if flavour == "general":
            values[role(6)[0]] = fmax
            values[role(7)[0]] = -fmax
            r = role(8 if len(groups) > 8 else 4)
            values[r[0]] = tiny
            values[r[-1]] = -tiny
        return
    if kind == "bool":
        for i in role(0):
            values[i] = True
        for i in role(1):
            values[i] = False
        return
    ii = np.iinfo(_NP[kind])
    lo, hi = int(ii.min), int(ii.max)
    values[role(0)[0]] = lo       # for int64 these are the identities
    values[role(1)[-1]] = hi
    r = role(2)                   # hi + hi (+ ...): wraps int64, exceeds int32
    for i in r[:3]:
        values[i] = hi
    r = role(3)
    for i in r[:3]:
        values[i] = lo
    r = role(4)
    values[r[0]] = lo
    values[r[-1]] = hi


def agg_case(name, kind, n, ngroups, pattern="random", with_validity=True,
             flavour="exact", unused_end=0, seed=0, gids=None):
    """One aggregate input. Layout rules, asserted below: with a validity
    tensor and ngroups >= 4 one group has only invalid rows; with
    ngroups >= 8 (>= 4 without validity) group 0 or ngroups-1 is used by
    no row; groups with no valid row are at most a quarter of all.
    `gids` reuses the gids of another case (several columns, one GROUP BY)."""
    rng = np.random.default_rng(seed)
    dead = None
    unused = ()
    if ngroups >= (8 if with_validity else 4):
        unused = (0,) if unused_end == 0 else (ngroups - 1,)
    if gids is None:
        gids = make_gids(n, ngroups, pattern, rng, unused)
    valid = [True] * n
    if with_validity:
        valid = (rng.random(n) >= 0.2).tolist()
        if ngroups >= 4:
            dead = ngroups // 2
        seen = set()
        for i, g in enumerate(gids):
            if g == dead:
                valid[i] = False
            elif g not in seen:
                seen.add(g)
                valid[i] = True  # every other used group keeps a valid row
    values = [_base_value(kind, flavour, rng) if ok else None for ok in valid]
    rows_of = [[] for _ in range(ngroups)]
    for i, g in enumerate(gids):
        if valid[i]:
            rows_of[g].append(i)
    _place_specials(kind, flavour, values, rows_of)
    empty = sum(1 for r in rows_of if not r)
    assert 4 * empty <= ngroups, (name, empty, ngroups)
    if with_validity and ngroups >= 4:
        assert dead in gids and not rows_of[dead]
    assert all(0 <= g < ngroups for g in gids)
    return AggCase(name, kind, gids, ngroups, values, with_validity)


def wave_pattern_gids():
    """192 rows = three waves of the segmented kernels, 6 groups:
    wave 0 is one run of 64; wave 1 holds A A B A recurrences and a run
    that goes on into wave 2 (lanes 63 -> 0); the last run ends at the
    last row."""
    g = [0] * 64
    g += [1, 1, 2, 1, 2, 2, 1, 3] * 7 + [3, 3, 3, 3] + [4] * 4   # lanes 0..63
    g += [4] * 10 + [1, 2] * 15 + [5] * 24
    assert len(g) == 192
    return g


def wave_pattern_case(kind, nan_at, with_validity=False):
    """wave_pattern_gids() with NaN (floats) or the type's extremes (ints)
    at the rows `nan_at`."""
    rng = np.random.default_rng(11)
    gids = wave_pattern_gids()
    values = [_base_value(kind, "exact", rng) for _ in gids]
    if with_validity:
        for i in (5, 64, 70, 128, 191):
            values[i] = None
    for j, i in enumerate(nan_at):
        if kind in FLOAT_KINDS:
            values[i] = NEG_NAN if j % 2 else math.nan
        else:
            ii = np.iinfo(_NP[kind])
            values[i] = int(ii.min) if j % 2 else int(ii.max)
    return AggCase(f"wave-{kind}-{'-'.join(map(str, nan_at))}", kind, gids, 6,
                   values, with_validity)


# ---------------------------------------------------------------- key cases
def column_over(kind, data, valid, device="cpu"):
    """Column whose NULL slots keep the given data (a NULL slot may hold
    the value of a valid row). -> (Column, oracle value list)."""
    vals = [v if ok else None for v, ok in zip(data, valid)]
    if kind == "string":
        col = string_column(data)
    else:
        col = Column(DTYPES[kind], torch.from_numpy(np.array(data, dtype=_NP[kind])))
    # assembled on the host and moved as a whole: Column.to() goes by the
    # data tensor's device alone and would leave a host validity behind
    col = Column(col.dtype, col.data, torch.tensor(valid, dtype=torch.bool),
                 col.offsets)
    assert col.device.type == "cpu"
    return col.to(device), vals


def _int_edges(kind):
    ii = np.iinfo(_NP[kind])
    lo, hi = int(ii.min), int(ii.max)
    mid = [0, -1, 1, 2, hi // 2, lo // 2, hi - 1, lo + 1]
    if hi > 2 ** 32:
        mid += [2 ** 32, 2 ** 32 + 1, -2 ** 32, 2 ** 31, -2 ** 31 - 1, 1 << 62]
    return [lo, hi] + mid


_ASCII = bytes((i * 37 + 11) % 94 + 33 for i in range(40))


def string_values(ref_safe=True):
    """Lengths 0..17, 31, 32, 33; pairs that differ only in the last byte,
    at byte 7 and at byte 8 (the edges of the 8-byte compare loop); bytes
    >= 0x80 (sign-extended tail bytes); "a" against "a\\0". ref_safe keeps
    out pairs that differ only inside invalid UTF-8, which the CPU
    reference decodes to one replacement character."""
    out = []
    for n in list(range(18)) + [31, 32, 33]:
        s = _ASCII[:n]
        out.append(s)
        if n:
            out.append(s[:-1] + bytes([s[-1] ^ 1]))
        for k in (7, 8):
            if n > k + 1:
                out.append(s[:k] + bytes([s[k] ^ 2]) + s[k + 1:])
    out += [b"a", b"a\0", b"a\0\0", b"\0", b"\x80", b"\xff\xfe", b"abc\xe9",
            b"abcd\xc3\xa9", b"abcde\xe2\x82\xac", b"\xe2\x82\xac",
            b"\x80\x81\x82", "天地".encode(), "😁".encode()]
    if not ref_safe:
        out += [b"\x81", b"\xff\xff", b"abc\xea", b"12345678\x80",
                b"12345678\x81"]
    return out


def key_values(kind, ref_safe=True):
    """Edge values of one key dtype, with repeats (groups of more than one
    row) and NULLs."""
    if kind == "bool":
        vals = [True, False, True]
    elif kind in FLOAT_KINDS:
        fmax, tiny = (F64_MAX, F64_TINY) if kind == "float64" else (F32_MAX, F32_TINY)
        vals = [0.0, -0.0, math.nan, NEG_NAN, math.inf, -math.inf, fmax, -fmax,
                tiny, -tiny, 1.5, -1.5, 0.1 if kind == "float64" else 0.125]
    elif kind == "string":
        vals = string_values(ref_safe)
    else:
        vals = _int_edges(kind)
    return vals + [None] + vals[::2] + [None]


# Vectorised murmur3 pieces over uint64 arrays holding 32-bit patterns. They
# only SEARCH for colliding keys; the scalar oracle then checks each key.
_NP_M32 = np.uint64(O.M32)


def _np_rotl(x, r):
    return ((x << np.uint64(r)) | (x >> np.uint64(32 - r))) & _NP_M32


def _np_mix_k1(k):
    k = (k * np.uint64(0xCC9E2D51)) & _NP_M32
    return (_np_rotl(k, 15) * np.uint64(0x1B873593)) & _NP_M32


def _np_mix_h1(h, k):
    return (_np_rotl(h ^ k, 13) * np.uint64(5) + np.uint64(0xE6546B64)) & _NP_M32


def _np_fmix(h, n):
    h = h ^ np.uint64(n)
    h ^= h >> np.uint64(16)
    h = (h * np.uint64(0x85EBCA6B)) & _NP_M32
    h ^= h >> np.uint64(13)
    h = (h * np.uint64(0xC2B2AE35)) & _NP_M32
    return h ^ (h >> np.uint64(16))


def colliding_keys(shape, slot, count, mask=1023):
    """`count` distinct keys of a shape whose row hash (seed 42) has
    `hash & mask == slot`: shape "int64", "int32", or "pair" = (int32 7,
    int64 k). Found with numpy, verified with the scalar oracle."""
    mixh, mixk, fmix, m = _np_mix_h1, _np_mix_k1, _np_fmix, _NP_M32
    k = np.arange(1, 700_001, dtype=np.uint64)
    seed = 42
    if shape == "pair":
        seed = O.hash_int(7, 42) & O.M32
    s = np.full_like(k, seed)
    if shape == "int32":
        h = fmix(mixh(s, mixk(k & m)), 4)
    else:
        h = mixh(s, mixk(k & m))
        h = fmix(mixh(h, mixk(k >> np.uint64(32))), 8)
    keys = [int(x) for x in k[(h & np.uint64(mask)) == np.uint64(slot)][:count]]
    assert len(keys) == count, (shape, slot, len(keys))
    for x in keys:  # the scalar oracle has the last word
        if shape == "int32":
            hv = O.hash_int(x, 42)
        elif shape == "int64":
            hv = O.hash_long(x, 42)
        else:
            hv = O.hash_long(x, O.hash_int(7, 42))
        assert hv & mask == slot
    return keys


def collision_columns(shape, keys, device="cpu"):
    """-> ([Column], kinds, oracle cols) for keys of colliding_keys()."""
    if shape == "pair":
        kinds = ["int32", "int64"]
        cols = [[7] * len(keys), list(keys)]
    else:
        kinds = [shape]
        cols = [list(keys)]
    return [column(kd, c, device) for kd, c in zip(kinds, cols)], kinds, cols
