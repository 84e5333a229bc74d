"""Hot-op dispatch: native HIP kernels on GPU, reference impls on CPU.

The CPU implementations are the correctness oracles (the analogue of the
reference's JVM-less test mode) — GPU numerics tests compare
kernel output against these bit-for-bit (hashes) or set-wise (tables).

GPU path REQUIRES the native library (no silent eager fallback): see
auron_amd.native.require().
"""
from __future__ import annotations

import os
from typing import List, Optional, Tuple

import torch

from . import dtypes, native
from .column import Column

SPARK_SEED = 42
_M32 = 0xFFFFFFFF
_M64 = (1 << 64) - 1


def _use_native(device: torch.device) -> bool:
    if device.type != "cuda":
        return False
    if os.environ.get("AURON_FORCE_REF", "0") == "1":
        return False  # debugging only: force torch/host reference paths
    if os.environ.get("AURON_REQUIRE_NATIVE", "1") == "0" and not native.available():
        return False
    native.require()  # raise loudly on GPU when missing
    return True


# ===================================================================== hash
def _rotl(x, r):
    return (((x << r) & _M32) | (x >> (32 - r))) & _M32


def _mixk1(k):
    k = (k * 0xCC9E2D51) & _M32
    k = _rotl(k, 15)
    k = (k * 0x1B873593) & _M32
    return k


def _mixh1(h, k):
    h = (h ^ k) & _M32
    h = _rotl(h, 13)
    h = (h * 5 + 0xE6546B64) & _M32
    return h


def _fmix(h, length):
    h = (h ^ length) & _M32
    h = h ^ (h >> 16)
    h = (h * 0x85EBCA6B) & _M32
    h = h ^ (h >> 13)
    h = (h * 0xC2B2AE35) & _M32
    h = h ^ (h >> 16)
    return h


def _hash_int_t(v, seed):
    return _fmix(_mixh1(seed, _mixk1(v & _M32)), 4)


def _hash_long_t(v, seed):
    h = _mixh1(seed, _mixk1(v & _M32))
    h = _mixh1(h, _mixk1((v >> 32) & _M32))
    return _fmix(h, 8)


def _hash_padded_bytes_t(padded, lens, maxlen, h):
    """hashUnsafeBytes over rows of a padded byte matrix: `padded` [n, >=
    maxlen] int64 byte values, `lens` [n] byte counts (<= maxlen), `h` [n]
    running seeds. Whole words little-endian, tail bytes sign-extended."""
    hv = h.clone()
    nwords = maxlen // 4
    for j in range(nwords):
        w = (padded[:, 4 * j] | (padded[:, 4 * j + 1] << 8)
             | (padded[:, 4 * j + 2] << 16) | (padded[:, 4 * j + 3] << 24))
        m = lens >= 4 * (j + 1)
        hv = torch.where(m, _mixh1(hv, _mixk1(w)), hv)
    aligned = lens & ~3
    for t in range(maxlen):
        m = (t >= aligned) & (t < lens)
        if not bool(m.any()):
            continue
        b = padded[:, t]
        sb = torch.where(b >= 128, (b - 256) & _M32, b)
        hv = torch.where(m, _mixh1(hv, _mixk1(sb)), hv)
    return _fmix(hv, lens & _M32)


def _hash_dec128_t(d, h):
    """Spark's hash of a decimal with precision > 18 over [n,2] limbs:
    hashUnsafeBytes(BigInteger.toByteArray(unscaled)). toByteArray is the
    minimal big-endian two's-complement encoding: the 16 bytes of the value
    less every leading byte that only repeats the sign (a byte equal to the
    sign byte whose successor's top bit is the sign bit too)."""
    lo, hi = d[:, 0], d[:, 1]
    shifts = range(56, -8, -8)
    B = torch.stack([(hi >> s) & 0xFF for s in shifts]
                    + [(lo >> s) & 0xFF for s in shifts], dim=1)  # big-endian
    sign = (hi >> 63) & 1
    redundant = ((B[:, :15] == (sign * 0xFF)[:, None])
                 & ((B[:, 1:] >> 7) == sign[:, None]))
    skip = torch.cumprod(redundant.to(torch.int64), dim=1).sum(dim=1)
    lens = 16 - skip
    idx = skip[:, None] + torch.arange(16, device=d.device)[None, :]
    return _hash_padded_bytes_t(B.gather(1, idx.clamp(max=15)), lens, 16, h)


def _spark_narrow_decimal(dt) -> bool:
    """A DECIMAL128-coded type that Spark hashes as a long: precision <= 18,
    so the value is its low limb."""
    return dt.code == dtypes.DECIMAL128 and dt.precision <= 18


def murmur3_ref(cols: List[Column], seed: int = SPARK_SEED) -> torch.Tensor:
    """Pure-torch Spark Murmur3_x86_32, bit-exact vs the HIP kernel.

    Reference semantics: spark_hash.rs (seed-chained per column, nulls
    skipped, -0.0 normalized, every NaN hashed as the canonical one,
    timestamps as longs, strings hashed as UTF-8 bytes, decimals by
    precision: <= 18 as the unscaled long, wider as the minimal big-endian
    bytes of the unscaled value).
    """
    n = len(cols[0])
    device = cols[0].device
    h = torch.full((n,), seed, dtype=torch.int64, device=device)
    for c in cols:
        if c.dtype.is_string:
            from . import strings as S

            lens = S.lengths(c)
            maxlen = int(lens.max().item()) if n else 0
            padded = S.to_padded(c, max(maxlen, 1)).to(torch.int64)
            hv = _hash_padded_bytes_t(padded, lens, maxlen, h)
        else:
            d = c.data
            code = c.dtype.code
            if code in (dtypes.BOOL,):
                v = d.to(torch.int64)
                hv = _hash_int_t(v, h)
            elif code in (dtypes.INT8, dtypes.INT16, dtypes.INT32, dtypes.DATE32):
                v = d.to(torch.int64) & _M32
                hv = _hash_int_t(v, h)
            elif code in (dtypes.INT64, dtypes.DECIMAL64, dtypes.TIMESTAMP):
                v = d.to(torch.int64)
                hv = _hash_long_t(v, h)
            elif code == dtypes.FLOAT32:
                # floatToIntBits: -0.0 as 0.0, every NaN as 0x7fc00000
                f = torch.where(d == 0, torch.zeros_like(d), d)
                v = f.view(torch.int32).to(torch.int64) & _M32
                v = torch.where(torch.isnan(d), torch.full_like(v, 0x7FC00000), v)
                hv = _hash_int_t(v, h)
            elif code == dtypes.FLOAT64:
                # doubleToLongBits: -0.0 as 0.0, every NaN as 0x7ff8000000000000
                f = torch.where(d == 0, torch.zeros_like(d), d)
                v = f.view(torch.int64)
                v = torch.where(torch.isnan(d), torch.full_like(v, 0x7FF8 << 48), v)
                hv = _hash_long_t(v, h)
            elif code == dtypes.DECIMAL128:
                if _spark_narrow_decimal(c.dtype):
                    hv = _hash_long_t(d[:, 0], h)
                else:
                    hv = _hash_dec128_t(d, h)
            else:
                raise TypeError(c.dtype.name)
        if c.validity is not None:
            h = torch.where(c.validity, hv, h)
        else:
            h = hv
    # reinterpret as signed int32
    h = torch.where(h >= 2 ** 31, h - 2 ** 32, h)
    return h.to(torch.int32)


def _key_cols(cols: List[Column]) -> List[Column]:
    """Key columns as the native kernels read them: a decimal128 column's
    limb pairs contiguous and 16-byte aligned (hash_one and keys_equal load
    a pair in one 16-byte access)."""
    out = []
    for c in cols:
        if c.dtype.code == dtypes.DECIMAL128:
            d = _i128_aligned(c.data)
            if d is not c.data:
                c = Column(c.dtype, d, c.validity)
        out.append(c)
    return out


def _spark_hash_cols(cols: List[Column]) -> List[Column]:
    """Columns as Spark's row hash sees them. AuColDesc carries no
    precision, so a DECIMAL128-coded column of precision <= 18 (hashed by
    Spark as a long) goes to the kernel as a DECIMAL64 over its low limb."""
    out = []
    for c in cols:
        if _spark_narrow_decimal(c.dtype):
            c = Column(dtypes.decimal64(c.dtype.precision, c.dtype.scale),
                       c.data[:, 0].contiguous(), c.validity)
        out.append(c)
    return out


def _murmur3_native(cols: List[Column], seed: int = SPARK_SEED) -> torch.Tensor:
    """k_murmur3 over the columns as they are: every DECIMAL128 column by
    the byte rule, whatever its precision."""
    device = cols[0].device
    n = len(cols[0])
    lib = native.lib()
    out = torch.empty(n, dtype=torch.int32, device=device)
    descs, keep = native.pack_descs(_key_cols(cols), device)
    rc = lib.au_murmur3(descs.data_ptr(), len(cols), n, seed, out.data_ptr(),
                        native.stream_ptr(device))
    native.check(rc, "au_murmur3")
    del keep
    return out


def murmur3(cols: List[Column], seed: int = SPARK_SEED) -> torch.Tensor:
    device = cols[0].device
    if not _use_native(device):
        return murmur3_ref(cols, seed)
    return _murmur3_native(_spark_hash_cols(cols), seed)


def _join_hash(cols: List[Column]) -> torch.Tensor:
    """Row hash of a join table. The fused probe kernels hash the probe key
    in-kernel from the same descriptors they compare with, so build and
    probe rows take the kernel's rule for the column's dtype code alone
    (a decimal128 key by its bytes at every precision). The table is
    internal: only the two sides have to agree."""
    return _murmur3_native(cols)


# ================================================================= group-by
def _next_pow2(x: int) -> int:
    p = 1024
    while p < x:
        p <<= 1
    return p


def _key_tuple_lists(cols: List[Column]):
    import math

    lists = []
    for c in cols:
        if c.dtype.code == dtypes.DECIMAL128:
            # exact unscaled ints: to_pylist divides into a float, which
            # merges neighbouring wide values
            d = c.data.to("cpu")
            valid = None if c.validity is None else c.validity.tolist()
            vals = [(h << 64) | (l & _M64) for l, h in
                    zip(d[:, 0].tolist(), d[:, 1].tolist())]
            if valid is not None:
                vals = [v if ok else None for v, ok in zip(vals, valid)]
            lists.append(vals)
            continue
        if c.dtype.code == dtypes.DECIMAL64:
            # exact unscaled ints as well: dividing by the scale merges
            # neighbouring values beyond 2**53
            vals = c.data.tolist()
            if c.validity is not None:
                vals = [v if ok else None
                        for v, ok in zip(vals, c.validity.tolist())]
            lists.append(vals)
            continue
        if c.dtype.is_string:
            # the bytes themselves: decoding merges strings that differ only
            # inside invalid UTF-8
            raw = c.data.to("cpu").numpy().tobytes()
            offs = c.offsets.tolist()
            vals = [raw[offs[i]:offs[i + 1]] for i in range(len(c))]
            if c.validity is not None:
                vals = [v if ok else None
                        for v, ok in zip(vals, c.validity.tolist())]
            lists.append(vals)
            continue
        vals = c.to_pylist()
        if c.dtype.is_float:
            vals = ["NaN" if (v is not None and isinstance(v, float) and math.isnan(v)) else v for v in vals]
        lists.append(vals)
    return list(zip(*lists)) if cols else []


def group_ids_ref(cols: List[Column]) -> Tuple[torch.Tensor, torch.Tensor]:
    keys = _key_tuple_lists(cols)
    d = {}
    gids = []
    reps = []
    for i, k in enumerate(keys):
        g = d.get(k)
        if g is None:
            g = len(d)
            d[k] = g
            reps.append(i)
        gids.append(g)
    device = cols[0].device
    return (torch.tensor(gids, dtype=torch.int64, device=device),
            torch.tensor(reps, dtype=torch.int64, device=device))


def group_ids(cols: List[Column]) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (gid per row [n] int64, representative row per group [G] int64).

    Group order is order-of-appearance on CPU, unspecified on GPU (atomic
    assignment) — SQL GROUP BY output order is unspecified anyway.
    """
    device = cols[0].device
    n = len(cols[0])
    if n == 0:
        return (torch.empty(0, dtype=torch.int64, device=device),
                torch.empty(0, dtype=torch.int64, device=device))
    if not _use_native(device):
        return group_ids_ref(cols)
    lib = native.lib()
    cols = _key_cols(cols)
    hashes = murmur3(cols)
    cap = _next_pow2(2 * n)
    slots = torch.full((cap,), -1, dtype=torch.int32, device=device)
    rep = torch.empty(n, dtype=torch.int32, device=device)
    gids = torch.empty(n, dtype=torch.int32, device=device)
    rep_rows = torch.empty(n, dtype=torch.int64, device=device)
    counter = torch.zeros(1, dtype=torch.int32, device=device)
    descs, keep = native.pack_descs(cols, device)
    rc = lib.au_group_ids(descs.data_ptr(), len(cols), n, slots.data_ptr(), cap,
                          hashes.data_ptr(), rep.data_ptr(), gids.data_ptr(),
                          rep_rows.data_ptr(), counter.data_ptr(),
                          native.stream_ptr(device))
    native.check(rc, "au_group_ids")
    ng = int(counter.item())
    del keep
    return gids.to(torch.int64), rep_rows[:ng]


# ==================================================================== joins
def hash_join_ref(build_cols, probe_cols, emit_unmatched_probe, need_build_matched):
    bkeys = _key_tuple_lists(build_cols)
    pkeys = _key_tuple_lists(probe_cols)
    table = {}
    for j, k in enumerate(bkeys):
        if any(v is None for v in k):
            continue
        table.setdefault(k, []).append(j)
    n_build = len(build_cols[0]) if build_cols else 0
    matched = [False] * n_build
    bi, pi = [], []
    for i, k in enumerate(pkeys):
        rows = [] if any(v is None for v in k) else table.get(k, [])
        if rows:
            for j in rows:
                bi.append(j)
                pi.append(i)
                matched[j] = True
        elif emit_unmatched_probe:
            bi.append(-1)
            pi.append(i)
    device = probe_cols[0].device
    bm = torch.tensor(matched, dtype=torch.bool, device=device) if need_build_matched else None
    return (torch.tensor(bi, dtype=torch.int64, device=device),
            torch.tensor(pi, dtype=torch.int64, device=device), bm)



class JoinTable:
    """Prebuilt chained hash table over a broadcast build side (the
    reference's cached_build_hash_map_id object,
    broadcast_join_exec.rs:90): heads/next chains + row hashes stay in
    HBM so repeated probes of the same relation skip the build pass."""

    __slots__ = ("heads", "nxt", "cap", "bhash", "n_build")

    def __init__(self, heads, nxt, cap, bhash, n_build):
        self.heads = heads
        self.nxt = nxt
        self.cap = cap
        self.bhash = bhash
        self.n_build = n_build

    @property
    def nbytes(self):
        return (self.heads.numel() + self.nxt.numel()) * 4 + self.bhash.numel() * 8


def join_build(build_cols: List[Column]) -> Optional["JoinTable"]:
    """Build the chained table once (au_join_build); None on the CPU
    reference path (which has no reusable native table)."""
    device = build_cols[0].device
    if not _use_native(device):
        return None
    lib = native.lib()
    sp = native.stream_ptr(device)
    n_build = len(build_cols[0])
    bhash = _join_hash(build_cols)
    cap = _next_pow2(2 * max(n_build, 1))
    heads = torch.full((cap,), -1, dtype=torch.int32, device=device)
    nxt = torch.empty(max(n_build, 1), dtype=torch.int32, device=device)
    if n_build:
        rc = lib.au_join_build(n_build, heads.data_ptr(), cap, nxt.data_ptr(),
                               bhash.data_ptr(), sp)
        native.check(rc, "au_join_build")
    return JoinTable(heads, nxt, cap, bhash, n_build)


JOIN_PROBE_MAX_KEYS = 8  # JP_MAX_KEYS in kernels.hip (au_join_probe_max_keys)


def _fused_probe_enabled() -> bool:
    from .config import JOIN_FUSED_PROBE, AuronConf

    return bool(AuronConf().get(JOIN_FUSED_PROBE))


def join_probe_tile() -> int:
    """Probe rows per tile of the fused probe kernels (JP_TILE)."""
    return int(native.lib().au_join_probe_tile())


def _join_key_descs(build_cols, probe_cols):
    """Host AuColDesc[2 * ncols], build keys then probe keys, for the
    kernels that take key descriptors by value."""
    import numpy as np

    barr, bkeep = native.pack_descs_host(_key_cols(build_cols))
    parr, pkeep = native.pack_descs_host(_key_cols(probe_cols))
    return np.concatenate([barr, parr]), (bkeep, pkeep)


def hash_join(build_cols: List[Column], probe_cols: List[Column],
              emit_unmatched_probe: bool = False,
              need_build_matched: bool = False,
              table: Optional["JoinTable"] = None):
    """Hash-join index computation.

    -> (build_idx [m] int64 (-1 = probe row had no match),
        probe_idx [m] int64,
        build_matched [n_build] bool | None)
    SQL NULL join keys never match (join_row_has_null in kernels.hip).
    Pairs come in ascending probe row, chain order within a row, on both
    the fused path (spark.auron.join.fusedProbe.enable) and the legacy one.
    """
    device = probe_cols[0].device
    n_probe = len(probe_cols[0])
    n_build = len(build_cols[0])
    if not _use_native(device):
        return hash_join_ref(build_cols, probe_cols, emit_unmatched_probe, need_build_matched)
    if table is None:
        table = join_build(build_cols)
    if len(build_cols) <= JOIN_PROBE_MAX_KEYS and _fused_probe_enabled():
        return _hash_join_fused(build_cols, probe_cols, emit_unmatched_probe,
                                need_build_matched, table)
    return _hash_join_legacy(build_cols, probe_cols, emit_unmatched_probe,
                             need_build_matched, table)


def _hash_join_fused(build_cols, probe_cols, emit_unmatched_probe,
                     need_build_matched, table):
    """k_join_probe_count -> cumsum over the per-tile sums -> one .item()
    for the output size -> k_join_probe_fill. build_matched is set by the
    count kernel, whose walk visits every match anyway, so the fill
    kernel's one-match rows touch neither the table nor a key."""
    device = probe_cols[0].device
    n_probe = len(probe_cols[0])
    n_build = len(build_cols[0])
    lib = native.lib()
    sp = native.stream_ptr(device)
    bm = torch.zeros(n_build, dtype=torch.uint8, device=device) if need_build_matched else None
    if n_probe == 0:
        empty = torch.empty(0, dtype=torch.int64, device=device)
        return empty, empty.clone(), (bm.bool() if bm is not None else None)
    ncols = len(build_cols)
    descs, keep = _join_key_descs(build_cols, probe_cols)
    tile = join_probe_tile()
    n_tiles = (n_probe + tile - 1) // tile
    counts = torch.empty(n_probe, dtype=torch.int32, device=device)
    first = torch.empty(n_probe, dtype=torch.int32, device=device)
    tile_sums = torch.empty(n_tiles, dtype=torch.int64, device=device)
    emit = 1 if emit_unmatched_probe else 0
    rc = lib.au_join_probe_count(descs.ctypes.data, ncols, n_probe,
                                 table.heads.data_ptr(), table.cap,
                                 table.nxt.data_ptr(), SPARK_SEED, emit,
                                 counts.data_ptr(), first.data_ptr(),
                                 tile_sums.data_ptr(),
                                 bm.data_ptr() if bm is not None and n_build else None,
                                 sp)
    native.check(rc, "au_join_probe_count")
    tile_ends = torch.cumsum(tile_sums, 0)
    total = int(tile_ends[-1].item())
    build_idx = torch.empty(max(total, 1), dtype=torch.int64, device=device)
    probe_idx = torch.empty(max(total, 1), dtype=torch.int64, device=device)
    rc = lib.au_join_probe_fill(descs.ctypes.data, ncols, n_probe,
                                table.nxt.data_ptr(), counts.data_ptr(),
                                first.data_ptr(), tile_ends.data_ptr(), emit,
                                build_idx.data_ptr(), probe_idx.data_ptr(), sp)
    native.check(rc, "au_join_probe_fill")
    del keep
    return build_idx[:total], probe_idx[:total], (bm.bool() if bm is not None else None)


def _hash_join_legacy(build_cols, probe_cols, emit_unmatched_probe,
                      need_build_matched, table):
    device = probe_cols[0].device
    n_probe = len(probe_cols[0])
    n_build = len(build_cols[0])
    lib = native.lib()
    sp = native.stream_ptr(device)
    heads, nxt, cap, bhash = table.heads, table.nxt, table.cap, table.bhash
    build_cols, probe_cols = _key_cols(build_cols), _key_cols(probe_cols)
    phash = _join_hash(probe_cols)
    bdescs, bkeep = native.pack_descs(build_cols, device)
    pdescs, pkeep = native.pack_descs(probe_cols, device)
    counts = torch.zeros(n_probe, dtype=torch.int32, device=device)
    rc = lib.au_join_count(bdescs.data_ptr(), pdescs.data_ptr(), len(build_cols),
                           n_probe, heads.data_ptr(), cap, nxt.data_ptr(),
                           phash.data_ptr(), counts.data_ptr(), sp)
    native.check(rc, "au_join_count")
    eff = counts.to(torch.int64)
    if emit_unmatched_probe:
        eff = eff.clamp(min=1)
    offsets = torch.zeros(n_probe + 1, dtype=torch.int64, device=device)
    torch.cumsum(eff, 0, out=offsets[1:])
    total = int(offsets[-1].item())
    build_idx = torch.empty(max(total, 1), dtype=torch.int64, device=device)
    probe_idx = torch.empty(max(total, 1), dtype=torch.int64, device=device)
    bm = torch.zeros(n_build, dtype=torch.uint8, device=device) if need_build_matched else None
    rc = lib.au_join_fill(bdescs.data_ptr(), pdescs.data_ptr(), len(build_cols),
                          n_probe, heads.data_ptr(), cap, nxt.data_ptr(),
                          phash.data_ptr(), offsets.data_ptr(),
                          build_idx.data_ptr(), probe_idx.data_ptr(),
                          bm.data_ptr() if bm is not None else None,
                          1 if emit_unmatched_probe else 0, sp)
    native.check(rc, "au_join_fill")
    del bkeep, pkeep
    return build_idx[:total], probe_idx[:total], (bm.bool() if bm is not None else None)


def join_exists(build_cols: List[Column], probe_cols: List[Column],
                table: Optional["JoinTable"] = None) -> torch.Tensor:
    """Per-probe-row "has at least one match" (semi/anti/existence joins),
    bool [n_probe]. k_join_exists stops at the first match and reuses a
    prebuilt `table`; with the fused probe switched off, or more than 8 key
    columns, it is join_counts(...) > 0."""
    device = probe_cols[0].device
    n_probe = len(probe_cols[0])
    if not _use_native(device):
        _, pi, _ = hash_join_ref(build_cols, probe_cols, False, False)
        out = torch.zeros(n_probe, dtype=torch.bool, device=device)
        if pi.numel():
            out[pi] = True
        return out
    if len(build_cols) > JOIN_PROBE_MAX_KEYS or not _fused_probe_enabled():
        return join_counts(build_cols, probe_cols) > 0
    if table is None:
        table = join_build(build_cols)
    out = torch.empty(n_probe, dtype=torch.bool, device=device)  # kernel writes 0/1 bytes
    if n_probe:
        descs, keep = _join_key_descs(build_cols, probe_cols)
        rc = native.lib().au_join_exists(descs.ctypes.data, len(build_cols),
                                         n_probe, table.heads.data_ptr(),
                                         table.cap, table.nxt.data_ptr(),
                                         SPARK_SEED, out.data_ptr(),
                                         native.stream_ptr(device))
        native.check(rc, "au_join_exists")
        del keep
    return out


def join_counts(build_cols: List[Column], probe_cols: List[Column]) -> torch.Tensor:
    """Per-probe-row match count (semi/anti/existence joins)."""
    device = probe_cols[0].device
    n_probe = len(probe_cols[0])
    n_build = len(build_cols[0])
    if not _use_native(device):
        bi, pi, _ = hash_join_ref(build_cols, probe_cols, False, False)
        counts = torch.zeros(n_probe, dtype=torch.int32)
        if pi.numel():
            counts.scatter_add_(0, pi, torch.ones(pi.numel(), dtype=torch.int32))
        return counts
    lib = native.lib()
    sp = native.stream_ptr(device)
    build_cols, probe_cols = _key_cols(build_cols), _key_cols(probe_cols)
    bhash = _join_hash(build_cols)
    phash = _join_hash(probe_cols)
    cap = _next_pow2(2 * max(n_build, 1))
    heads = torch.full((cap,), -1, dtype=torch.int32, device=device)
    nxt = torch.empty(max(n_build, 1), dtype=torch.int32, device=device)
    bdescs, bkeep = native.pack_descs(build_cols, device)
    pdescs, pkeep = native.pack_descs(probe_cols, device)
    if n_build:
        rc = lib.au_join_build(n_build, heads.data_ptr(), cap, nxt.data_ptr(),
                               bhash.data_ptr(), sp)
        native.check(rc, "au_join_build")
    counts = torch.zeros(n_probe, dtype=torch.int32, device=device)
    rc = lib.au_join_count(bdescs.data_ptr(), pdescs.data_ptr(), len(build_cols),
                           n_probe, heads.data_ptr(), cap, nxt.data_ptr(),
                           phash.data_ptr(), counts.data_ptr(), sp)
    native.check(rc, "au_join_count")
    del bkeep, pkeep
    return counts


def string_sort_ranks(c: Column) -> torch.Tensor:
    """Order-preserving dense ranks for a string column (device int64).

    Unique strings (group-table reps) are sorted on the host — uniques are
    small — and each row maps to its rank through the device group ids.
    Used by sort/window so string order-by keys never fall back to a host
    argsort over the full column."""
    gids, reps = group_ids([c])
    rep_vals = c.gather(reps).to_pylist()
    order = sorted(range(len(rep_vals)),
                   key=lambda i: (rep_vals[i] is None, rep_vals[i] or ""))
    rank = [0] * len(rep_vals)
    for r, i in enumerate(order):
        rank[i] = r
    rank_t = torch.tensor(rank, dtype=torch.int64, device=c.device)
    return rank_t[gids]


# ============================================================= range bucket
_MIN64 = -(1 << 63)


def _bytes_cmp_sign(a_data, a_start, a_len, b_data, b_start, b_len,
                    chunk: int = 64) -> torch.Tensor:
    """Row-wise sign of the unsigned-byte lexicographic compare a[i] vs b[i]
    (-1 / 0 / +1, int64); a proper prefix sorts first. Exact for any length:
    the padded compare walks `chunk` byte columns at a time over the rows
    still undecided (padding is -1, below every byte)."""
    n = a_start.numel()
    device = a_start.device
    sign = torch.zeros(n, dtype=torch.int64, device=device)
    if n == 0:
        return sign
    if a_data.numel() == 0:
        a_data = torch.zeros(1, dtype=torch.uint8, device=device)
    if b_data.numel() == 0:
        b_data = torch.zeros(1, dtype=torch.uint8, device=device)
    width = int(torch.maximum(a_len.max(), b_len.max()).item())
    und = torch.arange(n, dtype=torch.int64, device=device)
    pos = torch.arange(chunk, dtype=torch.int64, device=device)
    pad = torch.full((), -1, dtype=torch.int16, device=device)
    c = 0
    while c < width and und.numel():
        p = (c + pos)[None, :]

        def _pad(data, start, ln):
            idx = (start[und, None] + p).clamp(0, data.numel() - 1)
            return torch.where(p < ln[und, None], data[idx].to(torch.int16), pad)

        av = _pad(a_data, a_start, a_len)
        bv = _pad(b_data, b_start, b_len)
        neq = av != bv
        anyd = neq.any(1)
        first = neq.to(torch.int8).argmax(1, keepdim=True)
        d = (av.gather(1, first) - bv.gather(1, first)).squeeze(1).sign()
        sign[und[anyd]] = d[anyd].to(torch.int64)
        und = und[~anyd]
        c += chunk
    return sign


def range_bucket_ref(key: Column, bounds: Column, right: bool = False) -> torch.Tensor:
    """Oracle for range_bucket (pure torch, exact — no padded-width
    truncation): torch.searchsorted(bounds, key, right=right) semantics
    for string and decimal128 keys."""
    device = key.device
    n = len(key)
    nb = len(bounds)
    if key.dtype.is_string:
        k_start = key.offsets[:-1]
        k_len = key.offsets[1:] - k_start
        b_start = bounds.offsets[:-1]
        b_len = bounds.offsets[1:] - b_start
        lo = torch.zeros(n, dtype=torch.int64, device=device)
        hi = torch.full((n,), nb, dtype=torch.int64, device=device)
        # binary search vectorised over rows: the interval at least halves
        # per step, so bit_length(nb) steps close every row
        for _ in range(nb.bit_length()):
            active = lo < hi
            mid = ((lo + hi) >> 1).clamp(max=max(nb - 1, 0))
            c = _bytes_cmp_sign(bounds.data, b_start[mid], b_len[mid],
                                key.data, k_start, k_len)
            go = (c <= 0) if right else (c < 0)
            lo = torch.where(active & go, mid + 1, lo)
            hi = torch.where(active & ~go, mid, hi)
        return lo
    assert key.dtype.code == dtypes.DECIMAL128
    out = torch.zeros(n, dtype=torch.int64, device=device)
    lo_u = key.data[:, 0] ^ _MIN64
    hi_s = key.data[:, 1]
    for j in range(nb):
        bl = bounds.data[j, 0] ^ _MIN64
        bh = bounds.data[j, 1]
        gt = (hi_s > bh) | ((hi_s == bh) & (lo_u > bl))
        if right:
            gt = gt | ((hi_s == bh) & (lo_u == bl))
        out += gt.to(torch.int64)
    return out


def range_bucket(key: Column, bounds: Column, right: bool = False) -> torch.Tensor:
    """Range bucket of every row of `key` against the ascending, non-null
    `bounds` (-> int64 [len(key)] on the key's device), with the semantics
    of torch.searchsorted(bounds, key, right=right): the number of bounds
    strictly less than the row, or `<=` the row when `right`.

    Strings order by unsigned UTF-8 bytes (a proper prefix first);
    decimal128 by its full 128-bit value. Null rows get an arbitrary
    bucket — the caller overwrites them."""
    assert bounds.validity is None or bool(bounds.validity.all()), \
        "range_bucket: bounds must be non-null"
    device = key.device
    wide = key.dtype.is_string or key.dtype.code == dtypes.DECIMAL128
    if not wide:
        assert not bounds.dtype.is_string and bounds.dtype.code != dtypes.DECIMAL128, \
            f"range_bucket: {key.dtype.name} key vs {bounds.dtype.name} bounds"
        kd, bd = key.data, bounds.data.to(device)
        if kd.dtype == torch.bool:
            kd = kd.to(torch.int8)
        if bd.dtype != kd.dtype:
            t = torch.promote_types(kd.dtype, bd.dtype)
            kd, bd = kd.to(t), bd.to(t)
        return torch.searchsorted(bd, kd, right=right)
    assert bounds.dtype.code == key.dtype.code, \
        f"range_bucket: {key.dtype.name} key vs {bounds.dtype.name} bounds"
    bounds = bounds.to(device)
    if not _use_native(device):
        return range_bucket_ref(key, bounds, right)
    lib = native.lib()
    n = len(key)
    nb = len(bounds)
    out = torch.empty(n, dtype=torch.int32, device=device)
    sp = native.stream_ptr(device)
    if key.dtype.is_string:
        kdata, koff = key.data.contiguous(), key.offsets.contiguous()
        bdata, boff = bounds.data.contiguous(), bounds.offsets.contiguous()
        rc = lib.au_range_bucket_str(kdata.data_ptr(), koff.data_ptr(), n,
                                     bdata.data_ptr(), boff.data_ptr(), nb,
                                     int(bool(right)), out.data_ptr(), sp)
        native.check(rc, "au_range_bucket_str")
    else:
        kdata, bdata = key.data.contiguous(), bounds.data.contiguous()
        rc = lib.au_range_bucket_i128(kdata.data_ptr(), n, bdata.data_ptr(),
                                      nb, int(bool(right)), out.data_ptr(), sp)
        native.check(rc, "au_range_bucket_i128")
    return out.to(torch.int64)


# ============================================================ window frames
_MAX64 = (1 << 63) - 1


def _sat_add(k: torch.Tensor, d: int) -> torch.Tensor:
    """k + d over int64, saturating at the int64 limits (never wraps)."""
    d = int(d)
    assert -_MAX64 <= d <= _MAX64, "window offset out of int64 range"
    s = k + d  # wraps
    if d > 0:
        return torch.where(s < k, torch.full_like(k, _MAX64), s)
    if d < 0:
        return torch.where(s > k, torch.full_like(k, _MIN64), s)
    return s


def _window_bounds_args(key, slo, shi, lo, hi):
    assert key.dtype in (torch.int64, torch.float64), \
        f"window_range_bounds: int64 or float64 keys, got {key.dtype}"
    assert slo.dtype == torch.int64 and shi.dtype == torch.int64
    assert key.numel() == slo.numel() == shi.numel()
    is_int = key.dtype == torch.int64
    conv = int if is_int else float
    lo_v = conv(0) if lo is None else conv(lo)
    hi_v = conv(0) if hi == "U" else conv(hi)
    if is_int:
        assert -_MAX64 <= lo_v <= _MAX64 and -_MAX64 <= hi_v <= _MAX64, \
            "window offset out of int64 range"
    return lo_v, hi_v


def window_range_bounds_ref(key: torch.Tensor, slo: torch.Tensor,
                            shi: torch.Tensor, lo, hi,
                            descending: bool = False):
    """Oracle for window_range_bounds (pure torch): the same two binary
    searches, vectorised over rows."""
    lo_v, hi_v = _window_bounds_args(key, slo, shi, lo, hi)
    n = key.numel()
    is_int = key.dtype == torch.int64
    w0 = slo.clamp(min=0)
    w1 = shi.clamp(max=n - 1)
    if n == 0:
        return w0.clone(), w1.clone()

    def target(off):
        if is_int:
            return _sat_add(key, -off if descending else off)
        return key - off if descending else key + off

    steps = max(int((w1 - w0).max().item()) + 1, 1).bit_length()

    def search(inside, first):
        # first=True : first index whose key is inside  (inside is a suffix)
        # first=False: one past the last inside index   (inside is a prefix)
        l, h = w0.clone(), w1 + 1
        for _ in range(steps):
            active = l < h
            mid = (l + ((h - l) >> 1)).clamp(0, n - 1)
            ins = inside(key[mid])
            go_left = ins if first else ~ins
            h = torch.where(active & go_left, mid, h)
            l = torch.where(active & ~go_left, mid + 1, l)
        return l

    if lo is None:
        a = w0.clone()
    else:
        t = target(lo_v)
        a = search((lambda v: v <= t) if descending else (lambda v: v >= t),
                   True)
    if hi == "U":
        b = w1.clone()
    else:
        t = target(hi_v)
        b = search((lambda v: v >= t) if descending else (lambda v: v <= t),
                   False) - 1
    return a, b


def window_range_bounds(key: torch.Tensor, slo: torch.Tensor,
                        shi: torch.Tensor, lo, hi, descending: bool = False):
    """RANGE-frame resolution by key value -> (a, b), int64 [n] each.

    `key` (int64 or float64) is sorted so that inside every row's inclusive
    index window [slo[i], shi[i]] the keys are monotone — non-decreasing,
    or non-increasing when `descending` — with no null or NaN in it.
    `lo` / `hi` are signed offsets in the key domain (preceding < 0), or
    None (lo) / "U" (hi) for unbounded, which resolve to the window edge.
    With k = key[i]:
      a[i] = first j in the window with key[j] >= k+lo   (desc: <= k-lo)
      b[i] = last  j in the window with key[j] <= k+hi   (desc: >= k-hi)
    and a[i] = shi[i]+1 / b[i] = slo[i]-1 when no key qualifies, so
    a > b marks an empty frame. int64 k±offset saturates; float64 is IEEE."""
    lo_v, hi_v = _window_bounds_args(key, slo, shi, lo, hi)
    device = key.device
    if not _use_native(device):
        return window_range_bounds_ref(key, slo, shi, lo, hi, descending)
    lib = native.lib()
    n = key.numel()
    key, slo, shi = key.contiguous(), slo.contiguous(), shi.contiguous()
    a = torch.empty(n, dtype=torch.int64, device=device)
    b = torch.empty(n, dtype=torch.int64, device=device)
    flags = ((1 if lo is None else 0) | (2 if hi == "U" else 0)
             | (4 if descending else 0))
    fn = (lib.au_window_range_bounds_i64 if key.dtype == torch.int64
          else lib.au_window_range_bounds_f64)
    rc = fn(key.data_ptr(), slo.data_ptr(), shi.data_ptr(), n, lo_v, hi_v,
            flags, a.data_ptr(), b.data_ptr(), native.stream_ptr(device))
    native.check(rc, "au_window_range_bounds")
    return a, b


def _window_minmax_args(x, a, b, op):
    assert op in ("min", "max"), op
    assert x.dtype in (torch.int64, torch.float64), \
        f"window_frame_minmax: int64 or float64 values, got {x.dtype}"
    assert a.dtype == torch.int64 and b.dtype == torch.int64
    assert a.numel() == b.numel()
    if x.dtype == torch.int64:
        return _MIN64 if op == "max" else _MAX64
    return float("-inf") if op == "max" else float("inf")


def window_frame_minmax_ref(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                            op: str) -> torch.Tensor:
    """Oracle for window_frame_minmax (pure torch): doubling sparse table,
    two overlapping power-of-two blocks per query."""
    ident = _window_minmax_args(x, a, b, op)
    n = x.numel()
    combine = torch.minimum if op == "min" else torch.maximum
    out = torch.full((a.numel(),), ident, dtype=x.dtype, device=x.device)
    lo = a.clamp(min=0)
    hi = b.clamp(max=n - 1)
    ln = hi - lo + 1
    if a.numel() == 0 or n == 0 or int(ln.max().item()) <= 0:
        return out
    level = x
    k = 0
    maxlen = int(ln.max().item())
    while True:
        w = 1 << k
        # rows whose frame length is in [2^k, 2^(k+1))
        sel = (ln >= w) & (ln < 2 * w)
        if bool(sel.any()):
            out[sel] = combine(level[lo[sel]], level[hi[sel] - w + 1])
        if 2 * w > maxlen:
            break
        # level[i] = op(x[i .. i+2w-1]); the tail keeps shorter blocks,
        # which no query of that length can address
        nxt = level.clone()
        nxt[:n - w] = combine(level[:n - w], level[w:])
        level = nxt
        k += 1
    return out


def window_frame_minmax(x: torch.Tensor, a: torch.Tensor, b: torch.Tensor,
                        op: str) -> torch.Tensor:
    """Per-row min or max of x[a[i] .. b[i]] (inclusive; int64 or float64 x).

    Nulls must already be replaced by the identity (int64 max/min, ±inf);
    an empty frame (a > b) yields the identity. Floating NaN propagates,
    as with torch.minimum / torch.maximum. The native path builds a 64-ary
    min/max pyramid once, so the cost per row does not grow with the frame
    width."""
    _window_minmax_args(x, a, b, op)
    device = x.device
    if not _use_native(device):
        return window_frame_minmax_ref(x, a, b, op)
    lib = native.lib()
    n = x.numel()
    rows = a.numel()
    out = torch.empty(rows, dtype=x.dtype, device=device)
    if rows == 0:
        return out
    assert n > 0, "window_frame_minmax: frames over an empty array"
    x, a, b = x.contiguous(), a.contiguous(), b.contiguous()
    pyr_len = int(lib.au_window_pyramid_size(n))  # levels above x
    pyr = torch.empty(max(pyr_len, 1), dtype=x.dtype, device=device)
    fn = (lib.au_window_frame_minmax_i64 if x.dtype == torch.int64
          else lib.au_window_frame_minmax_f64)
    rc = fn(x.data_ptr(), n, pyr.data_ptr(), pyr_len, a.data_ptr(),
            b.data_ptr(), rows, int(op == "max"), out.data_ptr(),
            native.stream_ptr(device))
    native.check(rc, "au_window_frame_minmax")
    return out


# ------------------------------------------------- 128-bit frame aggregates
# A 128-bit value is two int64 limbs [lo bit pattern, hi signed], row-major
# [n,2] — the layout Column uses for DECIMAL128.
_I128_MAX = (-1, _MAX64)  # 2^127 - 1: identity of min
_I128_MIN = (0, _MIN64)   # -2^127:    identity of max


def _i128_args(x, valid=None):
    assert x.dtype == torch.int64 and x.dim() == 2 and x.shape[1] == 2, \
        f"expected int64 [n,2] limbs, got {x.dtype} {tuple(x.shape)}"
    assert x.shape[0] < (1 << 31), "batch too large for split accumulation"
    if valid is not None:
        assert valid.dtype == torch.bool and valid.numel() == x.shape[0]


def _i128_frame_args(a, b):
    assert a.dtype == torch.int64 and b.dtype == torch.int64
    assert a.numel() == b.numel()


def _i128_aligned(t: torch.Tensor) -> torch.Tensor:
    """Contiguous and 16-byte aligned, as the kernels' 16-byte loads need."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


def _ult(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Unsigned x < y over int64 bit patterns: flip the sign bit, then
    compare signed."""
    return (x ^ _MIN64) < (y ^ _MIN64)


def prefix_sum_i128_ref(x: torch.Tensor,
                        valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Oracle for prefix_sum_i128 (pure torch): four 32-bit digits (top one
    signed), each cumsum-ed in int64 and recomposed with carry propagation,
    as in the group-by decimal128 sum. Below 2^31 rows no digit sum can
    leave int64."""
    _i128_args(x, valid)
    lo, hi = x[:, 0], x[:, 1]
    if valid is not None:
        z = torch.zeros((), dtype=torch.int64, device=x.device)
        lo, hi = torch.where(valid, lo, z), torch.where(valid, hi, z)
    m = 0xFFFFFFFF
    s0, s1, s2, s3 = (torch.cumsum(d, 0) for d in
                      (lo & m, (lo >> 32) & m, hi & m, hi >> 32))
    t1 = s1 + (s0 >> 32)
    t2 = s2 + (t1 >> 32)
    t3 = s3 + (t2 >> 32)
    return torch.stack([((t1 & m) << 32) | (s0 & m),
                        (t3 << 32) | (t2 & m)], dim=1)


def prefix_sum_i128(x: torch.Tensor,
                    valid: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Inclusive prefix sum modulo 2^128 over int64 [n,2] limb pairs; a row
    whose `valid` is False adds zero. The scan is not segmented: a frame sum
    is a difference of two prefixes (window_frame_sum_i128), in which
    wrapped prefixes cancel."""
    _i128_args(x, valid)
    device = x.device
    if not _use_native(device):
        return prefix_sum_i128_ref(x, valid)
    lib = native.lib()
    n = x.shape[0]
    out = torch.empty((n, 2), dtype=torch.int64, device=device)
    if n == 0:
        return out
    x = _i128_aligned(x)
    vptr = None
    if valid is not None:
        valid = valid.contiguous()
        vptr = valid.data_ptr()
    tile = int(lib.au_i128_scan_tile())
    scratch = torch.empty(((n + tile - 1) // tile, 2), dtype=torch.int64,
                          device=device)
    rc = lib.au_prefix_sum_i128(x.data_ptr(), vptr, n, out.data_ptr(),
                                scratch.data_ptr(), native.stream_ptr(device))
    native.check(rc, "au_prefix_sum_i128")
    return out


def window_frame_sum_i128_ref(P: torch.Tensor, a: torch.Tensor,
                              b: torch.Tensor) -> torch.Tensor:
    """Oracle for window_frame_sum_i128 (pure torch): limb subtraction, the
    borrow from an unsigned compare of the low limbs."""
    _i128_args(P)
    _i128_frame_args(a, b)
    n = P.shape[0]
    rows = a.numel()
    lo = a.clamp(min=0)
    hi = b.clamp(max=n - 1)
    empty = lo > hi
    if n == 0 or rows == 0:
        return torch.zeros((rows, 2), dtype=torch.int64, device=P.device)
    top = P[hi.clamp(min=0)]
    below = torch.where((lo > 0).unsqueeze(1), P[(lo - 1).clamp(0, n - 1)],
                        torch.zeros((), dtype=torch.int64, device=P.device))
    d_lo = top[:, 0] - below[:, 0]
    borrow = _ult(top[:, 0], below[:, 0]).to(torch.int64)
    d_hi = top[:, 1] - below[:, 1] - borrow
    out = torch.stack([d_lo, d_hi], dim=1)
    return torch.where(empty.unsqueeze(1), torch.zeros_like(out), out)


def window_frame_sum_i128(P: torch.Tensor, a: torch.Tensor,
                          b: torch.Tensor) -> torch.Tensor:
    """Per-row sum over the inclusive frame [a[i], b[i]] from the inclusive
    128-bit prefix sum P (prefix_sum_i128): P[b] - (a > 0 ? P[a-1] : 0)
    modulo 2^128, zero for an empty frame (a > b). Exact whenever the frame
    sum itself fits in 128 bits. Frames are clamped to [0, n-1]."""
    _i128_args(P)
    _i128_frame_args(a, b)
    device = P.device
    if not _use_native(device):
        return window_frame_sum_i128_ref(P, a, b)
    lib = native.lib()
    rows = a.numel()
    out = torch.empty((rows, 2), dtype=torch.int64, device=device)
    if rows == 0:
        return out
    P, a, b = _i128_aligned(P), a.contiguous(), b.contiguous()
    rc = lib.au_window_frame_sum_i128(P.data_ptr(), P.shape[0], a.data_ptr(),
                                      b.data_ptr(), rows, out.data_ptr(),
                                      native.stream_ptr(device))
    native.check(rc, "au_window_frame_sum_i128")
    return out


def _i128_less(x: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """x < y over [m,2] limb pairs: signed hi first, then unsigned lo."""
    return (x[:, 1] < y[:, 1]) | ((x[:, 1] == y[:, 1])
                                  & _ult(x[:, 0], y[:, 0]))


def window_frame_minmax_i128_ref(x: torch.Tensor, a: torch.Tensor,
                                 b: torch.Tensor, op: str) -> torch.Tensor:
    """Oracle for window_frame_minmax_i128 (pure torch): the doubling sparse
    table of window_frame_minmax_ref with a 128-bit less-than."""
    assert op in ("min", "max"), op
    _i128_args(x)
    _i128_frame_args(a, b)
    n = x.shape[0]

    def combine(p, q):
        take_q = _i128_less(q, p) if op == "min" else _i128_less(p, q)
        return torch.where(take_q.unsqueeze(1), q, p)

    ident = torch.tensor(_I128_MAX if op == "min" else _I128_MIN,
                         dtype=torch.int64, device=x.device)
    out = ident.repeat(a.numel(), 1)
    lo = a.clamp(min=0)
    hi = b.clamp(max=n - 1)
    ln = hi - lo + 1
    if a.numel() == 0 or n == 0 or int(ln.max().item()) <= 0:
        return out
    level = x
    k = 0
    maxlen = int(ln.max().item())
    while True:
        w = 1 << k
        sel = (ln >= w) & (ln < 2 * w)
        if bool(sel.any()):
            out[sel] = combine(level[lo[sel]], level[hi[sel] - w + 1])
        if 2 * w > maxlen:
            break
        nxt = level.clone()
        nxt[:n - w] = combine(level[:n - w], level[w:])
        level = nxt
        k += 1
    return out


def window_frame_minmax_i128(x: torch.Tensor, a: torch.Tensor,
                             b: torch.Tensor, op: str) -> torch.Tensor:
    """window_frame_minmax over int64 [n,2] limb pairs (signed 128-bit
    order) -> [rows,2]. Nulls must already be replaced by the identity
    (2^127-1 for min, -2^127 for max); an empty frame yields it."""
    assert op in ("min", "max"), op
    _i128_args(x)
    _i128_frame_args(a, b)
    device = x.device
    if not _use_native(device):
        return window_frame_minmax_i128_ref(x, a, b, op)
    lib = native.lib()
    n = x.shape[0]
    rows = a.numel()
    out = torch.empty((rows, 2), dtype=torch.int64, device=device)
    if rows == 0:
        return out
    assert n > 0, "window_frame_minmax_i128: frames over an empty array"
    x, a, b = _i128_aligned(x), a.contiguous(), b.contiguous()
    pyr_len = int(lib.au_window_pyramid_size(n))  # levels above x
    pyr = torch.empty((max(pyr_len, 1), 2), dtype=torch.int64, device=device)
    rc = lib.au_window_frame_minmax_i128(
        x.data_ptr(), n, pyr.data_ptr(), pyr_len, a.data_ptr(), b.data_ptr(),
        rows, int(op == "max"), out.data_ptr(), native.stream_ptr(device))
    native.check(rc, "au_window_frame_minmax_i128")
    return out


# ------------------------------------------------ exact decimal128 arithmetic
# An operand is either int64 [n,2] limbs or an integer [n] tensor (decimal64
# or integer backing), read as a sign-extended 128-bit integer. Every op
# builds an exact wide intermediate, divides by a power of ten (or by b)
# rounding HALF_UP on the magnitude, and clears the row's validity when the
# result's magnitude reaches 10^p. The *_ref twins do the same in Python
# integers on the host: they are the CPU execution path and the oracle for
# the k_dec128_* kernels, and accept tensors on any device.
DEC128_MAX_POW10 = 38  # the kernels' powers of ten; more takes the reference
DEC128_CMP_OPS = {"==": 0, "!=": 1, "<": 2, "<=": 3, ">": 4, ">=": 5}
_DX_ABS, _DX_NEGATE, _DX_TRUNCATE, _DX_ASYM = 1, 2, 4, 8


def dec128_grid_threads() -> int:
    """Threads of the k_dec128_* kernels' largest grid; one more row wraps
    the grid-stride loop."""
    return int(native.lib().au_dec128_grid_threads())


def _dec128_native(device: torch.device, *powers: int) -> bool:
    if any(k > DEC128_MAX_POW10 for k in powers):
        return False
    if not _use_native(device):
        return False
    from .config import DECIMAL128_NATIVE_ARITH, AuronConf

    return bool(AuronConf().get(DECIMAL128_NATIVE_ARITH))


def _dec128_operand_args(x: torch.Tensor):
    if x.dim() == 2:
        _i128_args(x)
    else:
        assert x.dim() == 1 and x.dtype in (
            torch.int8, torch.int16, torch.int32, torch.int64), \
            f"expected int64 [n,2] limbs or integer [n], got {x.dtype} " \
            f"{tuple(x.shape)}"


def _dec128_pair_args(a, b, va, vb, *powers):
    _dec128_operand_args(a)
    _dec128_operand_args(b)
    assert a.shape[0] == b.shape[0], (tuple(a.shape), tuple(b.shape))
    for v in (va, vb):
        assert v is None or (v.dtype == torch.bool
                             and v.numel() == a.shape[0])
    assert all(k >= 0 for k in powers), powers


def _dec128_ints(x: torch.Tensor):
    """Rows as a numpy object array of Python ints."""
    import numpy as np

    h = x.detach().cpu().numpy()
    if h.ndim == 2:
        lo = h[:, 0].astype(np.uint64).astype(object)
        return h[:, 1].astype(object) * (1 << 64) + lo
    return h.astype(np.int64).astype(object)


def _dec128_valid(n, *vs):
    import numpy as np

    ok = np.ones(n, dtype=bool)
    for v in vs:
        if v is not None:
            ok &= v.detach().cpu().numpy()
    return ok


def _div_half_up(x: int, d: int, truncate: bool = False) -> int:
    q, r = divmod(abs(x), d)
    if not truncate and 2 * r >= d:
        q += 1
    return -q if x < 0 else q


def _dec128_pack(vals, ok, bound, device, narrow=False, asym=False):
    """(data, valid) tensors from Python ints: a row is kept when its input
    validity holds, its value is not None and |value| < bound (`asym` also
    keeps -bound); other rows store zero."""
    import numpy as np

    n = len(vals)
    lo = np.zeros(n, dtype=np.uint64)
    hi = np.zeros(n, dtype=np.int64)
    valid = np.zeros(n, dtype=bool)
    m64 = (1 << 64) - 1
    for i, v in enumerate(vals):
        if not ok[i] or v is None:
            continue
        if not (-bound < v < bound or (asym and v == -bound)):
            continue
        valid[i] = True
        lo[i] = v & m64
        hi[i] = v >> 64
    lo = lo.view(np.int64)
    data = lo if narrow else np.stack([lo, hi], axis=1)
    return (torch.from_numpy(np.ascontiguousarray(data)).to(device),
            torch.from_numpy(valid).to(device))


def _dec128_addsub_ref(a, b, ka, kb, d, p, va, vb, sub):
    _dec128_pair_args(a, b, va, vb, ka, kb, d)
    sign = -1 if sub else 1
    pa, pb, pd = 10 ** ka, 10 ** kb, 10 ** d
    vals = [_div_half_up(x * pa + sign * y * pb, pd)
            for x, y in zip(_dec128_ints(a), _dec128_ints(b))]
    return _dec128_pack(vals, _dec128_valid(a.shape[0], va, vb), 10 ** p,
                        a.device)


def dec128_add_ref(a, b, ka, kb, d, p, va=None, vb=None):
    """Oracle for dec128_add (Python integers on the host)."""
    return _dec128_addsub_ref(a, b, ka, kb, d, p, va, vb, False)


def dec128_sub_ref(a, b, ka, kb, d, p, va=None, vb=None):
    """Oracle for dec128_sub (Python integers on the host)."""
    return _dec128_addsub_ref(a, b, ka, kb, d, p, va, vb, True)


def dec128_mul_ref(a, b, d, p, va=None, vb=None):
    """Oracle for dec128_mul (Python integers on the host)."""
    _dec128_pair_args(a, b, va, vb, d)
    pd = 10 ** d
    vals = [_div_half_up(x * y, pd)
            for x, y in zip(_dec128_ints(a), _dec128_ints(b))]
    return _dec128_pack(vals, _dec128_valid(a.shape[0], va, vb), 10 ** p,
                        a.device)


def dec128_div_ref(a, b, k, p, va=None, vb=None):
    """Oracle for dec128_div (Python integers on the host)."""
    _dec128_pair_args(a, b, va, vb, k)
    pk = 10 ** k

    def one(x, y):
        if y == 0:
            return None
        q = _div_half_up(x * pk, abs(y))
        return -q if y < 0 else q

    vals = [one(x, y) for x, y in zip(_dec128_ints(a), _dec128_ints(b))]
    return _dec128_pack(vals, _dec128_valid(a.shape[0], va, vb), 10 ** p,
                        a.device)


def dec128_cmp_ref(a, b, ka, kb, op):
    """Oracle for dec128_cmp (Python integers on the host)."""
    import operator

    _dec128_pair_args(a, b, None, None, ka, kb)
    fn = {"==": operator.eq, "!=": operator.ne, "<": operator.lt,
          "<=": operator.le, ">": operator.gt, ">=": operator.ge}[op]
    pa, pb = 10 ** ka, 10 ** kb
    out = [fn(x * pa, y * pb)
           for x, y in zip(_dec128_ints(a), _dec128_ints(b))]
    return torch.tensor(out, dtype=torch.bool).to(a.device)


def _dec128_rescale_bound(p, bound, narrow_out):
    assert (p is None) != (bound is None), "give exactly one of p / bound"
    if bound is None:
        bound = 10 ** p
    assert 0 < bound < (1 << 127)
    assert not narrow_out or bound <= (1 << 63)
    return bound


def dec128_rescale_ref(x, k, p=None, vx=None, *, bound=None, abs_=False,
                       negate=False, truncate=False, asym=False,
                       narrow_out=False):
    """Oracle for dec128_rescale (Python integers on the host)."""
    _dec128_operand_args(x)
    bound = _dec128_rescale_bound(p, bound, narrow_out)
    pk = 10 ** abs(k)

    def one(v):
        if abs_:
            v = abs(v)
        if negate:
            v = -v
        return v * pk if k >= 0 else _div_half_up(v, pk, truncate)

    vals = [one(v) for v in _dec128_ints(x)]
    return _dec128_pack(vals, _dec128_valid(x.shape[0], vx), bound, x.device,
                        narrow=narrow_out, asym=asym)


def _dec128_operand(x: torch.Tensor):
    """(tensor, narrow flag) in the form the kernels load."""
    if x.dim() == 2:
        return _i128_aligned(x), 0
    return x.to(torch.int64).contiguous(), 1


def _dec128_vptr(v, keep):
    if v is None:
        return None
    v = v.contiguous()
    keep.append(v)
    return v.data_ptr()


def _dec128_binary(fn, what, a, b, va, vb, ints):
    lib = native.lib()
    device = a.device
    n = a.shape[0]
    out = torch.empty((n, 2), dtype=torch.int64, device=device)
    valid = torch.empty(n, dtype=torch.bool, device=device)
    if n == 0:
        return out, valid
    keep = []
    a, an = _dec128_operand(a)
    b, bn = _dec128_operand(b)
    rc = getattr(lib, fn)(a.data_ptr(), an, _dec128_vptr(va, keep),
                          b.data_ptr(), bn, _dec128_vptr(vb, keep), n, *ints,
                          out.data_ptr(), valid.data_ptr(),
                          native.stream_ptr(device))
    native.check(rc, what)
    return out, valid


def dec128_add(a, b, ka, kb, d, p, va=None, vb=None):
    """(a*10^ka + b*10^kb) / 10^d rounded HALF_UP -> ([n,2] limbs, valid).
    valid = va & vb & (|result| < 10^p); a row that is not valid stores
    zero. One kernel launch, no host sync."""
    _dec128_pair_args(a, b, va, vb, ka, kb, d)
    if not _dec128_native(a.device, ka, kb, d, p):
        return dec128_add_ref(a, b, ka, kb, d, p, va, vb)
    return _dec128_binary("au_dec128_addsub", "au_dec128_addsub", a, b, va,
                          vb, (ka, kb, d, p, 0))


def dec128_sub(a, b, ka, kb, d, p, va=None, vb=None):
    """(a*10^ka - b*10^kb) / 10^d, otherwise as dec128_add."""
    _dec128_pair_args(a, b, va, vb, ka, kb, d)
    if not _dec128_native(a.device, ka, kb, d, p):
        return dec128_sub_ref(a, b, ka, kb, d, p, va, vb)
    return _dec128_binary("au_dec128_addsub", "au_dec128_addsub", a, b, va,
                          vb, (ka, kb, d, p, 1))


def dec128_mul(a, b, d, p, va=None, vb=None):
    """(a*b) / 10^d rounded HALF_UP over the exact 256-bit product,
    otherwise as dec128_add."""
    _dec128_pair_args(a, b, va, vb, d)
    if not _dec128_native(a.device, d, p):
        return dec128_mul_ref(a, b, d, p, va, vb)
    return _dec128_binary("au_dec128_mul", "au_dec128_mul", a, b, va, vb,
                          (d, p))


def dec128_div(a, b, k, p, va=None, vb=None):
    """round_half_up(a*10^k / b); a zero divisor clears the row's validity.
    Otherwise as dec128_add."""
    _dec128_pair_args(a, b, va, vb, k)
    if not _dec128_native(a.device, k, p):
        return dec128_div_ref(a, b, k, p, va, vb)
    return _dec128_binary("au_dec128_div", "au_dec128_div", a, b, va, vb,
                          (k, p))


def dec128_cmp(a, b, ka, kb, op):
    """a*10^ka <op> b*10^kb -> bool [n], both sides aligned in 256 bits so
    a 38-digit value times 10^k cannot wrap."""
    _dec128_pair_args(a, b, None, None, ka, kb)
    assert op in DEC128_CMP_OPS, op
    device = a.device
    if not _dec128_native(device, ka, kb):
        return dec128_cmp_ref(a, b, ka, kb, op)
    n = a.shape[0]
    out = torch.empty(n, dtype=torch.bool, device=device)
    if n == 0:
        return out
    a, an = _dec128_operand(a)
    b, bn = _dec128_operand(b)
    rc = native.lib().au_dec128_cmp(a.data_ptr(), an, b.data_ptr(), bn, n, ka,
                                    kb, DEC128_CMP_OPS[op], out.data_ptr(),
                                    native.stream_ptr(device))
    native.check(rc, "au_dec128_cmp")
    return out


def dec128_rescale(x, k, p=None, vx=None, *, bound=None, abs_=False,
                   negate=False, truncate=False, asym=False,
                   narrow_out=False):
    """x*10^k for k >= 0, x/10^-k for k < 0 (HALF_UP, or toward zero with
    `truncate`), after `abs_` / `negate` -> (data, valid). valid = vx &
    (|result| < bound), bound = 10^p unless given; `asym` also keeps -bound
    (two's-complement integer ranges). data is [n,2] limbs, or int64 [n]
    with `narrow_out` (bound <= 2^63). Serves casts, CheckOverflow, abs."""
    _dec128_operand_args(x)
    assert vx is None or (vx.dtype == torch.bool
                          and vx.numel() == x.shape[0])
    bound = _dec128_rescale_bound(p, bound, narrow_out)
    device = x.device
    if not _dec128_native(device, abs(k)):
        return dec128_rescale_ref(x, k, None, vx, bound=bound, abs_=abs_,
                                  negate=negate, truncate=truncate,
                                  asym=asym, narrow_out=narrow_out)
    n = x.shape[0]
    out = torch.empty(n if narrow_out else (n, 2), dtype=torch.int64,
                      device=device)
    valid = torch.empty(n, dtype=torch.bool, device=device)
    if n == 0:
        return out, valid
    keep = []
    x, xn = _dec128_operand(x)
    flags = (_DX_ABS * abs_ | _DX_NEGATE * negate | _DX_TRUNCATE * truncate
             | _DX_ASYM * asym)
    rc = native.lib().au_dec128_rescale(
        x.data_ptr(), xn, _dec128_vptr(vx, keep), n, k, flags,
        bound & ((1 << 64) - 1), bound >> 64, out.data_ptr(),
        int(narrow_out), valid.data_ptr(), native.stream_ptr(device))
    native.check(rc, "au_dec128_rescale")
    return out, valid


# ================================================================ partition
def _normalize_hash_col(c: Column) -> Column:
    """Promote key columns to a canonical width before hashing: murmur3
    hashes int32 and int64 differently, so `week_seq` (int32) vs
    `week_seq - 52` (promoted int64) would land on different ranks. Our
    internal exchange only needs consistency, not Spark shuffle-file
    layout, so ints hash as int64 and floats as float64."""
    if c.dtype.code in (dtypes.BOOL, dtypes.INT8, dtypes.INT16, dtypes.INT32,
                        dtypes.DATE32):
        return Column(dtypes.int64, c.data.to(torch.int64), c.validity)
    if c.dtype.code == dtypes.FLOAT32:
        return Column(dtypes.float64, c.data.to(torch.float64), c.validity)
    return c


def partition_ids(cols: List[Column], nparts: int) -> torch.Tensor:
    """Internal hash partitioning: pmod(murmur3(normalized keys, 42), n)."""
    cols = [_normalize_hash_col(c) for c in cols]
    device = cols[0].device
    h = murmur3(cols)
    if not _use_native(device):
        return torch.remainder(h.to(torch.int64), nparts).to(torch.int32)
    lib = native.lib()
    n = h.numel()
    out = torch.empty(n, dtype=torch.int32, device=device)
    rc = lib.au_pmod(h.data_ptr(), n, nparts, out.data_ptr(), native.stream_ptr(device))
    native.check(rc, "au_pmod")
    return out


def partition_order(part_ids: torch.Tensor, nparts: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """-> (row order grouping rows by partition [n] int64, counts [nparts] int64)."""
    device = part_ids.device
    n = part_ids.numel()
    if not _use_native(device):
        counts = torch.bincount(part_ids.to(torch.int64), minlength=nparts)
        order = torch.argsort(part_ids.to(torch.int64), stable=True)
        return order, counts
    lib = native.lib()
    sp = native.stream_ptr(device)
    counts = torch.zeros(nparts, dtype=torch.int32, device=device)
    rc = lib.au_part_hist(part_ids.data_ptr(), n, nparts, counts.data_ptr(), sp)
    native.check(rc, "au_part_hist")
    counts64 = counts.to(torch.int64)
    base = torch.zeros(nparts, dtype=torch.int64, device=device)
    if nparts > 1:
        torch.cumsum(counts64[:-1], 0, out=base[1:])
    cursors = torch.zeros(nparts, dtype=torch.int32, device=device)
    order = torch.empty(n, dtype=torch.int64, device=device)
    rc = lib.au_part_scatter(part_ids.data_ptr(), n, base.data_ptr(),
                             cursors.data_ptr(), order.data_ptr(), sp)
    native.check(rc, "au_part_scatter")
    return order, counts64


# ============================================================== aggregation
_I64_MAX = torch.iinfo(torch.int64).max
_I64_MIN = torch.iinfo(torch.int64).min


def _f64_order_keys(v: torch.Tensor) -> torch.Tensor:
    """float64 -> int64 keys whose integer order is the aggregate MIN/MAX
    order of the floats: -inf < ... < -0.0 < 0.0 < ... < +inf < NaN, every
    NaN being the one canonical NaN (f64_order_key in csrc/agg.hip). Both
    int64 identities lie outside the keys of all floats, so a group of
    NaNs alone still leaves the identity."""
    bits = torch.where(torch.isnan(v), torch.full_like(v, float("nan")), v)
    bits = bits.contiguous().view(torch.int64)
    return torch.where(bits < 0, bits ^ _I64_MAX, bits)


def _f64_from_order_keys(k: torch.Tensor) -> torch.Tensor:
    """Inverse of _f64_order_keys. An identity (a group with no valid row)
    decodes to some NaN: such accumulators are unspecified."""
    return torch.where(k < 0, k ^ _I64_MAX, k).view(torch.float64)


def _agg_init(op: int, acc_f64: bool):
    """(accumulator dtype, identity): sums accumulate in f64 / i64; MIN and
    MAX in int64 for every input, floats as their order keys."""
    if op == 0:
        return (torch.float64, 0.0) if acc_f64 else (torch.int64, 0)
    return torch.int64, (_I64_MAX if op == 1 else _I64_MIN)


def _agg_minmax_out(acc: torch.Tensor, values: Column) -> torch.Tensor:
    """MIN/MAX accumulator -> the input dtype (state keeps the input dtype,
    reference acc.rs semantics), on every path."""
    tgt = values.data.dtype
    if tgt.is_floating_point:
        acc = _f64_from_order_keys(acc)
    return acc if acc.dtype == tgt else acc.to(tgt)


def _agg_scatter_native(gids: torch.Tensor, num_groups: int, values: Column, fn: str):
    """HIP atomic scatter-accumulate (csrc/agg.hip). torch's fp64
    scatter_add_ measured ~400x slower on gfx950 (rocprof, q23)."""
    lib = native.lib()
    device = gids.device
    sp = native.stream_ptr(device)
    n = gids.numel()
    g = gids.contiguous()
    counts = torch.zeros(num_groups, dtype=torch.int64, device=device)
    vptr = values.validity.contiguous().data_ptr() if values.validity is not None else None
    keep = [g, counts, values.validity, values.data]
    if fn == "count":
        rc = lib.au_agg_count(g.data_ptr(), n, vptr, counts.data_ptr(), sp)
        native.check(rc, "au_agg_count")
        return counts, counts
    v = values.data
    if v.dtype in (torch.int8, torch.int16, torch.bool):
        v = v.to(torch.int32)
    v = v.contiguous()
    keep.append(v)
    vtype = {torch.float64: 0, torch.int64: 1, torch.int32: 2, torch.float32: 3}[v.dtype]
    acc_f64 = v.dtype in (torch.float32, torch.float64)
    op = {"sum": 0, "avg": 0, "min": 1, "max": 2}[fn]
    acc_dtype, init = _agg_init(op, acc_f64)
    acc = torch.full((num_groups,), init, dtype=acc_dtype, device=device)
    rc = lib.au_agg_scatter(g.data_ptr(), n, vptr, v.data_ptr(), vtype, op,
                            1 if acc_f64 else 0, acc.data_ptr(), counts.data_ptr(),
                            num_groups, sp)
    native.check(rc, "au_agg_scatter")
    del keep
    if fn in ("min", "max"):
        acc = _agg_minmax_out(acc, values)
    # sums: the f64 / i64 accumulator is the widened sum dtype
    return acc, counts


def agg_scatter_multi(gids: torch.Tensor, num_groups: int, items):
    """Fused accumulate of several (values Column, fn) pairs in ONE kernel
    pass over the rows (gids read once, wave head-flags computed once).
    fn in sum/avg/min/max. -> [(acc, counts), ...] like agg_scatter."""
    device = gids.device
    if not items:
        return []
    if num_groups == 0 or not _use_native(device) or len(items) == 1:
        return [agg_scatter(gids, num_groups, c, f) for c, f in items]
    import numpy as np

    lib = native.lib()
    sp = native.stream_ptr(device)
    g = gids.contiguous()
    n = g.numel()
    descs = np.zeros((len(items), 6), dtype=np.int64)
    outs = []
    keep = [g]
    for j, (values, fn) in enumerate(items):
        v = values.data
        if v.dtype in (torch.int8, torch.int16, torch.bool):
            v = v.to(torch.int32)
        v = v.contiguous()
        keep.append(v)
        vtype = {torch.float64: 0, torch.int64: 1, torch.int32: 2,
                 torch.float32: 3}[v.dtype]
        acc_f64 = v.dtype in (torch.float32, torch.float64)
        op = {"sum": 0, "avg": 0, "min": 1, "max": 2}[fn]
        acc_dtype, init = _agg_init(op, acc_f64)
        acc = torch.full((num_groups,), init, dtype=acc_dtype, device=device)
        counts = torch.zeros(num_groups, dtype=torch.int64, device=device)
        vptr = 0
        if values.validity is not None:
            val = values.validity.contiguous()
            keep.append(val)
            vptr = val.data_ptr()
        descs[j] = (v.data_ptr(), vptr, vtype, op, acc.data_ptr(),
                    counts.data_ptr())
        outs.append((values, fn, acc, counts))
    from .pinned import to_device

    darr = to_device(descs.reshape(-1), device)
    keep.append(darr)
    rc = lib.au_agg_multi(g.data_ptr(), n, darr.data_ptr(), len(items), sp)
    native.check(rc, "au_agg_multi")
    del keep
    res = []
    for values, fn, acc, counts in outs:
        if fn in ("min", "max"):
            acc = _agg_minmax_out(acc, values)
        res.append((acc, counts))
    return res


def agg_count_star(gids: torch.Tensor, num_groups: int) -> torch.Tensor:
    """Per-group row counts (no values column): native wave-segmented
    count kernel on GPU, torch scatter_add_ on CPU."""
    device = gids.device
    if num_groups > 0 and _use_native(device):
        lib = native.lib()
        sp = native.stream_ptr(device)
        g = gids.contiguous()
        counts = torch.zeros(num_groups, dtype=torch.int64, device=device)
        rc = lib.au_agg_count(g.data_ptr(), g.numel(), None,
                              counts.data_ptr(), sp)
        native.check(rc, "au_agg_count")
        return counts
    cnt = torch.zeros(num_groups, dtype=torch.int64, device=device)
    if gids.numel():
        cnt.scatter_add_(0, gids, torch.ones_like(gids, dtype=torch.int64))
    return cnt


def agg_scatter(gids: torch.Tensor, num_groups: int, values: Column, fn: str):
    """Scatter-accumulate values into per-group accumulators.

    -> (acc tensor [G], count-of-valid [G] int64). Nulls are excluded.
    GPU: hand-written atomic scatter kernels; CPU: torch scatter_reduce.

    The same on both paths: SUM is int64 (wrapping) over integers and
    bools, plain IEEE float64 over floats (NaN and +-inf propagate).
    MIN/MAX return the input dtype, bool included; over floats NaN is the
    greatest value (Spark): MAX is NaN if any valid input is, MIN only if
    all are, and -0.0 equals 0.0. Window frame min/max differ: there NaN
    propagates into both (window_frame_minmax). The accumulator of a group
    with count 0 is unspecified.
    """
    device = gids.device
    if num_groups > 0 and _use_native(device):
        return _agg_scatter_native(gids, num_groups, values, fn)
    v = values.data
    valid = values.validity
    g = gids
    if valid is not None:
        keep = valid
        g = gids[keep]
        v = v[keep]
    cnt = torch.zeros(num_groups, dtype=torch.int64, device=device)
    cnt.scatter_add_(0, g, torch.ones_like(g, dtype=torch.int64))
    if fn == "count":
        return cnt, cnt
    if fn in ("sum", "avg"):
        if v.dtype in (torch.float32,):
            v = v.to(torch.float64)
        if v.dtype in (torch.int8, torch.int16, torch.int32, torch.bool):
            v = v.to(torch.int64)
        acc = torch.zeros(num_groups, dtype=v.dtype, device=device)
        acc.scatter_add_(0, g, v)
        return acc, cnt
    if fn in ("min", "max"):
        # the native path's rule: int64 accumulators, floats as order keys
        # (NaN above +inf, MIN is NaN only for a group of NaNs), identities
        # outside every value, result in the input dtype
        red = "amin" if fn == "min" else "amax"
        k = _f64_order_keys(v.to(torch.float64)) if v.dtype.is_floating_point \
            else v.to(torch.int64)
        acc = torch.full((num_groups,), _I64_MAX if fn == "min" else _I64_MIN,
                         dtype=torch.int64, device=device)
        acc.scatter_reduce_(0, g, k, reduce=red, include_self=True)
        return _agg_minmax_out(acc, values), cnt
    raise ValueError(fn)
