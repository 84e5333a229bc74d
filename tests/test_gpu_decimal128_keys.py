"""decimal128 key columns through the gfx950 kernels: k_murmur3,
k_group_insert, the legacy and fused join probes, k_join_exists and hash
partitioning, each against the CPU reference (murmur3_ref, group_ids_ref,
hash_join_ref), which covers every case here.

The join checks follow test_gpu_join_probe.py: fused, legacy and reference
on the same columns; probing one prebuilt table, fused and legacy agree
exactly and both equal the reference as sorted pair lists."""
import numpy as np
import pytest
import torch

from auron_amd import AggFunc, AuronSession, col, dtypes, ops
from auron_amd.column import Column
from auron_amd.exprs import Aliased
from auron_amd.plan import nodes as P

from test_decimal128_keys import (D38, _arrow_rows, _fact_batch, _fact_rows,
                                  d128_column, key_values)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 1024  # JP_TILE


def key_of(i):
    """Injective id -> unscaled value. Ids 2b and 2b+1 are +v and -v; b, b+1,
    b+2 (b % 3 == 0) share the low limb and differ in the high one; b and
    b+3 share the high limb and differ in the low one."""
    b = i // 2
    assert b // 3 < 127
    v = ((b % 3) << 64) + (b // 3 + 1) * ((1 << 57) + 1)
    return -v if i % 2 else v


def keyed_column(ids, nulls=None):
    vals = [key_of(int(i)) for i in ids]
    if nulls is not None:
        vals = [None if m else v for v, m in zip(vals, nulls)]
    return d128_column(vals)


def test_key_pool_has_the_close_pairs():
    lo = lambda v: v & ((1 << 64) - 1)
    assert lo(key_of(0)) == lo(key_of(2)) and key_of(0) >> 64 != key_of(2) >> 64
    assert key_of(0) >> 64 == key_of(6) >> 64 and lo(key_of(0)) != lo(key_of(6))
    assert key_of(0) == -key_of(1)
    assert len({key_of(i) for i in range(760)}) == 760


# ------------------------------------------------------------------ murmur3
_VALUES = key_values()


def _cycled(n, nulls):
    vals = [_VALUES[i % len(_VALUES)] for i in range(n)]
    if nulls:
        vals = [None if i % 4 == 2 else v for i, v in enumerate(vals)]
    return vals


@pytest.mark.parametrize("nulls", [False, True])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1025])
def test_murmur3_gpu_matches_reference(n, nulls):
    d = d128_column(_cycled(n, nulls))
    assert (d.validity is not None) == (nulls and n > 2)
    ints = Column(dtypes.int64, torch.arange(n, dtype=torch.int64) * 7919 - 5)
    strs = Column.from_pylist(
        [None if i % 5 == 0 else "s" * (i % 7) for i in range(n)], dtypes.string)
    for cols in ([d], [ints, d], [d, strs], [strs, d, ints]):
        want = ops.murmur3_ref(cols)
        got = ops.murmur3([c.to(DEV) for c in cols])
        assert got.dtype == torch.int32
        assert torch.equal(got.cpu(), want)
    assert torch.equal(ops.murmur3([d.to(DEV)], seed=7).cpu(),
                       ops.murmur3_ref([d], seed=7))


def test_murmur3_gpu_every_value_and_small_precision():
    d = d128_column(_VALUES)
    assert torch.equal(ops.murmur3([d.to(DEV)]).cpu(), ops.murmur3_ref([d]))
    small = [v for v in _VALUES if abs(v) < 10 ** 18] + [None]
    s = d128_column(small, dtypes.decimal128(18, 2))
    want = ops.murmur3_ref(
        [Column(dtypes.int64, s.data[:, 0].contiguous(), s.validity)])
    assert torch.equal(ops.murmur3([s.to(DEV)]).cpu(), want)


def test_murmur3_gpu_unaligned_and_strided_limbs():
    """A row slice starting 8 bytes off, and a strided view, must be made
    contiguous and 16-byte aligned before the kernel's 16-byte loads."""
    d = d128_column(_VALUES).to(DEV)
    flat = torch.zeros(2 * len(d) + 1, dtype=torch.int64, device=DEV)
    flat[1:] = d.data.reshape(-1)
    off = Column(D38, flat[1:].view(-1, 2))
    assert off.data.data_ptr() % 16 == 8
    wide = torch.zeros(len(d), 4, dtype=torch.int64, device=DEV)
    wide[:, :2] = d.data
    strided = Column(D38, wide[:, :2])
    want = ops.murmur3_ref([d.to("cpu")])
    assert torch.equal(ops.murmur3([off]).cpu(), want)
    assert torch.equal(ops.murmur3([strided]).cpu(), want)
    gids, reps = ops.group_ids([off])
    assert reps.numel() == len(set(_VALUES))


# ---------------------------------------------------------------- group ids
def _check_groups(cols):
    ref_gid, ref_reps = ops.group_ids_ref(cols)
    gids, reps = ops.group_ids([c.to(DEV) for c in cols])
    assert gids.dtype == reps.dtype == torch.int64
    gids, reps = gids.cpu(), reps.cpu()
    assert reps.numel() == ref_reps.numel()
    assert torch.equal(ref_gid[reps][gids], ref_gid)
    return reps.numel()


@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 5000])
def test_group_ids_gpu(n):
    rng = np.random.default_rng(n)
    ids = rng.integers(0, 400, n)
    nulls = rng.random(n) < 0.1
    ng = _check_groups([keyed_column(ids, nulls)])
    if n == 5000:
        assert ng == 401  # every key of the pool, and the NULL group
    ng = _check_groups([keyed_column(ids)])  # no validity buffer
    assert ng == len(set(ids.tolist()))
    # two key columns: the same decimal128 value under different int64 keys
    other = Column(dtypes.int64, torch.tensor(rng.integers(0, 3, n)))
    _check_groups([keyed_column(ids, nulls), other])
    _check_groups([other, keyed_column(ids)])


# -------------------------------------------------------------------- joins
def _build_ids(kind):
    rng = np.random.default_rng(11)
    if kind == "empty":
        return np.zeros(0, dtype=np.int64), 4
    if kind == "unique":  # only the cnt <= 1 path
        return rng.permutation(300).astype(np.int64), 300
    if kind == "dup40":  # 40 rows share id 7: the cnt > 1 re-walk
        ids = np.concatenate([np.full(40, 7), np.delete(np.arange(261), 7)])
        return rng.permutation(ids).astype(np.int64), 261
    raise AssertionError(kind)


def _case(build_kind, n_probe, seed=0, nulls=True):
    rng = np.random.default_rng(seed)
    bids, distinct = _build_ids(build_kind)
    pids = rng.integers(0, distinct + distinct // 4 + 1, n_probe)
    bn = rng.random(len(bids)) < 0.1 if nulls else None
    pn = rng.random(n_probe) < 0.1 if nulls else None
    return [keyed_column(bids, bn)], [keyed_column(pids, pn)]


def _check_join(monkeypatch, build, probe, emit, need_bm):
    ref_bi, ref_pi, ref_bm = ops.hash_join_ref(build, probe, emit, need_bm)
    bg = [c.to(DEV) for c in build]
    pg = [c.to(DEV) for c in probe]
    table = ops.join_build(bg)
    monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", "1")
    f_bi, f_pi, f_bm = ops.hash_join(bg, pg, emit, need_bm, table=table)
    monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", "0")
    l_bi, l_pi, l_bm = ops.hash_join(bg, pg, emit, need_bm, table=table)
    assert f_bi.dtype == l_bi.dtype == f_pi.dtype == l_pi.dtype == torch.int64
    assert torch.equal(f_pi, l_pi) and torch.equal(f_bi, l_bi)
    ref_pairs = sorted(zip(ref_bi.tolist(), ref_pi.tolist()))
    assert sorted(zip(f_bi.cpu().tolist(), f_pi.cpu().tolist())) == ref_pairs
    assert sorted(zip(l_bi.cpu().tolist(), l_pi.cpu().tolist())) == ref_pairs
    if need_bm:
        assert torch.equal(f_bm, l_bm) and torch.equal(f_bm.cpu(), ref_bm)
    else:
        assert f_bm is None and l_bm is None
    return len(ref_pairs)


@pytest.mark.parametrize("build_kind", ["unique", "dup40", "empty"])
@pytest.mark.parametrize("n_probe", [0, 1, 256, 257, TILE - 1, TILE, TILE + 1])
def test_hash_join_gpu(monkeypatch, n_probe, build_kind):
    build, probe = _case(build_kind, n_probe, seed=n_probe)
    for emit, need_bm in ((False, False), (False, True), (True, False),
                          (True, True)):
        _check_join(monkeypatch, build, probe, emit, need_bm)


def test_hash_join_gpu_without_validity_and_two_keys(monkeypatch):
    build, probe = _case("dup40", TILE + 1, seed=3, nulls=False)
    assert build[0].validity is None and probe[0].validity is None
    _check_join(monkeypatch, build, probe, True, True)
    # a second key column splits the 40 duplicates
    b2 = Column(dtypes.int64, torch.arange(len(build[0])) % 2)
    p2 = Column(dtypes.int64, torch.arange(len(probe[0])) % 2)
    _check_join(monkeypatch, build + [b2], probe + [p2], True, True)
    _check_join(monkeypatch, [b2] + build, [p2] + probe, False, False)


def test_small_precision_key_joins_a_wide_one(monkeypatch):
    """Same scale, precision 18 against 38: both sides of a join table are
    hashed by one rule."""
    vals = [5, -5, 10 ** 17, 0, None, 7]
    build = [d128_column(vals, dtypes.decimal128(18, 2))]
    probe = [d128_column(vals[::-1] + [8], dtypes.decimal128(38, 2))]
    assert _check_join(monkeypatch, build, probe, False, True) == 5
    assert _check_join(monkeypatch, probe, build, True, False) == 6


@pytest.mark.parametrize("build_kind", ["unique", "dup40", "empty"])
def test_join_exists_and_counts_gpu(monkeypatch, build_kind):
    for n_probe in (0, 1, 256, 257, TILE - 1, TILE, TILE + 1):
        build, probe = _case(build_kind, n_probe, seed=100 + n_probe)
        want = ops.join_counts(build, probe)  # CPU reference path
        bg = [c.to(DEV) for c in build]
        pg = [c.to(DEV) for c in probe]
        got = ops.join_counts(bg, pg)
        assert got.dtype == torch.int32
        assert torch.equal(got.cpu(), want)
        for with_table in (False, True):
            table = ops.join_build(bg) if with_table else None
            for switch in ("1", "0"):
                monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", switch)
                ex = ops.join_exists(bg, pg, table=table)
                assert ex.dtype == torch.bool
                assert torch.equal(ex.cpu(), want > 0), (n_probe, switch)


# ---------------------------------------------------------------- partition
@pytest.mark.parametrize("nparts", [1, 7, 64])
def test_partition_ids_gpu(nparts):
    d = d128_column(_cycled(1025, True))
    ints = Column(dtypes.int32, torch.arange(1025, dtype=torch.int32))
    for cols in ([d], [ints, d]):
        want = ops.partition_ids(cols, nparts)
        got = ops.partition_ids([c.to(DEV) for c in cols], nparts)
        assert torch.equal(got.cpu(), want)


# ------------------------------------------------------------------ session
def test_session_group_then_join_back():
    rows = _fact_rows(2000)

    def run(device):
        fact = _fact_batch(rows, device)
        agg = P.HashAgg(P.MemoryScan([fact]), [Aliased(col("k"), "gk")],
                        [AggFunc("sum", col("v"), name="sv"),
                         AggFunc("count_star", None, name="n")], mode="complete")
        plan = P.HashJoin(P.MemoryScan([fact]), agg, [col("k")], [col("gk")],
                          how="inner")
        out = AuronSession(device=device).collect(plan)
        return sorted(_arrow_rows(out, ["id", "k", "gk", "sv", "n"]))

    got, want = run(DEV), run("cpu")
    assert len(want) == sum(1 for r in rows if r[0] is not None)
    assert all(r[1] == r[2] for r in want)
    assert got == want
