"""Fused hash-join probe (k_join_probe_count / k_join_probe_fill /
k_join_exists) against its legacy twin and the CPU reference.

Every hash_join case runs three ways on the same columns: fused
(spark.auron.join.fusedProbe.enable on), legacy (off) and hash_join_ref on
CPU. Probing one prebuilt table, fused and legacy must be torch.equal on
build_idx, probe_idx and build_matched — same pairs in the same order — and
both must equal the reference as sorted pair lists. Without a prebuilt table
each call builds its own, whose chain order is the arrival order of that
build's atomics (two legacy calls differ the same way), so there build_idx
is compared per probe row as a set; everything else stays exact. Shapes sit on the tile edges of the fused
kernels (TILE probe rows per tile, 256 per slab)."""
import numpy as np
import pytest
import torch

from auron_amd import AuronSession, col, dtypes, ops
from auron_amd.column import Column, RecordBatch
from auron_amd.plan import nodes as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
TILE = 1024  # JP_TILE; test_tile_constant pins it to the library's value

N_PROBES = [0, 1, 255, 256, 257, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]
KEY_KINDS = ["int64", "int32", "date32", "decimal64", "string", "int64+string",
             "float64", "int64x9"]


def _build_ids(kind):
    """Key ids of a build side and the number of distinct ids in it."""
    rng = np.random.default_rng(11)
    if kind == "empty":
        return np.zeros(0, dtype=np.int64), 4
    if kind == "one":
        return np.array([3], dtype=np.int64), 4
    if kind == "unique":  # only the cnt <= 1 path
        return rng.permutation(300).astype(np.int64), 300
    if kind == "dup40":  # 40 rows share id 7: the cnt > 1 re-walk, early stop
        ids = np.concatenate([np.full(40, 7), np.delete(np.arange(261), 7)])
        return rng.permutation(ids).astype(np.int64), 261
    if kind == "many":  # 5000 rows over 700 keys, table cap 16384
        return rng.integers(0, 700, 5000).astype(np.int64), 700
    raise AssertionError(kind)


def _key_cols(kind, ids, nulls, side):
    """Columns holding key `ids` (injective per kind); `nulls` marks NULL
    rows (None = the column carries no validity at all)."""
    ids = [int(v) for v in ids]
    mask = [False] * len(ids) if nulls is None else [bool(b) for b in nulls]

    def colof(vals, dt):
        return Column.from_pylist([None if m else v for v, m in zip(vals, mask)], dt)

    if kind == "int64":
        return [colof([v * 7919 - 1000 for v in ids], dtypes.int64)]
    if kind == "int32":
        return [colof([v * 31 - 50 for v in ids], dtypes.int32)]
    if kind == "date32":
        return [colof([19000 + v for v in ids], dtypes.date32)]
    if kind == "decimal64":
        return [colof([v * 0.25 for v in ids], dtypes.decimal64(18, 2))]
    if kind == "string":  # id 0 is the empty string
        return [colof(["" if v == 0 else f"key-{v}" * (1 + v % 3) for v in ids],
                      dtypes.string)]
    if kind == "int64+string":
        return [colof([v // 4 for v in ids], dtypes.int64),
                colof(["" if v % 4 == 0 else "s" * (v % 4) for v in ids], dtypes.string)]
    if kind == "float64":  # id 0: -0.0 on the build side, 0.0 on the probe side
        zero = -0.0 if side == "build" else 0.0
        return [colof([zero if v == 0 else v * 0.5 for v in ids], dtypes.float64)]
    if kind == "int64x9":
        return [colof([v + c for v in ids], dtypes.int64) for c in range(9)]
    raise AssertionError(kind)


def _case(kind, build_kind, n_probe, probe_nulls="10%", build_nulls="10%", seed=0):
    rng = np.random.default_rng(seed)
    bids, distinct = _build_ids(build_kind)
    pids = rng.integers(0, distinct + distinct // 4 + 1, n_probe)
    frac = {"10%": 0.1, "all": 1.1, "none": None}

    def nulls(n, how):
        return None if frac[how] is None else rng.random(n) < frac[how]

    build = _key_cols(kind, bids, nulls(len(bids), build_nulls), "build")
    probe = _key_cols(kind, pids, nulls(n_probe, probe_nulls), "probe")
    return build, probe


def _spy(monkeypatch):
    calls = {"fused": 0, "legacy": 0}
    fused, legacy = ops._hash_join_fused, ops._hash_join_legacy

    def f(*a, **k):
        calls["fused"] += 1
        return fused(*a, **k)

    def l(*a, **k):
        calls["legacy"] += 1
        return legacy(*a, **k)

    monkeypatch.setattr(ops, "_hash_join_fused", f)
    monkeypatch.setattr(ops, "_hash_join_legacy", l)
    return calls


def _check(monkeypatch, build, probe, emit, need_bm, with_table=True,
           expect_fused=True):
    ref_bi, ref_pi, ref_bm = ops.hash_join_ref(build, probe, emit, need_bm)
    bg = [c.to(DEV) for c in build]
    pg = [c.to(DEV) for c in probe]
    table = ops.join_build(bg) if with_table else None
    calls = _spy(monkeypatch)
    monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", "1")
    f_bi, f_pi, f_bm = ops.hash_join(bg, pg, emit, need_bm, table=table)
    assert calls == ({"fused": 1, "legacy": 0} if expect_fused
                     else {"fused": 0, "legacy": 1})
    monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", "0")
    l_bi, l_pi, l_bm = ops.hash_join(bg, pg, emit, need_bm, table=table)
    assert calls["legacy"] == (1 if expect_fused else 2)
    assert f_bi.dtype == l_bi.dtype == torch.int64
    assert f_pi.dtype == l_pi.dtype == torch.int64
    assert torch.equal(f_pi, l_pi)
    if with_table:
        assert torch.equal(f_bi, l_bi)
    else:
        # each call built its own table, and k_join_build links a chain in
        # atomic arrival order: the order inside one probe row's matches is
        # that build's, so compare per probe row as sets (same multiset of
        # pairs, same probe_idx)
        key = lambda bi, pi: torch.sort(pi * (1 << 32) + (bi + 1)).values
        assert torch.equal(key(f_bi, f_pi), key(l_bi, l_pi))
    ref_pairs = sorted(zip(ref_bi.tolist(), ref_pi.tolist()))
    assert sorted(zip(f_bi.cpu().tolist(), f_pi.cpu().tolist())) == ref_pairs
    assert sorted(zip(l_bi.cpu().tolist(), l_pi.cpu().tolist())) == ref_pairs
    if need_bm:
        assert f_bm.dtype == l_bm.dtype == torch.bool
        assert torch.equal(f_bm, l_bm)
        assert torch.equal(f_bm.cpu(), ref_bm)
    else:
        assert f_bm is None and l_bm is None


def test_tile_constant():
    assert ops.join_probe_tile() == TILE
    assert ops.native.lib().au_join_probe_max_keys() == ops.JOIN_PROBE_MAX_KEYS


@pytest.mark.parametrize("build_kind", ["empty", "one", "dup40", "many"])
@pytest.mark.parametrize("n_probe", N_PROBES)
def test_probe_sizes(monkeypatch, n_probe, build_kind):
    build, probe = _case("int64", build_kind, n_probe, seed=n_probe)
    _check(monkeypatch, build, probe, True, True)


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("build_kind", ["unique", "dup40", "many"])
@pytest.mark.parametrize("emit,need_bm", [(False, False), (False, True),
                                          (True, False), (True, True)])
def test_flags_and_prebuilt_table(monkeypatch, emit, need_bm, build_kind, with_table):
    build, probe = _case("int64", build_kind, 3 * TILE + 17, seed=5)
    _check(monkeypatch, build, probe, emit, need_bm, with_table=with_table)


@pytest.mark.parametrize("build_kind", ["dup40", "many"])
@pytest.mark.parametrize("kind", KEY_KINDS)
def test_key_shapes(monkeypatch, kind, build_kind):
    build, probe = _case(kind, build_kind, TILE + 1, seed=3)
    _check(monkeypatch, build, probe, True, True,
           expect_fused=(kind != "int64x9"))


@pytest.mark.parametrize("kind", ["int64", "int32", "string", "int64+string"])
@pytest.mark.parametrize("probe_nulls,build_nulls", [("all", "10%"), ("none", "none")])
def test_null_layouts(monkeypatch, kind, probe_nulls, build_nulls):
    build, probe = _case(kind, "dup40", TILE + 1, probe_nulls, build_nulls, seed=7)
    assert (probe[0].validity is None) == (probe_nulls == "none")
    _check(monkeypatch, build, probe, True, True)
    _check(monkeypatch, build, probe, False, False)


@pytest.mark.parametrize("with_table", [False, True])
@pytest.mark.parametrize("build_kind", ["empty", "unique", "dup40", "many"])
@pytest.mark.parametrize("kind", ["int64", "int32", "string", "int64+string", "int64x9"])
def test_join_exists(monkeypatch, kind, build_kind, with_table):
    build, probe = _case(kind, build_kind, 2 * TILE + 17, seed=9)
    want = ops.join_counts(build, probe) > 0  # CPU reference path
    bg = [c.to(DEV) for c in build]
    pg = [c.to(DEV) for c in probe]
    table = ops.join_build(bg) if with_table else None
    for switch in ("1", "0"):
        monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", switch)
        got = ops.join_exists(bg, pg, table=table)
        assert got.dtype == torch.bool
        assert torch.equal(got.cpu(), want), switch
    monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", "1")
    assert ops.join_exists(bg, [c.gather(torch.empty(0, dtype=torch.int64, device=DEV))
                                for c in pg], table=table).numel() == 0


def _join_batches():
    rng = np.random.default_rng(21)

    def side(n, key_range, prefix):
        k = [None if rng.random() < 0.1 else int(v)
             for v in rng.integers(0, key_range, n)]
        return RecordBatch.from_pydict(
            {prefix + "k": k, prefix + "v": [int(v) for v in rng.integers(0, 100, n)]},
            {prefix + "k": dtypes.int64, prefix + "v": dtypes.int64})

    return side(2000, 900, "l"), side(2000, 900, "r")


_JOIN_BATCHES = _join_batches()


def _sorted_rows(d):
    return sorted(zip(*d.values()), key=lambda r: tuple((v is None, str(v)) for v in r))


@pytest.mark.parametrize("how,residual", [
    ("inner", False), ("left", False), ("right", False), ("full", False),
    ("semi", False), ("anti", False), ("existence", False),
    ("inner", True), ("left", True)])
def test_executor_join_types(monkeypatch, how, residual):
    monkeypatch.setenv("AURON_JOIN_FUSED_PROBE", "1")
    left, right = _JOIN_BATCHES

    def run(device):
        plan = P.HashJoin(P.MemoryScan([left.to(device)]),
                          P.MemoryScan([right.to(device)]),
                          [col("lk")], [col("rk")], how=how,
                          residual=(col("lv") < col("rv")) if residual else None)
        return _sorted_rows(AuronSession(device=device).collect(plan).to_pydict())

    got, want = run(DEV), run("cpu")
    assert len(want) > 0
    assert got == want
