"""Route equivalence of the hash aggregate: the same aggregates computed

1. `complete`: one HashAgg(mode="complete") over the whole batch,
2. `tower`:    three HashAgg(mode="partial") over row slices, Union,
               HashAgg(mode="final"),
3. `stream`:   the complete plan forced through the chunked path (peek,
               per-chunk partial states, several state self-merges, one
               final pass)

must give identical values and result types. The inputs make every sum
exact in any accumulation order (integers, decimals, multiples of 0.25), so
the comparison needs no tolerance on either device. An int64 dict oracle
keeps three routes that are wrong in the same way from passing.

Runs on whatever the `device` fixture returns: the torch-expressed path on
CPU, the native kernels on a GPU.
"""
import math
from functools import lru_cache

import numpy as np
import pytest
import torch

from auron_amd import col, dtypes
from auron_amd.column import Column, RecordBatch
from auron_amd.engine.executor import ExecContext, Executor
from auron_amd.exprs import AggFunc, Aliased
from auron_amd.plan import nodes as P

N = 3000
NKEYS = 37  # group 36 has every value column null
D7 = dtypes.decimal64(7, 2)     # sum state decimal64(17,2): stays 64-bit
D15 = dtypes.decimal64(15, 2)   # sum state decimal128(25,2)
D16 = dtypes.decimal64(16, 2)   # |v| < 2e15: avg takes the exact split sum
D128 = dtypes.decimal128(30, 2)
VALUE_TYPES = {"i32": dtypes.int32, "i64": dtypes.int64, "f64": dtypes.float64,
               "b": dtypes.bool_, "d7": D7, "d15": D15, "d16": D16,
               "d128": D128}
FNS = ("sum", "avg", "min", "max", "count", "first")
# avg/min/max over decimal128 raise in every route (a feature gap, not
# pinned here)
AGGS = [AggFunc(fn, col(c), name=f"{fn}_{c}")
        for c in VALUE_TYPES for fn in FNS
        if not (c == "d128" and fn in ("avg", "min", "max"))]
AGGS.append(AggFunc("count_star", None, name="n"))
assert len(AGGS) == 46
KEYS = [Aliased(col("k"), "k")]
ORACLE_NAMES = {"sum_i64", "count_i64", "min_i64", "max_i64"}
# `first` over a keyless 0-row input raises IndexError in every route (it
# gathers row 0 of nothing): a gap like the decimal128 one, not pinned here
AGGS_NO_FIRST = [a for a in AGGS if a.fn != "first"]


@lru_cache(maxsize=None)
def _host_batch() -> RecordBatch:
    rng = np.random.default_rng(20260117)
    k = rng.integers(0, NKEYS, N)
    k_valid = rng.random(N) >= 0.05
    all_null_group = k_valid & (k == NKEYS - 1)
    assert all_null_group.any()

    def valid():
        return (rng.random(N) >= 0.15) & ~all_null_group

    f = rng.integers(-4000, 4001, N) * 0.25
    f_valid = valid()
    f[rng.random(N) < 0.02] = math.nan
    special = np.flatnonzero(f_valid & k_valid)
    f[special[0]] = math.inf
    f[special[1]] = -0.0
    lim16 = 2 * 10 ** 15
    data = {
        "i32": torch.from_numpy(
            rng.integers(-(1 << 31), 1 << 31, N)).to(torch.int32),
        "i64": torch.from_numpy(rng.integers(-(1 << 40), (1 << 40) + 1, N)),
        "f64": torch.from_numpy(f),
        "b": torch.from_numpy(rng.random(N) < 0.5),
        "d7": torch.from_numpy(rng.integers(-10 ** 7 + 1, 10 ** 7, N)),
        "d15": torch.from_numpy(rng.integers(-10 ** 15 + 1, 10 ** 15, N)),
        "d16": torch.from_numpy(rng.integers(-lim16 + 1, lim16, N)),
        "d128": torch.from_numpy(np.stack(
            [rng.integers(-(1 << 63), (1 << 63) - 1, N, endpoint=True),
             rng.integers(-(1 << 30) + 1, 1 << 30, N)], axis=1)),
    }
    validity = {c: torch.from_numpy(f_valid if c == "f64" else valid())
                for c in data}
    # the split-sum route of avg(d16) needs n * max|v| >= 2^62
    assert N * int(data["d16"].abs().max()) >= 1 << 62
    cols = [Column(dtypes.int64, torch.from_numpy(k),
                   torch.from_numpy(k_valid))]
    cols += [Column(VALUE_TYPES[c], data[c], validity[c]) for c in data]
    return RecordBatch(["k"] + list(data), cols)


def _executor(device, **kw):
    ex = Executor(ExecContext(device=device, **kw))
    ex._rewrite = lambda n: n  # keep explicit partial -> final towers
    return ex


def _slices(b: RecordBatch, rows: int):
    return [b.slice(lo, min(rows, b.num_rows - lo))
            for lo in range(0, max(b.num_rows, 1), rows)]


def _complete(device, batches, keys, aggs, **ctx):
    return _executor(device, **ctx).collect(
        P.HashAgg(P.MemoryScan(batches), keys, aggs, mode="complete"))


def _tower(device, b, keys, aggs):
    parts = [P.HashAgg(P.MemoryScan([s]), keys, aggs, mode="partial")
             for s in _slices(b, 1000)]
    return _executor(device).collect(
        P.HashAgg(P.Union(parts), keys, aggs, mode="final"))


def _stream(device, b, keys, aggs, monkeypatch):
    """The complete plan through the chunked path: 64-row chunks, and the
    accumulated states re-merge after every 500-row input batch."""
    monkeypatch.setenv("AURON_STREAM_BYTES", "0")
    try:
        return _complete(device, _slices(b, 500), keys, aggs, batch_rows=64)
    finally:
        monkeypatch.delenv("AURON_STREAM_BYTES")


def _routes(device, b, keys, aggs, monkeypatch):
    return {"complete": _complete(device, [b], keys, aggs),
            "tower": _tower(device, b, keys, aggs),
            "stream": _stream(device, b, keys, aggs, monkeypatch)}


def _same(a, b) -> bool:
    if isinstance(a, float) and isinstance(b, float) \
            and math.isnan(a) and math.isnan(b):
        return True
    return (a is None) == (b is None) and a == b


def _exact(c: Column):
    """Decimal cells as unscaled Python ints (to_pylist divides by the
    scale in floating point, which could hide a low-limb difference)."""
    h = c.to("cpu")
    if c.dtype.code == dtypes.DECIMAL128:
        raw = [(hi << 64) | (lo & ((1 << 64) - 1))
               for lo, hi in h.data.tolist()]
    else:
        raw = h.data.tolist()
    if h.validity is None:
        return raw
    return [v if ok else None for v, ok in zip(raw, h.validity.tolist())]


def _sorted_cells(out: RecordBatch, keyed: bool):
    """{column: cells} with rows ordered by key, the NULL key last."""
    order = list(range(out.num_rows))
    if keyed:
        ks = out.column("k").to_pylist()
        order.sort(key=lambda i: (ks[i] is None, ks[i] or 0))
    cells = {}
    for name, c in zip(out.names, out.columns):
        vals = c.to_pylist()
        cells[name] = [vals[i] for i in order]
        if c.dtype.code in (dtypes.DECIMAL64, dtypes.DECIMAL128):
            raw = _exact(c)
            cells[name + "#raw"] = [raw[i] for i in order]
    return cells


def _schema(out: RecordBatch):
    return {n: (c.dtype.code, c.dtype.precision, c.dtype.scale)
            for n, c in zip(out.names, out.columns)}


def _assert_schemas(complete, tower):
    """Identical result types, with the one recorded difference:
    avg(decimal64(7,2)) is declared p+4 = 11 by the complete route and
    min(17 + 4, 18) = 18 by the routes that finalize from the sum state."""
    want = dict(_schema(complete))
    if "avg_d7" in want:
        assert want["avg_d7"] == (dtypes.DECIMAL64, 11, 6)
        want["avg_d7"] = (dtypes.DECIMAL64, 18, 6)
    assert _schema(tower) == want


def _assert_routes_agree(outs, keyed):
    _assert_schemas(outs["complete"], outs["tower"])
    assert _schema(outs["stream"]) == _schema(outs["tower"])
    ref = _sorted_cells(outs["complete"], keyed)
    for route in ("tower", "stream"):
        got = _sorted_cells(outs[route], keyed)
        assert list(got) == list(ref)
        for name in ref:
            assert len(got[name]) == len(ref[name]), (route, name)
            for r, (a, b) in enumerate(zip(ref[name], got[name])):
                assert _same(a, b), (route, name, r, a, b)
    return ref


def _i64_oracle(keyed):
    """{key: (sum, count, min, max)} of the int64 column."""
    b = _host_batch()
    groups = {}
    for k, x in zip(b.column("k").to_pylist(), b.column("i64").to_pylist()):
        groups.setdefault(k if keyed else 0, []).append(x)
    want = {}
    for k, rows in groups.items():
        xs = [x for x in rows if x is not None]
        want[k] = (sum(xs) if xs else None, len(xs),
                   min(xs) if xs else None, max(xs) if xs else None)
    return want


def _assert_i64_oracle(cells, keyed):
    got = {}
    ks = cells["k"] if keyed else [0]
    for fn in ("sum", "count", "min", "max"):
        name = f"{fn}_i64"
        if name in cells:
            for k, v in zip(ks, cells[name]):
                got.setdefault(k, {})[fn] = v
    want = _i64_oracle(keyed)
    assert set(got) == set(want)
    for k, (s, c, mn, mx) in want.items():
        full = {"sum": s, "count": c, "min": mn, "max": mx}
        for fn, v in got[k].items():
            assert v == full[fn], (k, fn, v, full[fn])


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "keyless"])
@pytest.mark.parametrize("kind", ["single", "all"])
def test_routes_agree(device, monkeypatch, kind, keyed):
    b = _host_batch().to(device)
    keys = KEYS if keyed else []
    plans = [[a] for a in AGGS] if kind == "single" else [AGGS]
    checked = set()
    for aggs in plans:
        outs = _routes(device, b, keys, aggs, monkeypatch)
        cells = _assert_routes_agree(outs, keyed)
        assert outs["complete"].num_rows == (NKEYS + 1 if keyed else 1)
        assert outs["complete"].names == \
            [a.name for a in keys] + [a.name for a in aggs]
        if ORACLE_NAMES & {a.name for a in aggs}:
            _assert_i64_oracle(cells, keyed)
            checked |= {a.name for a in aggs}
    assert ORACLE_NAMES <= checked


def test_all_null_group_and_null_key(device):
    """NULL is a group; group 36 has no valid value in any column."""
    out = _complete(device, [_host_batch().to(device)], KEYS, AGGS)
    cells = _sorted_cells(out, True)
    assert cells["k"] == list(range(NKEYS)) + [None]
    for a in AGGS:
        v = cells[a.name][NKEYS - 1]
        if a.fn == "count":
            assert v == 0, a.name
        elif a.fn == "count_star":
            assert v > 0
        else:
            assert v is None, a.name
    assert cells["n"][NKEYS] > 0 and sum(cells["n"]) == N


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "keyless"])
def test_empty_input(device, monkeypatch, keyed):
    b = _host_batch().slice(0, 0).to(device)
    keys, aggs = (KEYS, AGGS) if keyed else ([], AGGS_NO_FIRST)
    outs = _routes(device, b, keys, aggs, monkeypatch)
    _assert_schemas(outs["complete"], outs["tower"])
    # nothing to stream: the peek finds the input exhausted and the
    # one-shot path answers
    assert _schema(outs["stream"]) == _schema(outs["complete"])
    for route, out in outs.items():
        assert out.names == [a.name for a in keys] + [a.name for a in aggs]
        if keyed:
            assert out.num_rows == 0, route
            continue
        assert out.num_rows == 1, route
        row = out.to_pydict()
        for a in aggs:
            want = 0 if a.fn in ("count", "count_star") else None
            assert row[a.name] == [want], (route, a.name, row[a.name])


def test_keyless_final_over_empty_emits_only_on_rank0(device):
    """Only rank 0 may emit the global aggregate's null row over an empty
    input, else every rank would contribute a duplicate."""
    empty = _host_batch().slice(0, 0).to(device)
    aggs = AGGS_NO_FIRST
    states = _executor(device).collect(
        P.HashAgg(P.MemoryScan([empty]), KEYS, aggs, mode="partial"))
    assert states.num_rows == 0
    states = states.select(states.names[1:])  # keyless state schema
    fin = P.HashAgg(P.MemoryScan([states]), [], aggs, mode="final")
    out0 = _executor(device, rank=0, world_size=2).collect(fin)
    out1 = _executor(device, rank=1, world_size=2).collect(fin)
    assert out0.num_rows == 1 and out1.num_rows == 0
    assert out0.names == out1.names == [a.name for a in aggs]
    assert _schema(out0) == _schema(out1)


def test_decimal_sum_overflow_is_reported(device):
    """3000 addends near 1e18 (unscaled) in one group: the exact split sum
    detects that the total leaves the 64-bit backing instead of wrapping."""
    rng = np.random.default_rng(7)
    raw = torch.from_numpy(rng.integers(10 ** 18, 2 * 10 ** 18, N))
    b = RecordBatch(["k", "v"],
                    [Column(dtypes.int64, torch.zeros(N, dtype=torch.int64)),
                     Column(dtypes.decimal64(18, 2), raw)]).to(device)
    with pytest.raises(ArithmeticError, match="decimal sum overflow"):
        _complete(device, [b], KEYS, [AggFunc("avg", col("v"), name="a")])


@pytest.mark.parametrize("keyed", [True, False], ids=["keyed", "keyless"])
def test_routes_agree_where_states_need_the_split_sum(device, monkeypatch, keyed):
    """avg over decimal64(18,2) where not only the rows but also the partial
    STATES are so large that a plain int64 sum of them could wrap
    (rows * max >= 2^62): the tower's final stage and the stream's state
    merges then combine states with the exact split sum. Rows 0..999 hold
    2e15..3e15, rows 1000..1999 the same keys with those values negated plus
    a little, the rest is small: every state fits int64 and every group's
    avg fits decimal64(18,6)."""
    rng = np.random.default_rng(11)
    k = _host_batch().column("k")
    kd, kv = k.data.clone(), k.validity.clone()
    kd[1000:2000], kv[1000:2000] = kd[:1000], kv[:1000]
    big = rng.integers(2 * 10 ** 15, 3 * 10 ** 15, 1000)
    raw = np.concatenate([big, rng.integers(0, 10 ** 6, 1000) - big,
                          rng.integers(-10 ** 6, 10 ** 6, 1000)])
    valid = rng.random(N) >= 0.15
    valid[1000:2000] = valid[:1000]
    b = RecordBatch(["k", "v"],
                    [Column(dtypes.int64, kd, kv),
                     Column(dtypes.decimal64(18, 2), torch.from_numpy(raw),
                            torch.from_numpy(valid))]).to(device)
    keys = KEYS if keyed else []
    outs = _routes(device, b, keys, [AggFunc("avg", col("v"), name="a")],
                   monkeypatch)
    cells = _assert_routes_agree(outs, keyed)
    groups = {}
    for kk, v, ok in zip(b.column("k").to_pylist(), raw.tolist(), valid.tolist()):
        if ok:
            groups.setdefault(kk if keyed else 0, []).append(v)
    for kk, got in zip(cells["k"] if keyed else [0], cells["a#raw"]):
        total, c = sum(groups[kk]), len(groups[kk])
        half_up = (abs(total) * 20000 + c) // (2 * c)  # at scale + 4
        assert got == (half_up if total >= 0 else -half_up), kk
