"""Window RANGE frames with value offsets, ROWS min/max beyond the old span
limit, and the frame bounds on the wire — against a brute-force O(n^2)
oracle written here in plain Python (no engine code).

Every comparison is exact: float sums use integer-valued floats, so prefix
differences carry no rounding."""
import random

import pytest
import torch

from auron_amd import AuronSession, col, dtypes, ops
from auron_amd.column import Column, RecordBatch
from auron_amd.exprs import Aliased, WindowFunc
from auron_amd.plan import nodes as P
from auron_amd.plan import proto, serde
from auron_amd.plan.pbwire import decode_fields
from auron_amd.sql import sql_to_plan
from auron_amd.sql.parser import SqlError

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1
NAN = float("nan")
INF = float("inf")
DAY_US = 86_400_000_000

# key type -> (dtype, unit of the key domain the bound sets are scaled by)
KEY_TYPES = {
    "int64": (dtypes.int64, 1),
    "int32": (dtypes.int32, 1),
    "date32": (dtypes.date32, 1),
    "timestamp": (dtypes.timestamp, DAY_US // 2),
    "decimal64": (dtypes.decimal64(9, 2), 50),
    "float64": (dtypes.float64, 0.5),
}
# in units of the key domain; the last one is wider than the whole key span
BOUNDS = [(-3, 0), (0, 0), (-2, 5), (2, 4), (-4, -2), (None, 3), (-3, "U"),
          (None, "U"), (-1000, 1000)]
FUNCS = [("sum", "x"), ("avg", "x"), ("count", "x"), ("min", "x"),
         ("max", "x"), ("sum", "xf"), ("min", "xf"), ("max", "xf"),
         ("first_value", "fv"), ("last_value", "fv")]


# ------------------------------------------------------------------ oracle
def _cls(k, asc):
    """Sort class of a key: NULLs first and NaN last ascending, NaN first
    and NULLs last descending; ordinary keys in between."""
    if k is None:
        return 0 if asc else 2
    if k != k:
        return 2 if asc else 0
    return 1


def _shift(k, d):
    """k + d in the key domain: saturating for ints, IEEE for floats."""
    if isinstance(k, float):
        return k + d
    return max(INT64_MIN, min(INT64_MAX, k + d))


def _sorted_partitions(rows, asc):
    parts = {}
    for r in rows:
        parts.setdefault(r["p"], []).append(r)
    for part in parts.values():
        def sk(r):
            c = _cls(r["k"], asc)
            return (c, (r["k"] if asc else -r["k"]) if c == 1 else 0)

        yield sorted(part, key=sk)  # stable


def _aggregate(frame):
    res = {}
    for name in ("x", "xf"):
        xs = [q[name] for q in frame if q[name] is not None]
        res["count_" + name] = len(xs)
        res["sum_" + name] = sum(xs) if xs else None
        res["avg_" + name] = sum(xs) / len(xs) if xs else None
        res["min_" + name] = min(xs) if xs else None
        res["max_" + name] = max(xs) if xs else None
    res["first_value_fv"] = frame[0]["fv"] if frame else None
    res["last_value_fv"] = frame[-1]["fv"] if frame else None
    return res


def oracle_range(rows, asc, lo, hi):
    """{rid: aggregates} for RANGE BETWEEN lo AND hi (None / "U" unbounded,
    else a signed offset in the key domain) over ORDER BY k [asc|desc]."""
    out = {}
    for part in _sorted_partitions(rows, asc):
        ck = [(_cls(q["k"], asc), q["k"]) for q in part]
        for r in part:
            c, k = _cls(r["k"], asc), r["k"]
            if c == 1:
                t_lo = None if lo is None else _shift(k, lo if asc else -lo)
                t_hi = None if hi == "U" else _shift(k, hi if asc else -hi)

            def lower_ok(qc, qk):
                if lo is None:
                    return True
                if c != 1:  # special row: its own peer group onwards
                    return qc >= c
                if qc != 1:  # an offset bound never reaches special rows
                    return qc > 1
                return qk >= t_lo if asc else qk <= t_lo

            def upper_ok(qc, qk):
                if hi == "U":
                    return True
                if c != 1:
                    return qc <= c
                if qc != 1:
                    return qc < 1
                return qk <= t_hi if asc else qk >= t_hi

            frame = [q for q, (qc, qk) in zip(part, ck)
                     if lower_ok(qc, qk) and upper_ok(qc, qk)]
            out[r["rid"]] = _aggregate(frame)
    return out


def oracle_rows(rows, asc, lo, hi):
    """{rid: aggregates} for ROWS BETWEEN lo AND hi (row offsets)."""
    out = {}
    for part in _sorted_partitions(rows, asc):
        m = len(part)
        for i, r in enumerate(part):
            a = 0 if lo is None else max(0, i + lo)
            b = m - 1 if hi == "U" else min(m - 1, i + hi)
            out[r["rid"]] = _aggregate(part[a:b + 1] if a <= b else [])
    return out


# -------------------------------------------------------------------- data
def make_rows(key_type, n, nparts, seed):
    """Rows with heavily duplicated keys (peer groups), NULL keys and, for
    floats, NaN and ±inf. With 7 partitions, partition 5 has only NULL keys
    and partition 6 a single row."""
    rnd = random.Random(seed)
    _, unit = KEY_TYPES[key_type]
    base = {"date32": 19000, "timestamp": 1_600_000_000_000_000}.get(key_type, 0)
    rows = []
    for rid in range(n):
        if nparts == 1:
            p = 0
        elif rid == 0:
            p = 6
        else:
            p = rnd.choice([0, 1, 2, 3, 4, 5, None])
        u = rnd.random()
        if p == 5 or u < 0.12:
            k = None
        elif key_type == "float64" and u < 0.22:
            k = rnd.choice([NAN, INF, -INF])
        else:
            k = base + rnd.randint(-8, 8) * unit
        x = None if rnd.random() < 0.15 else rnd.randint(-500, 500)
        xf = None if rnd.random() < 0.15 else float(rnd.randint(-500, 500))
        # first/last_value argument: a function of (partition, key), so the
        # order among peers cannot matter
        if k is None:
            fv = None
        elif k != k:
            fv = -1
        else:
            fv = hash((p, k)) % 100_003
        rows.append({"rid": rid, "p": p, "k": k, "x": x, "xf": xf, "fv": fv})
    return rows


def _column(dt, vals):
    valid = torch.tensor([v is not None for v in vals], dtype=torch.bool)
    data = torch.tensor([0 if v is None else v for v in vals],
                        dtype=dt.torch_dtype)
    return Column(dt, data, None if bool(valid.all()) else valid)


def make_batch(rows, key_dt, device="cpu"):
    names = ["rid", "p", "k", "x", "xf", "fv"]
    types = [dtypes.int64, dtypes.int64, key_dt, dtypes.int64, dtypes.float64,
             dtypes.int64]
    cols = [_column(dt, [r[nm] for r in rows]) for nm, dt in zip(names, types)]
    return RecordBatch(names, cols).to(device)


def raw(c):
    """Column -> python list of raw storage values (None for NULL)."""
    c = c.to("cpu")
    vals = c.data.tolist()
    if c.validity is None:
        return vals
    return [v if ok else None for v, ok in zip(vals, c.validity.tolist())]


def same(got, want):
    if got is None or want is None:
        return got is None and want is None
    if isinstance(want, float) and want != want:
        return got != got
    return got == want and type(got) is type(want)


def run_window(rows, key_dt, asc, frame, lo, hi, device="cpu", funcs=FUNCS,
               partitioned=True):
    fns = [Aliased(WindowFunc(fn, col(arg)), f"{fn}_{arg}")
           for fn, arg in funcs]
    plan = P.Window(P.MemoryScan([make_batch(rows, key_dt, device)]),
                    [col("p")] if partitioned else [], [(col("k"), asc)],
                    fns, frame=frame, frame_lo=lo, frame_hi=hi)
    s = AuronSession(device=device)
    out = s.collect(plan)
    return out, s.metrics()


def check_against(out, want, funcs=FUNCS, ctx=""):
    rid = raw(out.columns[out.names.index("rid")])
    assert sorted(rid) == sorted(want)
    for fn, arg in funcs:
        name = f"{fn}_{arg}"
        got = raw(out.columns[out.names.index(name)])
        for r, g in zip(rid, got):
            w = want[r][name]
            assert same(g, w), f"{ctx} {name} rid={r}: got {g!r} want {w!r}"


def scaled(bound, unit):
    return bound if bound in (None, "U") else bound * unit


# ------------------------------------------------------------- plan level
@pytest.mark.parametrize("nparts", [1, 7])
@pytest.mark.parametrize("n", [1, 2, 65, 300])
@pytest.mark.parametrize("key_type", list(KEY_TYPES))
def test_range_frames_match_oracle(key_type, n, nparts):
    key_dt, unit = KEY_TYPES[key_type]
    rows = make_rows(key_type, n, nparts, seed=n * 10 + nparts)
    for blo, bhi in BOUNDS:
        lo, hi = scaled(blo, unit), scaled(bhi, unit)
        for asc in (True, False):
            out, metrics = run_window(rows, key_dt, asc, "range", lo, hi)
            check_against(out, oracle_range(rows, asc, lo, hi),
                          ctx=f"{key_type} n={n} ({lo},{hi}) asc={asc}")
            by_value = any(v not in (None, "U", 0) for v in (lo, hi))
            assert metrics.get("window.range_frame_rows", 0) == \
                (n if by_value else 0)


def test_range_frames_produce_empty_frames():
    """(2, 4) and (-4, -2) exclude the current row: sparse keys leave
    frames empty -> count 0, everything else NULL."""
    rows = [{"rid": i, "p": 0, "k": k, "x": 1, "xf": 1.0, "fv": 7}
            for i, k in enumerate([0, 10, 20, 21])]
    for lo, hi in ((2, 4), (-4, -2)):
        want = oracle_range(rows, True, lo, hi)
        assert all(w["count_x"] == 0 and w["sum_x"] is None
                   and w["first_value_fv"] is None for w in want.values())
        out, _ = run_window(rows, dtypes.int64, True, "range", lo, hi)
        check_against(out, want)
        assert raw(out.columns[out.names.index("count_x")]) == [0, 0, 0, 0]


@pytest.mark.parametrize("offset", [5, INT64_MAX])
def test_range_frame_offsets_saturate(offset):
    keys = [INT64_MIN, INT64_MIN + 1, -1, 0, INT64_MAX - 1, INT64_MAX]
    rows = [{"rid": i, "p": 0, "k": k, "x": i + 1, "xf": float(i + 1),
             "fv": i} for i, k in enumerate(keys)]
    for lo, hi in ((-offset, 0), (0, offset), (-offset, offset),
                   (offset, "U"), (None, -offset)):
        for asc in (True, False):
            out, _ = run_window(rows, dtypes.int64, asc, "range", lo, hi)
            check_against(out, oracle_range(rows, asc, lo, hi),
                          ctx=f"({lo},{hi}) asc={asc}")


def test_range_frame_decimal_values_keep_their_type():
    """A decimal64 sum narrow enough to stay in 64 bits stays decimal64
    (unscaled prefix sums), avg divides by 10^scale, min/max keep the value
    type."""
    dt = dtypes.decimal64(7, 2)
    k = _column(dtypes.int64, [1, 2, 3, 5])
    v = Column(dt, torch.tensor([150, 250, 100, 1000], dtype=torch.int64))
    batch = RecordBatch(["k", "v"], [k, v])
    fns = [Aliased(WindowFunc(f, col("v")), f) for f in ("sum", "avg", "min")]
    out = AuronSession(device="cpu").collect(
        P.Window(P.MemoryScan([batch]), [], [(col("k"), True)], fns,
                 frame="range", frame_lo=-1, frame_hi=0))
    got = dict(zip(out.names, out.columns))
    assert got["sum"].dtype == dt and raw(got["sum"]) == [150, 400, 350, 1000]
    assert got["min"].dtype == dt and raw(got["min"]) == [150, 150, 100, 1000]
    assert raw(got["avg"]) == [1.5, 2.0, 1.75, 10.0]


def test_range_frame_plan_level_rejections():
    rows = make_rows("int64", 5, 1, seed=1)
    batch = make_batch(rows, dtypes.int64)
    strs = Column.from_pylist(["a", "b", "c", "d", "e"], dtypes.string)
    d128 = Column.from_pylist([1, 2, 3, 4, 5], dtypes.decimal128(30, 2))
    batch = RecordBatch(batch.names + ["s", "w"], batch.columns + [strs, d128])
    fns = [Aliased(WindowFunc("sum", col("x")), "sx")]
    s = AuronSession(device="cpu")
    for key in ("s", "w"):
        with pytest.raises(NotImplementedError):
            s.collect(P.Window(P.MemoryScan([batch]), [], [(col(key), True)],
                               fns, frame="range", frame_lo=-1, frame_hi=0))
    with pytest.raises(ValueError):  # two ORDER BY keys with an offset
        s.collect(P.Window(P.MemoryScan([batch]), [],
                           [(col("k"), True), (col("x"), True)], fns,
                           frame="range", frame_lo=-1, frame_hi=0))
    with pytest.raises(ValueError):  # fractional offset on an int key
        s.collect(P.Window(P.MemoryScan([batch]), [], [(col("k"), True)],
                           fns, frame="range", frame_lo=-1.5, frame_hi=0))


# --------------------------------------------------------------------- SQL
class _Cat:
    def __init__(self, batch):
        self.batch = batch

    def scan(self, table, columns=None):
        node = P.MemoryScan([self.batch])
        if columns is None:
            return node
        return P.Project(node, [Aliased(col(c), c) for c in columns])


def run_sql(rows, key_dt, over, device="cpu", fn="sum(x)"):
    batch = make_batch(rows, key_dt, device)
    schema = {"t": {"rid": dtypes.int64, "p": dtypes.int64, "k": key_dt,
                    "x": dtypes.int64, "xf": dtypes.float64,
                    "fv": dtypes.int64}}
    s = AuronSession(device=device)
    plan = sql_to_plan(f"select rid, {fn} over ({over}) as s from t",
                       _Cat(batch), s, schemas=schema)
    out = s.collect(plan)
    return out, s.metrics()


SQL_CASES = [
    ("date32", "partition by p order by k "
     "range between 7 preceding and current row", -7, 0, True),
    ("date32", "partition by p order by k "
     "range between interval 7 days preceding and current row", -7, 0, True),
    ("timestamp", "partition by p order by k range between "
     "interval 1 day preceding and interval 1 day following",
     -DAY_US, DAY_US, True),
    ("decimal64", "partition by p order by k "
     "range between 0.50 preceding and current row", -50, 0, True),
    ("float64", "partition by p order by k desc "
     "range between current row and 1.5 following", 0, 1.5, False),
]


@pytest.mark.parametrize("key_type,over,lo,hi,asc", SQL_CASES)
def test_sql_range_frames_match_oracle(key_type, over, lo, hi, asc):
    key_dt, _ = KEY_TYPES[key_type]
    rows = make_rows(key_type, 120, 7, seed=5)
    out, metrics = run_sql(rows, key_dt, over)
    want = oracle_range(rows, asc, lo, hi)
    got = dict(zip(raw(out.columns[0]), raw(out.columns[1])))
    assert len(got) == len(rows)
    for rid, w in want.items():
        assert same(got[rid], w["sum_x"]), (rid, got[rid], w["sum_x"])
    assert metrics.get("window.range_frame_rows", 0) == len(rows)


@pytest.mark.parametrize("key_type,over", [
    # two ORDER BY keys with an offset
    ("int64", "order by k, x range between 1 preceding and current row"),
    # no ORDER BY key
    ("int64", "partition by p range between 1 preceding and current row"),
    # fractional offset on an integer key
    ("int64", "order by k range between 1.5 preceding and current row"),
    ("date32", "order by k range between 1.5 preceding and current row"),
    # bare number on a timestamp key
    ("timestamp", "order by k range between 1 preceding and current row"),
    # interval on an int key
    ("int64", "order by k range between interval 1 day preceding "
              "and current row"),
    # too many fractional digits for decimal(9,2)
    ("decimal64", "order by k range between 0.125 preceding and current row"),
    # reversed frames, RANGE and ROWS
    ("int64", "order by k range between 1 following and 1 preceding"),
    ("int64", "order by k rows between 1 following and 1 preceding"),
    ("int64", "order by k rows between unbounded following and current row"),
    ("int64", "order by k rows between current row and unbounded preceding"),
    ("int64", "order by k range between current row and 2 preceding"),
    # ROWS takes integers only
    ("int64", "order by k rows between 1.5 preceding and current row"),
])
def test_sql_frame_errors(key_type, over):
    key_dt, _ = KEY_TYPES[key_type]
    rows = make_rows(key_type, 5, 1, seed=2)
    with pytest.raises(SqlError):
        run_sql(rows, key_dt, over)


def test_sql_range_offset_on_string_or_decimal128_key():
    batch = RecordBatch(
        ["s", "w", "x"],
        [Column.from_pylist(["a", "b"], dtypes.string),
         Column.from_pylist([1, 2], dtypes.decimal128(30, 2)),
         Column.from_pylist([1, 2], dtypes.int64)])
    schema = {"t": {"s": dtypes.string, "w": dtypes.decimal128(30, 2),
                    "x": dtypes.int64}}
    s = AuronSession(device="cpu")
    for key in ("s", "w"):
        with pytest.raises(SqlError) as ei:
            sql_to_plan(f"select sum(x) over (order by {key} range between "
                        "1 preceding and current row) as r from t",
                        _Cat(batch), s, schemas=schema)
        assert "1 PRECEDING" in str(ei.value)


def test_sql_range_current_row_and_unbounded_need_no_single_key():
    """Without a value offset any ORDER BY works: CURRENT ROW is the peer
    group over all keys."""
    rows = make_rows("int64", 60, 1, seed=8)
    for r in rows:  # a NULL-free second key that only refines the order
        r["x"] = r["rid"] % 3
    out, metrics = run_sql(
        rows, dtypes.int64,
        "order by k, x range between current row and unbounded following",
        fn="count(xf)")
    got = dict(zip(raw(out.columns[0]), raw(out.columns[1])))

    def rank(r):
        return (r["k"] is not None, r["k"] or 0, r["x"])

    for r in rows:
        want = sum(1 for q in rows
                   if q["xf"] is not None and rank(q) >= rank(r))
        assert got[r["rid"]] == want
    assert metrics.get("window.range_frame_rows", 0) == 0


# ----------------------------------------------------------- ROWS min/max
def _unique_key_rows(n, nparts, seed):
    rnd = random.Random(seed)
    ks = list(range(n))
    rnd.shuffle(ks)
    return [{"rid": i, "p": i % nparts, "k": ks[i],
             "x": None if rnd.random() < 0.1 else rnd.randint(-10**6, 10**6),
             "xf": None if rnd.random() < 0.1
             else float(rnd.randint(-10**6, 10**6)),
             "fv": 0} for i in range(n)]


MINMAX = [("min", "x"), ("max", "x"), ("min", "xf"), ("max", "xf")]


def test_rows_minmax_unbounded_side():
    rows = _unique_key_rows(200, 3, seed=3)
    for lo, hi in ((None, 1), (-2, "U")):
        out, metrics = run_window(rows, dtypes.int64, True, "rows", lo, hi,
                                  funcs=MINMAX)
        check_against(out, oracle_rows(rows, True, lo, hi), funcs=MINMAX)
        assert metrics.get("window.frame_minmax_rows", 0) == 4 * len(rows)


def test_rows_minmax_wide_span():
    rows = _unique_key_rows(4097, 1, seed=4)
    out, metrics = run_window(rows, dtypes.int64, True, "rows", -1500, 0,
                              funcs=MINMAX)
    check_against(out, oracle_rows(rows, True, -1500, 0), funcs=MINMAX)
    assert metrics.get("window.frame_minmax_rows", 0) == 4 * len(rows)


def test_rows_minmax_short_span_keeps_old_path():
    rows = _unique_key_rows(200, 3, seed=6)
    funcs = MINMAX + [("sum", "x"), ("count", "x")]
    out, metrics = run_window(rows, dtypes.int64, True, "rows", -3, 2,
                              funcs=funcs)
    check_against(out, oracle_rows(rows, True, -3, 2), funcs=funcs)
    assert metrics.get("window.frame_minmax_rows", 0) == 0
    assert metrics.get("window.range_frame_rows", 0) == 0


# -------------------------------------------------------------------- wire
def _wire_window(frame, lo, hi):
    batch = RecordBatch.from_pydict({"k": [1, 2, 3], "x": [1, 2, 3]},
                                    {"k": dtypes.int64, "x": dtypes.int64})
    return P.Window(P.MemoryScan([batch]), [], [(col("k"), True)],
                    [Aliased(WindowFunc("sum", col("x")), "sx")],
                    frame=frame, frame_lo=lo, frame_hi=hi)


@pytest.mark.parametrize("frame,lo,hi", [
    ("rows", -1, 1), ("range", -2.5, "U"), ("range", None, 3),
    ("rows", 0, 0), ("range", None, 0)])
def test_frame_bounds_round_trip(frame, lo, hi):
    node = _wire_window(frame, lo, hi)
    for back in (proto.decode_plan(proto.encode_plan(node)),
                 serde.deserialize_plan(serde.serialize_plan(node))):
        assert isinstance(back, P.Window) and back.frame == frame
        assert same(back.frame_lo, lo) and same(back.frame_hi, hi)


def _window_fields(node):
    top = decode_fields(proto.encode_plan(node))
    assert list(top) == [22]
    return decode_fields(top[22][-1])


def test_default_frame_encoding_has_no_bound_fields():
    for frame in ("range", "rows"):
        assert max(_window_fields(_wire_window(frame, None, 0))) <= 5
    assert {6, 7, 9, 10} <= set(_window_fields(_wire_window("rows", -1, 1)))


# --------------------------------------------------------- reference twins
def sorted_key_case(n, is_float, asc, seed):
    """Sorted keys in random partitions (lengths 1 and 64 and one long run
    of a single key among them) -> (key, slo, shi). Some windows are shrunk
    by one at either end, as when special rows sit at a partition's ends."""
    rnd = random.Random(seed)
    lens = []
    left = n
    for want in (1, 64, max(n // 3, 1)):
        if left >= want:
            lens.append(want)
            left -= want
    while left:
        ln = min(left, rnd.choice([1, 2, 3, 17, 64, 65, 200, 1000]))
        lens.append(ln)
        left -= ln
    rnd.shuffle(lens)
    keys, slo, shi = [], [], []
    start = 0
    long_run = max(n // 3, 1)
    for ln in lens:
        if ln == long_run and ln > 64:
            part = [7] * ln  # one repeated key
        else:
            part = [rnd.randint(-30, 30) for _ in range(ln)]
            if is_float and ln > 2:
                part[0], part[1] = -INF, INF
        part.sort(reverse=not asc)
        keys += [float(k) / 2 if is_float else k for k in part]
        w0, w1 = start, start + ln - 1
        if ln > 3 and rnd.random() < 0.3:
            w0, w1 = w0 + 1, w1 - 1
        slo += [w0] * ln
        shi += [w1] * ln
        start += ln
    key = torch.tensor(keys, dtype=torch.float64 if is_float else torch.int64)
    return (key, torch.tensor(slo, dtype=torch.int64),
            torch.tensor(shi, dtype=torch.int64))


def brute_bounds(key, slo, shi, lo, hi, desc):
    ks, s0, s1 = key.tolist(), slo.tolist(), shi.tolist()
    a, b = [], []
    for i, k in enumerate(ks):
        win = range(s0[i], s1[i] + 1)
        if lo is None:
            a.append(s0[i])
        else:
            t = _shift(k, -lo if desc else lo)
            ok = [j for j in win if (ks[j] <= t if desc else ks[j] >= t)]
            a.append(ok[0] if ok else s1[i] + 1)
        if hi == "U":
            b.append(s1[i])
        else:
            t = _shift(k, -hi if desc else hi)
            ok = [j for j in win if (ks[j] >= t if desc else ks[j] <= t)]
            b.append(ok[-1] if ok else s0[i] - 1)
    return a, b


@pytest.mark.parametrize("is_float", [False, True])
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_window_range_bounds_ref_matches_brute_force(n, is_float):
    for asc in (True, False):
        key, slo, shi = sorted_key_case(n, is_float, asc, seed=n)
        for blo, bhi in BOUNDS:
            lo = scaled(blo, 0.5 if is_float else 1)
            hi = scaled(bhi, 0.5 if is_float else 1)
            a, b = ops.window_range_bounds_ref(key, slo, shi, lo, hi,
                                               descending=not asc)
            wa, wb = brute_bounds(key, slo, shi, lo, hi, not asc)
            assert a.tolist() == wa and b.tolist() == wb, (n, lo, hi, asc)


def test_window_range_bounds_ref_saturates():
    for asc in (True, False):
        keys = sorted([INT64_MIN, INT64_MIN + 1, -1, 0, INT64_MAX - 1,
                       INT64_MAX], reverse=not asc)
        key = torch.tensor(keys, dtype=torch.int64)
        slo = torch.zeros(6, dtype=torch.int64)
        shi = torch.full((6,), 5, dtype=torch.int64)
        for off in (5, INT64_MAX):
            for lo, hi in ((-off, 0), (0, off), (-off, off), (off, "U"),
                           (None, -off)):
                a, b = ops.window_range_bounds_ref(key, slo, shi, lo, hi,
                                                   descending=not asc)
                wa, wb = brute_bounds(key, slo, shi, lo, hi, not asc)
                assert a.tolist() == wa and b.tolist() == wb, (lo, hi, asc)


def frame_cases(n, seed, rows=None):
    """Frames over an n-element array: single elements, exactly one aligned
    64-tile, a tile straddled by one on each side, the whole array, empty
    ones, and random ones -> (a, b) int64 tensors."""
    rnd = random.Random(seed)
    fr = [(0, n - 1), (n - 1, n - 1), (0, 0), (n - 1, 0) if n > 1 else (1, 0),
          (n, n - 1), (0, -1)]
    for t in range(0, (n + 63) // 64, max(1, n // 64 // 8)):
        fr.append((64 * t, min(64 * t + 63, n - 1)))
        fr.append((max(64 * t - 1, 0), min(64 * t + 64, n - 1)))
    for _ in range(rows if rows is not None else min(4 * n, 3000)):
        i, j = rnd.randrange(n), rnd.randrange(n)
        kind = rnd.random()
        if kind < 0.1:
            fr.append((i, i))
        elif kind < 0.2:
            fr.append((max(i, j), min(i, j) - 1))  # empty
        elif kind < 0.6:
            fr.append((i, min(n - 1, i + rnd.randrange(200))))
        else:
            fr.append((min(i, j), max(i, j)))
    a = torch.tensor([f[0] for f in fr], dtype=torch.int64)
    b = torch.tensor([f[1] for f in fr], dtype=torch.int64)
    return a, b


def minmax_values(n, is_float, seed, with_nan=False):
    g = torch.Generator().manual_seed(seed)
    if not is_float:
        x = torch.randint(-1000, 1000, (n,), generator=g, dtype=torch.int64)
        if n > 4:
            x[1], x[n // 2] = INT64_MIN, INT64_MAX
        return x
    x = torch.randint(-1000, 1000, (n,), generator=g).to(torch.float64) / 4
    if n > 4:
        x[0], x[n // 2] = INF, -INF
    if with_nan:
        x[torch.rand(n, generator=g) < 0.02] = NAN
        x[n - 1] = NAN
    return x


@pytest.mark.parametrize("is_float,with_nan",
                         [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("n", [1, 2, 65, 300])
def test_window_frame_minmax_ref_matches_brute_force(n, is_float, with_nan):
    x = minmax_values(n, is_float, seed=n, with_nan=with_nan)
    a, b = frame_cases(n, seed=n)
    xs = x.tolist()
    for op in ("min", "max"):
        got = ops.window_frame_minmax_ref(x, a, b, op).tolist()
        if is_float:
            ident = INF if op == "min" else -INF
        else:
            ident = INT64_MAX if op == "min" else INT64_MIN
        for i, (lo, hi) in enumerate(zip(a.tolist(), b.tolist())):
            vals = xs[max(lo, 0):hi + 1] if lo <= hi else []
            if any(v != v for v in vals):
                want = NAN  # NaN propagates, as torch.minimum does
            else:
                want = (min if op == "min" else max)(vals, default=ident)
            assert same(got[i], want), (op, lo, hi, got[i], want)
