"""Exact decimal128 window aggregates: the 128-bit prefix / frame-sum /
frame-min-max reference twins against Python integers, and window sum, avg,
min and max over a decimal128 column at plan and SQL level against a
brute-force oracle written here (no engine code).

Every decimal and limb comparison is exact equality. The oracle works on
unscaled Python integers (the limbs decoded), because `Column.to_pylist`
renders decimal128 as float and would round what is being checked."""
import random
from fractions import Fraction

import pytest
import torch

from auron_amd import AuronSession, col, dtypes, ops
from auron_amd.column import Column, RecordBatch
from auron_amd.exprs import Aliased, WindowFunc
from auron_amd.plan import nodes as P
from auron_amd.sql import sql_to_plan

from test_window_range_frames import (_Cat, _column, frame_cases,
                                      oracle_range, oracle_rows, raw)

M64 = (1 << 64) - 1
M128 = (1 << 128) - 1
I128_MAX = (1 << 127) - 1
I128_MIN = -(1 << 127)
D38 = 10 ** 38 - 1
SIZES = [0, 1, 2, 63, 64, 65, 1000]
AVG_RTOL = 2.0 ** -48


# ------------------------------------------------------------ limb helpers
def to_limbs(vals):
    """Python ints (any, reduced modulo 2^128) -> int64 [n,2] limbs."""
    rows = []
    for v in vals:
        v &= M128
        lo, hi = v & M64, v >> 64
        rows.append((lo - (1 << 64) if lo >> 63 else lo,
                     hi - (1 << 64) if hi >> 63 else hi))
    if not rows:
        return torch.empty((0, 2), dtype=torch.int64)
    return torch.tensor(rows, dtype=torch.int64)


def from_limbs(t):
    """int64 [n,2] limbs -> signed Python ints."""
    out = []
    for lo, hi in t.to("cpu").tolist():
        out.append((hi << 64) | (lo & M64))
    return out


def wrap(v):
    """Reduce to the signed 128-bit range."""
    v &= M128
    return v - (1 << 128) if v >> 127 else v


def value_sets(n, seed):
    """name -> n Python ints, the inputs the 128-bit arithmetic can get
    wrong."""
    rnd = random.Random(seed)
    return {
        "random": [rnd.getrandbits(128) - (1 << 127) for _ in range(n)],
        # lo = 0xFFFF...F, hi = 0: every add carries into hi
        "all_carry": [M64] * n,
        "alternating": [D38 if i % 2 == 0 else -D38 for i in range(n)],
        # the prefix passes 2^127 after a few rows and keeps wrapping, while
        # any short frame's sum still fits
        "wrapping": [(1 << 125) + rnd.getrandbits(64) for _ in range(n)],
    }


def mask(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) < 0.7


# ------------------------------------------------- twins vs Python integers
@pytest.mark.parametrize("n", SIZES)
def test_prefix_sum_i128_ref_matches_python_ints(n):
    for name, vals in value_sets(n, seed=n).items():
        for valid in (None, mask(n, n + 1)):
            got = from_limbs(ops.prefix_sum_i128_ref(to_limbs(vals), valid))
            keep = [True] * n if valid is None else valid.tolist()
            want, run = [], 0
            for v, ok in zip(vals, keep):
                run += v if ok else 0
                want.append(wrap(run))
            assert got == want, (name, n, valid is not None)
            # the public entry point takes the twin on the CPU
            assert torch.equal(ops.prefix_sum_i128(to_limbs(vals), valid),
                               ops.prefix_sum_i128_ref(to_limbs(vals), valid))


def _frames(n, seed):
    if n == 0:
        return (torch.tensor([0, 0, 1], dtype=torch.int64),
                torch.tensor([-1, 0, 0], dtype=torch.int64))
    return frame_cases(n, seed=seed, rows=min(4 * n, 400))


@pytest.mark.parametrize("n", SIZES)
def test_window_frame_sum_i128_ref_matches_python_ints(n):
    a, b = _frames(n, n)
    for name, vals in value_sets(n, seed=n + 7).items():
        for valid in (None, mask(n, n + 2)):
            keep = [True] * n if valid is None else valid.tolist()
            x = [v if ok else 0 for v, ok in zip(vals, keep)]
            prefix = ops.prefix_sum_i128_ref(to_limbs(vals), valid)
            got = from_limbs(ops.window_frame_sum_i128_ref(prefix, a, b))
            assert torch.equal(ops.window_frame_sum_i128(prefix, a, b),
                               ops.window_frame_sum_i128_ref(prefix, a, b))
            for i, (lo, hi) in enumerate(zip(a.tolist(), b.tolist())):
                lo, hi = max(lo, 0), min(hi, n - 1)
                # brute force per frame, modulo 2^128
                want = wrap(sum(x[lo:hi + 1])) if lo <= hi else 0
                assert got[i] == want, (name, n, lo, hi)


def test_frame_sums_stay_exact_while_the_prefix_wraps():
    """The premise of the unsegmented scan: the running prefix leaves the
    signed range (and wraps more than once), yet every frame of up to 3
    rows is the true, unwrapped sum."""
    n = 200
    vals = value_sets(n, seed=3)["wrapping"]
    true_prefix = [sum(vals[:i + 1]) for i in range(n)]
    assert true_prefix[-1] > 4 * (1 << 128)
    prefix = ops.prefix_sum_i128_ref(to_limbs(vals))
    assert from_limbs(prefix) != true_prefix
    i = torch.arange(n, dtype=torch.int64)
    a, b = (i - 2).clamp(min=0), i
    got = from_limbs(ops.window_frame_sum_i128_ref(prefix, a, b))
    assert got == [sum(vals[max(j - 2, 0):j + 1]) for j in range(n)]


def minmax_sets(n, seed):
    rnd = random.Random(seed)
    his = [-3, -1, 0, 2]
    return {
        "random": [rnd.getrandbits(128) - (1 << 127) for _ in range(n)],
        # same hi, lo with and without bit 63: lo must compare unsigned
        "lo_only": [(5 << 64) | (rnd.getrandbits(63) | (rnd.getrandbits(1) << 63))
                    for _ in range(n)],
        "negative_hi": [(rnd.choice(his) << 64) | rnd.getrandbits(64)
                        for _ in range(n)],
        "extremes": [rnd.choice([I128_MAX, I128_MIN, 0, -1, 1, M64, -M64 - 1])
                     for _ in range(n)],
    }


@pytest.mark.parametrize("n", SIZES)
def test_window_frame_minmax_i128_ref_matches_python_ints(n):
    a, b = _frames(n, n + 1)
    assert bool((a > b).any())  # empty frames are among the cases
    for name, vals in minmax_sets(n, seed=n + 11).items():
        x = to_limbs(vals)
        for op in ("min", "max"):
            ident = I128_MAX if op == "min" else I128_MIN
            got = from_limbs(ops.window_frame_minmax_i128_ref(x, a, b, op))
            assert torch.equal(ops.window_frame_minmax_i128(x, a, b, op),
                               ops.window_frame_minmax_i128_ref(x, a, b, op))
            for i, (lo, hi) in enumerate(zip(a.tolist(), b.tolist())):
                frame = vals[max(lo, 0):hi + 1] if lo <= hi else []
                want = (min if op == "min" else max)(frame, default=ident)
                assert got[i] == want, (name, op, n, lo, hi)


# ------------------------------------------------------------- plan level
DT = dtypes.decimal128(38, 2)
FUNCS = [("sum", "x"), ("avg", "x"), ("min", "x"), ("max", "x")]
FRAMES = [
    ("rows", None, 0), ("range", None, 0),          # default frames
    ("rows", -2, 1), ("rows", None, -1), ("rows", 1, "U"),
    ("range", -1, 1),
]


def make_rows(n, seed):
    """~7 partitions; unscaled decimal(38,2) values near 10^36 of both signs
    (each beyond 2^53), NULLs among them, partition 5 all NULL; an int key
    with duplicates, so peers exist."""
    rnd = random.Random(seed)
    rows = []
    for rid in range(n):
        p = rnd.choice([0, 1, 2, 3, 4, 5, 6])
        if p == 5 or rnd.random() < 0.15:
            x = None
        else:
            x = rnd.choice([-1, 1]) * (10 ** 36 + rnd.getrandbits(100))
        rows.append({"rid": rid, "p": p, "k": rnd.randint(-6, 6), "x": x,
                     "xf": None, "fv": None})
    return rows


def dec128_column(vals, dt=DT, device="cpu"):
    valid = torch.tensor([v is not None for v in vals], dtype=torch.bool)
    data = to_limbs([0 if v is None else v for v in vals])
    return Column(dt, data, None if bool(valid.all()) else valid).to(device)


def make_batch(rows, device="cpu"):
    cols = [_column(dtypes.int64, [r[nm] for r in rows])
            for nm in ("rid", "p", "k")]
    return RecordBatch(["rid", "p", "k", "x"],
                       [c.to(device) for c in cols]
                       + [dec128_column([r["x"] for r in rows],
                                        device=device)])


def run_window(rows, frame, lo, hi, device="cpu", funcs=FUNCS, ordered=True):
    """As run_window in test_window_range_frames, over a decimal128 x."""
    fns = [Aliased(WindowFunc(fn, col(arg)), f"{fn}_{arg}")
           for fn, arg in funcs]
    plan = P.Window(P.MemoryScan([make_batch(rows, device)]), [col("p")],
                    [(col("k"), True)] if ordered else [], fns,
                    frame=frame, frame_lo=lo, frame_hi=hi)
    s = AuronSession(device=device)
    out = s.collect(plan)
    return out, s.metrics()


def oracle(rows, frame, lo, hi, ordered=True):
    """{rid: {sum_x, cnt, min_x, max_x}} over unscaled ints, from the
    brute-force frame oracles of test_window_range_frames. ROWS frames
    depend on the order among peers, so they are only used with rows whose
    (p, k) order the engine's stable sort reproduces: the oracle's sort is
    stable too, over the same input order."""
    if not ordered:
        flat = [dict(r, k=0) for r in rows]
        return oracle_range(flat, True, None, "U")
    if frame == "range":
        return oracle_range(rows, True, lo, hi)
    return oracle_rows(rows, True, lo, hi)


def decoded(c):
    """DECIMAL128 column -> unscaled Python ints, None for NULL."""
    c = c.to("cpu")
    vals = from_limbs(c.data)
    if c.validity is None:
        return vals
    return [v if ok else None for v, ok in zip(vals, c.validity.tolist())]


def check_decimal_window(out, want, scale=2, ctx=""):
    """sum/min/max exact and typed like the input, NULL exactly where the
    frame holds no valid value; avg within 2^-48 relative of the exactly
    rounded quotient. Returns the largest avg relative error seen."""
    got = dict(zip(out.names, out.columns))
    rid = raw(got["rid"])
    assert sorted(rid) == sorted(want)
    worst = 0.0
    for name in ("sum_x", "min_x", "max_x"):
        if name not in got:
            continue
        assert got[name].dtype == DT, (ctx, name, got[name].dtype)
        for r, g in zip(rid, decoded(got[name])):
            w = want[r][name]
            assert g == w and type(g) is type(w), \
                f"{ctx} {name} rid={r}: got {g!r} want {w!r}"
    if "avg_x" in got:
        assert got["avg_x"].dtype == dtypes.float64
        for r, g in zip(rid, raw(got["avg_x"])):
            w = want[r]
            if w["count_x"] == 0:
                assert g is None, (ctx, r, g)
                continue
            exact = float(Fraction(w["sum_x"], w["count_x"] * 10 ** scale))
            if exact == 0.0:
                assert g == 0.0, (ctx, r, g)
                continue
            err = abs(g - exact) / abs(exact)
            worst = max(worst, err)
            assert err <= AVG_RTOL, \
                f"{ctx} avg_x rid={r}: got {g!r} want {exact!r} rel {err:.3e}"
    return worst


@pytest.fixture(scope="module")
def rows120():
    rows = make_rows(120, seed=21)
    by_p = {}
    for r in rows:
        by_p.setdefault(r["p"], []).append(r["x"])
    assert len(by_p) == 7 and all(v is None for v in by_p[5])
    assert all(abs(r["x"]) > 2 ** 53 for r in rows if r["x"] is not None)
    return rows


@pytest.mark.parametrize("frame,lo,hi", FRAMES)
def test_decimal128_window_frames_match_oracle(rows120, frame, lo, hi):
    out, metrics = run_window(rows120, frame, lo, hi)
    worst = check_decimal_window(out, oracle(rows120, frame, lo, hi),
                                 ctx=f"{frame} ({lo},{hi})")
    print(f"{frame} ({lo},{hi}): worst avg relative error {worst:.3e}")
    assert metrics.get("window.frame_i128_rows", 0) == 4 * len(rows120)


def test_decimal128_rows_frames_are_empty_at_partition_edges(rows120):
    """ROWS (None,-1) and (1,"U") leave the first / last row of every
    partition without a frame: NULL there, not zero."""
    for lo, hi in ((None, -1), (1, "U")):
        want = oracle(rows120, "rows", lo, hi)
        assert sum(1 for w in want.values() if w["count_x"] == 0) >= 7
        out, _ = run_window(rows120, "rows", lo, hi)
        got = dict(zip(out.names, out.columns))
        nulls = sum(v is None for v in decoded(got["sum_x"]))
        assert nulls == sum(1 for w in want.values() if w["count_x"] == 0)


def test_decimal128_window_without_order_by(rows120):
    funcs = [("min", "x"), ("max", "x"), ("avg", "x")]
    out, metrics = run_window(rows120, "range", None, 0, funcs=funcs,
                              ordered=False)
    check_decimal_window(out, oracle(rows120, "range", None, 0,
                                     ordered=False), ctx="no order by")
    assert metrics.get("window.frame_i128_rows", 0) == 3 * len(rows120)


def test_whole_partition_decimal128_sum_keeps_its_path(rows120):
    out, metrics = run_window(rows120, "range", None, 0,
                              funcs=[("sum", "x")], ordered=False)
    check_decimal_window(out, oracle(rows120, "range", None, 0,
                                     ordered=False), ctx="whole partition")
    assert metrics.get("window.frame_i128_rows", 0) == 0


def test_decimal128_window_over_empty_input():
    out, _ = run_window([], "rows", -2, 1)
    got = dict(zip(out.names, out.columns))
    assert out.num_rows == 0
    assert got["sum_x"].dtype == DT and got["min_x"].dtype == DT
    assert got["avg_x"].dtype == dtypes.float64


# --------------------------------------------------------------------- SQL
def test_sql_running_sum_of_decimal128_group_sums():
    """sum(sum(x)) over a decimal(12,2) column: the inner sum is
    decimal128(22,2), the running total stays exact and decimal-typed."""
    rnd = random.Random(9)
    days = [rnd.randrange(12) for _ in range(12000)]
    # unscaled cents near the top of decimal(12,2): the running total
    # passes 2^53
    cents = [rnd.randrange(9 * 10 ** 11, 10 ** 12 - 1) for _ in days]
    dt = dtypes.decimal64(12, 2)
    batch = RecordBatch(
        ["d", "x"],
        [Column(dtypes.int64, torch.tensor(days, dtype=torch.int64)),
         Column(dt, torch.tensor(cents, dtype=torch.int64))])
    s = AuronSession(device="cpu")
    plan = sql_to_plan(
        "select d, sum(sum(x)) over (order by d rows between unbounded "
        "preceding and current row) as s from t group by d",
        _Cat(batch), s, schemas={"t": {"d": dtypes.int64, "x": dt}})
    out = s.collect(plan)
    got = dict(zip(out.names, out.columns))
    assert got["s"].dtype.code == dtypes.DECIMAL128
    assert got["s"].dtype.scale == 2
    per_day = {}
    for d, c in zip(days, cents):
        per_day[d] = per_day.get(d, 0) + c
    want, run = {}, 0
    for d in sorted(per_day):
        run += per_day[d]
        want[d] = run
    assert run > 2 ** 53
    assert dict(zip(raw(got["d"]), decoded(got["s"]))) == want
    assert s.metrics().get("window.frame_i128_rows", 0) == len(per_day)


# ---------------------------------------------------------- unchanged paths
def test_decimal64_wide_running_sum_is_unchanged():
    """A decimal64(17,2) running sum needs 128 bits by the planner's rule
    and keeps the float64 accumulator: a float64 column of the values
    divided by 10^scale, exactly as before this path existed."""
    dt = dtypes.decimal64(17, 2)
    k = _column(dtypes.int64, [1, 2, 3, 4])
    v = Column(dt, torch.tensor([150, 250, -100, 1000], dtype=torch.int64))
    s = AuronSession(device="cpu")
    out = s.collect(P.Window(
        P.MemoryScan([RecordBatch(["k", "v"], [k, v])]), [],
        [(col("k"), True)], [Aliased(WindowFunc("sum", col("v")), "s")],
        frame="rows", frame_lo=None, frame_hi=0))
    got = dict(zip(out.names, out.columns))
    assert got["s"].dtype == dtypes.float64
    assert raw(got["s"]) == [1.5, 4.0, 3.0, 13.0]
    assert s.metrics().get("window.frame_i128_rows", 0) == 0
