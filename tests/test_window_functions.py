"""Window functions under the default frames, without ORDER BY, all at once
in one node, and over an empty input — against the brute-force oracles of
test_window_range_frames and a small ranking/offset oracle written here in
plain Python (no engine code). Every comparison is exact."""
import pytest

from auron_amd import AuronSession, col, dtypes
from auron_amd.exprs import Aliased, WindowFunc
from auron_amd.plan import nodes as P

from test_window_range_frames import (FUNCS, KEY_TYPES, _sorted_partitions,
                                      _unique_key_rows, check_against,
                                      make_batch, make_rows, oracle_range,
                                      oracle_rows, raw, run_window, same)

SIZES = [1, 2, 65, 300]
AGGS = [(fn, arg) for fn, arg in FUNCS if "value" not in fn]
DEFAULT = -7  # third argument of the lead/lag variants that have one
FRAMES = [("range", None, 0), ("rows", None, 0), ("rows", -2, 1),
          ("range", None, "U")]

RANKING = [(fn, WindowFunc(fn))
           for fn in ("rank", "dense_rank", "percent_rank", "cume_dist")]


def offset_funcs(n):
    fns = [("row_number", WindowFunc("row_number"))]
    fns += [(f"ntile_{k}", WindowFunc("ntile", None, k)) for k in (1, 3, n + 1)]
    for fn in ("lag", "lead"):
        for off in (1, 2):
            fns.append((f"{fn}_{off}", WindowFunc(fn, col("x"), off)))
            fns.append((f"{fn}_{off}_d", WindowFunc(fn, col("x"), off, DEFAULT)))
    fns += [("first_value_x", WindowFunc("first_value", col("x"))),
            ("last_value_x", WindowFunc("last_value", col("x"))),
            ("nth_value_x", WindowFunc("nth_value", col("x"), 2))]
    return fns


def all_funcs(n):
    return (RANKING + offset_funcs(n)
            + [(f"{fn}_{arg}", WindowFunc(fn, col(arg))) for fn, arg in FUNCS])


def window(rows, fns, frame="range", lo=None, hi=0, asc=True,
           partitioned=True, ordered=True, device="cpu"):
    plan = P.Window(P.MemoryScan([make_batch(rows, dtypes.int64, device)]),
                    [col("p")] if partitioned else [],
                    [(col("k"), asc)] if ordered else [],
                    [Aliased(wf, name) for name, wf in fns],
                    frame=frame, frame_lo=lo, frame_hi=hi)
    s = AuronSession(device=device)
    return s.collect(plan), s.metrics()


def by_rid(out, name):
    rid = raw(out.columns[out.names.index("rid")])
    return dict(zip(rid, raw(out.columns[out.names.index(name)])))


def check_columns(out, want, names, ctx=""):
    """`want`: {rid: {name: value}}."""
    for name in names:
        got = by_rid(out, name)
        assert got.keys() == want.keys()
        for r, g in got.items():
            assert same(g, want[r][name]), \
                f"{ctx} {name} rid={r}: got {g!r} want {want[r][name]!r}"


def running_path_only(metrics):
    return (metrics.get("window.range_frame_rows", 0) == 0
            and metrics.get("window.frame_minmax_rows", 0) == 0)


# ---------------------------------------------------------- default frames
@pytest.mark.parametrize("nparts", [1, 7])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("key_type", [k for k in KEY_TYPES if k != "float64"])
def test_default_range_frame_matches_oracle(key_type, n, nparts):
    """float64 keys are left out: make_rows gives them NaN keys, which the
    default RANGE frame does not treat as peers of each other."""
    key_dt, _ = KEY_TYPES[key_type]
    rows = make_rows(key_type, n, nparts, seed=n * 10 + nparts)
    for asc in (True, False):
        out, metrics = run_window(rows, key_dt, asc, "range", None, 0)
        check_against(out, oracle_range(rows, asc, None, 0),
                      ctx=f"{key_type} n={n} asc={asc}")
        assert running_path_only(metrics)


@pytest.mark.parametrize("nparts", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_default_rows_frame_matches_oracle(n, nparts):
    rows = _unique_key_rows(n, nparts, seed=n + nparts)
    for asc in (True, False):
        out, metrics = run_window(rows, dtypes.int64, asc, "rows", None, 0,
                                  funcs=AGGS)
        check_against(out, oracle_rows(rows, asc, None, 0), funcs=AGGS,
                      ctx=f"n={n} asc={asc}")
        assert running_path_only(metrics)


# ------------------------------------------------- ranking, offset, value
def oracle_ranking(rows, asc):
    """{rid: rank, dense_rank, percent_rank, cume_dist}; rows with equal
    keys (NULL equals NULL) are peers."""
    out = {}
    for part in _sorted_partitions(rows, asc):
        keys = [r["k"] for r in part]
        m = len(part)
        for i, r in enumerate(part):
            first = keys.index(keys[i])
            last = m - 1 - keys[::-1].index(keys[i])
            out[r["rid"]] = {
                "rank": first + 1,
                "dense_rank": len(set(keys[:first])) + 1,
                "percent_rank": first / (m - 1) if m > 1 else 0.0,
                "cume_dist": (last + 1) / m}
    return out


def oracle_offsets(rows, asc, n):
    """{rid: the offset_funcs(n) values} over unique ORDER BY keys, where
    the default ROWS and RANGE frames both end at the current row."""
    out = {}
    for part in _sorted_partitions(rows, asc):
        xs = [r["x"] for r in part]
        m = len(part)
        for i, r in enumerate(part):
            w = {"row_number": i + 1, "first_value_x": xs[0],
                 "last_value_x": xs[i],
                 "nth_value_x": xs[1] if i >= 1 else None}
            for k in (1, 3, n + 1):
                # the first m % k buckets hold one row more
                base, rem = divmod(m, k)
                cut = rem * (base + 1)
                w[f"ntile_{k}"] = (i // (base + 1) + 1 if i < cut
                                   else rem + (i - cut) // base + 1)
            for fn, sign in (("lag", -1), ("lead", 1)):
                for off in (1, 2):
                    j = i + sign * off
                    inside = 0 <= j < m
                    w[f"{fn}_{off}"] = xs[j] if inside else None
                    w[f"{fn}_{off}_d"] = xs[j] if inside else DEFAULT
            out[r["rid"]] = w
    return out


@pytest.mark.parametrize("nparts", [1, 7])
@pytest.mark.parametrize("n", SIZES)
def test_ranking_functions_match_oracle(n, nparts):
    rows = make_rows("int64", n, nparts, seed=n * 7 + nparts)
    for asc in (True, False):
        out, _ = window(rows, RANKING, asc=asc)
        check_columns(out, oracle_ranking(rows, asc),
                      [name for name, _ in RANKING], ctx=f"asc={asc}")


@pytest.mark.parametrize("nparts", [1, 7])
@pytest.mark.parametrize("n", SIZES)
def test_offset_and_value_functions_match_oracle(n, nparts):
    rows = _unique_key_rows(n, nparts, seed=n * 3 + nparts)
    fns = offset_funcs(n)
    for asc in (True, False):
        want = oracle_offsets(rows, asc, n)
        for frame in ("rows", "range"):
            out, _ = window(rows, fns, frame=frame, asc=asc)
            check_columns(out, want, [name for name, _ in fns],
                          ctx=f"{frame} asc={asc}")


# ------------------------------------------------------------- no ORDER BY
@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("nparts", [1, 7])
@pytest.mark.parametrize("n", SIZES)
def test_aggregates_without_order_by_cover_the_partition(n, nparts,
                                                         partitioned):
    rows = make_rows("int64", n, nparts, seed=n * 5 + nparts)
    fns = [(f"{fn}_{arg}", WindowFunc(fn, col(arg))) for fn, arg in AGGS]
    out, metrics = window(rows, fns, partitioned=partitioned, ordered=False)
    whole = rows if partitioned else [dict(r, p=0) for r in rows]
    check_columns(out, oracle_rows(whole, True, None, "U"),
                  [name for name, _ in fns])
    assert running_path_only(metrics)


# ------------------------------------------------- every function at once
@pytest.mark.parametrize("nparts", [1, 7])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("frame,lo,hi", FRAMES)
def test_all_functions_in_one_node_match_single_function_plans(
        frame, lo, hi, n, nparts):
    rows = make_rows("int64", n, nparts, seed=n * 11 + nparts)
    fns = all_funcs(n)
    out, _ = window(rows, fns, frame, lo, hi)
    assert out.names == ["rid", "p", "k", "x", "xf", "fv"] + \
        [name for name, _ in fns]
    for name, wf in fns:
        alone, _ = window(rows, [(name, wf)], frame, lo, hi)
        got, want = by_rid(out, name), by_rid(alone, name)
        assert got.keys() == want.keys()
        for r in want:
            assert same(got[r], want[r]), (name, r, got[r], want[r])


# -------------------------------------------------------------- empty input
@pytest.mark.parametrize("ordered", [True, False])
@pytest.mark.parametrize("partitioned", [True, False])
@pytest.mark.parametrize("frame,lo,hi", FRAMES)
def test_all_functions_over_an_empty_input(frame, lo, hi, partitioned,
                                           ordered):
    """Zero rows in, zero rows out, with the types of a one-row run.

    Before the window operator got a layout that is defined for n == 0 this
    failed for cume_dist only, which raised IndexError; every other function
    already returned a zero-row column."""
    fns = all_funcs(1)
    one, _ = window(make_rows("int64", 1, 7, seed=1), fns, frame, lo, hi,
                    partitioned=partitioned, ordered=ordered)
    out, _ = window([], fns, frame, lo, hi, partitioned=partitioned,
                    ordered=ordered)
    assert out.names == one.names and one.num_rows == 1
    assert out.num_rows == 0 and all(len(c) == 0 for c in out.columns)
    for name, c, c1 in zip(out.names, out.columns, one.columns):
        assert c.dtype.name == c1.dtype.name, name
        assert c.data.dtype == c1.data.dtype, name
