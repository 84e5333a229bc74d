"""gfx950 window frame kernels (csrc/window.hip) against their pure-torch
reference twins, exactly; plus RANGE frames end to end on the device
against the CPU run of the same plan."""
import pytest
import torch

from auron_amd import dtypes, native, ops

from test_window_range_frames import (BOUNDS, FUNCS, INT64_MAX, INT64_MIN,
                                      KEY_TYPES, SQL_CASES, frame_cases,
                                      make_rows, minmax_values, raw,
                                      run_sql, run_window, same, scaled,
                                      sorted_key_case)
from test_window_functions import all_funcs, by_rid, window

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (1, 63, 64, 65, 257, 4097, 100_000)


def _check_bounds(key, slo, shi, lo, hi, desc):
    native.require()
    want_a, want_b = ops.window_range_bounds_ref(key, slo, shi, lo, hi,
                                                 descending=desc)
    a, b = ops.window_range_bounds(key.to(DEV), slo.to(DEV), shi.to(DEV),
                                   lo, hi, descending=desc)
    assert a.dtype == torch.int64 and a.device.type == "cuda"
    assert b.dtype == torch.int64 and b.device.type == "cuda"
    assert torch.equal(a.cpu(), want_a), (key.numel(), lo, hi, desc)
    assert torch.equal(b.cpu(), want_b), (key.numel(), lo, hi, desc)


@pytest.mark.parametrize("is_float", [False, True])
@pytest.mark.parametrize("n", SIZES)
def test_range_bounds_kernel_matches_reference(n, is_float):
    for asc in (True, False):
        key, slo, shi = sorted_key_case(n, is_float, asc, seed=n)
        for blo, bhi in BOUNDS:
            unit = 0.5 if is_float else 1
            _check_bounds(key, slo, shi, scaled(blo, unit), scaled(bhi, unit),
                          not asc)


def test_range_bounds_kernel_saturates():
    for asc in (True, False):
        keys = sorted([INT64_MIN, INT64_MIN + 1, -1, 0, INT64_MAX - 1,
                       INT64_MAX], reverse=not asc)
        key = torch.tensor(keys, dtype=torch.int64)
        slo = torch.zeros(6, dtype=torch.int64)
        shi = torch.full((6,), 5, dtype=torch.int64)
        for off in (5, INT64_MAX):
            for lo, hi in ((-off, 0), (0, off), (-off, off), (off, "U"),
                           (None, -off)):
                _check_bounds(key, slo, shi, lo, hi, not asc)


# 64/65 and 4096/4097 cross the pyramid level edges; 262_145 needs level 4
@pytest.mark.parametrize("is_float,with_nan",
                         [(False, False), (True, False), (True, True)])
@pytest.mark.parametrize("n", SIZES + (4096, 262_145))
def test_frame_minmax_kernel_matches_reference(n, is_float, with_nan):
    native.require()
    x = minmax_values(n, is_float, seed=n, with_nan=with_nan)
    a, b = frame_cases(n, seed=n, rows=3000)
    xd, ad, bd = x.to(DEV), a.to(DEV), b.to(DEV)
    for op in ("min", "max"):
        want = ops.window_frame_minmax_ref(x, a, b, op)
        got = ops.window_frame_minmax(xd, ad, bd, op)
        assert got.dtype == x.dtype and got.device.type == "cuda"
        got = got.cpu()
        if is_float:  # NaN in the same places, equal everywhere else
            assert torch.equal(got.isnan(), want.isnan()), (n, op)
            got, want = got.nan_to_num(nan=0.0), want.nan_to_num(nan=0.0)
        assert torch.equal(got, want), (n, op)


def _by_rid(out, names):
    rid = raw(out.columns[out.names.index("rid")])
    cols = [raw(out.columns[out.names.index(nm)]) for nm in names]
    return {r: tuple(c[i] for c in cols) for i, r in enumerate(rid)}


def test_sql_date_range_frame_on_device_matches_cpu():
    native.require()
    key_type, over, _, _, _ = SQL_CASES[0]
    key_dt, _ = KEY_TYPES[key_type]
    rows = make_rows(key_type, 120, 7, seed=5)
    out, metrics = run_sql(rows, key_dt, over, device=DEV)
    cpu, _ = run_sql(rows, key_dt, over)
    assert all(c.data.device.type == "cuda" for c in out.columns)
    assert metrics.get("window.range_frame_rows", 0) > 0
    assert _by_rid(out, ["s"]) == _by_rid(cpu, ["s"])


def test_desc_float_range_frame_on_device_matches_cpu():
    native.require()
    key_dt, unit = KEY_TYPES["float64"]
    rows = make_rows("float64", 300, 7, seed=3007)
    names = [f"{fn}_{arg}" for fn, arg in FUNCS]
    for blo, bhi in ((-2, 5), (2, 4), (-3, "U")):
        lo, hi = scaled(blo, unit), scaled(bhi, unit)
        out, metrics = run_window(rows, key_dt, False, "range", lo, hi,
                                  device=DEV)
        cpu, _ = run_window(rows, key_dt, False, "range", lo, hi)
        assert all(c.data.device.type == "cuda" for c in out.columns)
        assert metrics.get("window.range_frame_rows", 0) > 0
        assert metrics.get("window.frame_minmax_rows", 0) > 0
        got, want = _by_rid(out, names), _by_rid(cpu, names)
        assert got.keys() == want.keys()
        for r in want:
            assert all(same(g, w) for g, w in zip(got[r], want[r])), \
                (lo, hi, r, got[r], want[r])


def test_all_functions_in_one_node_on_device_match_cpu():
    """Every window function in one node, so that they share the node's
    partitions, peer groups and frame: the default RANGE frame and a
    bounded ROWS frame."""
    native.require()
    rows = make_rows("int64", 300, 7, seed=3307)
    fns = all_funcs(300)
    for frame, lo, hi in (("range", None, 0), ("rows", -2, 1)):
        out, _ = window(rows, fns, frame, lo, hi, device=DEV)
        cpu, _ = window(rows, fns, frame, lo, hi)
        assert out.names == cpu.names
        assert all(c.data.device.type == "cuda" for c in out.columns)
        for name, _ in fns:
            got, want = by_rid(out, name), by_rid(cpu, name)
            assert got.keys() == want.keys()
            for r in want:
                assert same(got[r], want[r]), \
                    (frame, name, r, got[r], want[r])
