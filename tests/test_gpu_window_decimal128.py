"""The 128-bit window kernels (prefix sum, frame sum, frame min/max) against
their torch twins on the device, bit for bit, at the sizes where the wave,
block, tile and pyramid-level edges sit; and one decimal128 window plan on
the GPU against its CPU run."""
import pytest
import torch

from auron_amd import dtypes, native, ops

from test_window_range_frames import frame_cases, raw
from test_window_decimal128 import (AVG_RTOL, DT, FUNCS, decoded, make_rows,
                                    run_window)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _tile():
    return int(native.require().au_i128_scan_tile())


# sizes as (k, d) -> n = k * T + d with T the scan tile, known only once the
# library is loaded: the wave, block and tile edges, and 257 tiles — more
# tile totals than the one-block scan of the totals has threads
SCAN_SIZES = [(0, 1), (0, 63), (0, 64), (0, 65), (0, 255), (0, 256),
              (0, 257), (1, -1), (1, 0), (1, 1), (2, 1), (257, 3)]
# the 64-ary pyramid's level edges
PYRAMID_SIZES = [(0, 4096), (0, 4097), (0, 262145)]


def _size_id(kd):
    k, d = kd
    return str(d) if k == 0 else f"{k}T{d:+d}"


def _n(kd):
    return kd[0] * _tile() + kd[1]


def _limbs(n, seed, kind="random"):
    """int64 [n,2] limbs on the device."""
    g = torch.Generator().manual_seed(seed)
    if kind == "all_carry":  # lo = 0xFFFF...F, hi = 0: every add carries
        x = torch.zeros((n, 2), dtype=torch.int64)
        x[:, 0] = -1
        return x.to(DEV)
    x = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), generator=g,
                      dtype=torch.int64)
    if kind == "close":  # few distinct hi, so lo decides; bit 63 set in half
        x[:, 1] = torch.randint(-2, 2, (n,), generator=g, dtype=torch.int64)
    return x.to(DEV)


def _mask(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, generator=g) < 0.7).to(DEV)


def _is_device_limbs(t, rows):
    return (t.is_cuda and t.dtype == torch.int64
            and tuple(t.shape) == (rows, 2))


def test_scan_tile_is_exported():
    t = _tile()
    assert t >= 256 and t % 256 == 0


@pytest.mark.parametrize("with_valid", [False, True])
@pytest.mark.parametrize("size", SCAN_SIZES, ids=_size_id)
def test_prefix_and_frame_sum_kernels_match_twins(size, with_valid):
    native.require()
    n = _n(size)
    a, b = frame_cases(n, seed=n, rows=3000)
    a, b = a.to(DEV), b.to(DEV)
    valid = _mask(n, n + 1) if with_valid else None
    for kind in ("random", "all_carry"):
        x = _limbs(n, n + 2, kind)
        got = ops.prefix_sum_i128(x, valid)
        want = ops.prefix_sum_i128_ref(x, valid)
        assert _is_device_limbs(got, n)
        assert torch.equal(got, want), (n, kind)
        fs = ops.window_frame_sum_i128(want, a, b)
        assert _is_device_limbs(fs, a.numel())
        assert torch.equal(fs, ops.window_frame_sum_i128_ref(want, a, b)), \
            (n, kind)


@pytest.mark.parametrize("size", SCAN_SIZES + PYRAMID_SIZES, ids=_size_id)
def test_frame_minmax_i128_kernel_matches_twin(size):
    native.require()
    n = _n(size)
    a, b = frame_cases(n, seed=n + 5, rows=3000)
    a, b = a.to(DEV), b.to(DEV)
    for kind in ("random", "close"):
        x = _limbs(n, n + 3, kind)
        for op in ("min", "max"):
            got = ops.window_frame_minmax_i128(x, a, b, op)
            assert _is_device_limbs(got, a.numel())
            assert torch.equal(
                got, ops.window_frame_minmax_i128_ref(x, a, b, op)), \
                (n, kind, op)


def test_decimal128_window_plan_matches_cpu_run():
    native.require()
    rows = make_rows(300, seed=33)
    for frame, lo, hi in (("range", -1, 1), ("rows", None, 0)):
        out, metrics = run_window(rows, frame, lo, hi, device=DEV)
        ref, _ = run_window(rows, frame, lo, hi, device="cpu")
        assert metrics.get("window.frame_i128_rows", 0) == 4 * len(rows)
        assert all(c.data.device.type == "cuda" for c in out.columns)
        got = dict(zip(out.names, out.columns))
        want = dict(zip(ref.names, ref.columns))
        order_g = {r: i for i, r in enumerate(raw(got["rid"]))}
        order_w = raw(want["rid"])
        for fn, arg in FUNCS:
            name = f"{fn}_{arg}"
            assert got[name].data.is_cuda, name
            if fn == "avg":
                g, w = raw(got[name]), raw(want[name])
            else:
                assert got[name].dtype == DT
                g, w = decoded(got[name]), decoded(want[name])
            for j, rid in enumerate(order_w):
                gv, wv = g[order_g[rid]], w[j]
                if fn != "avg" or gv is None or wv is None:
                    assert gv == wv, (frame, name, rid, gv, wv)
                else:
                    assert abs(gv - wv) <= AVG_RTOL * abs(wv), \
                        (frame, name, rid, gv, wv)
        assert got["avg_x"].dtype == dtypes.float64
