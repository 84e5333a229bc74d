"""gfx950 range-bucket kernels (csrc/rangepart.hip) against the CPU
reference, exactly; plus the string-key external sort end to end on the
device."""
import pytest
import torch

from auron_amd import dtypes, ops
from auron_amd.column import Column

from test_external_sort_wide_keys import _rids, run_sort, string_batches
from test_range_bucket import (i128_bounds, i128_column, i128_values,
                               slice_view, string_bounds, string_values)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = (10_000, 1, 63, 64, 65, 257)
BOUND_COUNTS = (0, 1, 2, 7, 64, 300)


def _check(key_cpu: Column, bounds_cpu: Column):
    key_gpu, bounds_gpu = key_cpu.to(DEV), bounds_cpu.to(DEV)
    for right in (False, True):
        want = ops.range_bucket_ref(key_cpu, bounds_cpu, right)
        got = ops.range_bucket(key_gpu, bounds_gpu, right)
        assert got.dtype == torch.int64 and got.device.type == "cuda"
        assert torch.equal(got.cpu(), want), (len(key_cpu), len(bounds_cpu), right)


@pytest.mark.parametrize("n", SIZES)
def test_string_kernel_matches_reference(n):
    values = string_values(n, seed=n, distinct=400)
    key = Column.from_pylist(values, dtypes.string)
    pool_rows = string_values(2000, seed=7, null_frac=0.0, distinct=400)
    for nb in BOUND_COUNTS:
        # bounds from the rows themselves (equal to rows) and from the wider
        # value set when there are too few rows to fill them
        src = values if n >= nb else pool_rows
        bounds = string_bounds(src, nb, seed=nb)
        _check(key, Column.from_pylist(bounds, dtypes.string))


def test_string_kernel_sliced_key():
    values = string_values(1000, seed=3, distinct=400)
    key = Column.from_pylist(values, dtypes.string)
    sl = slice_view(key, 3, 990)
    assert int(sl.offsets[0]) != 0
    for nb in (1, 7, 64):
        _check(sl, Column.from_pylist(string_bounds(values, nb, seed=nb),
                                      dtypes.string))


def test_string_kernel_row_ends_at_buffer_end():
    """Last row and last bound end at the final byte of their buffers with
    a length that is no multiple of 8: the word loop must stop short."""
    tail = "abcdefghijk"  # 11 bytes
    values = string_values(300, seed=9, null_frac=0.0) + [tail + "l", tail]
    bounds = sorted(["abcdefgh", tail, tail, tail + "l", "abcdefghijkm"],
                    key=lambda s: s.encode("utf-8"))
    key = Column.from_pylist(values, dtypes.string)
    bcol = Column.from_pylist(bounds, dtypes.string)
    assert int(key.offsets[-1]) == key.data.numel()
    assert (int(key.offsets[-1]) - int(key.offsets[-2])) % 8 != 0
    assert int(bcol.offsets[-1]) == bcol.data.numel()
    _check(key, bcol)


@pytest.mark.parametrize("n", SIZES)
def test_decimal128_kernel_matches_reference(n):
    vals, valid = i128_values(n, seed=n)
    key = i128_column(vals, valid)
    wide, _ = i128_values(2000, seed=5)
    for nb in BOUND_COUNTS:
        bounds = i128_bounds(vals if n >= nb else wide, nb, seed=nb)
        _check(key, i128_column(bounds))
    if n > 8:
        _check(slice_view(key, 3, n - 2), i128_column(i128_bounds(vals, 7, 1)))


def test_string_external_sort_on_device_matches_cpu():
    for asc in (True, False):
        out, ctx = run_sort(string_batches(device=DEV), asc, device=DEV)
        assert ctx.metrics.get("sort.external_buckets", 0) > 0
        assert len(out) > 1 and out[0].device.type == "cuda"
        want, _ = run_sort(string_batches(), asc)
        assert _rids(out) == _rids(want)
