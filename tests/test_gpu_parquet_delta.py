"""DELTA_BINARY_PACKED / DELTA_LENGTH_BYTE_ARRAY decode on the device: the
k_pq_delta_* kernels against the numpy reference over the payload set, and
the reader wiring (counters, staged-bytes cache, switch) on cuda."""
import random

import numpy as np
import pytest
import torch

import delta_payloads as dp
from auron_amd import native, parquet_native
from auron_amd.column import RecordBatch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def _upload(raw: bytes, pad: int = 8):
    """Host copy and device copy of `raw` with exactly `pad` tail bytes."""
    buf = np.frombuffer(raw + b"\0" * pad, dtype=np.uint8).copy()
    return buf, torch.from_numpy(buf).to(DEV)


def _decode_both(raw, descs, esize):
    buf, dbuf = _upload(raw)
    assert dbuf.numel() == len(raw) + 8
    idx = parquet_native.delta_index(buf, descs)
    ref = parquet_native.delta_decode_ref(buf, idx, esize)
    got = parquet_native.delta_decode(dbuf, idx, esize, DEV)
    assert got.dtype == (torch.int32 if esize == 4 else torch.int64)
    assert got.device == torch.device(DEV)
    assert got.shape == (idx.total,)
    return ref, got


def test_kernels_equal_reference_over_payload_set():
    native.require()
    pending = []
    for name, vals, esize, raw in dp.payload_set():
        ref, got = _decode_both(raw, [(0, len(raw), len(vals))], esize)
        pending.append((name, ref, got))
    for name, ref, got in pending:
        assert np.array_equal(got.cpu().numpy(), ref), name


def test_kernels_multi_page_chunk():
    for name, esize, pages in dp.multi_page_chunks():
        raw = b"".join(b for _v, b in pages)
        descs, off, want = [], 0, []
        for vals, b in pages:
            descs.append((off, len(b), len(vals)))
            off += len(b)
            want += vals
        ref, got = _decode_both(raw, descs, esize)
        assert ref.tolist() == want, name
        assert np.array_equal(got.cpu().numpy(), ref), name


def test_kernels_many_miniblocks():
    """More than 8192 miniblocks: the sums/emit grids (2048 blocks of four
    waves) stride, and the base scan runs several 2048-entry rounds with a
    carry between them."""
    rng = random.Random(77)
    n = 8192 * 32 + 1000
    vals, v = [], 0
    for _ in range(n):
        vals.append(v)
        v = dp.wrap(v + rng.randint(-(1 << 40), 1 << 41), 8)
    raw = dp.encode(vals, 128, 4, 8)
    ref, got = _decode_both(raw, [(0, len(raw), n)], 8)
    assert np.array_equal(ref, np.array(vals, dtype=np.int64))
    assert torch.equal(got.cpu(), torch.from_numpy(ref))


def test_decode_refuses_a_buffer_without_tail_pad():
    vals = dp.values_with_width(65, 33, 8, 5)
    raw = dp.encode(vals, 256, 4, 8)
    buf, dbuf = _upload(raw, pad=7)
    idx = parquet_native.delta_index(buf, [(0, len(raw), 65)])
    with pytest.raises(ValueError):
        parquet_native.delta_decode(dbuf, idx, 8, DEV)


# ------------------------------------------------------- pyarrow-written files
@pytest.fixture(scope="module")
def table():
    return dp.delta_table()


def _check(cols, t):
    want = RecordBatch.from_arrow(t)
    assert set(cols) == set(t.schema.names)
    for name in t.schema.names:
        c = cols[name]
        assert c.data.is_cuda, name
        assert c.validity is None or c.validity.is_cuda, name
        assert c.offsets is None or c.offsets.is_cuda, name
        assert c.to("cpu").to_pylist() == want.column(name).to_pylist(), name


@pytest.mark.parametrize("codec", ["NONE", "snappy"])
@pytest.mark.parametrize("pv", ["1.0", "2.0"])
def test_pyarrow_files_gpu(tmp_path, table, pv, codec):
    p = str(tmp_path / "d.parquet")
    dp.write_delta_file(table, p, pv, codec)
    names = table.schema.names
    cols = parquet_native.read_columns_native(p, names, "cuda")
    assert cols is not None
    _check(cols, table)
    meta = parquet_native._get_meta(p, names)
    assert not any(j[0] == "delta" for j in meta.jobs)
    if codec == "NONE":
        assert meta.extra_total == 0 and not meta.jobs
    # the parsed form is shared with CPU reads of the same path
    ref = parquet_native.read_columns_native(p, names, "cpu", _np_only=True)
    for name in names:
        assert ref[name].to_pylist() == cols[name].to("cpu").to_pylist()


def test_counters_cache_and_switch(tmp_path, table, monkeypatch):
    p = str(tmp_path / "d.parquet")
    dp.write_delta_file(table, p, "2.0", "snappy")
    names = table.schema.names
    present = sum(len(table[c]) - table[c].null_count for c in dp.INT_COLS)
    strings = len(table["s"]) - table["s"].null_count
    stats = parquet_native.STATS

    s0 = dict(stats)
    first = parquet_native.read_columns_native(p, names, "cuda")
    _check(first, table)
    assert stats["delta_values_device"] - s0["delta_values_device"] == present
    assert stats["delta_values_host"] == s0["delta_values_host"]
    assert stats["delta_length_strings"] - s0["delta_length_strings"] == strings

    # second read: staged bytes come from the HBM cache, no host buffer
    key = (p, parquet_native.os.path.getmtime(p), tuple(names), True)
    assert parquet_native._dbuf_cache_get(key) is not None
    s1 = dict(stats)
    second = parquet_native.read_columns_native(p, names, "cuda")
    _check(second, table)
    assert stats["delta_values_device"] - s1["delta_values_device"] == present
    assert stats["delta_values_host"] == s1["delta_values_host"]

    monkeypatch.setenv("AURON_SCAN_DELTA_NATIVE", "0")
    s2 = dict(stats)
    off = parquet_native.read_columns_native(p, names, "cuda")
    assert off is not None and set(off) == set(dp.INT_COLS)
    for c in dp.INT_COLS:
        assert off[c].data.is_cuda
        assert off[c].to("cpu").to_pylist() == first[c].to("cpu").to_pylist()
    assert stats["delta_values_host"] - s2["delta_values_host"] == present
    assert stats["delta_values_device"] == s2["delta_values_device"]
    assert stats["delta_length_strings"] == s2["delta_length_strings"]
