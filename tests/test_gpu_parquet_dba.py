"""DELTA_BYTE_ARRAY decode on the device: k_pq_dba_bytes against the host
reference over the payload set at several segment sizes, and the reader
wiring (pyarrow files, counters, staged-bytes cache) on cuda."""
import numpy as np
import pytest
import torch

import dba_payloads as dbp
from auron_amd import native, parquet_native
from auron_amd.column import RecordBatch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SEGS = [1, 3, 64, None]  # None = DBA_SEG_VALUES


def _stage(pages):
    raw, descs = dbp.chunk(pages)
    buf = np.frombuffer(raw + b"\0" * 8, dtype=np.uint8).copy()
    pidx, sidx = parquet_native.delta_byte_array_index(buf, descs)
    ends = np.array([o + ln for o, ln, _n in descs], dtype=np.int64)
    return buf, torch.from_numpy(buf).to(DEV), pidx, sidx, ends


@pytest.fixture(scope="module")
def staged():
    """[(name, device bytes, indexes, page ends, reference)], the reference
    computed once per payload."""
    native.require()
    out = []
    for name, _strings, pages in dbp.payload_set(parquet_native.dba_tile()):
        buf, dbuf, pidx, sidx, ends = _stage(pages)
        ref = parquet_native.delta_byte_array_decode_ref(buf, pidx, sidx, ends)
        out.append((name, dbuf, pidx, sidx, ends, ref))
    return out


@pytest.mark.parametrize("seg", SEGS)
def test_kernel_equals_reference_over_payload_set(staged, seg):
    assert len(staged) > 15
    pending = []
    for name, dbuf, pidx, sidx, ends, ref in staged:
        data, offsets = parquet_native.delta_byte_array_decode(
            dbuf, pidx, sidx, ends, DEV, seg=seg)
        assert data.dtype == torch.uint8 and offsets.dtype == torch.int64
        assert data.device == offsets.device == torch.device(DEV)
        pending.append((name, data, offsets, ref))
    for name, data, offsets, (rdata, roffsets) in pending:
        assert offsets.cpu().numpy().tolist() == roffsets.tolist(), name
        assert np.array_equal(data.cpu().numpy(), rdata), name


def test_grid_strides_over_segments():
    """More segments than the 2048 x 4 waves of the largest grid."""
    n = 2048 * 4 * 2 + 100
    strings = [b"%05d" % (i // 3) for i in range(n)]
    buf, dbuf, pidx, sidx, ends = _stage([dbp.encode(strings)])
    rdata, roffsets = parquet_native.delta_byte_array_decode_ref(
        buf, pidx, sidx, ends)
    assert rdata.tobytes() == b"".join(strings)
    data, offsets = parquet_native.delta_byte_array_decode(
        dbuf, pidx, sidx, ends, DEV, seg=1)
    assert torch.equal(offsets.cpu(), torch.from_numpy(roffsets))
    assert torch.equal(data.cpu(), torch.from_numpy(rdata))


def test_corrupt_payload_raises_before_any_launch():
    """The lengths are checked on the device and read back in the one sync;
    the byte kernel never sees them."""
    page = dbp.encode_raw([0, 5], [2, 1], b"abc")  # prefix 5 of a 2-byte string
    _buf, dbuf, pidx, sidx, ends = _stage([page])
    with pytest.raises(ValueError, match="corrupt DELTA_BYTE_ARRAY"):
        parquet_native.delta_byte_array_decode(dbuf, pidx, sidx, ends, DEV)
    page = dbp.encode_raw([0, 1], [2, 1], b"abcd")  # one byte left over
    _buf, dbuf, pidx, sidx, ends = _stage([page])
    with pytest.raises(ValueError, match="corrupt DELTA_BYTE_ARRAY"):
        parquet_native.delta_byte_array_decode(dbuf, pidx, sidx, ends, DEV)


# ------------------------------------------------------- pyarrow-written files
@pytest.fixture(scope="module")
def table():
    return dbp.dba_table()


def _check(col, t):
    assert col.data.is_cuda and col.offsets.is_cuda
    assert col.validity is None or col.validity.is_cuda
    want = RecordBatch.from_arrow(t).column("s")
    assert col.to("cpu").to_pylist() == want.to_pylist()


@pytest.mark.parametrize("codec", ["NONE", "snappy"])
@pytest.mark.parametrize("pv", ["1.0", "2.0"])
def test_pyarrow_files_gpu(tmp_path, table, pv, codec):
    p = str(tmp_path / "d.parquet")
    dbp.write_dba_file(table, p, pv, codec)
    cols = parquet_native.read_columns_native(p, ["s"], "cuda")
    assert cols is not None and set(cols) == {"s"}
    _check(cols["s"], table)
    assert cols["s"].to("cpu").to_pylist() == table["s"].to_pylist()
    # the parsed form is shared with CPU reads of the same path
    ref = parquet_native.read_columns_native(p, ["s"], "cpu", _np_only=True)
    got = cols["s"].to("cpu")
    assert torch.equal(got.data, ref["s"].data)
    assert torch.equal(got.offsets, ref["s"].offsets)
    assert ref["s"].to_pylist() == got.to_pylist()


def test_counters_and_staged_bytes_cache(tmp_path, table, monkeypatch):
    p = str(tmp_path / "d.parquet")
    dbp.write_dba_file(table, p, "2.0", "snappy")
    strings = len(table["s"]) - table["s"].null_count
    stats = parquet_native.STATS

    s0 = dict(stats)
    first = parquet_native.read_columns_native(p, ["s"], "cuda")
    _check(first["s"], table)
    assert stats["delta_byte_array_strings"] \
        - s0["delta_byte_array_strings"] == strings

    # second read: staged bytes come from the HBM cache, no host buffer
    key = (p, parquet_native.os.path.getmtime(p), ("s",), True)
    assert parquet_native._dbuf_cache_get(key) is not None

    def no_host_buffer(*a, **k):
        raise AssertionError("a cache hit must not map the file")

    monkeypatch.setattr(parquet_native.np, "memmap", no_host_buffer)
    s1 = dict(stats)
    second = parquet_native.read_columns_native(p, ["s"], "cuda")
    _check(second["s"], table)
    assert stats["delta_byte_array_strings"] \
        - s1["delta_byte_array_strings"] == strings


def test_all_null_chunk_launches_nothing(tmp_path):
    import pyarrow as pa

    t = pa.table({"s": pa.array([None] * 300, pa.string())})
    p = str(tmp_path / "nulls.parquet")
    dbp.write_dba_file(t, p, "2.0", "NONE")
    col = parquet_native.read_columns_native(p, ["s"], "cuda")["s"]
    assert col.data.numel() == 0
    assert col.to("cpu").to_pylist() == [None] * 300
