"""DELTA_BINARY_PACKED / DELTA_LENGTH_BYTE_ARRAY decode, host side: the
miniblock index (au_host_delta_index), the numpy reference decoder that is
the oracle for the kernels, and the reader wiring on the CPU path."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import delta_payloads as dp
from auron_amd import native, parquet_native
from auron_amd.column import RecordBatch


@pytest.fixture(scope="module")
def payloads():
    return dp.payload_set()


def _as_np(vals, esize):
    return np.array(vals, dtype=np.int32 if esize == 4 else np.int64)


def _buf(raw: bytes, pad: int = 8) -> np.ndarray:
    return np.frombuffer(raw + b"\0" * pad, dtype=np.uint8).copy()


def test_delta_index_exists():
    assert callable(getattr(parquet_native, "delta_index", None))
    assert hasattr(native.host_lib(), "au_host_delta_index")


def test_ref_equals_encoder_input(payloads):
    assert len(payloads) > 150
    for name, vals, esize, raw in payloads:
        buf = _buf(raw)
        idx = parquet_native.delta_index(buf, [(0, len(raw), len(vals))])
        assert idx.total == len(vals), name
        got = parquet_native.delta_decode_ref(buf, idx, esize)
        assert got.dtype == (np.int32 if esize == 4 else np.int64), name
        assert np.array_equal(got, _as_np(vals, esize)), name


def test_payload_set_covers_the_listed_bit_widths(payloads):
    """The encoder really produced every width the set is meant to hold."""
    seen = {8: set(), 4: set()}
    for name, vals, esize, raw in payloads:
        buf = _buf(raw)
        idx = parquet_native.delta_index(buf, [(0, len(raw), len(vals))])
        seen[esize] |= set(idx.mb_fields()[0].tolist())
    assert set(dp.BIT_WIDTHS) <= seen[8]
    assert {b for b in dp.BIT_WIDTHS if b <= 32} <= seen[4]


def test_ref_equals_host_unpack(payloads):
    lib = native.host_lib()
    for name, vals, esize, raw in payloads:
        buf = _buf(raw)
        idx = parquet_native.delta_index(buf, [(0, len(raw), len(vals))])
        ref = parquet_native.delta_decode_ref(buf, idx, esize)
        out = np.zeros(max(len(vals), 1) * esize, dtype=np.uint8)
        got = lib.au_host_delta_unpack(buf.ctypes.data, 0, len(raw),
                                       len(vals), esize, out.ctypes.data)
        assert got == len(vals), name
        host = out[:got * esize].view(ref.dtype)
        assert np.array_equal(ref, host), name


def test_index_descriptors():
    """First value, total, stream end and per-miniblock fields of a known
    payload: 65 values in 128/4 -> 64 deltas = two full 32-value
    miniblocks, two unused ones with junk widths that must be skipped."""
    vals = dp.values_with_width(65, 7, 8, 3)
    raw = dp.encode(vals, 128, 4, 8, junk_unused=True)
    buf = _buf(b"\xAA" * 5 + raw)
    idx = parquet_native.delta_index(buf, [(5, len(raw), 70)])
    assert idx.pg[0].tolist() == [vals[0], 65, 5 + len(raw), 0, 0]
    bw, cnt, page = idx.mb_fields()
    assert bw.tolist() == [7, 7] and cnt.tolist() == [32, 32]
    assert page.tolist() == [0, 0]
    assert idx.mb[:, 2].tolist() == [1, 33]
    assert idx.mb[1, 0] - idx.mb[0, 0] == 32 * 7 // 8
    assert idx.last_byte == 5 + len(raw)
    # a short last miniblock counts only the values it holds
    vals = dp.values_with_width(40, 9, 8, 4)
    raw = dp.encode(vals, 128, 4, 8)
    idx = parquet_native.delta_index(_buf(raw), [(0, len(raw), 40)])
    assert idx.mb_fields()[1].tolist() == [32, 7]
    assert idx.pg[0, 2] == len(raw)  # padded to the nominal size
    assert idx.last_byte == idx.mb[1, 0] + (7 * 9 + 7) // 8


def test_multi_page_chunk():
    for name, esize, pages in dp.multi_page_chunks():
        raw = b"".join(b for _v, b in pages)
        descs, off, want = [], 0, []
        for vals, b in pages:
            descs.append((off, len(b), len(vals) + 3))
            off += len(b)
            want += vals
        buf = _buf(raw)
        idx = parquet_native.delta_index(buf, descs)
        assert idx.pg[:, 1].tolist() == [len(v) for v, _b in pages], name
        got = parquet_native.delta_decode_ref(buf, idx, esize)
        assert np.array_equal(got, _as_np(want, esize)), name


# ---------------------------------------------------------- corrupt payloads
def test_corrupt_payloads_raise():
    vals = dp.values_with_width(65, 11, 8, 9)  # 64 deltas: one full miniblock
    raw = dp.encode(vals, 256, 4, 8)
    buf = _buf(raw)
    parquet_native.delta_index(buf, [(0, len(raw), 65)])  # sane as written
    with pytest.raises(ValueError):  # cut one byte short
        parquet_native.delta_index(buf, [(0, len(raw) - 1, 65)])
    with pytest.raises(ValueError):  # total above the page's rows
        parquet_native.delta_index(buf, [(0, len(raw), 64)])
    with pytest.raises(ValueError):  # header runs past the payload
        parquet_native.delta_index(buf, [(0, 3, 65)])
    # bit width 65 on the miniblock that holds the values
    hdr = len(dp.encode(vals[:1], 256, 4, 8))
    pos = hdr
    while raw[pos] & 0x80:  # skip the min_delta varint
        pos += 1
    pos += 1
    assert raw[pos] == 11
    bad = bytearray(raw)
    bad[pos] = 65
    with pytest.raises(ValueError):
        parquet_native.delta_index(_buf(bytes(bad) + b"\0" * 600),
                                   [(0, len(raw) + 600, 65)])
    # the same byte on an unused miniblock is fine
    ok = bytearray(raw)
    ok[pos + 1] = 65
    idx = parquet_native.delta_index(_buf(bytes(ok)), [(0, len(raw), 65)])
    assert np.array_equal(
        parquet_native.delta_decode_ref(_buf(bytes(ok)), idx, 8),
        _as_np(vals, 8))
    # block size not a multiple of the miniblock count / of 32 values
    for block, minis in ((130, 4), (64, 4)):
        hdr_bad = dp._uvarint(block) + dp._uvarint(minis) + raw[3:]
        assert raw[:3] == dp._uvarint(256) + dp._uvarint(4)
        with pytest.raises(ValueError):
            parquet_native.delta_index(_buf(hdr_bad), [(0, len(hdr_bad), 65)])


# ------------------------------------------------------- pyarrow-written files
@pytest.fixture(scope="module")
def table():
    return dp.delta_table()


def _check(cols, t):
    want = RecordBatch.from_arrow(t)
    assert set(cols) == set(t.schema.names)
    for name in t.schema.names:
        assert cols[name].to_pylist() == want.column(name).to_pylist(), name


@pytest.mark.parametrize("codec", ["NONE", "snappy"])
@pytest.mark.parametrize("pv", ["1.0", "2.0"])
def test_pyarrow_files_cpu(tmp_path, table, pv, codec):
    p = str(tmp_path / "d.parquet")
    dp.write_delta_file(table, p, pv, codec)
    md = pq.ParquetFile(p).metadata
    assert md.num_row_groups == 2
    for ci in range(md.num_columns):
        encs = md.row_group(0).column(ci).encodings
        want = "DELTA_LENGTH_BYTE_ARRAY" if ci == 4 else "DELTA_BINARY_PACKED"
        assert want in encs, (ci, encs)
    names = table.schema.names
    before = dict(parquet_native.STATS)
    cols = parquet_native.read_columns_native(p, names, "cpu", _np_only=True)
    assert cols is not None
    _check(cols, table)
    meta = parquet_native._get_meta(p, names)
    assert [c.name for c in meta.cols] == names
    for cm in meta.cols:
        assert len(cm.pages) == 2
        assert all(len(ck.pages) > 1 for ck in cm.pages), cm.name
        assert all(ck.delta_idx is not None for ck in cm.pages)
    s_pages = meta.cols[4].pages
    assert {p_.encoding for ck in s_pages for p_ in ck.pages} == {6}
    # the all-NULL page and the all-"" page made it into the file
    assert s_pages[0].delta_idx.pg[-1, 1] == 0
    assert s_pages[0].pages[-1].row_start == 2816
    assert s_pages[1].pages[-1].row_start == 4792 - 3000
    assert not any(j[0] == "delta" for j in meta.jobs)
    if codec == "NONE":
        assert meta.extra_total == 0 and not meta.jobs
    present = sum(len(table[c]) - table[c].null_count for c in dp.INT_COLS)
    after = parquet_native.STATS
    assert after["delta_values_host"] - before["delta_values_host"] == present
    assert after["delta_values_device"] == before["delta_values_device"]
    assert after["delta_length_strings"] - before["delta_length_strings"] \
        == len(table["s"]) - table["s"].null_count


def test_delta_length_strings_are_native(tmp_path):
    vals = ["", "é", "x" * 300, None, "tail"] * 40
    t = pa.table({"s": pa.array(vals)})
    p = str(tmp_path / "s.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="NONE",
                   column_encoding={"s": "DELTA_LENGTH_BYTE_ARRAY"})
    out = parquet_native.read_columns_native(p, ["s"], "cpu", _np_only=True)
    assert out is not None
    assert out["s"].to_pylist() == vals


def test_string_lengths_must_fill_the_page(tmp_path):
    """Flip one length delta inside the file: the lengths of that page no
    longer add up to the bytes behind the length stream."""
    vals = [f"value-{i}" * (1 + i % 3) for i in range(200)]
    t = pa.table({"s": pa.array(vals)})
    p = str(tmp_path / "s.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="NONE",
                   column_encoding={"s": "DELTA_LENGTH_BYTE_ARRAY"})
    assert parquet_native.read_columns_native(
        p, ["s"], "cpu", _np_only=True)["s"].to_pylist() == vals
    meta = parquet_native._get_meta(p, ["s"])
    ck = meta.cols[0].pages[0]
    src, _clen, dst = meta.ranges[0]
    at = int(ck.delta_idx.mb[0, 0]) - dst + src  # first packed-delta byte
    raw = bytearray(open(p, "rb").read())
    raw[at] ^= 0x01
    p2 = str(tmp_path / "bad.parquet")
    open(p2, "wb").write(bytes(raw))
    with pytest.raises(ValueError):
        parquet_native.read_columns_native(p2, ["s"], "cpu", _np_only=True)


def test_switch_off_restores_host_paths(tmp_path, table, monkeypatch):
    p = str(tmp_path / "d.parquet")
    dp.write_delta_file(table, p, "1.0", "NONE")
    names = table.schema.names
    on = parquet_native.read_columns_native(p, names, "cpu", _np_only=True)
    monkeypatch.setenv("AURON_SCAN_DELTA_NATIVE", "0")
    off = parquet_native.read_columns_native(p, names, "cpu", _np_only=True)
    assert off is not None and "s" not in off
    assert set(off) == set(dp.INT_COLS)
    for c in dp.INT_COLS:
        assert off[c].to_pylist() == on[c].to_pylist(), c
    meta = parquet_native._get_meta(p, names)
    assert any(j[0] == "delta" for j in meta.jobs) and meta.extra_total > 0
    monkeypatch.setenv("AURON_SCAN_DELTA_NATIVE", "1")
    again = parquet_native.read_columns_native(p, names, "cpu", _np_only=True)
    assert "s" in again  # the parse of the other setting was not reused


def test_end_to_end_scan_with_list_fallback(tmp_path):
    from auron_amd import AuronSession
    from auron_amd.plan import nodes as P

    n = 1200
    rng = np.random.default_rng(23)
    t = pa.table({
        "k": pa.array(np.cumsum(rng.integers(0, 9, n)), mask=rng.random(n) < .1),
        "s": pa.array([None if i % 7 == 0 else f"row-{i}-é" for i in range(n)]),
        "lst": pa.array([[i, i + 1] for i in range(n)]),
    })
    p = str(tmp_path / "e2e.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="snappy",
                   column_encoding={"k": "DELTA_BINARY_PACKED",
                                    "s": "DELTA_LENGTH_BYTE_ARRAY"})
    ok, rest = parquet_native.split_supported(p, ["k", "s", "lst"])
    assert ok == ["k", "s"] and rest == ["lst"]
    before = dict(parquet_native.STATS)
    out = AuronSession().collect(P.ParquetScan([p], columns=["k", "s", "lst"]))
    got = out.to_pydict()
    assert got["k"] == t["k"].to_pylist()
    assert got["s"] == t["s"].to_pylist()
    assert got["lst"] == t["lst"].to_pylist()
    after = parquet_native.STATS
    assert after["delta_length_strings"] - before["delta_length_strings"] \
        == n - t["s"].null_count
    moved = (after["delta_values_host"] - before["delta_values_host"]
             + after["delta_values_device"] - before["delta_values_device"])
    assert moved == n - t["k"].null_count
