"""DELTA_BYTE_ARRAY decode, host side: the two-stream page index, the
reference decoder that is the oracle for k_pq_dba_bytes, the checks that
stand between a corrupt page and the kernel, and the reader wiring on the
CPU path."""
import numpy as np
import pyarrow as pa
import pyarrow.parquet as pq
import pytest

import dba_payloads as dbp
from auron_amd import parquet_native
from auron_amd.column import RecordBatch


def _buf(raw: bytes, pad: int = 8) -> np.ndarray:
    return np.frombuffer(raw + b"\0" * pad, dtype=np.uint8).copy()


def _ref(pages):
    raw, descs = dbp.chunk(pages)
    buf = _buf(raw)
    pidx, sidx = parquet_native.delta_byte_array_index(buf, descs)
    ends = np.array([o + ln for o, ln, _n in descs], dtype=np.int64)
    return parquet_native.delta_byte_array_decode_ref(buf, pidx, sidx, ends)


@pytest.fixture(scope="module")
def payloads():
    return dbp.payload_set(parquet_native.dba_tile())


def test_ref_equals_encoder_input(payloads):
    assert len(payloads) > 15
    for name, strings, pages in payloads:
        data, offsets = _ref(pages)
        assert data.dtype == np.uint8 and offsets.dtype == np.int64, name
        want = np.cumsum([0] + [len(s) for s in strings])
        assert offsets.tolist() == want.tolist(), name
        assert data.tobytes() == b"".join(strings), name


def test_index_splits_a_page_into_its_two_streams():
    strings = dbp.sorted_strings(70, 1)
    page = dbp.encode(strings)
    buf = _buf(b"\xAA" * 3 + page)
    pidx, sidx = parquet_native.delta_byte_array_index(buf, [(3, len(page), 70)])
    plen = len(dbp.dp.encode(dbp.max_prefixes(strings), 128, 4, 4))
    assert pidx.pg[0, 2] == 3 + plen
    suffix_bytes = sum(len(s) - p
                       for s, p in zip(strings, dbp.max_prefixes(strings)))
    assert sidx.pg[0, 2] == 3 + len(page) - suffix_bytes
    assert pidx.total == sidx.total == 70


# ---------------------------------------------------------- corrupt payloads
def _page(prefixes, suffixes, data: bytes) -> bytes:
    return dbp.encode_raw(prefixes, suffixes, data)


@pytest.mark.parametrize("name,page", [
    ("first prefix not 0", _page([1, 0], [1, 2], b"bcd")),
    ("prefix longer than the previous string", _page([0, 5], [2, 1], b"abc")),
    ("negative prefix", _page([0, -1], [2, 2], b"abcd")),
    ("negative suffix", _page([0, 1], [3, -1], b"ab")),
    ("suffixes stop short of the page end", _page([0, 1], [2, 1], b"abcd")),
    ("suffixes run past the page end", _page([0, 1], [2, 3], b"abcd")),
])
def test_corrupt_lengths_raise(name, page):
    assert _ref([dbp.encode([b"ab", b"ac"])])[0].tobytes() == b"abac"
    with pytest.raises(ValueError, match="corrupt DELTA_BYTE_ARRAY"):
        _ref([page])


def test_corrupt_second_page_and_header_totals():
    good = dbp.encode([b"ab", b"ac"])
    # the check on P[i] <= L[i-1] runs across the page boundary
    _ref([good, _page([2, 1], [0, 1], b"x")])
    with pytest.raises(ValueError, match="corrupt DELTA_BYTE_ARRAY"):
        _ref([good, _page([3, 1], [0, 1], b"x")])
    # prefix stream of 2 values, suffix stream of 3
    bad = dbp.dp.encode([0, 1], 128, 4, 4) + dbp.dp.encode([2, 1, 0], 128, 4, 4) \
        + b"abc"
    buf = _buf(bad)
    with pytest.raises(ValueError, match="corrupt DELTA_BYTE_ARRAY"):
        parquet_native.delta_byte_array_index(buf, [(0, len(bad), 3)])


# ------------------------------------------------------- pyarrow-written files
@pytest.fixture(scope="module")
def table():
    return dbp.dba_table()


@pytest.mark.parametrize("codec", ["NONE", "snappy"])
@pytest.mark.parametrize("pv", ["1.0", "2.0"])
def test_pyarrow_files_cpu(tmp_path, table, pv, codec):
    p = str(tmp_path / "d.parquet")
    dbp.write_dba_file(table, p, pv, codec)
    md = pq.ParquetFile(p).metadata
    assert md.num_row_groups == 2
    assert "DELTA_BYTE_ARRAY" in md.row_group(0).column(0).encodings
    before = dict(parquet_native.STATS)
    cols = parquet_native.read_columns_native(p, ["s"], "cpu", _np_only=True)
    assert cols is not None and set(cols) == {"s"}
    want = RecordBatch.from_arrow(table).column("s")
    assert cols["s"].to_pylist() == want.to_pylist()
    assert cols["s"].to_pylist() == table["s"].to_pylist()
    meta = parquet_native._get_meta(p, ["s"])
    chunks = meta.cols[0].pages
    assert len(chunks) == 2 and all(len(ck.pages) > 1 for ck in chunks)
    assert {p_.encoding for ck in chunks for p_ in ck.pages} == {7}
    assert all(ck.delta_idx is not None and ck.delta_idx2 is not None
               for ck in chunks)
    # the all-NULL page and the all-"" page made it into the file
    assert chunks[0].delta_idx.pg[-1, 1] == 0
    assert chunks[0].pages[-1].row_start == 2816
    assert chunks[1].pages[-1].row_start == 4792 - 3000
    if codec == "NONE":
        assert meta.extra_total == 0 and not meta.jobs
    after = parquet_native.STATS
    assert after["delta_byte_array_strings"] \
        - before["delta_byte_array_strings"] \
        == len(table["s"]) - table["s"].null_count
    assert after["delta_length_strings"] == before["delta_length_strings"]


def test_all_null_chunk_and_required_column(tmp_path):
    t = pa.table({"s": pa.array([None] * 300, pa.string())})
    p = str(tmp_path / "nulls.parquet")
    dbp.write_dba_file(t, p, "2.0", "NONE")
    out = parquet_native.read_columns_native(p, ["s"], "cpu", _np_only=True)
    assert out["s"].to_pylist() == [None] * 300
    vals = [f"key-{i // 3:05d}" for i in range(700)]
    schema = pa.schema([pa.field("s", pa.string(), nullable=False)])
    t = pa.table({"s": pa.array(vals)}, schema=schema)
    p = str(tmp_path / "required.parquet")
    dbp.write_dba_file(t, p, "1.0", "snappy")
    out = parquet_native.read_columns_native(p, ["s"], "cpu", _np_only=True)
    assert out["s"].to_pylist() == vals and out["s"].validity is None


def test_flipped_suffix_length_in_a_file(tmp_path):
    """Flip one suffix-length delta inside the file: the suffixes of that
    page no longer add up to the bytes behind the two length streams."""
    vals = sorted(f"value-{i % 50}-{i}" for i in range(200))
    t = pa.table({"s": pa.array(vals)})
    p = str(tmp_path / "s.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="NONE",
                   column_encoding={"s": "DELTA_BYTE_ARRAY"})
    assert parquet_native.read_columns_native(
        p, ["s"], "cpu", _np_only=True)["s"].to_pylist() == vals
    meta = parquet_native._get_meta(p, ["s"])
    ck = meta.cols[0].pages[0]
    src, _clen, dst = meta.ranges[0]
    at = int(ck.delta_idx2.mb[0, 0]) - dst + src  # first packed-delta byte
    raw = bytearray(open(p, "rb").read())
    raw[at] ^= 0x01
    p2 = str(tmp_path / "bad.parquet")
    open(p2, "wb").write(bytes(raw))
    with pytest.raises(ValueError, match="corrupt DELTA_BYTE_ARRAY"):
        parquet_native.read_columns_native(p2, ["s"], "cpu", _np_only=True)


def test_switch_off_falls_back_to_pyarrow(tmp_path, table, monkeypatch):
    from auron_amd import AuronSession
    from auron_amd.plan import nodes as P

    t = table.append_column("k", pa.array(np.arange(len(table))))
    p = str(tmp_path / "d.parquet")
    dbp.write_dba_file(t, p, "2.0", "snappy")
    on = parquet_native.read_columns_native(p, ["s", "k"], "cpu",
                                            _np_only=True)
    assert set(on) == {"s", "k"}
    monkeypatch.setenv("AURON_SCAN_DELTA_NATIVE", "0")
    before = dict(parquet_native.STATS)
    off = parquet_native.read_columns_native(p, ["s", "k"], "cpu",
                                             _np_only=True)
    assert off is not None and set(off) == {"k"}
    out = AuronSession().collect(P.ParquetScan([p], columns=["s", "k"]))
    got = out.to_pydict()
    assert got["s"] == t["s"].to_pylist()
    assert got["k"] == t["k"].to_pylist()
    assert parquet_native.STATS["delta_byte_array_strings"] \
        == before["delta_byte_array_strings"]


def test_end_to_end_scan_with_list_fallback(tmp_path):
    from auron_amd import AuronSession
    from auron_amd.plan import nodes as P

    n = 1200
    rng = np.random.default_rng(31)
    t = pa.table({
        "k": pa.array(np.cumsum(rng.integers(0, 9, n)), mask=rng.random(n) < .1),
        "s": pa.array([None if i % 7 == 0 else f"row-{i // 5:04d}-é{i % 5}"
                       for i in range(n)]),
        "lst": pa.array([[i, i + 1] for i in range(n)]),
    })
    p = str(tmp_path / "e2e.parquet")
    pq.write_table(t, p, use_dictionary=False, compression="snappy",
                   column_encoding={"k": "DELTA_BINARY_PACKED",
                                    "s": "DELTA_BYTE_ARRAY"})
    ok, rest = parquet_native.split_supported(p, ["k", "s", "lst"])
    assert ok == ["k", "s"] and rest == ["lst"]
    before = dict(parquet_native.STATS)
    out = AuronSession().collect(P.ParquetScan([p], columns=["k", "s", "lst"]))
    got = out.to_pydict()
    assert got["k"] == t["k"].to_pylist()
    assert got["s"] == t["s"].to_pylist()
    assert got["lst"] == t["lst"].to_pylist()
    after = parquet_native.STATS
    assert after["delta_byte_array_strings"] \
        - before["delta_byte_array_strings"] == n - t["s"].null_count
    moved = (after["delta_values_host"] - before["delta_values_host"]
             + after["delta_values_device"] - before["delta_values_device"])
    assert moved == n - t["k"].null_count
