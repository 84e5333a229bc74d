#!/usr/bin/env python3
"""A/B the DELTA_BYTE_ARRAY string scan: spark.auron.scan.deltaNative.enable
off (pyarrow host read of the column, Arrow -> torch, upload) vs on
(k_pq_delta_* lengths + k_pq_dba_bytes), in one process and one build,
alternating the two settings.

Input: a generated file with one DELTA_BYTE_ARRAY string column of sorted,
prefix-heavy URL-like keys (47 bytes each), pyarrow's default page size and
compression, row groups of 2^20 rows. Each timed read starts with the
staged-bytes cache cleared and is timed on the host clock from the call to
torch.cuda.synchronize(); the file stays in the OS page cache. The off
setting reads the column through pyarrow the way the executor's per-column
fallback does. --segs also times the on setting at other values per wave
than DBA_SEG_VALUES.

  python profiles/measure_dba_scan.py --rows 4000000 --reps 10 --out result.json
  python profiles/measure_dba_scan.py --profile on   # one setting, for rocprofv3
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

import numpy as np
import pyarrow as pa
import pyarrow.compute as pc
import pyarrow.parquet as pq
import torch

from auron_amd import parquet_native
from auron_amd.column import RecordBatch

COLS = ["s"]


def write_file(path: str, rows: int) -> None:
    rng = np.random.default_rng(1)
    keys = np.sort(rng.integers(0, 10 ** 12, rows))
    d = pc.utf8_lpad(pc.cast(pa.array(keys), pa.string()), 12, "0")
    s = pc.binary_join_element_wise(
        "https://example.org/catalog/", pc.utf8_slice_codeunits(d, 0, 4), "/",
        pc.utf8_slice_codeunits(d, 4, 8), "/item-",
        pc.utf8_slice_codeunits(d, 8, 12), "")
    pq.write_table(pa.table({"s": s}), path, use_dictionary=False,
                   column_encoding={"s": "DELTA_BYTE_ARRAY"},
                   row_group_size=1 << 20)


def read(path: str, dev: str):
    """What the executor's ParquetScan does for this column."""
    got = parquet_native.read_columns_native(path, COLS, dev) or {}
    missing = [c for c in COLS if c not in got]
    if missing:
        hb = RecordBatch.from_arrow(pq.read_table(path, columns=missing), dev)
        for n, c in zip(hb.names, hb.columns):
            got[n] = c
    return got


def timed(path: str, dev: str, setting: str) -> float:
    os.environ["AURON_SCAN_DELTA_NATIVE"] = "1" if setting == "on" else "0"
    parquet_native.dbuf_cache_clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    read(path, dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def summary(v):
    return {"median_ms": statistics.median(v), "min_ms": min(v),
            "max_ms": max(v), "all_ms": [round(x, 2) for x in v]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--segs", default="64,1024",
                    help="further values per wave to time the on setting at")
    ap.add_argument("--out", default="")
    ap.add_argument("--profile", choices=["on", "off"], default="",
                    help="three reads of one setting, for rocprofv3")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    default_seg = parquet_native.DBA_SEG_VALUES
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "dba.parquet")
        write_file(path, args.rows)
        if args.profile:
            for _ in range(3):
                timed(path, dev, args.profile)
            return
        for setting in ("off", "on", "off", "on"):  # warm both
            timed(path, dev, setting)
        before = parquet_native.STATS["delta_byte_array_strings"]
        on = read(path, dev)["s"]
        assert parquet_native.STATS["delta_byte_array_strings"] - before \
            == args.rows, "the on setting did not take the device path"
        os.environ["AURON_SCAN_DELTA_NATIVE"] = "0"
        off = read(path, dev)["s"]
        # faster and different is not faster
        assert torch.equal(on.data, off.data)
        assert torch.equal(on.offsets, off.offsets.to(on.offsets.dtype))
        ms = {"off": [], "on": []}
        for _ in range(args.reps):
            for setting in ("off", "on"):
                ms[setting].append(timed(path, dev, setting))
        md = pq.ParquetFile(path).metadata
        res = {"rows": args.rows, "reps": args.reps,
               "file_bytes": os.path.getsize(path),
               "string_bytes": int(on.data.numel()),
               "row_groups": md.num_row_groups,
               "compression": md.row_group(0).column(0).compression,
               "dba_seg_values": default_seg,
               "dba_tile": parquet_native.dba_tile(),
               "off": summary(ms["off"]), "on": summary(ms["on"])}
        for seg in [int(x) for x in args.segs.split(",") if x]:
            parquet_native.DBA_SEG_VALUES = seg
            timed(path, dev, "on")
            got = read(path, dev)["s"]
            assert torch.equal(got.data, on.data)
            res[f"on_seg{seg}"] = summary(
                [timed(path, dev, "on") for _ in range(args.reps)])
        parquet_native.DBA_SEG_VALUES = default_seg
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
