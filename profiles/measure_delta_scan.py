#!/usr/bin/env python3
"""A/B the delta-page scan: spark.auron.scan.deltaNative.enable off
(host delta unpack + pyarrow strings) vs on (k_pq_delta_* kernels), in one
process and one build, alternating the two settings.

Input: a generated file with four DELTA_BINARY_PACKED int64 columns (one
sorted, one 20-bit random, one 40-bit random, one with 10% nulls) and one
DELTA_LENGTH_BYTE_ARRAY string column, snappy. Each timed read starts with
the staged-bytes cache cleared and is timed on the host clock from the
call to torch.cuda.synchronize(). The off setting reads the string column
through pyarrow the way the executor's per-column fallback does.

  python profiles/measure_delta_scan.py --rows 16000000 --reps 10 --out result.json
  python profiles/measure_delta_scan.py --profile on   # one setting, for rocprofv3
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

COLS = ["sorted", "r20", "r40", "nulls", "s"]


def write_file(path: str, rows: int) -> None:
    rng = np.random.default_rng(1)
    t = pa.table({
        "sorted": pa.array(np.cumsum(rng.integers(0, 1000, rows))),
        "r20": pa.array(rng.integers(0, 1 << 20, rows)),
        "r40": pa.array(rng.integers(0, 1 << 40, rows)),
        "nulls": pa.array(rng.integers(0, 1 << 30, rows),
                          mask=rng.random(rows) < 0.10),
        "s": pc.cast(pa.array(rng.integers(0, 10 ** 9, rows)), pa.string()),
    })
    enc = {c: "DELTA_BINARY_PACKED" for c in COLS[:4]}
    enc["s"] = "DELTA_LENGTH_BYTE_ARRAY"
    pq.write_table(t, path, use_dictionary=False, compression="snappy",
                   column_encoding=enc, row_group_size=1 << 20)


def read(path: str, dev: str):
    """What the executor's ParquetScan does for these columns."""
    got = parquet_native.read_columns_native(path, COLS, dev)
    missing = [c for c in COLS if c not in got]
    if missing:
        hb = RecordBatch.from_arrow(pq.read_table(path, columns=missing), dev)
        for n, c in zip(hb.names, hb.columns):
            got[n] = c
    return got


def staged_bytes(path: str) -> int:
    meta = parquet_native._get_meta(path, COLS)
    live = {c.name for c in meta.cols}
    raw = sum(ch[1] for c in meta.cols for ch in c.chunks if c.name in live)
    return raw + meta.extra_total


def timed(path: str, dev: str, setting: str) -> float:
    os.environ["AURON_SCAN_DELTA_NATIVE"] = "1" if setting == "on" else "0"
    parquet_native.dbuf_cache_clear()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    read(path, dev)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--profile", choices=["on", "off"], default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = "cuda:0"
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "delta.parquet")
        write_file(path, args.rows)
        if args.profile:
            for _ in range(3):
                timed(path, dev, args.profile)
            return
        ms = {"off": [], "on": []}
        for setting in ("off", "on", "off", "on"):  # warm both
            timed(path, dev, setting)
        on = read(path, dev)
        os.environ["AURON_SCAN_DELTA_NATIVE"] = "0"
        off = read(path, dev)
        for c in COLS:  # faster and different is not faster
            a, b = on[c], off[c]
            assert torch.equal(a.data, b.data), c
            assert (a.validity is None) == (b.validity is None), c
            assert a.validity is None or torch.equal(a.validity, b.validity), c
            assert a.offsets is None or torch.equal(a.offsets, b.offsets), c
        for _ in range(args.reps):
            for setting in ("off", "on"):
                ms[setting].append(timed(path, dev, setting))
        res = {"rows": args.rows, "reps": args.reps,
               "file_bytes": os.path.getsize(path)}
        for setting in ("off", "on"):
            os.environ["AURON_SCAN_DELTA_NATIVE"] = \
                "1" if setting == "on" else "0"
            v = ms[setting]
            res[setting] = {"median_ms": statistics.median(v), "min_ms": min(v),
                            "max_ms": max(v), "all_ms": [round(x, 2) for x in v],
                            "staged_bytes": staged_bytes(path)}
        line = json.dumps(res)
        print(line)
        if args.out:
            with open(args.out, "w") as f:
                f.write(line + "\n")


if __name__ == "__main__":
    main()
