#!/usr/bin/env python3
"""Flagship benchmark: TPC-DS query suite on auron_amd.

Driver contract: `python bench.py --gpus N --steps K --warmup W` (for N>1
launched under torch.distributed.run, one rank per GPU over RCCL). One
step = run the full implemented TPC-DS query suite once against the
synthetic dsdgen dataset at --sf (strong scaling: fixed dataset, fact
files sharded across ranks, exchange over RCCL/xGMI).

Rank 0 prints ONE JSON line with the suite wall-clock per step (max over
ranks). BASELINE.md's published number (1519 s, TPC-DS 1TB / 99 queries,
unknown CPU hardware) is not directly comparable to this config, so
vs_baseline is null until the full 99-query/1TB config runs.

A plain run only sets up, warms up, times the steps and prints the
result line. `--dump-outputs DIR` additionally writes the query results of
the last timed step as DIR/<query>.cNN_<column>.npy (all finite; NULLs are
marked in DIR/<query>.flags.npy, the row count is in DIR/<query>.rows.npy) so two builds can be compared output for
output. `--full` is where every extra measurement
lives; today that is the per-operator time breakdown on stderr.
"""
import argparse
import json
import shutil
import os
import sys
import time

import os as _os

_os.environ.setdefault("PYTORCH_ALLOC_CONF", "expandable_segments:True")

import torch
import torch.distributed as dist


def log(msg):
    r = os.environ.get("RANK", "0")
    print(f"[bench r{r}] {msg}", file=sys.stderr, flush=True)


DUMP_BUDGET_BYTES = 48 << 20  # stays well under 64 MB in all
DUMP_SAMPLE_SEED = 20240912
# Queries whose ORDER BY keys tie across rows (duplicate s_store_id /
# customer attributes), so LIMIT 100 keeps an engine-order-dependent subset
# of the tied rows and two runs of ONE build legitimately return different
# rows (measured: q59 columns differ by up to 7% between two SF=10 runs).
# tests/test_tpcds.py compares exactly these against the full result as a
# subset (SUBSET_OF_FULL); they carry no signal file by file, so the dump
# leaves them out.
DUMP_TIE_LIMITED = frozenset({"q18", "q59"})


def _column_as_float(col):
    """One result column as (values, flags): two finite numpy arrays.

    values (float64): numerics, dates and decimals keep their value;
    strings become the crc32 of their utf-8 bytes (exact in float64) so
    they compare too. flags (float32): 0 = a value, 1 = SQL NULL,
    2 = NaN, 3 = +inf, 4 = -inf; values holds 0.0 wherever flags != 0."""
    import zlib

    import numpy as np

    from auron_amd import dtypes

    c = col.to("cpu")
    n = len(c)
    if c.dtype.is_string:
        raw = c.data.numpy().tobytes()
        offs = c.offsets.numpy()
        out = np.fromiter((zlib.crc32(raw[offs[i]:offs[i + 1]]) for i in range(n)),
                          dtype=np.float64, count=n)
    elif c.dtype.is_list:
        offs = c.offsets.numpy()
        flat = c.data.numpy().astype(np.float64)
        out = np.array([flat[offs[i]:offs[i + 1]].sum() for i in range(n)],
                       dtype=np.float64)
    elif c.dtype.code == dtypes.DECIMAL128:
        # exact python ints: hi * 2**64 + lo cancels badly in float64
        m64, s = (1 << 64) - 1, 10 ** c.dtype.scale
        out = np.array([((h << 64) | (l & m64)) / s
                        for l, h in zip(c.data[:, 0].tolist(), c.data[:, 1].tolist())],
                       dtype=np.float64)
    elif c.dtype.code == dtypes.DECIMAL64:
        out = c.data.numpy().astype(np.float64) / float(10 ** c.dtype.scale)
    else:
        out = c.data.numpy().astype(np.float64)
    flags = np.zeros(n, dtype=np.float32)
    flags[np.isnan(out)] = 2
    flags[np.isposinf(out)] = 3
    flags[np.isneginf(out)] = 4
    if c.validity is not None:
        flags[~c.validity.numpy()] = 1  # the slot under a NULL is undefined
    out = np.where(flags == 0, out, 0.0)
    return np.ascontiguousarray(out, dtype=np.float64), flags


def dump_outputs(results, out_dir):
    """Write the result batches of one suite pass as finite, non-empty
    .npy files: <query>.rows.npy (float64 [n_rows, n_columns] of the full
    result, always written), and for a result that has rows
    <query>.cNN_<column>.npy (float64 values, one per column) and
    <query>.flags.npy (float32, rows x columns, see _column_as_float).
    A query that returns no rows writes its rows.npy only.

    SQL leaves the order among ORDER BY ties (and of unordered results)
    to the engine, and the hash tables fill in atomic order, so rows are
    written in a canonical order: sorted by column 0 (values, then
    flags), then column 1, ... Oversized results are cut to a fixed
    seeded row sample."""
    import re

    import numpy as np

    os.makedirs(out_dir, exist_ok=True)
    tables = {}
    for qn, batch in results.items():
        if qn in DUMP_TIE_LIMITED:
            continue
        pairs = [_column_as_float(c) for c in batch.columns]
        cols = [v for v, _ in pairs]
        n = len(cols[0]) if cols else 0
        flags = np.stack([f for _, f in pairs], axis=1) if cols else \
            np.zeros((0, 0), dtype=np.float32)
        if n > 1:
            keys = [k for v, f in pairs for k in (v, f)]
            order = np.lexsort(tuple(reversed(keys)))
            cols = [a[order] for a in cols]
            flags = flags[order]
        tables[qn] = (batch.names, cols, flags)
    n_arrays = max(1, sum(len(cols) for _, cols, _ in tables.values()))
    max_rows = max(1, DUMP_BUDGET_BYTES // 12 // n_arrays)  # 8 B value + 4 B flag
    for qn, (names, cols, flags) in tables.items():
        n = len(cols[0]) if cols else 0
        for stale in os.listdir(out_dir):  # an earlier dump of this query
            if stale.startswith(qn + ".") and stale.endswith(".npy"):
                os.remove(os.path.join(out_dir, stale))
        np.save(os.path.join(out_dir, f"{qn}.rows.npy"),
                np.array([n, len(cols)], dtype=np.float64))
        if n == 0:
            continue
        keep = slice(None)
        if n > max_rows:
            rng = np.random.default_rng(DUMP_SAMPLE_SEED)
            keep = np.sort(rng.choice(n, size=max_rows, replace=False))
        for i, (name, arr) in enumerate(zip(names, cols)):
            safe = re.sub(r"[^A-Za-z0-9_]+", "_", name).strip("_")[:48]
            np.save(os.path.join(out_dir, f"{qn}.c{i:02d}_{safe}.npy"), arr[keep])
        np.save(os.path.join(out_dir, f"{qn}.flags.npy"),
                np.ascontiguousarray(flags[keep]))
    return len(tables)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--sf", type=float, default=float(os.environ.get("AURON_BENCH_SF", "10")))
    ap.add_argument("--queries", type=str, default="all")
    ap.add_argument("--data-root", type=str,
                    default=os.environ.get("AURON_DATA_ROOT", ""))
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="write the last timed step's query results as "
                         "DIR/<query>.cNN_<column>.npy (float64) plus "
                         "DIR/<query>.flags.npy (NULL / non-finite markers)")
    ap.add_argument("--full", action="store_true",
                    help="also run every extra measurement (today: the "
                         "per-operator time breakdown on stderr)")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    from auron_amd import AuronSession, init_distributed
    from auron_amd.tpcds import datagen
    from auron_amd.tpcds.queries import QUERIES, Catalog

    if not args.data_root:
        # prefer a RAM-backed root when it has more headroom than the
        # repo filesystem (GPU boxes: ~80 GB disk, TBs of DRAM; dsdgen
        # data in tmpfs = the page-cache residency every published
        # TPC-DS run assumes)
        repo_root = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data")
        args.data_root = repo_root
        try:
            shm = "/dev/shm"
            if os.path.isdir(shm) and os.access(shm, os.W_OK):
                free_shm = shutil.disk_usage(shm).free
                free_repo = shutil.disk_usage(os.path.dirname(repo_root)).free
                if free_shm > free_repo:
                    args.data_root = os.path.join(shm, "auron_tpcds")
        except OSError:
            pass

    ctx = init_distributed()
    rank, world = ctx.rank, ctx.world_size
    have_gpu = torch.cuda.is_available()
    device = args.device or ("cuda" if have_gpu else "cpu")
    if have_gpu and world > 1:
        torch.cuda.set_device(int(os.environ.get("LOCAL_RANK", "0")))

    qnames = sorted(QUERIES.keys()) if args.queries == "all" else args.queries.split(",")

    # ---- dataset (generated once, sharded across ranks, cached on disk)
    t0 = time.perf_counter()
    datagen.write_dataset(args.data_root, args.sf, rank=rank, world=world)
    if world > 1:
        dist.barrier()
    log(f"dataset sf={args.sf} ready in {time.perf_counter() - t0:.1f}s")

    session = AuronSession(device=device)
    cat = Catalog(args.data_root, args.sf)

    trace = os.environ.get("AURON_BENCH_TRACE", "") == "1"

    keep_results = args.dump_outputs is not None
    last_results = {}

    def run_suite():
        per_q = {}
        last_results.clear()
        for qn in qnames:
            if trace:
                log(f"start {qn}")
            tq = time.perf_counter()
            plan = QUERIES[qn](cat, session)
            res = session.collect(plan)
            if have_gpu:
                torch.cuda.synchronize()
            per_q[qn] = time.perf_counter() - tq
            if keep_results:
                last_results[qn] = res
            if trace:
                log(f"done  {qn} {per_q[qn]:.2f}s")
        return per_q

    def barrier_sync():
        if world > 1:
            dist.barrier()
        if have_gpu:
            torch.cuda.synchronize()

    for w in range(args.warmup):
        pq = run_suite()
        log(f"warmup {w}: {sum(pq.values()):.3f}s " +
            " ".join(f"{k}={v:.2f}" for k, v in pq.items()))

    barrier_sync()
    t_start = time.perf_counter()
    per_q_last = None
    for k in range(args.steps):
        per_q_last = run_suite()
    barrier_sync()
    elapsed = time.perf_counter() - t_start

    # max over ranks
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64,
                         device="cuda" if dist.get_backend() == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    suite_seconds = elapsed / args.steps
    if keep_results:
        # every rank collects the same final result; rank 0 writes it
        out_dir = args.dump_outputs
        if rank == 0:
            n_written = dump_outputs(last_results, out_dir)
            log(f"wrote {n_written} of {len(last_results)} query results to {out_dir}")
        last_results.clear()
    if rank == 0 and (args.full or
                      os.environ.get("AURON_BENCH_METRICS", "0") == "1"):
        for k, v in sorted(session.metrics().items(), key=lambda kv: -kv[1]):
            log(f"metric {k}: {v:.3f}s")
    if rank == 0:
        out = {
            "metric": "tpcds_suite_seconds",
            "value": suite_seconds,
            "unit": "s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": suite_seconds * 1000.0,
            "higher_is_better": False,
            "scaling": "strong",
            # Auron total TPC-DS **1TB** = ~1519 s on the
            # reference's (unspecified CPU) hardware; only an SF=1000 run
            # here is the same config, so smaller SFs report null
            "vs_baseline": (suite_seconds / 1519.0) if args.sf >= 1000 else None,
            "dtype": "decimal64/fp64",
            "data": "synthetic",
            "config": {
                "model": f"tpcds-{len(qnames)}q",
                "queries": qnames,
                "sf": args.sf,
                "parallelism": f"dp{world}",
                "caches": "HBM staged-bytes + decoded-column buffer pool "
                          "persist across queries/steps (buffer-pool "
                          "semantics; warmup steps warm them)",
                "per_query_s": {k: round(v, 4) for k, v in (per_q_last or {}).items()},
            },
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
