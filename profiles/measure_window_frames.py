"""Time the window frame kernels against their torch reference twins.

    python profiles/measure_window_frames.py [--rows N] [--partitions P]

Sorted int64 keys in P partitions; per case, `ops.window_range_bounds`
followed by `ops.window_frame_minmax` (min) — once through the native
kernels, once with AURON_FORCE_REF=1 — on the same GPU in one process.
Device events around each call, warm-up first; both paths must return the
same (a, b, min). Prints one JSON line per case."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from auron_amd import native, ops  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4_000_000)
    ap.add_argument("--partitions", type=int, default=1000)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    native.require()
    dev = "cuda:0"
    n = args.rows
    g = torch.Generator().manual_seed(0)
    seg = torch.sort(torch.randint(0, args.partitions, (n,), generator=g)).values
    key = torch.randint(0, 10_000, (n,), generator=g, dtype=torch.int64)
    key = key[torch.argsort(seg * 20_000 + key, stable=True)]
    first = torch.ones(n, dtype=torch.bool)
    first[1:] = seg[1:] != seg[:-1]
    starts = torch.nonzero(first).flatten()
    ends = torch.cat([starts[1:] - 1, torch.tensor([n - 1])])
    segid = torch.cumsum(first.to(torch.int64), 0) - 1
    slo, shi = starts[segid].to(dev), ends[segid].to(dev)
    x = torch.randint(-10**9, 10**9, (n,), generator=g, dtype=torch.int64).to(dev)
    key = key.to(dev)

    def run(lo, hi):
        a, b = ops.window_range_bounds(key, slo, shi, lo, hi)
        return a, b, ops.window_frame_minmax(x, a, b, "min")

    def timed(lo, hi, warm, reps):
        for _ in range(warm):
            out = run(lo, hi)
        torch.cuda.synchronize()
        ts = []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = run(lo, hi)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return out, {"median": statistics.median(ts), "min": min(ts),
                     "max": max(ts)}

    for name, lo, hi in (("100 preceding .. current row", -100, 0),
                         ("5000 preceding .. current row", -5000, 0),
                         ("unbounded preceding .. current row", None, 0)):
        os.environ["AURON_FORCE_REF"] = "0"
        nat, t_native = timed(lo, hi, 3, 20)
        os.environ["AURON_FORCE_REF"] = "1"
        ref, t_ref = timed(lo, hi, 1, 5)
        os.environ["AURON_FORCE_REF"] = "0"
        print(json.dumps({
            "case": name, "rows": n,
            "mean_frame_rows": float((nat[1] - nat[0] + 1).double().mean()),
            "same_result": all(torch.equal(p, q) for p, q in zip(nat, ref)),
            "native_ms": t_native, "ref_ms": t_ref}), flush=True)


if __name__ == "__main__":
    main()
