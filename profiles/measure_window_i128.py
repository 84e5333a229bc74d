"""Time the 128-bit window kernels against their torch reference twins.

    python profiles/measure_window_i128.py [--rows N] [--partitions P]

Random decimal128 limbs in P partitions; per frame shape two separately
timed calls — `ops.prefix_sum_i128` followed by `ops.window_frame_sum_i128`
(the frame sum), and `ops.window_frame_minmax_i128` (min) — each once
through the native kernels and once with AURON_FORCE_REF=1, interleaved, on
the same GPU and the same device tensors in one process. Device events
around each call, warm-up first; both paths must return the same limbs.
Prints one JSON line per (frame, call) with median/min/max in ms and, for
the native path, the bytes the algorithm has to move over the median."""
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
    first = torch.ones(n, dtype=torch.bool)
    first[1:] = seg[1:] != seg[:-1]
    starts = torch.nonzero(first).flatten()
    segid = torch.cumsum(first.to(torch.int64), 0) - 1
    start = starts[segid].to(dev)
    i = torch.arange(n, dtype=torch.int64, device=dev)
    # decimal(38,2)-like magnitudes: |value| < 2^100, both signs
    x = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), generator=g,
                      dtype=torch.int64)
    x[:, 1] = torch.randint(-(1 << 36), 1 << 36, (n,), generator=g,
                            dtype=torch.int64)
    x = x.to(dev)
    valid = (torch.rand(n, generator=g) < 0.9).to(dev)

    def frame_sum(a, b):
        return ops.window_frame_sum_i128(ops.prefix_sum_i128(x, valid), a, b)

    def frame_min(a, b):
        return ops.window_frame_minmax_i128(x, a, b, "min")

    def timed(fn, a, b, reps):
        ts = []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(a, b)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return out, ts

    def stats(ts):
        return {"median": statistics.median(ts), "min": min(ts),
                "max": max(ts)}

    # bytes the algorithm needs per row: the scan reads x twice (16 B) and
    # valid twice (1 B) and writes the prefix (16 B); the frame sum reads
    # a, b (8 B each) and two prefix entries and writes 16 B
    scan_bytes = n * (2 * 17 + 16)
    sum_bytes = scan_bytes + n * (16 + 2 * 16 + 16)

    for name, width in (("100 preceding .. current row", 100),
                        ("5000 preceding .. current row", 5000),
                        ("unbounded preceding .. current row", None)):
        a = start if width is None else torch.maximum(i - width, start)
        b = i
        for call, fn in (("prefix_sum + frame_sum", frame_sum),
                         ("frame_minmax (min)", frame_min)):
            for force in ("0", "1"):  # warm-up, both paths
                os.environ["AURON_FORCE_REF"] = force
                for _ in range(3 if force == "0" else 1):
                    fn(a, b)
            torch.cuda.synchronize()
            t_nat, t_ref = [], []
            for _ in range(5):  # interleaved: 4 native calls, 1 twin call
                os.environ["AURON_FORCE_REF"] = "0"
                nat, ts = timed(fn, a, b, 4)
                t_nat += ts
                os.environ["AURON_FORCE_REF"] = "1"
                ref, ts = timed(fn, a, b, 1)
                t_ref += ts
            os.environ["AURON_FORCE_REF"] = "0"
            rec = {"case": name, "call": call, "rows": n,
                   "mean_frame_rows": float((b - a + 1).double().mean()),
                   "same_result": bool(torch.equal(nat, ref)),
                   "native_ms": stats(t_nat), "ref_ms": stats(t_ref)}
            if fn is frame_sum:
                rec["native_GBps"] = sum_bytes / stats(t_nat)["median"] / 1e6
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
