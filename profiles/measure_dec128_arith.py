"""Time the exact decimal128 kernels (add, sub, mul, div, cmp, rescale).

    python profiles/measure_dec128_arith.py [--rows N] [--ref-rows M]

Random decimal(38,2)-like limbs (|value| < 2^100, both signs) and decimal64-
like int64 operands on the device. Each case is one `ops.dec128_*` call, one
kernel launch, timed with device events after a warm-up. The Python-integer
reference is not tolerable at 16M rows (tens of seconds per call), so the
native path is timed alone at --rows, and native and AURON_FORCE_REF=1 are
interleaved in this process at --ref-rows, where both must return the same
limbs and validity. Prints one JSON line per case with median/min/max in ms
and the bytes the operation has to move (computed from the shapes: operands
read once, result and validity written once) over the median."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from auron_amd import native, ops  # noqa: E402


def limbs(n, hi_bits, g):
    x = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), generator=g,
                      dtype=torch.int64)
    x[:, 1] = torch.randint(-(1 << hi_bits), 1 << hi_bits, (n,), generator=g,
                            dtype=torch.int64)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--ref-rows", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    native.require()
    dev = "cuda:0"
    n, m = args.rows, args.ref_rows
    g = torch.Generator().manual_seed(0)
    a = limbs(n, 36, g).to(dev)        # |a| < 2^100 ~ 1.3e30
    b = limbs(n, 36, g).to(dev)
    # |s| < 2^36 in limb form: about half the products a*s cross 2^128, and
    # a*s / 10^4 still fits 38 digits
    s = torch.randint(-(1 << 36), 1 << 36, (n,), generator=g)
    s = torch.where(s == 0, torch.ones_like(s), s)
    s = torch.stack([s, s >> 63], dim=1).to(dev)
    e = torch.randint(-10 ** 7, 10 ** 7, (n,), generator=g).to(dev)  # dec64
    e = torch.where(e == 0, torch.ones_like(e), e)

    W, N, V, B = 16, 8, 1, 1  # limb pair, int64, validity byte, bool byte
    cases = [
        ("add same scale", lambda a, b, s, e: ops.dec128_add(a, b, 0, 0, 0, 38),
         2 * W + W + V),
        ("add scales 2/0, d=1", lambda a, b, s, e: ops.dec128_add(a, b, 2, 0, 1, 38),
         2 * W + W + V),
        ("add dec128 + int64", lambda a, b, s, e: ops.dec128_add(a, e, 0, 0, 0, 38),
         W + N + W + V),
        ("sub same scale", lambda a, b, s, e: ops.dec128_sub(a, b, 0, 0, 0, 38),
         2 * W + W + V),
        ("mul dec128 * int64, d=0", lambda a, b, s, e: ops.dec128_mul(a, e, 0, 38),
         W + N + W + V),
        ("mul dec128 * int64, d=2", lambda a, b, s, e: ops.dec128_mul(a, e, 2, 38),
         W + N + W + V),
        ("mul dec128 * dec128, d=4", lambda a, b, s, e: ops.dec128_mul(a, s, 4, 38),
         2 * W + W + V),
        ("div dec128 / int64, k=6", lambda a, b, s, e: ops.dec128_div(a, e, 6, 38),
         W + N + W + V),
        ("div dec128 / dec128, k=6", lambda a, b, s, e: ops.dec128_div(a, s, 6, 38),
         2 * W + W + V),
        ("cmp < same scale", lambda a, b, s, e: ops.dec128_cmp(a, b, 0, 0, "<"),
         2 * W + B),
        ("cmp < scales 0/4", lambda a, b, s, e: ops.dec128_cmp(a, b, 0, 4, "<"),
         2 * W + B),
        ("rescale up 4", lambda a, b, s, e: ops.dec128_rescale(a, 4, 38),
         W + W + V),
        ("rescale down 4", lambda a, b, s, e: ops.dec128_rescale(a, -4, 38),
         W + W + V),
        ("rescale bound check only", lambda a, b, s, e: ops.dec128_rescale(a, 0, 30),
         W + W + V),
    ]

    def timed(fn, argv, reps):
        ts = []
        for _ in range(reps):
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn(*argv)
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
        return out, ts

    def stats(ts):
        return {"median": statistics.median(ts), "min": min(ts),
                "max": max(ts)}

    def same(x, y):
        if isinstance(x, tuple):
            return all(torch.equal(p, q) for p, q in zip(x, y))
        return bool(torch.equal(x, y))

    full = (a, b, s, e)
    small = tuple(t[:m] for t in full)
    for name, fn, row_bytes in cases:
        os.environ["AURON_FORCE_REF"] = "0"
        for _ in range(3):
            fn(*full)
        torch.cuda.synchronize()
        _, t_nat = timed(fn, full, args.reps)
        # native and reference interleaved at the small size
        t_small, t_ref = [], []
        for _ in range(3):
            os.environ["AURON_FORCE_REF"] = "0"
            nat, ts = timed(fn, small, 4)
            t_small += ts
            os.environ["AURON_FORCE_REF"] = "1"
            ref, ts = timed(fn, small, 1)
            t_ref += ts
        os.environ["AURON_FORCE_REF"] = "0"
        med = stats(t_nat)["median"]
        print(json.dumps({
            "case": name, "rows": n, "native_ms": stats(t_nat),
            "bytes": n * row_bytes, "native_GBps": n * row_bytes / med / 1e6,
            "ref_rows": m, "native_small_ms": stats(t_small),
            "ref_small_ms": stats(t_ref), "same_result": same(nat, ref),
        }), flush=True)


if __name__ == "__main__":
    main()
