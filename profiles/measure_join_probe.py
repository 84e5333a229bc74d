"""A/B the hash-join probe: spark.auron.join.fusedProbe.enable off vs on.

    python profiles/measure_join_probe.py [--rows N] [--reps R]

One process; per case the switch alternates off / on on the same device
tensors (3 warm-up calls each, then R timed calls each, interleaved one by
one), device events around each whole `ops.hash_join` / `ops.join_exists`
call (so the host-side glue and the output-size sync are inside the time).
The table is prebuilt (`ops.join_build`) unless the case says otherwise,
as the executor's broadcast cache does. Both settings must return identical
tensors. Prints one JSON line per case: median (min - max) in ms."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from auron_amd import dtypes, native, ops  # noqa: E402
from auron_amd.column import Column  # noqa: E402

DEV = "cuda:0"


def _int_col(t):
    return Column(dtypes.int64, t.to(DEV), None, None)


def _str_col(ids):
    """'k<id>' zero-padded to 12 bytes, built on the host with numpy."""
    import numpy as np

    a = np.char.zfill(ids.numpy().astype(str), 11)
    raw = np.char.add("k", a).astype("S12")
    data = torch.from_numpy(np.frombuffer(raw.tobytes(), dtype=np.uint8).copy())
    offs = torch.arange(0, 12 * (len(ids) + 1), 12, dtype=torch.int64)
    return Column(dtypes.string, data.to(DEV), None, offs.to(DEV))


def _timed(fn, switch_env, warm, reps):
    """Alternate off/on call by call; -> (result_off, result_on, ms_off, ms_on)."""
    out, ts = {}, {"0": [], "1": []}
    for s in ("0", "1"):
        os.environ[switch_env] = s
        for _ in range(warm):
            out[s] = fn()
    torch.cuda.synchronize()
    for _ in range(reps):
        for s in ("0", "1"):
            os.environ[switch_env] = s
            e0 = torch.cuda.Event(enable_timing=True)
            e1 = torch.cuda.Event(enable_timing=True)
            e0.record()
            out[s] = fn()
            e1.record()
            torch.cuda.synchronize()
            ts[s].append(e0.elapsed_time(e1))
    os.environ.pop(switch_env, None)

    def stat(v):
        return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
                "max": round(max(v), 4)}

    return out["0"], out["1"], stat(ts["0"]), stat(ts["1"])


def _same(a, b):
    a = a if isinstance(a, tuple) else (a,)
    b = b if isinstance(b, tuple) else (b,)
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=16_000_000)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    native.require()
    n = args.rows
    g = torch.Generator().manual_seed(0)
    env = "AURON_JOIN_FUSED_PROBE"

    def report(name, n_probe, n_build, res):
        off, on, t_off, t_on = res
        first = on[0] if isinstance(on, tuple) else on
        print(json.dumps({"case": name, "probe_rows": n_probe, "build_rows": n_build,
                          "out_rows": int(first.numel()) if isinstance(on, tuple)
                          else int(first.sum().item()),
                          "same_result": _same(off, on),
                          "legacy_ms": t_off, "fused_ms": t_on,
                          "speedup_median": round(t_off["median"] / t_on["median"], 3)}),
              flush=True)

    def join_case(name, build_ids, probe_ids, emit=False, as_str=False):
        mk = _str_col if as_str else _int_col
        b, p = [mk(build_ids)], [mk(probe_ids)]
        table = ops.join_build(b)
        res = _timed(lambda: ops.hash_join(b, p, emit, False, table=table),
                     env, 3, args.reps)
        report(name, len(probe_ids), len(build_ids), res)

    # date_dim after a filter: 73k unique keys, ~20 % of probe rows match
    join_case("73k unique build, ~20% match", torch.randperm(73_000, generator=g),
              torch.randint(0, 365_000, (n,), generator=g))
    join_case("500k unique build, all match", torch.randperm(500_000, generator=g),
              torch.randint(0, 500_000, (n,), generator=g))
    dup_build = torch.randperm(2_000_000, generator=g) // 4
    join_case("2M build, 4 rows per key, all match", dup_build,
              torch.randint(0, 500_000, (n,), generator=g))
    join_case("left join, 500k unique build, ~50% match",
              torch.randperm(500_000, generator=g),
              torch.randint(0, 1_000_000, (n,), generator=g), emit=True)
    join_case("string key, 100k build, 4M probe", torch.randperm(100_000, generator=g),
              torch.randint(0, 120_000, (min(n, 4_000_000),), generator=g), as_str=True)

    # semi/anti/existence: legacy = join_counts (rebuilds the table each call)
    b, p = [_int_col(dup_build)], [_int_col(torch.randint(0, 600_000, (n,), generator=g))]
    table = ops.join_build(b)
    for name, tb in (("exists vs counts, cached table", table),
                     ("exists vs counts, no cached table", None)):
        res = _timed(lambda: ops.join_exists(b, p, table=tb), env, 3, args.reps)
        report(name, n, len(dup_build), res)


if __name__ == "__main__":
    main()
