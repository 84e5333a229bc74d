"""bench.py --dump-outputs: result batches -> float64 .npy files that are
comparable between two builds (canonical row order, all values finite,
NULLs and non-finite values marked in a flags array)."""
import importlib.util
import os
import zlib

import numpy as np

from auron_amd import dtypes
from auron_amd.column import RecordBatch

_BENCH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "bench.py")


def _bench():
    spec = importlib.util.spec_from_file_location("auron_bench", _BENCH)
    mod = importlib.util.module_from_spec(spec)
    saved = dict(os.environ)
    try:
        spec.loader.exec_module(mod)
    finally:  # bench.py sets allocator defaults for its own process only
        for k in set(os.environ) - set(saved):
            del os.environ[k]
    return mod


ROWS = [("b", 2, 1.25, -3.5, -5.25), ("a", 2, None, 7.0, 1.5),
        ("a", 1, 0.5, 12345678901.25, 2.0), ("c", 3, float("inf"), None, 1.0),
        ("c", 4, float("nan"), 1.0, None), ("c", 5, float("-inf"), 1.0, 1.0)]


def _batch(order):
    rows = [ROWS[i] for i in order]
    d = {"s": [r[0] for r in rows], "k": [r[1] for r in rows],
         "f": [r[2] for r in rows], "money": [r[3] for r in rows],
         "big": [r[4] for r in rows]}
    types = {"s": dtypes.string, "k": dtypes.int64, "f": dtypes.float64,
             "money": dtypes.decimal64(18, 2), "big": dtypes.decimal128(38, 2)}
    return RecordBatch.from_pydict(d, types)


def test_dump_outputs_values_and_canonical_order(tmp_path):
    bench = _bench()
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs({"q0": _batch([0, 1, 2, 3, 4, 5])}, str(a))
    bench.dump_outputs({"q0": _batch([4, 2, 5, 0, 3, 1])}, str(b))
    names = sorted(os.listdir(a))
    assert names == ["q0.c00_s.npy", "q0.c01_k.npy", "q0.c02_f.npy", "q0.c03_money.npy",
                     "q0.c04_big.npy", "q0.flags.npy", "q0.rows.npy"]
    assert sorted(os.listdir(b)) == names
    got = [np.load(a / n) for n in names]
    for n, arr in zip(names, got):
        assert arr.dtype == (np.float32 if n.endswith("flags.npy") else np.float64)
        assert arr.size > 0 and np.isfinite(arr).all(), n
        # engine row order among ties must not show in the dump
        assert np.array_equal(arr, np.load(b / n)), n

    def cell(v):  # -> (value, flag)
        if v is None:
            return 0.0, 1.0
        if isinstance(v, str):
            return float(zlib.crc32(v.encode())), 0.0
        if v != v:
            return 0.0, 2.0
        if v in (float("inf"), float("-inf")):
            return 0.0, 3.0 if v > 0 else 4.0
        return float(v), 0.0

    want = sorted([tuple(cell(v) for v in r) for r in ROWS])  # (s, k) is unique
    for i in range(5):
        assert np.array_equal(got[i], np.array([r[i][0] for r in want])), names[i]
    assert np.array_equal(got[5], np.array([[c[1] for c in r] for r in want],
                                           dtype=np.float32))
    assert np.array_equal(got[6], np.array([6.0, 5.0]))


def test_dump_outputs_empty_result_writes_row_count_only(tmp_path):
    bench = _bench()
    out = tmp_path / "a"
    bench.dump_outputs({"q0": _batch([0, 1])}, str(out))
    bench.dump_outputs({"q0": _batch([])}, str(out))  # replaces the earlier dump
    assert os.listdir(out) == ["q0.rows.npy"]
    assert np.array_equal(np.load(out / "q0.rows.npy"), np.array([0.0, 5.0]))


def test_dump_outputs_samples_oversized_results(tmp_path, monkeypatch):
    bench = _bench()
    monkeypatch.setattr(bench, "DUMP_BUDGET_BYTES", 12 * 2 * 10)  # 10 rows x 2 cols
    n = 1000
    batch = RecordBatch.from_pydict({"k": list(range(n)), "v": [i * 0.5 for i in range(n)]},
                                    {"k": dtypes.int64, "v": dtypes.float64})
    bench.dump_outputs({"q0": batch}, str(tmp_path / "a"))
    bench.dump_outputs({"q0": batch}, str(tmp_path / "b"))
    k = np.load(tmp_path / "a" / "q0.c00_k.npy")
    v = np.load(tmp_path / "a" / "q0.c01_v.npy")
    assert k.shape == v.shape == (10,)
    assert np.array_equal(v, k * 0.5)  # the same rows in every column
    assert np.load(tmp_path / "a" / "q0.flags.npy").shape == (10, 2)
    assert np.array_equal(k, np.load(tmp_path / "b" / "q0.c00_k.npy"))  # fixed sample
