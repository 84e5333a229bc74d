"""k_murmur3, k_group_insert / keys_equal, the join probes, k_pmod,
k_part_hist and k_part_scatter against the independent oracle
(agg_oracle.py): every key dtype at its extremes, NaN payloads and +-0.0,
string length and byte edges, NULL layouts, forced hash collisions (keys
chosen on the CPU so that one table slot or one join chain holds them
all), and the partition kernels at their size edges.

Pinned rules: NaN == NaN and -0.0 == 0.0 as keys, in GROUP BY and in
joins; every NaN hashes as the canonical NaN; NULL groups with NULL and
never joins."""
import functools
import math

import numpy as np
import pytest
import torch

from auron_amd import ops

import agg_cases as C
import agg_oracle as O
from test_agg_semantics import F32_NANS, F64_NANS, KEY_KINDS, multi_column_rows

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def cycle_to(vals, n):
    return [vals[i % len(vals)] for i in range(n)]


# ------------------------------------------------------------------ murmur3
@pytest.mark.parametrize("kind", KEY_KINDS)
@pytest.mark.parametrize("seed", [42, 0])
def test_murmur3_per_dtype(kind, seed):
    vals = C.key_values(kind, ref_safe=False)
    got = ops.murmur3([C.column(kind, vals, DEV)], seed)
    assert got.dtype == torch.int32
    assert got.cpu().tolist() == O.hash_rows([kind], [vals], seed)


@pytest.mark.parametrize("kind,bits", [("float64", F64_NANS), ("float32", F32_NANS)])
def test_murmur3_every_nan_hashes_as_canonical(kind, bits):
    col = C.bits_column(kind, bits, DEV)
    canon = O.hash_value(kind, math.nan, 42)
    assert ops.murmur3([col], 42).cpu().tolist() == [canon] * len(bits)


@pytest.mark.parametrize("seed", [42, 0])
def test_murmur3_multi_column_chaining(seed):
    a, b, s, f = multi_column_rows()
    kinds = ["int32", "int64", "string", "float64"]
    cols = [C.column(k, v, DEV) for k, v in zip(kinds, (a, b, s, f))]
    assert ops.murmur3(cols, seed).cpu().tolist() == \
        O.hash_rows(kinds, [a, b, s, f], seed)


def test_murmur3_second_grid_round():
    n = 2048 * 256 + 1
    vals = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)) \
        .view(np.int64).tolist()
    got = ops.murmur3([C.column("int64", vals, DEV)], 42).cpu().tolist()
    assert got == O.hash_rows(["int64"], [vals], 42)


# ----------------------------------------------------------------- group ids
def check_gpu_group_ids(kinds, cols, columns=None):
    columns = columns or [C.column(k, v, DEV) for k, v in zip(kinds, cols)]
    gids, reps = ops.group_ids(columns)
    assert gids.dtype == torch.int64 and reps.dtype == torch.int64
    O.check_group_ids(gids.cpu().tolist(), reps.cpu().tolist(), cols)


@pytest.mark.parametrize("kind", KEY_KINDS)
@pytest.mark.parametrize("n", [1, 2, 65, 513, None])
def test_group_ids_per_dtype(kind, n):
    vals = C.key_values(kind, ref_safe=False)
    if n is not None:
        vals = cycle_to(vals, n)
    check_gpu_group_ids([kind], [vals])


@pytest.mark.parametrize("n", [1, 2, 65, 513])
def test_group_ids_mixed_columns(n):
    a, b, s, f = (cycle_to(c, n) for c in multi_column_rows())
    check_gpu_group_ids(["int32", "int64"], [a, b])
    check_gpu_group_ids(["int32", "int64", "string"], [a, b, s])
    check_gpu_group_ids(["float64", "string", "int32"], [f, s, a])
    if n >= 2:
        gids, _ = ops.group_ids([C.column("int32", a, DEV), C.column("int64", b, DEV)])
        assert int(gids[0]) != int(gids[1])  # (1, NULL) against (NULL, 1)


def test_group_ids_null_slots_hold_valid_values():
    data = cycle_to([5, 5, 6, 6, 7], 130)
    valid = cycle_to([True, False, True, False, True, True, False], 130)
    col, vals = C.column_over("int64", data, valid, DEV)
    check_gpu_group_ids(["int64"], [vals], [col])
    fdata = cycle_to([math.nan, 0.0, -0.0, 1.5], 130)
    col, vals = C.column_over("float64", fdata, valid, DEV)
    check_gpu_group_ids(["float64"], [vals], [col])
    sdata = cycle_to([b"", b"a", b"a\0", b"null"], 130)
    col, vals = C.column_over("string", sdata, valid, DEV)
    check_gpu_group_ids(["string"], [vals], [col])  # "" against NULL


@pytest.mark.parametrize("n", [1, 2, 65, 513])
def test_group_ids_all_nan_and_all_null(n):
    for kind, bits in (("float64", F64_NANS), ("float32", F32_NANS)):
        col = C.bits_column(kind, cycle_to(bits, n), DEV)
        gids, reps = ops.group_ids([col])
        assert reps.numel() == 1 and gids.cpu().tolist() == [0] * n
    for kind in ("int64", "float64", "string"):
        check_gpu_group_ids([kind], [[None] * n])


@functools.lru_cache(maxsize=None)
def bucket(shape, slot):
    return tuple(C.colliding_keys(shape, slot, 400))


@pytest.mark.parametrize("shape", ["int64", "int32", "pair"])
@pytest.mark.parametrize("slot", [5, 1023])
def test_group_ids_forced_collisions(shape, slot):
    """300 distinct keys whose hashes all start probing at one slot of the
    1024-slot table (n <= 512 -> _next_pow2(2n) = 1024); slot 1023 makes
    linear probing wrap to 0."""
    keys = list(bucket(shape, slot)[:300])
    rows = keys + keys[:212][::-1]
    assert len(rows) == 512 and ops._next_pow2(2 * len(rows)) == 1024
    columns, kinds, cols = C.collision_columns(shape, rows, DEV)
    gids, reps = ops.group_ids(columns)
    assert reps.numel() == 300
    O.check_group_ids(gids.cpu().tolist(), reps.cpu().tolist(), cols)


# --------------------------------------------------------------------- joins
def check_join(bcols, pcols, kinds, emit, columns=None):
    if columns is None:
        columns = ([C.column(k, v, DEV) for k, v in zip(kinds, bcols)],
                   [C.column(k, v, DEV) for k, v in zip(kinds, pcols)])
    bi, pi, bm = ops.hash_join(columns[0], columns[1], emit_unmatched_probe=emit,
                               need_build_matched=True)
    pairs, matched = O.join_pairs(bcols, pcols, emit)
    got = list(zip(bi.cpu().tolist(), pi.cpu().tolist()))
    assert len(got) == len(pairs) and set(got) == pairs
    assert bm.cpu().tolist() == matched
    counts = ops.join_counts(columns[0], columns[1]).cpu().tolist()
    want = [0] * len(pcols[0])
    for j, i in pairs:
        if j >= 0:
            want[i] += 1
    assert counts == want


@pytest.mark.parametrize("shape", ["int64", "int32", "pair"])
@pytest.mark.parametrize("emit", [False, True])
@pytest.mark.parametrize("slot", [5, 1023])
def test_join_forced_collisions(shape, emit, slot):
    """One chain of the 1024-bucket table holds all 420 build rows (300
    keys, 120 of them twice); the probe has keys of that bucket, present and
    absent, and keys of another bucket."""
    keys = list(bucket(shape, slot))
    build = keys[:300] + keys[:120]
    assert ops._next_pow2(2 * len(build)) == 1024
    probe = keys[250:400] + keys[:60] + list(bucket(shape, 5 if slot != 5 else 1023)[:40])
    bcolumns, kinds, bcols = C.collision_columns(shape, build, DEV)
    pcolumns, _, pcols = C.collision_columns(shape, probe, DEV)
    check_join(bcols, pcols, kinds, emit, (bcolumns, pcolumns))


@pytest.mark.parametrize("emit", [False, True])
def test_join_null_keys_in_a_collision_chain(emit):
    keys = list(bucket("int64", 5))
    build = keys[:100] + [None] * 5 + keys[:30]
    probe = [None, keys[0], keys[150], None] + keys[90:110]
    check_join([build], [probe], ["int64"], emit)
    check_join([[7] * len(build), build], [[7, None] + [7] * (len(probe) - 2), probe],
               ["int32", "int64"], emit)


@pytest.mark.parametrize("kind", C.FLOAT_KINDS)
@pytest.mark.parametrize("emit", [False, True])
def test_join_float_keys(kind, emit):
    """NaN joins NaN (any sign) and -0.0 joins 0.0."""
    build = [math.nan, 0.0, 1.5, None, C.NEG_NAN, -0.0, math.inf, 2.5]
    probe = [C.NEG_NAN, -0.0, None, 2.5, 1.5, math.nan, -math.inf, 0.0, 3.5]
    check_join([build], [probe], [kind], emit)
    pairs, _ = O.join_pairs([build], [probe], emit)
    assert {(0, 0), (4, 0), (1, 1), (5, 1), (0, 5), (5, 7)} <= pairs
    # two columns: the generic compare, with a string beside the float
    s_b = cycle_to([b"a", b"a\0"], len(build))
    s_p = cycle_to([b"a", b"a\0", b"a"], len(probe))
    check_join([build, s_b], [probe, s_p], [kind, "string"], emit)


@pytest.mark.parametrize("emit", [False, True])
def test_join_string_keys(emit):
    vals = C.string_values(ref_safe=False)
    build = vals + [None] + vals[::3]
    probe = vals[::2] + [None, b"absent", b"a\0\0\0"] + vals[1::5]
    check_join([build], [probe], ["string"], emit)


# ---------------------------------------------------------------- partitions
@pytest.mark.parametrize("nparts", [1, 2, 7, 200, 1000])
def test_partition_ids(nparts):
    # _normalize_hash_col: ints hash as int64 and floats as float64
    i32 = cycle_to(C.key_values("int32"), 300)
    f32 = cycle_to(C.key_values("float32"), 300)
    hashes = O.hash_rows(["int64", "float64"], [i32, f32])
    assert any(h < 0 for h in hashes) and any(h > 0 for h in hashes)
    got = ops.partition_ids([C.column("int32", i32, DEV), C.column("float32", f32, DEV)],
                            nparts)
    assert got.dtype == torch.int32
    assert got.cpu().tolist() == [O.pmod(h, nparts) for h in hashes]


def check_partition_order(pids, nparts):
    t = torch.tensor(pids, dtype=torch.int32, device=DEV)
    order, counts = ops.partition_order(t, nparts)
    want = np.bincount(np.array(pids, dtype=np.int64), minlength=nparts)
    assert counts.dtype == torch.int64 and counts.cpu().tolist() == want.tolist()
    order = order.cpu().numpy()
    assert sorted(order.tolist()) == list(range(len(pids)))  # a permutation
    seg = np.array(pids, dtype=np.int64)[order]
    assert seg.tolist() == np.repeat(np.arange(nparts), want).tolist()


@pytest.mark.parametrize("n", [1, 255, 257, 100_000])
def test_partition_order(n):
    rng = np.random.default_rng(n)
    check_partition_order([0] * n, 1)                        # nparts = 1
    check_partition_order([3] * n, 7)                        # one partition has all
    pids = rng.choice([0, 1, 2, 4, 5, 6, 199], n).tolist()   # 3 and most others empty
    check_partition_order(pids, 200)
    check_partition_order(rng.integers(0, 1000, n).tolist(), 1000)
