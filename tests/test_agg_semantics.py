"""GROUP BY semantics on the CPU paths (agg_scatter, group_ids_ref,
murmur3_ref, partition_ids, hash_join_ref) against the independent oracle
of agg_oracle.py: the special-value and dtype cases of the GPU files
test_gpu_agg_edges.py / test_gpu_group_keys.py at tiny n.

Pinned rules: aggregate MIN/MAX treat NaN as the greatest float (MAX is
NaN if any input is, MIN only if all are); float keys group and hash with
NaN == NaN (one canonical NaN) and -0.0 == 0.0; a timestamp hashes as a
long; MIN/MAX return the input dtype (bool included: the executor wraps
the accumulator in a Column of the input type)."""
import math

import pytest
import torch

from auron_amd import dtypes, ops

import agg_cases as C
import agg_oracle as O
from test_hash import GOLDEN_I8, GOLDEN_I32, GOLDEN_I64, GOLDEN_STR

KEY_KINDS = ("bool", "int8", "int16", "int32", "int64", "date32", "timestamp",
             "decimal64", "float32", "float64", "string")

F64_NANS = [0x7FF8000000000000, 0xFFF8000000000000, 0x7FF0000000000001,
            0xFFF0000000000001, 0x7FFFFFFFFFFFFFFF, 0xFFFFFFFFFFFFFFFF,
            0x7FF8000000000001, 0xFFF4000000000000, 0x7FF00000DEADBEEF]
F32_NANS = [0x7FC00000, 0xFFC00000, 0x7F800001, 0xFF800001, 0x7FFFFFFF,
            0xFFFFFFFF, 0x7FC00001, 0xFFA00000, 0x7F80BEEF]


# ------------------------------------------------------------ oracle check
def test_oracle_matches_spark_goldens():
    for v, want in GOLDEN_I32.items():
        assert O.hash_int(v, 42) == want
    for v, want in GOLDEN_I8:
        assert O.hash_int(v, 42) == want
    for v, want in GOLDEN_I64:
        assert O.hash_long(v, 42) == want
    for s, want in GOLDEN_STR:
        assert O.hash_bytes(s.encode("utf-8"), 42) == want
    # Spark: doubleToLongBits / floatToIntBits collapse every NaN
    assert O.hash_long(O.F64_NAN_BITS, 42) == -1281358385
    assert O.hash_long(0xFFF8000000000000, 42) == -1489914710
    assert O.hash_double(C.NEG_NAN, 42) == O.hash_double(math.nan, 42) == -1281358385
    assert O.hash_double(-0.0, 42) == O.hash_double(0.0, 42) == O.hash_long(0, 42)
    assert O.hash_float(-0.0, 42) == O.hash_int(0, 42)


def test_oracle_float_rules():
    inf, nan = math.inf, math.nan
    assert O.float_min([nan, 1.0]) == 1.0 and O.float_min([1.0, nan]) == 1.0
    assert O.float_min([inf, nan]) == inf and math.isnan(O.float_min([nan, nan]))
    assert math.isnan(O.float_max([nan, 1.0])) and math.isnan(O.float_max([inf, nan]))
    assert O.float_max([-inf, 2.0]) == 2.0
    assert math.isnan(O.float_sum([inf, -inf])[0]) and O.float_sum([inf, 1.0])[0] == inf
    assert O.float_sum([0.5, 0.25, -0.75]) == (0.0, 1.01 * 2 * 2.0 ** -53 * 1.5)
    assert O.aggregate([0, 0], 1, [O.I64_MAX, 1], "sum", False)[0] == [O.I64_MIN]


# ------------------------------------------------------------------ hashing
@pytest.mark.parametrize("kind,bits", [("float64", F64_NANS), ("float32", F32_NANS)])
@pytest.mark.parametrize("seed", [42, 0])
def test_murmur3_ref_every_nan_hashes_as_canonical(kind, bits, seed):
    col = C.bits_column(kind, bits)
    assert bool(torch.isnan(col.data).all())
    canon = O.hash_value(kind, math.nan, seed)
    assert ops.murmur3_ref([col], seed).tolist() == [canon] * len(bits)


@pytest.mark.parametrize("kind", KEY_KINDS)
@pytest.mark.parametrize("seed", [42, 0])
def test_murmur3_ref_per_dtype(kind, seed):
    vals = C.key_values(kind)
    got = ops.murmur3_ref([C.column(kind, vals)], seed).tolist()
    assert got == O.hash_rows([kind], [vals], seed)


def multi_column_rows():
    """Three key columns with NULLs in different columns: (NULL, 1) against
    (1, NULL) hash alike (nulls are skipped) and must still differ as keys."""
    a = [1, None, 1, None, 2, 1, None, 7, 7]
    b = [None, 1, 1, None, 2, None, 1, -1, -1]
    s = [b"x", b"x", None, None, b"", b"x", b"x", b"a\0", b"a"]
    f = [math.nan, C.NEG_NAN, 0.0, -0.0, None, math.nan, math.nan, 1.5, 1.5]
    return a, b, s, f


@pytest.mark.parametrize("seed", [42, 0])
def test_murmur3_ref_multi_column_chaining(seed):
    a, b, s, f = multi_column_rows()
    kinds = ["int32", "int64", "string", "float64"]
    cols = [C.column(k, v) for k, v in zip(kinds, (a, b, s, f))]
    want = O.hash_rows(kinds, [a, b, s, f], seed)
    assert ops.murmur3_ref(cols, seed).tolist() == want
    two = O.hash_rows(["int64", "int64"], [a, b], seed)
    assert two[0] == two[1]  # (1, NULL) and (NULL, 1)


@pytest.mark.parametrize("nparts", [1, 2, 7, 200, 1000])
def test_partition_ids_cpu(nparts):
    # _normalize_hash_col: ints hash as int64 and floats as float64
    i32 = C.key_values("int32")
    f32 = C.key_values("float32")
    want = [O.pmod(h, nparts) for h in
            O.hash_rows(["int64", "float64"], [i32, f32[:len(i32)]])]
    assert any(h < 0 for h in O.hash_rows(["int64"], [i32]))
    got = ops.partition_ids([C.column("int32", i32),
                             C.column("float32", f32[:len(i32)])], nparts)
    assert got.dtype == torch.int32 and got.tolist() == want


# ----------------------------------------------------------------- group ids
@pytest.mark.parametrize("kind", KEY_KINDS)
def test_group_ids_ref_per_dtype(kind):
    vals = C.key_values(kind)
    gids, reps = ops.group_ids_ref([C.column(kind, vals)])
    O.check_group_ids(gids.tolist(), reps.tolist(), [vals])


def test_group_ids_ref_multi_column_and_null_slots():
    a, b, s, f = multi_column_rows()
    kinds = ["int32", "int64", "string", "float64"]
    gids, reps = ops.group_ids_ref([C.column(k, v) for k, v in zip(kinds, (a, b, s, f))])
    O.check_group_ids(gids.tolist(), reps.tolist(), [a, b, s, f])
    gids, reps = ops.group_ids_ref([C.column("int32", a), C.column("int64", b)])
    O.check_group_ids(gids.tolist(), reps.tolist(), [a, b])
    assert gids[0] != gids[1]
    # a NULL slot whose data equals a valid row's value
    col, vals = C.column_over("int64", [5, 5, 6, 6], [True, False, True, False])
    gids, reps = ops.group_ids_ref([col])
    O.check_group_ids(gids.tolist(), reps.tolist(), [vals])
    assert reps.numel() == 3


def test_hash_join_ref_float_keys():
    build = [math.nan, 0.0, 1.5, None, C.NEG_NAN]
    probe = [C.NEG_NAN, -0.0, None, 2.5, 1.5]
    for emit in (False, True):
        bi, pi, bm = ops.hash_join_ref([C.column("float64", build)],
                                       [C.column("float64", probe)], emit, True)
        pairs, matched = O.join_pairs([build], [probe], emit)
        assert set(zip(bi.tolist(), pi.tolist())) == pairs
        assert len(bi) == len(pairs) and bm.tolist() == matched
    assert (0, 0) in pairs and (4, 0) in pairs and (1, 1) in pairs


# ---------------------------------------------------------------- aggregates
def result_dtype(kind, fn):
    if fn == "sum":
        return torch.float64 if kind in C.FLOAT_KINDS else torch.int64
    return C.DTYPES[kind].torch_dtype  # MIN/MAX keep the input dtype


def run_case(case, device="cpu", scatter=ops.agg_scatter):
    gids = case.gids_t(device)
    col = case.column(device)
    for fn in C.ops_for(case.kind):
        acc, cnt = scatter(gids, case.ngroups, col, fn)
        assert acc.dtype == result_dtype(case.kind, fn), (case.name, fn, acc.dtype)
        assert cnt.dtype == torch.int64
        O.check_agg(acc.cpu().tolist(), cnt.cpu().tolist(), case.want(fn),
                    f"{case.name} {fn}", exact=True)
    _, cnt = scatter(gids, case.ngroups, col, "count")
    assert cnt.cpu().tolist() == case.want("count")[1]


@pytest.mark.parametrize("kind", C.VALUE_KINDS)
@pytest.mark.parametrize("with_validity", [True, False])
@pytest.mark.parametrize("n,ngroups", [(1, 1), (16, 1), (63, 8), (200, 17)])
def test_agg_scatter_cpu(kind, with_validity, n, ngroups):
    for pattern in ("runs", "random"):
        run_case(C.agg_case(f"{kind}-{n}-{pattern}", kind, n, ngroups, pattern,
                            with_validity, "exact", unused_end=n % 2, seed=n))


@pytest.mark.parametrize("kind", C.FLOAT_KINDS)
def test_agg_scatter_cpu_general_floats(kind):
    """+-max, subnormals and arbitrary values: SUM within the derived bound
    of any summation order, 1.01 (m-1) 2**-53 sum|v| per group."""
    case = C.agg_case(f"{kind}-general", kind, 400, 17, "runs", True, "general", seed=3)
    gids, col = case.gids_t(), case.column()
    for fn in ("sum", "min", "max"):
        acc, cnt = ops.agg_scatter(gids, case.ngroups, col, fn)
        O.check_agg(acc.tolist(), cnt.tolist(), case.want(fn), f"{kind} {fn}")


@pytest.mark.parametrize("kind", ["float64", "float32", "int64", "int8"])
def test_agg_wave_patterns_cpu(kind):
    for nan_at in ((0,), (63,), (64, 67), (127, 128), (191,), tuple(range(168, 192))):
        run_case(C.wave_pattern_case(kind, nan_at, with_validity=len(nan_at) == 2))


def merge_partials(case, fn, device="cpu"):
    """Aggregate each half, then combine the partials with a second
    agg_scatter: the executor's partial -> final merge."""
    from auron_amd.column import Column

    n = len(case.gids)
    gids, col = case.gids_t(device), case.column(device)
    accs, cnts = [], []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        a, c = ops.agg_scatter(gids[lo:hi], case.ngroups, col.slice(lo, hi - lo), fn)
        accs.append(a)
        cnts.append(c)
    pg = torch.arange(case.ngroups, device=device).repeat(2)
    pc = torch.cat(cnts)
    sum_dt = dtypes.float64 if case.is_float else dtypes.int64
    state = Column(col.dtype if fn != "sum" else sum_dt, torch.cat(accs), pc > 0)
    acc, _ = ops.agg_scatter(pg, case.ngroups, state, fn)
    cnt, _ = ops.agg_scatter(pg, case.ngroups, Column(dtypes.int64, pc), "sum")
    return acc, cnt


@pytest.mark.parametrize("kind", ["float64", "float32", "int64", "int16", "bool"])
def test_partial_final_merge_cpu(kind):
    case = C.agg_case(f"merge-{kind}", kind, 300, 17, "runs", True, "exact", seed=5)
    for fn in C.ops_for(kind):
        acc, cnt = merge_partials(case, fn)
        O.check_agg(acc.tolist(), cnt.tolist(), case.want(fn),
                    f"merge {kind} {fn}", exact=True)


def test_pack_descs_rejects_buffers_on_two_devices():
    """A kernel must never get a host validity pointer beside device data."""
    from auron_amd import native
    from auron_amd.column import Column

    data = torch.arange(4, dtype=torch.int64)
    stray = torch.empty(4, dtype=torch.bool, device="meta")
    with pytest.raises(ValueError, match="move the whole Column"):
        native.pack_descs_host([Column(dtypes.int64, data, stray)])
    arr, _ = native.pack_descs_host([Column(dtypes.int64, data, data > 1)])
    assert int(arr[0]["validity"]) != 0
