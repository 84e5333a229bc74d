"""decimal128 columns as keys on the CPU paths: the Spark row hash
(murmur3_ref), hash partitioning, join-key normalisation, and GROUP BY /
DISTINCT / count(distinct) / hash joins / window partitions end to end."""
import random
from decimal import Decimal

import pytest
import torch

from auron_amd import AggFunc, AuronSession, col, dtypes, ops
from auron_amd.column import Column, RecordBatch
from auron_amd.engine.executor import _normalize_join_keys
from auron_amd.exprs import Aliased, WindowFunc
from auron_amd.plan import nodes as P

M64 = (1 << 64) - 1
D38 = dtypes.decimal128(38, 2)


def key_values():
    """Unscaled values around every byte-length boundary of the encoding,
    the limb boundaries, the 38-digit extremes, and seeded random values of
    random bit length."""
    vals = [0, 1, -1, 127, -127, 128, -128, 129, -129]
    for k in range(1, 16):
        b = 1 << (8 * k - 1)
        vals += [b, -b, b + 1, b - 1, -b + 1, -b - 1]
    vals += [1 << 63, -(1 << 63), 1 << 64, -(1 << 64),
             (1 << 64) + 1, (1 << 64) - 1, -(1 << 64) - 1, -(1 << 64) + 1]
    vals += [10 ** 38 - 1, -(10 ** 38 - 1)]
    rng = random.Random(20240607)
    for _ in range(300):
        v = rng.getrandbits(rng.randint(1, 126))
        vals.append(-v if rng.random() < 0.5 else v)
    return vals


def d128_column(vals, dt=D38, device="cpu"):
    """decimal128 column from unscaled Python ints (None = NULL)."""
    limbs = []
    for v in vals:
        v = 0 if v is None else v
        lo = v & M64
        limbs.append((lo - (1 << 64) if lo >= (1 << 63) else lo, v >> 64))
    data = torch.tensor(limbs, dtype=torch.int64).reshape(-1, 2)
    validity = None
    if any(v is None for v in vals):
        validity = torch.tensor([v is not None for v in vals], dtype=torch.bool)
    return Column(dt, data, validity).to(device)


def to_byte_array(v):
    """BigInteger.toByteArray: bitLength/8 + 1 big-endian two's-complement
    bytes. BigInteger's bitLength leaves the sign bit out and, for a
    negative value, is that of ~v (so -128 is the one byte 80); Python's
    int.bit_length is that of abs(v), one more at -2^(8k-1)."""
    bit_length = (v if v >= 0 else ~v).bit_length()
    return v.to_bytes(bit_length // 8 + 1, "big", signed=True)


def to_byte_array_column(vals):
    """String column holding BigInteger.toByteArray of each value."""
    raw, offs = bytearray(), [0]
    for v in vals:
        if v is not None:
            raw += to_byte_array(v)
        offs.append(len(raw))
    data = torch.frombuffer(bytearray(raw), dtype=torch.uint8) if raw else \
        torch.empty(0, dtype=torch.uint8)
    validity = None
    if any(v is None for v in vals):
        validity = torch.tensor([v is not None for v in vals], dtype=torch.bool)
    return Column(dtypes.string, data, validity,
                  torch.tensor(offs, dtype=torch.int64))


def with_nulls(vals, every=3):
    return [None if i % every == 1 else v for i, v in enumerate(vals)]


# ------------------------------------------------------------------ the hash
def test_byte_encoding_examples():
    enc = to_byte_array
    assert enc(0) == b"\x00" and enc(-1) == b"\xff"
    assert enc(128) == b"\x00\x80" and enc(-128) == b"\x80"
    assert len(enc(10 ** 38 - 1)) == 16 and len(enc(-(1 << 127))) == 16


def test_murmur3_ref_decimal128_matches_byte_rule():
    """Spark hashes a decimal of precision > 18 as
    hashUnsafeBytes(BigInteger.toByteArray(unscaled), seed). No Spark runs
    here, so the reference is derived from that documented rule: the test
    encodes each value with int.to_bytes at BigInteger's length
    (bitLength/8 + 1, see to_byte_array), stores the bytes as a string
    column, and hashes it with murmur3_ref's string path, which is
    golden-vector tested against Spark. The decimal128 branch must be bit-equal to it."""
    vals = key_values()
    got = ops.murmur3_ref([d128_column(vals)])
    want = ops.murmur3_ref([to_byte_array_column(vals)])
    assert torch.equal(got, want)
    assert got.dtype == torch.int32 and got.unique().numel() > len(vals) // 2


def test_murmur3_ref_decimal128_nulls_seed_and_chaining():
    vals = with_nulls(key_values())
    d, s = d128_column(vals), to_byte_array_column(vals)
    assert torch.equal(ops.murmur3_ref([d]), ops.murmur3_ref([s]))
    assert torch.equal(ops.murmur3_ref([d], seed=7), ops.murmur3_ref([s], seed=7))
    # a null row keeps the incoming seed
    assert int(ops.murmur3_ref([d], seed=7)[1]) == 7
    ints = Column(dtypes.int64,
                  torch.arange(len(vals), dtype=torch.int64) * 1_000_003 - 17)
    assert torch.equal(ops.murmur3_ref([ints, d]), ops.murmur3_ref([ints, s]))
    assert torch.equal(ops.murmur3_ref([d, ints]), ops.murmur3_ref([s, ints]))
    # murmur3 is the reference on CPU
    assert torch.equal(ops.murmur3([ints, d]), ops.murmur3_ref([ints, s]))


def test_murmur3_ref_empty_and_scale_independent():
    assert ops.murmur3_ref([d128_column([])]).numel() == 0
    vals = key_values()[:40]
    a = ops.murmur3_ref([d128_column(vals, dtypes.decimal128(38, 0))])
    b = ops.murmur3_ref([d128_column(vals, dtypes.decimal128(30, 9))])
    assert torch.equal(a, b)  # the unscaled value alone is hashed


def test_small_precision_decimal128_hashes_as_long():
    rng = random.Random(5)
    vals = [0, 1, -1, 10 ** 18 - 1, -(10 ** 18 - 1), 1 << 40, -(1 << 40)]
    vals += [rng.randint(-10 ** 18 + 1, 10 ** 18 - 1) for _ in range(100)]
    vals = with_nulls(vals, every=5)
    c = d128_column(vals, dtypes.decimal128(18, 2))
    as_long = Column(dtypes.int64, c.data[:, 0].contiguous(), c.validity)
    want = ops.murmur3_ref([as_long])
    assert torch.equal(ops.murmur3_ref([c]), want)
    assert torch.equal(ops.murmur3([c]), want)
    seed = torch.full((len(vals),), 42, dtype=torch.int64)
    h = ops._hash_long_t(c.data[:, 0], seed)
    h = torch.where(c.validity, h, seed)
    h = torch.where(h >= 2 ** 31, h - 2 ** 32, h).to(torch.int32)
    assert torch.equal(want, h)
    # precision 19 takes the byte rule
    wide = d128_column(vals, dtypes.decimal128(19, 2))
    assert torch.equal(ops.murmur3_ref([wide]),
                       ops.murmur3_ref([to_byte_array_column(vals)]))


def test_partition_ids_cpu():
    vals = with_nulls(key_values())
    vals = vals + vals[::-1]  # every value twice, at different rows
    c = d128_column(vals)
    for nparts in (1, 2, 7, 64):
        ids = ops.partition_ids([c], nparts)
        assert ids.dtype == torch.int32 and ids.numel() == len(vals)
        assert int(ids.min()) >= 0 and int(ids.max()) < nparts
        want = torch.remainder(ops.murmur3_ref([c]).to(torch.int64), nparts)
        assert torch.equal(ids.to(torch.int64), want)
        by_value = {}
        for v, p in zip(vals, ids.tolist()):
            assert by_value.setdefault(v, p) == p
    assert ops.partition_ids([c], 64).unique().numel() > 32


# ------------------------------------------------------- the CPU references
def test_group_ids_ref_is_exact_for_wide_values():
    """Neighbouring 128-bit values round to one float64; the reference must
    still tell them apart."""
    base = 3 << 64
    vals = [base + 5, base + 6, -(base + 5), base + 5, None, (4 << 64) + 5,
            None, base + 6]
    gids, reps = ops.group_ids([d128_column(vals)])
    assert reps.tolist() == [0, 1, 2, 4, 5]
    assert gids.tolist() == [0, 1, 2, 0, 3, 4, 3, 1]
    bi, pi, _ = ops.hash_join(
        [d128_column([base + 5, base + 6, None])],
        [d128_column([base + 6, None, base + 7, base + 5])], False, False)
    assert sorted(zip(pi.tolist(), bi.tolist())) == [(0, 1), (3, 0)]


# -------------------------------------------------- join-key normalisation
def _unscaled(c):
    d = c.data
    out = [(h << 64) | (l & M64) for l, h in
           zip(d[:, 0].tolist(), d[:, 1].tolist())]
    if c.validity is not None:
        out = [v if ok else None for v, ok in zip(out, c.validity.tolist())]
    return out


def _check_normalised(l, r, want_dt, lvals, rvals):
    """lvals / rvals: the cells as Decimal; numerically equal cells must be
    limb-equal after normalisation, unequal ones not."""
    (ln,), (rn,) = _normalize_join_keys([l], [r])
    assert ln.dtype == rn.dtype == want_dt
    lu, ru = _unscaled(ln), _unscaled(rn)
    assert lu == [int(v.scaleb(want_dt.scale)) for v in lvals]
    assert ru == [int(v.scaleb(want_dt.scale)) for v in rvals]
    for a, x in zip(lvals, lu):
        for b, y in zip(rvals, ru):
            assert (a == b) == (x == y)
    # and the other way round
    (rn2,), (ln2,) = _normalize_join_keys([r], [l])
    assert rn2.dtype == ln2.dtype == want_dt
    assert _unscaled(ln2) == lu and _unscaled(rn2) == ru


def test_normalize_join_keys_decimal128_scales():
    lun = [12345, -700, 10 ** 19 + 50, 0]                 # (20,2)
    run = [1234500, -70000, 10 ** 21 + 5000, 1]           # (22,4)
    _check_normalised(
        d128_column(lun, dtypes.decimal128(20, 2)),
        d128_column(run, dtypes.decimal128(22, 4)),
        dtypes.decimal128(22, 4),
        [Decimal(v).scaleb(-2) for v in lun],
        [Decimal(v).scaleb(-4) for v in run])


def test_normalize_join_keys_decimal128_vs_decimal64():
    lun = [12345, -700, 10 ** 19 + 50, 99999]             # (20,2)
    run = [12345, -700, 99999, 5]                         # decimal64(7,2)
    r = Column(dtypes.decimal64(7, 2), torch.tensor(run, dtype=torch.int64))
    _check_normalised(
        d128_column(lun, dtypes.decimal128(20, 2)), r,
        dtypes.decimal128(20, 2),
        [Decimal(v).scaleb(-2) for v in lun],
        [Decimal(v).scaleb(-2) for v in run])


def test_normalize_join_keys_decimal128_vs_int64():
    lun = [7, -3, 10 ** 19, -(1 << 63), 0]                # (20,0)
    run = [7, -3, (1 << 63) - 1, -(1 << 63), 1]
    r = Column(dtypes.int64, torch.tensor(run, dtype=torch.int64))
    _check_normalised(
        d128_column(lun, dtypes.decimal128(20, 0)), r,
        dtypes.decimal128(20, 0),
        [Decimal(v) for v in lun], [Decimal(v) for v in run])


def test_normalize_join_keys_int32_widens_scale_and_digits():
    l = d128_column([150, -2500], dtypes.decimal128(20, 2))
    r = Column(dtypes.int32, torch.tensor([1, -25], dtype=torch.int32))
    (ln,), (rn,) = _normalize_join_keys([l], [r])
    assert ln.dtype == rn.dtype == dtypes.decimal128(20, 2)
    assert _unscaled(rn) == [100, -2500] and _unscaled(ln) == [150, -2500]


def test_normalize_join_keys_over_38_digits_keeps_float64():
    l = d128_column([5 * 10 ** 10, 7], dtypes.decimal128(38, 10))
    r = d128_column([5, 10 ** 30], dtypes.decimal128(38, 0))  # needs 48 digits
    (ln,), (rn,) = _normalize_join_keys([l], [r])
    assert ln.dtype == rn.dtype == dtypes.float64
    assert ln.data.tolist() == [5.0, 7e-10] and rn.data.tolist() == [5.0, 1e30]
    r64 = Column(dtypes.int64, torch.tensor([5], dtype=torch.int64))
    l30 = d128_column([5 * 10 ** 30], dtypes.decimal128(38, 30))  # 19 + 30
    (ln,), (rn,) = _normalize_join_keys([l30], [r64])
    assert ln.dtype == rn.dtype == dtypes.float64


def test_normalize_join_keys_leaves_other_pairs_alone():
    a = d128_column([1, 2], dtypes.decimal128(20, 2))
    b = d128_column([2, 3], dtypes.decimal128(30, 2))  # same scale: comparable
    (an,), (bn,) = _normalize_join_keys([a], [b])
    assert an is a and bn is b
    i32 = Column(dtypes.int32, torch.tensor([1, 2], dtype=torch.int32))
    i64 = Column(dtypes.int64, torch.tensor([1, 2], dtype=torch.int64))
    (x,), (y,) = _normalize_join_keys([i32], [i64])
    assert x.dtype == y.dtype == dtypes.int64
    d64 = Column(dtypes.decimal64(7, 2), torch.tensor([100, 200]))
    (x,), (y,) = _normalize_join_keys([d64], [d64])
    assert x is d64 and y is d64


# ----------------------------------------------------- end to end on the CPU
BIG = 10 ** 21  # far past int64 and past float64's 53 bits at scale 2
KEYS = [BIG + 1, BIG + 2, -(BIG + 1), 5, -5, 0, (3 << 64) + 5, (3 << 64) + 6]


def _dec(u, scale=2):
    return None if u is None else Decimal(u).scaleb(-scale)


def _fact_rows(n=200):
    rng = random.Random(11)
    rows = []
    for i in range(n):
        k = None if i % 17 == 3 else KEYS[rng.randrange(len(KEYS))]
        rows.append((k, rng.randint(-50, 50), i))
    return rows


def _fact_batch(rows, device="cpu", dt=D38):
    return RecordBatch(
        ["k", "v", "id"],
        [d128_column([r[0] for r in rows], dt, device),
         Column(dtypes.int64, torch.tensor([r[1] for r in rows])).to(device),
         Column(dtypes.int64, torch.tensor([r[2] for r in rows])).to(device)])


def _arrow_rows(out, names):
    t = out.to_arrow()
    return list(zip(*[t.column(n).to_pylist() for n in names]))


def test_group_by_decimal128_sum_count():
    rows = _fact_rows()
    plan = P.HashAgg(P.MemoryScan([_fact_batch(rows)]),
                     [Aliased(col("k"), "k")],
                     [AggFunc("sum", col("v"), name="sv"),
                      AggFunc("count_star", None, name="n")], mode="complete")
    out = AuronSession(device="cpu").collect(plan)
    want = {}
    for k, v, _ in rows:
        s, n = want.get(k, (0, 0))
        want[k] = (s + v, n + 1)
    got = {k: (sv, n) for k, sv, n in _arrow_rows(out, ["k", "sv", "n"])}
    assert len(got) == out.num_rows == len(want) == len(KEYS) + 1
    assert got == {_dec(k): sn for k, sn in want.items()}


def test_select_distinct_decimal128():
    rows = _fact_rows()
    plan = P.HashAgg(P.MemoryScan([_fact_batch(rows)]),
                     [Aliased(col("k"), "k")], [], mode="complete")
    out = AuronSession(device="cpu").collect(plan)
    got = [k for (k,) in _arrow_rows(out, ["k"])]
    assert len(got) == len(set(got))
    assert set(got) == {_dec(r[0]) for r in rows}


def test_count_distinct_decimal128():
    rows = _fact_rows()
    # group on the small int v's sign, count the distinct wide keys
    batch = _fact_batch(rows)
    g = Column(dtypes.int64, torch.tensor([1 if r[1] >= 0 else 0 for r in rows]))
    batch = RecordBatch(["g", "k"], [g, batch.column("k")])
    plan = P.HashAgg(P.MemoryScan([batch]), [Aliased(col("g"), "g")],
                     [AggFunc("count_distinct", col("k"), distinct=True,
                              name="nd")], mode="complete")
    out = AuronSession(device="cpu").collect(plan)
    want = {}
    for k, v, _ in rows:
        if k is not None:
            want.setdefault(1 if v >= 0 else 0, set()).add(k)
    got = dict(_arrow_rows(out, ["g", "nd"]))
    assert got == {g: len(s) for g, s in want.items()}


def _dim_rows():
    # two rows for BIG + 2, one NULL key, one key the fact side never has
    keys = [BIG + 1, BIG + 2, BIG + 2, (3 << 64) + 5, 5, None, BIG + 3]
    return [(k, 100 + i) for i, k in enumerate(keys)]


def _dim_batch(rows, dt=D38, scale_by=1):
    return RecordBatch(
        ["dk", "w"],
        [d128_column([None if k is None else k * scale_by for k, _ in rows], dt),
         Column(dtypes.int64, torch.tensor([w for _, w in rows]))])


def _join_oracle(fact, dim, how):
    out = []
    for k, v, i in fact:
        hits = [w for dk, w in dim if k is not None and dk == k]
        if how == "inner":
            out += [(i, w) for w in hits]
        elif how == "left":
            out += [(i, w) for w in hits] or [(i, None)]
        elif how == "semi":
            out += [(i,)] if hits else []
        elif how == "anti":
            out += [] if hits else [(i,)]
    return sorted(out, key=repr)


@pytest.mark.parametrize("mismatched_scale", [False, True])
@pytest.mark.parametrize("how", ["inner", "left", "semi", "anti"])
def test_hash_join_on_decimal128_key(how, mismatched_scale):
    fact, dim = _fact_rows(120), _dim_rows()
    factb = _fact_batch(fact, dt=dtypes.decimal128(30, 2))
    if mismatched_scale:
        # the dimension holds the same numbers at scale 4; the common type
        # is decimal128(32, 4)
        dimb = _dim_batch(dim, dtypes.decimal128(32, 4), scale_by=100)
    else:
        dimb = _dim_batch(dim, dtypes.decimal128(30, 2))
    plan = P.HashJoin(P.MemoryScan([factb]), P.MemoryScan([dimb]),
                      [col("k")], [col("dk")], how=how)
    out = AuronSession(device="cpu").collect(plan)
    names = ["id", "w"] if how in ("inner", "left") else ["id"]
    got = sorted(_arrow_rows(out, names), key=repr)
    assert got == _join_oracle(fact, dim, how)


def test_existence_join_on_decimal128_key():
    fact, dim = _fact_rows(120), _dim_rows()
    plan = P.HashJoin(P.MemoryScan([_fact_batch(fact)]),
                      P.MemoryScan([_dim_batch(dim)]),
                      [col("k")], [col("dk")], how="existence")
    out = AuronSession(device="cpu").collect(plan)
    dim_keys = {dk for dk, _ in dim if dk is not None}
    got = dict(_arrow_rows(out, ["id", "exists"]))
    assert got == {i: k in dim_keys for k, _, i in fact}
    assert 0 < sum(got.values()) < len(fact)


def test_pyudaf_groups_by_decimal128():
    rows = _fact_rows()
    plan = P.PyUdaf(P.MemoryScan([_fact_batch(rows)]), [Aliased(col("k"), "k")],
                    [col("id")], lambda ids: (min(ids), len(ids)),
                    [("first_id", dtypes.int64), ("n", dtypes.int64)])
    out = AuronSession(device="cpu").collect(plan)
    want = {}
    for k, _, i in rows:
        f, n = want.get(k, (i, 0))
        want[k] = (min(f, i), n + 1)
    got = {k: (f, n) for k, f, n in _arrow_rows(out, ["k", "first_id", "n"])}
    assert got == {_dec(k): fn for k, fn in want.items()}


def test_window_row_number_partition_by_decimal128():
    rows = _fact_rows(150)
    plan = P.Window(P.MemoryScan([_fact_batch(rows)]), [col("k")],
                    [(col("id"), True)],
                    [Aliased(WindowFunc("row_number", None), "rn")])
    out = AuronSession(device="cpu").collect(plan)
    seen, want = {}, {}
    for k, _, i in rows:  # ids ascend with the row order
        seen[k] = seen.get(k, 0) + 1
        want[i] = seen[k]
    got = dict(_arrow_rows(out, ["id", "rn"]))
    assert got == want
