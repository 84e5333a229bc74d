"""Exact decimal128 arithmetic, comparison and casts: Spark's result types,
the Python-integer references of the k_dec128_* kernels against an oracle
written here, the expression layer over batches with nulls, and SQL."""
import random
from decimal import Context, Decimal

import pyarrow as pa
import pyarrow.parquet as pq
import pytest
import torch

from auron_amd import AuronSession, dtypes, fused, functions, ops
from auron_amd.column import Column, RecordBatch
from auron_amd.exprs import Abs, Arith, Cast, Cmp, Col, Literal
from auron_amd.plan import nodes as P
from auron_amd.sql import sql_to_plan
from auron_amd.sql.planner import infer_dtype

M64 = (1 << 64) - 1
P38 = 10 ** 38 - 1
D128 = dtypes.decimal128
D64 = dtypes.decimal64
WIDE = Context(prec=80)  # Decimal.scaleb rounds to its context


# ------------------------------------------------------------------ oracle
def rhu(x, d, truncate=False):
    """x / d rounded HALF_UP on the magnitude (ties away from zero)."""
    q, r = divmod(abs(x), d)
    if not truncate and 2 * r >= d:
        q += 1
    return -q if x < 0 else q


def bounded(v, p):
    return None if v is None or abs(v) >= 10 ** p else v


def o_add(a, b, ka, kb, d, p):
    return bounded(rhu(a * 10 ** ka + b * 10 ** kb, 10 ** d), p)


def o_sub(a, b, ka, kb, d, p):
    return bounded(rhu(a * 10 ** ka - b * 10 ** kb, 10 ** d), p)


def o_mul(a, b, d, p):
    return bounded(rhu(a * b, 10 ** d), p)


def o_div(a, b, k, p):
    if b == 0:
        return None
    q = rhu(a * 10 ** k, abs(b))
    return bounded(-q if b < 0 else q, p)


def limbs(vals):
    rows = []
    for v in vals:
        lo = v & M64
        rows.append([lo - (1 << 64) if lo >> 63 else lo, v >> 64])
    return torch.tensor(rows, dtype=torch.int64).reshape(len(rows), 2)


def unlimbs(t):
    return [(int(h) << 64) | (int(l) & M64) for l, h in t.tolist()]


def got_rows(data, valid):
    vals = unlimbs(data) if data.dim() == 2 else [int(v) for v in data.tolist()]
    return [v if ok else None for v, ok in zip(vals, valid.tolist())]


def check(data, valid, want):
    assert got_rows(data, valid) == want
    # a null row stores zero
    zero = [v for v, ok in zip(got_rows(data, torch.ones_like(valid)),
                               valid.tolist()) if not ok]
    assert all(v == 0 for v in zero)


# the edge block: pairs (a, b) for every binary op
EDGE = [
    (0, 0), (0, 1), (1, -1), (-1, 1), (-1, -1),
    (P38, 1), (-P38, -1), (P38, -P38), (-P38, P38), (P38, P38),
    (1 << 63, 1 << 63),            # lo = 2^63
    ((1 << 64) - 1, 1),            # lo = 2^64 - 1: carry into hi
    (-(1 << 64), 1),               # negative with lo = 0
    (-(3 << 64), (1 << 64) + 7),
    (1 << 70, 1 << 60),            # product crosses 2^128
    (-(1 << 100), 1 << 95),        # product crosses 2^192
    ((1 << 120) + 12345, -((1 << 80) + 999)),
    (10, 5), (-10, -5), (20, 5), (-20, -5),  # a+b = +-15, +-25: .5 ties
    (3, 5), (-3, 5), (5, -10), (-5, -10),    # a*b = +-15, +-50: .5 ties
    (1, 2), (-1, 2), (3, -2), (-3, -2),      # a/b = +-0.5, +-1.5: ties
    (7, 0), (-P38, 0),                       # divisor 0
    (P38, 1), (P38, -1),                     # divisor +-1
    (P38, (1 << 64) + 3), (1 << 100, -(1 << 70)),  # divisor > 2^64
    (10 ** 38 - 2, 1), (10 ** 38 - 1, 1),    # sum 10^38 - 1 kept, 10^38 null
    (-(10 ** 38 - 2), -1), (-(10 ** 38 - 1), -1),
    (10 ** 21 - 6, 0), (10 ** 21 - 5, 0),    # /10 at p=20: kept, null
    (10 ** 19, 10 ** 19 - 1), (10 ** 19, 10 ** 19),  # product at 10^38
    (10 ** 20 - 1, 1), (10 ** 20, 1),        # quotient at 10^20
]


def rand_pairs(rng, n, la, lb):
    """Random pairs with up to la / lb decimal digits, a tenth of them tiny."""
    out = []
    for _ in range(n):
        da = rng.randint(0, la) if rng.random() < 0.9 else 1
        db = rng.randint(0, lb) if rng.random() < 0.9 else 1
        out.append((rng.randint(-10 ** da, 10 ** da),
                    rng.randint(-10 ** db, 10 ** db)))
    return out


def assert_mostly_valid(want):
    assert 2 * sum(w is not None for w in want) >= len(want), \
        "random case must keep at least half its rows non-null"


# -------------------------------------------------------------- result type
@pytest.mark.parametrize("op,a,b,want", [
    ("+", D128(38, 2), D64(18, 2), (38, 2)),
    ("-", D128(38, 2), D64(18, 2), (38, 2)),
    ("*", D128(38, 2), D64(7, 2), (38, 4)),
    ("/", D128(38, 2), D64(7, 2), (38, 6)),
    ("*", D128(20, 2), D128(20, 0), (38, 2)),
    ("/", D128(38, 30), D128(38, 30), (38, 6)),
    ("+", D128(20, 2), D128(22, 4), (23, 4)),      # p <= 38: no adjustment
    ("*", D128(20, 2), D64(10, 3), (31, 5)),
    ("/", D128(20, 2), D64(5, 1), (27, 8)),
    ("+", D128(20, 2), dtypes.int32, (21, 2)),     # int32 is (10,0)
    ("*", D128(20, 2), dtypes.int64, (38, 2)),     # int64 is (20,0): p = 41
    ("+", dtypes.int8, D128(20, 0), (21, 0)),
    ("-", dtypes.int16, D128(20, 0), (21, 0)),
    ("+", dtypes.date32, D128(20, 0), (21, 0)),
    ("*", D128(38, 30), D128(38, 30), (38, 21)),
    ("+", D128(38, 10), D128(38, 2), (38, 6)),      # 37 integer digits
])
def test_result_type_table(op, a, b, want):
    dt = dtypes.decimal_result_type(op, a, b)
    assert dt.code == dtypes.DECIMAL128
    assert (dt.precision, dt.scale) == want


def test_result_type_rule_scope():
    # no DECIMAL128 operand, a float operand, or % keep their other routes
    assert dtypes.decimal_result_type("+", D64(18, 2), D64(18, 2)) is None
    assert dtypes.decimal_result_type("+", D128(38, 2), dtypes.float64) is None
    assert dtypes.decimal_result_type("*", dtypes.float32, D128(38, 2)) is None
    assert dtypes.decimal_result_type("%", D128(38, 2), D128(38, 2)) is None
    assert dtypes.decimal_result_type("+", D128(38, 2), dtypes.string) is None


# ------------------------------------------------------- references vs oracle
ADDSUB_PARAMS = [(0, 0, 0, 38), (2, 0, 0, 38), (0, 4, 1, 38), (0, 0, 1, 20),
                 (6, 0, 38, 38), (0, 38, 2, 38)]


@pytest.mark.parametrize("ka,kb,d,p", ADDSUB_PARAMS)
def test_add_sub_ref(ka, kb, d, p):
    rng = random.Random(ka * 100 + kb * 10 + d)
    pairs = EDGE + rand_pairs(rng, 300, min(38, p - 1 - ka + d),
                              min(38, p - 1 - kb + d))
    a, b = limbs([x for x, _ in pairs]), limbs([y for _, y in pairs])
    for fn, oracle in ((ops.dec128_add_ref, o_add), (ops.dec128_sub_ref, o_sub)):
        want = [oracle(x, y, ka, kb, d, p) for x, y in pairs]
        assert_mostly_valid(want[len(EDGE):])
        check(*fn(a, b, ka, kb, d, p), want)


def test_add_edges_named():
    # the bound and the ties, spelled out rather than left to the oracle
    a = limbs([10 ** 38 - 2, 10 ** 38 - 1, 10, -10, 20, -20, (1 << 64) - 1,
               10 ** 21 - 6, 10 ** 21 - 5])
    b = limbs([1, 1, 5, -5, 5, -5, 1, 0, 0])
    data, valid = ops.dec128_add_ref(a, b, 0, 0, 0, 38)
    assert got_rows(data, valid)[:2] == [10 ** 38 - 1, None]
    assert got_rows(data, valid)[6] == 1 << 64
    data, valid = ops.dec128_add_ref(a, b, 0, 0, 1, 20)
    assert got_rows(data, valid)[2:6] == [2, -2, 3, -3]
    assert got_rows(data, valid)[7:] == [10 ** 20 - 1, None]


@pytest.mark.parametrize("d,p", [(0, 38), (1, 38), (2, 38), (38, 38), (4, 20)])
def test_mul_ref(d, p):
    rng = random.Random(d * 50 + p)
    half = (p - 1 + d) // 2
    pairs = EDGE + rand_pairs(rng, 300, min(38, half), min(38, half))
    a, b = limbs([x for x, _ in pairs]), limbs([y for _, y in pairs])
    want = [o_mul(x, y, d, p) for x, y in pairs]
    assert_mostly_valid(want[len(EDGE):])
    check(*ops.dec128_mul_ref(a, b, d, p), want)
    if (d, p) == (0, 38):
        by_pair = dict(zip(pairs, want))
        assert by_pair[(10 ** 19, 10 ** 19 - 1)] == 10 ** 38 - 10 ** 19
        assert by_pair[(10 ** 19, 10 ** 19)] is None
    if d == 1:
        by_pair = dict(zip(pairs, want))
        assert (by_pair[(3, 5)], by_pair[(-3, 5)]) == (2, -2)
        assert (by_pair[(5, -10)], by_pair[(-5, -10)]) == (-5, 5)


@pytest.mark.parametrize("k,p", [(0, 38), (1, 38), (6, 38), (38, 38), (0, 20),
                                 (44, 38)])
def test_div_ref(k, p):
    rng = random.Random(k * 50 + p)
    pairs = list(EDGE)
    for _ in range(300):
        # enough divisor digits that a * 10^k / b stays below 10^(p-1)
        db = rng.randint(max(1, k - p + 2), 38)
        da = rng.randint(0, min(38, p - 1 - k + db - 1))
        b = rng.randint(10 ** (db - 1), 10 ** db - 1) * rng.choice((-1, 1))
        pairs.append((rng.randint(-10 ** da, 10 ** da), b))
    a, b = limbs([x for x, _ in pairs]), limbs([y for _, y in pairs])
    want = [o_div(x, y, k, p) for x, y in pairs]
    assert_mostly_valid(want[len(EDGE):])
    check(*ops.dec128_div_ref(a, b, k, p), want)
    by_pair = dict(zip(pairs, want))
    assert by_pair[(7, 0)] is None and by_pair[(-P38, 0)] is None
    if (k, p) == (0, 38):
        assert [by_pair[q] for q in ((1, 2), (-1, 2), (3, -2), (-3, -2))] \
            == [1, -1, -2, 2]
        assert (by_pair[(P38, 1)], by_pair[(P38, -1)]) == (P38, -P38)
    if (k, p) == (0, 20):
        assert by_pair[(10 ** 20 - 1, 1)] == 10 ** 20 - 1
        assert by_pair[(10 ** 20, 1)] is None


@pytest.mark.parametrize("ka,kb", [(0, 0), (4, 0), (0, 38), (38, 0)])
def test_cmp_ref(ka, kb):
    import operator

    rng = random.Random(ka + kb)
    pairs = EDGE + rand_pairs(rng, 200, 38, 38)
    pairs += [(x * 10 ** kb, x * 10 ** ka) for x in (-1, 0, 1)]  # equal
    a, b = limbs([x for x, _ in pairs]), limbs([y for _, y in pairs])
    for op, fn in (("==", operator.eq), ("!=", operator.ne), ("<", operator.lt),
                   ("<=", operator.le), (">", operator.gt), (">=", operator.ge)):
        want = [fn(x * 10 ** ka, y * 10 ** kb) for x, y in pairs]
        assert ops.dec128_cmp_ref(a, b, ka, kb, op).tolist() == want


def test_rescale_ref():
    vals = [x for pair in EDGE for x in pair] + [-(1 << 127), (1 << 127) - 1,
                                                  149, 150, -149, -150]
    x = limbs(vals)
    for k, p in ((0, 38), (2, 38), (-2, 38), (-38, 38), (38, 38), (-1, 20),
                 (0, 5)):
        pk = 10 ** abs(k)
        want = [bounded(v * pk if k >= 0 else rhu(v, pk), p) for v in vals]
        check(*ops.dec128_rescale_ref(x, k, p), want)
    want = [bounded(abs(v), 38) for v in vals]
    check(*ops.dec128_rescale_ref(x, 0, 38, abs_=True), want)
    want = [bounded(-v, 38) for v in vals]
    check(*ops.dec128_rescale_ref(x, 0, 38, negate=True), want)
    # into int64: toward zero, the two's-complement range kept whole
    big = limbs([-(1 << 63) * 100 - 99, -(1 << 63) * 100 - 100,
                 ((1 << 63) - 1) * 100 + 99, (1 << 63) * 100, 199, -199])
    data, valid = ops.dec128_rescale_ref(big, -2, bound=1 << 63, truncate=True,
                                         asym=True, narrow_out=True)
    assert data.dim() == 1
    assert got_rows(data, valid) == [-(1 << 63), None, (1 << 63) - 1, None,
                                     1, -1]


def test_narrow_operands_and_validity():
    """int64 [n] operands are sign-extended; input validities fold in."""
    a = [5, -7, (1 << 63) - 1, -(1 << 63), 0, 123]
    b = [P38, -P38, 1 << 100, -(1 << 100), 9, 10]
    ta, tb = torch.tensor(a, dtype=torch.int64), limbs(b)
    va = torch.tensor([True, True, True, True, False, True])
    vb = torch.tensor([True, False, True, True, True, True])

    def mask(want):
        return [w if x and y else None
                for w, x, y in zip(want, va.tolist(), vb.tolist())]

    check(*ops.dec128_add_ref(ta, tb, 2, 0, 0, 38, va, vb),
          mask([o_add(x, y, 2, 0, 0, 38) for x, y in zip(a, b)]))
    check(*ops.dec128_sub_ref(tb, ta, 0, 2, 0, 38, vb, va),
          mask([o_sub(y, x, 0, 2, 0, 38) for x, y in zip(a, b)]))
    check(*ops.dec128_mul_ref(ta, tb, 3, 38, va, vb),
          mask([o_mul(x, y, 3, 38) for x, y in zip(a, b)]))
    check(*ops.dec128_div_ref(tb, ta, 4, 38, vb, va),
          mask([o_div(y, x, 4, 38) for x, y in zip(a, b)]))
    i32 = torch.tensor([1, -2, 3, -4, 5, -6], dtype=torch.int32)
    assert ops.dec128_cmp_ref(i32, tb, 0, 0, "<").tolist() == \
        [x < y for x, y in zip(i32.tolist(), b)]
    # on the CPU the dispatching names run the reference
    check(*ops.dec128_add(ta, tb, 2, 0, 0, 38, va, vb),
          mask([o_add(x, y, 2, 0, 0, 38) for x, y in zip(a, b)]))


# ----------------------------------------------------------- expression layer
def dec_col(ints, p, s, nulls=()):
    valid = None
    if nulls:
        valid = torch.tensor([i not in nulls for i in range(len(ints))])
    return Column(D128(p, s), limbs(ints), valid)


def dec_values(c):
    """Unscaled ints (None = null) of a decimal column, exactly."""
    sc = c.dtype.scale
    return [None if v is None else int(v.scaleb(sc, context=WIDE))
            for v in c.to_arrow().to_pylist()]


@pytest.fixture(scope="module")
def batch():
    rng = random.Random(42)
    n = 64
    d1 = [rng.randint(-10 ** 30, 10 ** 30) for _ in range(n)]
    d2 = [rng.randint(-10 ** 20, 10 ** 20) for _ in range(n)]
    d1[:4] = [P38, -P38, 0, 10 ** 37]
    d2[:4] = [P38 // 10 ** 4, 1, 0, 0]
    e = [rng.randint(-10 ** 7 + 1, 10 ** 7 - 1) for _ in range(n)]
    e[5] = 0
    i = [rng.randint(-2 ** 31, 2 ** 31 - 1) for _ in range(n)]
    i[6] = 0
    f = [rng.uniform(-100, 100) for _ in range(n)]
    cols = [dec_col(d1, 38, 2, nulls={7, 9}), dec_col(d2, 30, 6, nulls={9, 11}),
            Column(D64(7, 2), torch.tensor(e), torch.tensor(
                [k != 13 for k in range(n)])),
            Column(dtypes.int32, torch.tensor(i, dtype=torch.int32)),
            Column(dtypes.float64, torch.tensor(f, dtype=torch.float64))]
    b = RecordBatch(["d1", "d2", "e", "i", "f"], cols)
    raw = {"d1": [None if k in (7, 9) else v for k, v in enumerate(d1)],
           "d2": [None if k in (9, 11) else v for k, v in enumerate(d2)],
           "e": [None if k == 13 else v for k, v in enumerate(e)],
           "i": i}
    return b, raw


def _scale(dt):
    return dtypes.decimal_operand(dt)[1]


def expect_arith(op, x, y, lt, rt):
    out = dtypes.decimal_result_type(op, lt, rt)
    s1, s2 = _scale(lt), _scale(rt)
    want = []
    for a, b in zip(x, y):
        if a is None or b is None:
            want.append(None)
        elif op in "+-":
            s = max(s1, s2)
            f = o_add if op == "+" else o_sub
            want.append(f(a, b, s - s1, s - s2, s - out.scale, out.precision))
        elif op == "*":
            want.append(o_mul(a, b, s1 + s2 - out.scale, out.precision))
        else:
            want.append(o_div(a, b, out.scale - s1 + s2, out.precision))
    return out, want


PAIRS = [("d1", "d2"), ("d2", "d1"), ("d1", "d1"), ("d1", "e"), ("e", "d1"),
         ("d2", "i"), ("i", "d2")]


@pytest.mark.parametrize("op", ["+", "-", "*", "/"])
@pytest.mark.parametrize("ln,rn", PAIRS)
def test_arith_expr(batch, op, ln, rn):
    b, raw = batch
    lt, rt = b.column(ln).dtype, b.column(rn).dtype
    e = Arith(op, Col(ln), Col(rn))
    got = e.eval(b)
    out, want = expect_arith(op, raw[ln], raw[rn], lt, rt)
    assert got.dtype == out
    assert dec_values(got) == want
    assert any(w is not None for w in want)
    types = {nm: b.column(nm).dtype for nm in b.names}
    assert infer_dtype(e, types) == got.dtype


@pytest.mark.parametrize("op", ["==", "!=", "<", "<=", ">", ">="])
@pytest.mark.parametrize("ln,rn", PAIRS)
def test_cmp_expr(batch, op, ln, rn):
    import operator

    b, raw = batch
    fn = {"==": operator.eq, "!=": operator.ne, "<": operator.lt,
          "<=": operator.le, ">": operator.gt, ">=": operator.ge}[op]
    s1, s2 = _scale(b.column(ln).dtype), _scale(b.column(rn).dtype)
    got = Cmp(op, Col(ln), Col(rn)).eval(b)
    assert got.dtype == dtypes.bool_ and got.data.shape == (b.num_rows,)
    want = [None if x is None or y is None
            else fn(x * 10 ** s2, y * 10 ** s1)
            for x, y in zip(raw[ln], raw[rn])]
    assert got.to_pylist() == want


def test_int_literal_operand(batch):
    b, raw = batch
    got = Arith("*", Col("d1"), Literal(3)).eval(b)
    assert got.dtype == D128(38, 2)
    assert dec_values(got) == [None if v is None else bounded(3 * v, 38)
                               for v in raw["d1"]]
    got = Cmp(">", Col("d1"), Literal(0)).eval(b)
    assert got.to_pylist() == [None if v is None else v > 0 for v in raw["d1"]]


def test_float_operand_stays_float64(batch):
    b, _ = batch
    for op in "+-*/":
        assert Arith(op, Col("d1"), Col("f")).eval(b).dtype == dtypes.float64
        assert Arith(op, Col("f"), Col("d2")).eval(b).dtype == dtypes.float64
    got = Cmp(">", Col("d2"), Literal(0.0)).eval(b)
    assert got.data.shape == (b.num_rows,)


def test_abs_expr(batch):
    b, raw = batch
    got = Abs(Col("d1")).eval(b)
    assert got.dtype == b.column("d1").dtype
    assert dec_values(got) == [None if v is None else abs(v) for v in raw["d1"]]


def test_cast_decimal_to_decimal(batch):
    b, raw = batch
    # widen the scale: exact; 38-digit rows no longer fit
    got = Cast(Col("d1"), D128(38, 6)).eval(b)
    assert dec_values(got) == [None if v is None else bounded(v * 10 ** 4, 38)
                               for v in raw["d1"]]
    # narrow the scale: HALF_UP
    got = Cast(Col("d2"), D128(30, 1)).eval(b)
    assert dec_values(got) == [None if v is None else bounded(rhu(v, 10 ** 5), 30)
                               for v in raw["d2"]]
    # narrow the precision only
    got = Cast(Col("d1"), D128(20, 2)).eval(b)
    assert dec_values(got) == [None if v is None else bounded(v, 20)
                               for v in raw["d1"]]
    # into decimal64: overflow is NULL, not an exception
    got = Cast(Col("d2"), D64(18, 2)).eval(b)
    assert got.dtype.code == dtypes.DECIMAL64 and got.data.dim() == 1
    want = [None if v is None else bounded(rhu(v, 10 ** 4), 18)
            for v in raw["d2"]]
    assert dec_values(got) == want
    assert any(w is None and v is not None for w, v in zip(want, raw["d2"]))
    got = Cast(Col("d1"), D64(18, 2)).eval(b)  # same scale
    assert dec_values(got) == [None if v is None else bounded(v, 18)
                               for v in raw["d1"]]


def test_cast_to_decimal128_from_narrow(batch):
    b, raw = batch
    got = Cast(Col("e"), D128(38, 30)).eval(b)
    assert dec_values(got) == [None if v is None else v * 10 ** 28
                               for v in raw["e"]]
    got = Cast(Col("e"), D128(20, 1)).eval(b)
    assert dec_values(got) == [None if v is None else rhu(v, 10)
                               for v in raw["e"]]
    got = Cast(Col("i"), D128(38, 25)).eval(b)
    assert dec_values(got) == [v * 10 ** 25 for v in raw["i"]]
    big = Column(dtypes.int64, torch.tensor([2 ** 63 - 1, -2 ** 63, 0, 12]))
    got = Cast(Col("x"), D128(38, 19)).eval(RecordBatch(["x"], [big]))
    assert dec_values(got) == [(2 ** 63 - 1) * 10 ** 19, -2 ** 63 * 10 ** 19,
                               0, 12 * 10 ** 19]
    got = Cast(Col("x"), D128(20, 2)).eval(RecordBatch(["x"], [big]))
    assert dec_values(got) == [None, None, 0, 1200]


def test_cast_decimal128_to_integers():
    vals = [199, -199, 0, (2 ** 63 - 1) * 100 + 99, 2 ** 63 * 100,
            -2 ** 63 * 100 - 99, -2 ** 63 * 100 - 100, (2 ** 31 - 1) * 100,
            2 ** 31 * 100, -2 ** 31 * 100 - 50, P38]
    b = RecordBatch(["d"], [dec_col(vals, 38, 2, nulls={2})])
    got = Cast(Col("d"), dtypes.int64).eval(b)
    assert got.data.dtype == torch.int64
    assert got.to_pylist() == [1, -1, None, 2 ** 63 - 1, None, -2 ** 63, None,
                               2 ** 31 - 1, 2 ** 31, -2 ** 31, None]
    got = Cast(Col("d"), dtypes.int32).eval(b)
    assert got.data.dtype == torch.int32
    assert got.to_pylist() == [1, -1, None, None, None, None, None,
                               2 ** 31 - 1, None, -2 ** 31, None]


def test_cast_string_to_decimal128():
    strs = ["123456789012345678901.455", "-123456789012345678901.445",
            "0.005", "-0.005", " 42 ", "abc", None, "9" * 36 + ".994",
            "9" * 36 + ".995", "1e3", "NaN", ""]
    b = RecordBatch(["s"], [Column.from_pylist(strs, dtypes.string)])
    got = Cast(Col("s"), D128(38, 2)).eval(b)
    assert got.dtype == D128(38, 2)
    assert dec_values(got) == [
        12345678901234567890146, -12345678901234567890145, 1, -1, 4200, None,
        None, 10 ** 38 - 1, None, 100000, None, None]


def test_check_overflow_and_make_decimal(batch):
    b, raw = batch
    got = functions.CheckOverflow(Col("d1"), 25, 2).eval(b)
    assert got.dtype == D128(25, 2)
    want = [None if v is None else bounded(v, 25) for v in raw["d1"]]
    assert dec_values(got) == want
    assert any(w is None and v is not None for w, v in zip(want, raw["d1"]))
    x = Column(dtypes.int64, torch.tensor([2 ** 63 - 1, -2 ** 63, 5, 0]),
               torch.tensor([True, True, True, False]))
    got = functions.MakeDecimal(Col("x"), 30, 4).eval(RecordBatch(["x"], [x]))
    assert got.dtype == D128(30, 4)
    assert dec_values(got) == [2 ** 63 - 1, -2 ** 63, 5, None]
    got = functions.MakeDecimal(Col("x"), 18, 4).eval(RecordBatch(["x"], [x]))
    assert got.dtype.code == dtypes.DECIMAL64


def test_exotic_scales_take_reference():
    """(38,30)*(38,30) divides by 10^39 and (38,0)/(38,38) multiplies by
    10^76: beyond the kernels' table, still exact."""
    a = dec_col([3 * 10 ** 30 + 5, -7 * 10 ** 29], 38, 30)
    b = RecordBatch(["a"], [a])
    got = Arith("*", Col("a"), Col("a")).eval(b)
    assert got.dtype == D128(38, 21)
    assert dec_values(got) == [o_mul(v, v, 39, 38) for v in unlimbs(a.data)]
    x, y = dec_col([5, -1], 38, 0), dec_col([2 * 10 ** 38 // 10, 3], 38, 38)
    got = Arith("/", Col("x"), Col("y")).eval(RecordBatch(["x", "y"], [x, y]))
    assert got.dtype == D128(38, 6)
    assert dec_values(got) == [o_div(5, 2 * 10 ** 37, 44, 38),
                               o_div(-1, 3, 44, 38)]


def test_fused_interpreter_refuses_decimal128():
    schema = {"d": D128(38, 2), "x": dtypes.int64, "e": D64(7, 2)}
    trees = [Arith("+", Col("d"), Col("x")), Cmp(">", Col("d"), Col("e")),
             Cast(Col("x"), D128(38, 2)), Cast(Col("d"), dtypes.int64),
             Col("d"), Arith("*", Col("x"), Literal(1, D128(20, 0))),
             Col("d").is_null()]
    for t in trees:
        assert fused.compile_exprs([t], schema) is None, t
    # a neighbour without decimal128 still compiles
    prog = fused.compile_exprs([trees[0], Arith("+", Col("x"), Literal(1))],
                               schema)
    assert prog is not None and prog.expr_idx == [1]


def test_config_option_registered():
    from auron_amd.config import DECIMAL128_NATIVE_ARITH, AuronConf

    assert DECIMAL128_NATIVE_ARITH.key == \
        "spark.auron.decimal128.nativeArith.enable"
    assert AuronConf().get(DECIMAL128_NATIVE_ARITH) is True


# ------------------------------------------------------------------------ SQL
S21 = ["123456789012345678901", "-987654321098765432109.995", None,
       "555555555555555555555.005", "not a number", "100000000000000000000"]
A64 = [2 ** 63 - 1, -2 ** 63, 12, None, 7, -7]
B64 = [3, -4, 5, 6, None, 1000]
G = [0, 1, 0, 1, 0, 1]
DA = [P38, -P38, 150, 150, None, 0]        # decimal(38,2)
DB = [10 ** 29, -10 ** 29, 15000, 15001, 1, 0]  # decimal(30,4)


@pytest.fixture()
def env(tmp_path):
    p = str(tmp_path / "t.parquet")
    tbl = pa.table({
        "s": S21,
        "a": pa.array(A64, pa.int64()),
        "b": pa.array(B64, pa.int64()),
        "g": pa.array(G, pa.int64()),
        "d1": pa.array([None if v is None else Decimal(v).scaleb(-2, context=WIDE)
                        for v in DA], pa.decimal128(38, 2)),
        "d2": pa.array([Decimal(v).scaleb(-4, context=WIDE) for v in DB],
                       pa.decimal128(30, 4)),
    })
    pq.write_table(tbl, p)
    sch = {"t": {"s": dtypes.string, "a": dtypes.int64, "b": dtypes.int64,
                 "g": dtypes.int64, "d1": D128(38, 2), "d2": D128(30, 4)}}

    class Cat:
        def scan(self, table, columns=None):
            return P.ParquetScan([p], columns=columns)

    s = AuronSession()
    return lambda sql: s.collect(sql_to_plan(sql, Cat(), s, schemas=sch))


def test_sql_cast_to_decimal38(env):
    out = env("select cast(s as decimal(38,2)) cs, cast(a as decimal(38,2)) ca "
              "from t")
    assert out.column("cs").dtype == D128(38, 2)
    assert out.column("ca").dtype == D128(38, 2)
    assert dec_values(out.column("cs")) == [
        12345678901234567890100, -98765432109876543211000, None,
        55555555555555555555501, None, 10000000000000000000000]
    assert dec_values(out.column("ca")) == [
        None if v is None else v * 100 for v in A64]


def test_sql_grouped_sum_of_product(env):
    out = env("select g, sum(cast(a as decimal(38,2)) * b) sp from t "
              "group by g order by g")
    assert out.column("sp").dtype.code == dtypes.DECIMAL128
    assert out.column("sp").dtype.scale == 2
    want = {}
    for g, a, b in zip(G, A64, B64):
        if a is not None and b is not None:
            want[g] = want.get(g, 0) + a * 100 * b
    assert any(abs(v) > 2 ** 64 for v in want.values())
    assert dict(zip(out.column("g").to_pylist(),
                    dec_values(out.column("sp")))) == want


def test_sql_where_compares_two_scales(env):
    out = env("select g, b from t where d1 > d2 order by b")
    want = sorted(b for b, x, y in zip(B64, DA, DB)
                  if x is not None and b is not None and x * 100 > y)
    assert out.column("b").to_pylist() == want
    out = env("select b from t where d1 = d2 order by b")
    assert out.column("b").to_pylist() == sorted(
        b for b, x, y in zip(B64, DA, DB)
        if x is not None and b is not None and x * 100 == y)


def test_sql_division_with_zero_divisor(env):
    out = env("select a, d2 / d1 q, d1 + d2 s, d1 - d2 m from t")
    lt, rt = D128(30, 4), D128(38, 2)
    dt, want = expect_arith("/", DB, DA, lt, rt)
    assert out.column("q").dtype == dt
    assert dec_values(out.column("q")) == want
    assert want[5] is None and DA[5] == 0  # the zero-divisor row
    assert sum(w is not None for w in want) >= 3
    dt, want = expect_arith("+", DA, DB, rt, lt)
    assert out.column("s").dtype == dt and dec_values(out.column("s")) == want
    dt, want = expect_arith("-", DA, DB, rt, lt)
    assert out.column("m").dtype == dt and dec_values(out.column("m")) == want
