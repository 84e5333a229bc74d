"""Inputs, the expression battery and the comparison for the scalar-
expression tests. It is a plain module like agg_cases.py, not a conftest:
the CPU file (test_expr_semantics.py) and the GPU file
(test_gpu_expr_edges.py) share one deterministic 777-row batch, one battery
and one oracle result (expr_oracle.py), computed once per process.

Batch layout. 777 rows: no multiple of 64 or 256, so the last wave and the
last block are partial. Rows 0..342 are edge rows, every column valid:
  i32a x i32b x d    the full 7 x 7 x 7 product of the int32 edge list
  i64a x i64b, i8 x i16, p x q    full 7 x 7 products (rows 0..48, repeated)
  f x g              the full 17 x 17 product of the float edges (0..288)
Rows 343..776 are random with about 36 % NULL per column, which makes about
20 % over the whole column; the data under a NULL is random, not zero.
`i16` has validity None, `nul` is NULL in every row.
"""
import math
import random
import struct

import torch

import expr_oracle as O
from auron_amd import dtypes
from auron_amd.column import Column, RecordBatch
from auron_amd.exprs import (Arith, BoolOp, CaseWhen, Cast, Cmp, Coalesce,
                             Col, InList, IsNull, Literal, Not)

N = 777
N_EDGE = 343
DEC = dtypes.decimal64(7, 2)
DEC4 = dtypes.decimal64(12, 4)
DEC18 = dtypes.decimal64(18, 4)

SCHEMA = {
    "i8": dtypes.int8, "i16": dtypes.int16,
    "i32a": dtypes.int32, "i32b": dtypes.int32,
    "i64a": dtypes.int64, "i64b": dtypes.int64,
    "d": dtypes.date32, "d2": dtypes.date32,
    "flag": dtypes.bool_, "flag2": dtypes.bool_,
    "f": dtypes.float64, "g": dtypes.float64,
    "p": DEC, "q": DEC, "p4": DEC4,
    "nul": dtypes.int64,
}


def int_edges(bits):
    lo, hi = -(1 << (bits - 1)), (1 << (bits - 1)) - 1
    return [lo, lo + 1, -1, 0, 1, hi - 1, hi]


SUBNORMAL = 5e-324
FLOAT_EDGES = [
    0.0, -0.0, 1.5, -1.5, math.inf, -math.inf, math.nan,
    0.125, 0.375,                      # x100 lands exactly on .5
    2.0 ** 31, -2.0 ** 31 - 1, 3e9, 2.0 ** 53 + 2, 2.0 ** 63, -2.0 ** 63,
    1e19, SUBNORMAL,
]
# unscaled decimal(7,2) edges; precision is not enforced, so the int64
# bounds are legal contents and make p + q wrap and Cast(p, int32) saturate
DEC_EDGES = [O.I64_MIN, -150, -1, 0, 1, 125, O.I64_MAX]


def _build():
    rng = random.Random(20240611)
    e8, e16, e32, e64 = (int_edges(b) for b in (8, 16, 32, 64))
    nf = len(FLOAT_EDGES)

    def rint(bits):
        # half small (so % and == find partners), half anywhere in range
        if rng.random() < 0.5:
            return rng.randint(-100, 100) if bits > 8 else rng.randint(-9, 9)
        return rng.randint(-(1 << (bits - 1)), (1 << (bits - 1)) - 1)

    def rfloat():
        k = rng.random()
        if k < 0.4:
            return rng.uniform(-1000.0, 1000.0)
        if k < 0.7:
            return rng.randint(-4000, 4000) / 8.0      # exact, many ties
        if k < 0.85:
            return rng.uniform(-1.0, 1.0) * 10.0 ** rng.randint(-300, 300)
        return rng.choice(FLOAT_EDGES)

    gen = {
        "i8": lambda r: e8[r % 7] if r < N_EDGE else rint(8),
        "i16": lambda r: e16[(r // 7) % 7] if r < N_EDGE else rint(16),
        "i32a": lambda r: e32[(r // 7) % 7] if r < N_EDGE else rint(32),
        "i32b": lambda r: e32[r % 7] if r < N_EDGE else rint(32),
        "i64a": lambda r: e64[(r // 7) % 7] if r < N_EDGE else rint(64),
        "i64b": lambda r: e64[r % 7] if r < N_EDGE else rint(64),
        "d": lambda r: (e32[(r // 49) % 7] if r < N_EDGE
                        else 10950 + rng.randint(0, 20)),
        "d2": lambda r: 10957 + (r % 5),
        "flag": lambda r: rng.random() < 0.5,
        "flag2": lambda r: rng.random() < 0.5,
        "f": lambda r: (FLOAT_EDGES[r // nf] if r < nf * nf else rfloat()),
        "g": lambda r: (FLOAT_EDGES[r % nf] if r < nf * nf else rfloat()),
        "p": lambda r: (DEC_EDGES[r % 7] if r < N_EDGE
                        else rng.randint(-10 ** 7 + 1, 10 ** 7 - 1)),
        "q": lambda r: (DEC_EDGES[(r // 7) % 7] if r < N_EDGE
                        else rng.randint(-10 ** 7 + 1, 10 ** 7 - 1)),
        "p4": lambda r: rng.randint(-10 ** 12 + 1, 10 ** 12 - 1),
        "nul": lambda r: rng.randint(-5, 5),
    }
    raw, valid = {}, {}
    for nm in SCHEMA:
        raw[nm] = [gen[nm](r) for r in range(N)]
        if nm == "i16":
            valid[nm] = None
        elif nm == "nul":
            valid[nm] = [False] * N
        else:
            valid[nm] = [r < N_EDGE or rng.random() >= 0.36
                         for r in range(N)]
    cols = {nm: [v if (valid[nm] is None or valid[nm][r]) else None
                 for r, v in enumerate(raw[nm])] for nm in SCHEMA}
    tcols = []
    for nm, dt in SCHEMA.items():
        data = torch.tensor(raw[nm], dtype=dt.torch_dtype)
        v = None if valid[nm] is None else torch.tensor(valid[nm],
                                                        dtype=torch.bool)
        tcols.append(Column(dt, data, v))
    return cols, RecordBatch(list(SCHEMA), tcols)


_CACHE = {}


def columns():
    """The oracle's view: column name -> list of values (None = NULL)."""
    if "b" not in _CACHE:
        _CACHE["b"] = _build()
    return _CACHE["b"][0]


def batch(device="cpu"):
    """The same rows as a RecordBatch (built once; never mutated)."""
    columns()
    rb = _CACHE["b"][1]
    return rb if str(device) == "cpu" else rb.to(device)


def c(name):
    return Col(name)


def battery():
    """[(name, expr)]: everything tests/test_fused.py's battery holds, every
    opcode the compiler can emit, and each known defect by construction."""
    i8, i16, i32a, i32b, i64a, i64b = (c(n) for n in
                                       "i8 i16 i32a i32b i64a i64b".split())
    d, flag, f, g, p, q, p4, nul = (c(n) for n in
                                    "d flag f g p q p4 nul".split())
    nullable_cmp = Cmp(">", i64a, Literal(0))
    out = [
        # ---- the test_fused battery, on this batch's columns
        ("arith_chain", (i64a + i32a) * Literal(3) - Literal(1)),
        ("mod_lit", Arith("%", i64a, Literal(7))),
        ("int_div", i64a / i32b),
        ("dec_add", p + q),
        ("dec_mul", p * q),
        ("dec_sub_lit", p - Literal(1.5, DEC)),
        ("dec_lt_lit", Cmp("<", p, Literal(9.0))),
        ("ge_mixed", Cmp(">=", i64a, i32b)),
        ("date_eq", Cmp("==", d, Literal(10957))),
        ("and3", BoolOp("and", [Cmp(">", i64a, Literal(2)),
                                Cmp("<", i32b, Literal(50)),
                                Not(Cmp("==", i64a, i32b))])),
        ("or_isnull", BoolOp("or", [IsNull(p), Cmp(">", q, Literal(1.0))])),
        ("case_dec", CaseWhen([(Cmp(">", i64a, Literal(5)), p),
                               (Cmp(">", i64a, Literal(2)), q)],
                              otherwise=Literal(0.0, DEC))),
        ("case_noelse", CaseWhen([(Cmp(">", f, Literal(0.5)), i64a)])),
        ("coalesce_dec", Coalesce([p, q, Literal(7.5, DEC)])),
        ("in_i32", InList(i32b, [1, 5, 9, 33])),
        ("in_dec", InList(p, [1.25, 3.5])),
        ("cast_i64_f64", Cast(i64a, dtypes.float64)),
        ("cast_f_i64", Cast(f, dtypes.int64)),
        ("cast_dec_f64", Cast(p, dtypes.float64)),
        ("cast_f_dec", Cast(f, DEC)),
        ("date_add_lit", Arith("+", d, Literal(30))),
        ("not_flag", Not(flag)),
        ("and_flag", BoolOp("and", [flag, Cmp("!=", i64a, Literal(0))])),
        # ---- narrow integers must wrap between operators
        ("wrap_add_gt", Cmp(">", i32a + i32b, Literal(0))),
        ("wrap_mul_cast", Cast(i32a * i32b, dtypes.int64)),
        ("wrap_i8_div", (i8 + i8) / Literal(2)),
        ("wrap_mul_mod", Arith("%", i32a * i32b, i32b)),
        ("wrap_date_add", d + i32a),
        ("wrap_sub_i32", Cmp("<", i32a - i32b, Literal(0))),
        ("wrap_i16_mul", Cast(i16 * i8, dtypes.int32)),
        ("mul_i64", i64a * i64b),
        # ---- % : MIN % -1, x % 0, sign of the dividend
        ("mod_i64", Arith("%", i64a, i64b)),
        ("mod_i32", Arith("%", i32a, i32b)),
        ("mod_f", Arith("%", f, g)),             # eval path only
        # ---- float -> int, decimal -> int, -> decimal
        ("cast_f_i8", Cast(f, dtypes.int8)),
        ("cast_f_i16", Cast(f, dtypes.int16)),
        ("cast_f_i32", Cast(f, dtypes.int32)),
        ("cast_dec_i32", Cast(p, dtypes.int32)),
        ("cast_i64_dec18", Cast(i64a, DEC18)),
        ("cast_i32_dec", Cast(i32a, DEC)),       # too narrow to overflow
        ("cast_dec_down", Cast(p4, DEC)),
        ("cast_dec_up", Cast(p, DEC4)),
        ("cast_i32_bool", Cast(i32a, dtypes.bool_)),
        ("cast_i64_i8", Cast(i64a, dtypes.int8)),
        # ---- float comparisons and arithmetic
        ("f_lt", Cmp("<", f, g)), ("f_le", Cmp("<=", f, g)),
        ("f_gt", Cmp(">", f, g)), ("f_ge", Cmp(">=", f, g)),
        ("f_eq", Cmp("==", f, g)), ("f_ne", Cmp("!=", f, g)),
        ("f_add", f + g), ("f_sub", f - g), ("f_mul", f * g),
        ("f_div", f / g),
        ("dec_mixed_scale", p4 + p),
        ("le_narrow", Cmp("<=", i16, i8)),
        # ---- three-valued logic
        ("kleene_and", BoolOp("and", [flag, nullable_cmp])),
        ("kleene_or", BoolOp("or", [flag, nullable_cmp])),
        ("and_nonbool", BoolOp("and", [i8, flag])),
        ("case_nullcond_else", CaseWhen([(flag, i32a)], otherwise=i64b)),
        ("case_nullcond_noelse", CaseWhen([(flag, f)])),
        ("coalesce3", Coalesce([i64a, nul, i64b])),
        ("coalesce3_null_last", Coalesce([i32a, i32b, Literal(None)])),
        ("in_empty", InList(i32a, [])),
        ("in_with_none", InList(i64a, [0, None, -1, O.I64_MAX])),
        ("in_f", InList(f, [1.5, 0.0, 3e9])),
    ]
    return out


def right_nested_sum(n):
    """c0 + (c1 + (... + c15)): n operands, so the stack grows n deep.
    The first operand (c0) and the deepest (c15) are columns no other
    operand uses; the ones between cycle through c1..c14."""
    names = ["c0"] + [f"c{1 + (k - 1) % 14}" for k in range(1, n - 1)] \
        + ["c15"]
    e = Col(names[-1])
    for nm in reversed(names[:-1]):
        e = Arith("+", Col(nm), e)
    return e


EVAL_ONLY = {"mod_f"}   # the fused compiler refuses float `%`


def expected():
    """name -> (dtype, values): the oracle over the 777 rows, once."""
    if "exp" not in _CACHE:
        cols = columns()
        _CACHE["exp"] = {nm: O.eval_column(e, cols, SCHEMA)
                         for nm, e in battery()}
    return _CACHE["exp"]


# -------------------------------------------------------------- comparison
_NAN_BITS = 0x7FF8000000000000


def _bits(x):
    if x != x:
        return _NAN_BITS
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def expected_tensors(dt, values):
    """(data, valid) CPU tensors of an oracle column; float64 data is kept
    as int64 bit patterns with every NaN folded into one."""
    valid = torch.tensor([v is not None for v in values], dtype=torch.bool)
    if dt.code == dtypes.FLOAT64:
        bits = [0 if v is None else _bits(v) for v in values]
        data = torch.tensor([b - (1 << 64) if b >> 63 else b for b in bits],
                            dtype=torch.int64)
    elif dt.code == dtypes.BOOL:
        data = torch.tensor([bool(v) for v in values], dtype=torch.bool)
    else:
        data = torch.tensor([0 if v is None else v for v in values],
                            dtype=torch.int64)
    return data, valid


def comparable(col):
    """(data, valid) of a result Column in the form expected_tensors uses."""
    n = len(col)
    data = col.data.cpu()
    valid = (torch.ones(n, dtype=torch.bool) if col.validity is None
             else col.validity.cpu().bool())
    if col.dtype.code == dtypes.FLOAT64:
        assert data.dtype == torch.float64
        nan = data != data
        data = data.contiguous().view(torch.int64)
        data = torch.where(nan, torch.full_like(data, _NAN_BITS), data)
    elif col.dtype.code == dtypes.BOOL:
        data = data.bool()
    else:
        assert data.dtype == col.dtype.torch_dtype
        data = data.to(torch.int64)
    return data, valid


def mismatch(col, dt, want_data, want_valid, label=""):
    """None when `col` equals the expected column, else a message: dtype
    code and scale equal, validity equal (None = all valid), integers and
    bools exactly equal where valid, float64 bit-identical where valid
    with all NaNs treated as one value."""
    if col.dtype.code != dt.code or col.dtype.scale != dt.scale:
        return f"{label}: dtype {col.dtype} != {dt}"
    if len(col) != want_valid.shape[0]:
        return f"{label}: {len(col)} rows != {want_valid.shape[0]}"
    data, valid = comparable(col)
    bad = valid != want_valid
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return (f"{label}: validity differs in {int(bad.sum())} rows, first "
                f"row {i}: got {bool(valid[i])}, want {bool(want_valid[i])}")
    bad = (data != want_data) & want_valid
    if bool(bad.any()):
        i = int(torch.nonzero(bad)[0])
        return (f"{label}: value differs in {int(bad.sum())} rows, first "
                f"row {i}: got {data[i].item()!r}, want "
                f"{want_data[i].item()!r}")
    return None


def check_all(results, names=None, tile=None):
    """results: name -> Column. Asserts every one against the oracle and
    reports all failing expressions at once. `tile`: an index tensor that
    maps result rows to the 777 oracle rows."""
    exp = expected()
    errors = []
    for nm in (names or list(results)):
        dt, values = exp[nm]
        wd, wv = expected_tensors(dt, values)
        if tile is not None:
            wd, wv = wd[tile], wv[tile]
        msg = mismatch(results[nm], dt, wd, wv, nm)
        if msg:
            errors.append(msg)
    assert not errors, "\n".join(errors)


def run_fused(exprs, rb):
    """compile_all + run, outputs scattered by expr_idx; entries stay None
    for expressions that did not compile. Returns (columns, programs)."""
    from auron_amd import fused

    progs = fused.compile_all(exprs, {nm: col.dtype for nm, col in
                                      zip(rb.names, rb.columns)})
    got = [None] * len(exprs)
    for prog in progs or ():
        for k, col in enumerate(fused.run(prog, rb)):
            got[prog.expr_idx[k]] = col
    return got, progs or []
