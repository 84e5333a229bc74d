"""Scalar-expression semantics on CPU: Expr.eval against the independent
oracle (expr_oracle.py) over the shared edge batch (expr_cases.py), the
oracle's own self-check of that batch, and the structure of what the fused
compiler emits. The GPU file (test_gpu_expr_edges.py) runs the same battery
through k_expr_exec and through eval on the device.

float64 results are compared bit for bit. That is derived, not measured:
every float result is a chain of single correctly-rounded binary64
operations (+ - * / fmod, int -> double, double -> int) done in the same
order by the oracle, by torch and by the kernel, with no fast-math and no
contraction possible across separate operators. Two places where torch is
NOT such an operation were found by this comparison and are routed round
in exprs.py: the vectorised CPU fmod (NaN where a / b overflows) and, on
the device, division by a Python scalar (a multiplication by the
reciprocal, 1 ulp off in decimal64 -> float64).
"""
import math

import pytest

import expr_cases as C
import expr_oracle as O
from auron_amd import dtypes, fused
from auron_amd.exprs import (Arith, Cast, Cmp, Coalesce, Col, InList,
                             Literal, eval_scope)


# ------------------------------------------------- self-check of the inputs
def test_inputs_reach_every_edge():
    """Conditions on the oracle's own output and on the raw inputs: they
    cannot be met by the code under test."""
    cols, exp = C.columns(), C.expected()
    assert all(len(v) == C.N for v in cols.values())
    assert cols["i16"].count(None) == 0
    assert cols["nul"].count(None) == C.N
    for nm, vals in cols.items():
        if nm not in ("i16", "nul"):
            assert 0.15 < vals.count(None) / C.N < 0.25, nm
    for nm, (_, vals) in exp.items():
        assert len(vals) == C.N
        nn = sum(v is not None for v in vals)
        assert nn >= 0.25 * C.N, f"{nm}: only {nn} non-NULL rows"
        if nm != "coalesce_dec":     # its last argument is a literal
            assert nn < C.N, f"{nm}: no NULL row"

    def rows(pred, *names):
        return [r for r in range(C.N)
                if all(cols[n][r] is not None for n in names)
                and pred(*(cols[n][r] for n in names))]

    i32 = (O.I32_MIN, O.I32_MAX)
    # overflow that wraps, in both directions, for + and *
    assert rows(lambda a, b: a + b > i32[1], "i32a", "i32b")
    assert rows(lambda a, b: a + b < i32[0], "i32a", "i32b")
    assert rows(lambda a, b: not i32[0] <= a * b <= i32[1], "i32a", "i32b")
    assert rows(lambda a: not -128 <= a + a <= 127, "i8")
    assert rows(lambda a, b: not i32[0] <= a + b <= i32[1], "d", "i32a")
    assert rows(lambda a, b: a + b > O.I64_MAX, "p", "q")
    # the wrapped sum changes the comparison's answer
    r = rows(lambda a, b: a == i32[1] and b == 1, "i32a", "i32b")[0]
    assert exp["wrap_add_gt"][1][r] is False
    # MIN % -1 and x % 0
    for a, b, nm, lo in (("i64a", "i64b", "mod_i64", O.I64_MIN),
                         ("i32a", "i32b", "mod_i32", O.I32_MIN)):
        r = rows(lambda x, y: x == lo and y == -1, a, b)
        assert r and all(exp[nm][1][k] == 0 for k in r)
        r = rows(lambda x, y: y == 0, a, b)
        assert r and all(exp[nm][1][k] is None for k in r)
        assert any(v is not None and v < 0 for v in exp[nm][1])
    # float %: sign of the dividend, NULL on +-0.0
    assert any(v is not None and v == v and math.copysign(1, v) < 0
               for v in exp["mod_f"][1])
    assert rows(lambda x, y: y == 0 and math.copysign(1, y) < 0, "f", "g")
    # NaN comparisons: NaN on the left only, the right only, both sides
    assert rows(lambda x, y: x != x and y == y, "f", "g")
    assert rows(lambda x, y: x == x and y != y, "f", "g")
    r = rows(lambda x, y: x != x and y != y, "f", "g")
    assert r and all(exp["f_eq"][1][k] is True for k in r)
    r = rows(lambda x, y: x != x and y == math.inf, "f", "g")
    assert r and all(exp["f_gt"][1][k] is True for k in r)
    # saturation in each direction, NaN -> 0
    for nm, lo, hi in (("cast_f_i64", O.I64_MIN, O.I64_MAX),
                       ("cast_f_i32", O.I32_MIN, O.I32_MAX)):
        up = rows(lambda x: x > hi, "f")
        down = rows(lambda x: x < lo, "f")
        assert up and all(exp[nm][1][k] == hi for k in up)
        assert down and all(exp[nm][1][k] == lo for k in down)
        nan = rows(lambda x: x != x, "f")
        assert nan and all(exp[nm][1][k] == 0 for k in nan)
    # saturate at int32, THEN wrap: 3e9 -> INT32_MAX -> -1
    r = rows(lambda x: x == 3e9, "f")
    assert r and exp["cast_f_i16"][1][r[0]] == -1 == exp["cast_f_i8"][1][r[0]]
    r = rows(lambda x: x == O.I64_MAX, "p")
    assert r and exp["cast_dec_i32"][1][r[0]] == O.I32_MAX
    # .5 ties go to even; NaN, inf and overflow become NULL
    r = rows(lambda x: x == 0.125, "f")
    assert r and exp["cast_f_dec"][1][r[0]] == 12
    r = rows(lambda x: x == 0.375, "f")
    assert r and exp["cast_f_dec"][1][r[0]] == 38
    for bad in (math.nan, math.inf, -math.inf, 1e19):
        r = rows(lambda x: x == bad or (x != x and bad != bad), "f")
        assert r and all(exp["cast_f_dec"][1][k] is None for k in r)
    r = rows(lambda x: x == O.I64_MAX, "i64a")
    assert r and exp["cast_i64_dec18"][1][r[0]] is None
    # Kleene: all nine (value, NULL) pairs of flag and the comparison
    seen = {(cols["flag"][r], None if cols["i64a"][r] is None
             else cols["i64a"][r] > 0) for r in range(C.N)}
    assert len(seen) == 9
    # CASE: NULL condition rows, COALESCE: rows decided by each argument
    assert None in cols["flag"]
    assert any(cols["i64a"][r] is None and cols["i64b"][r] is not None
               for r in range(C.N))
    assert any(cols["i32a"][r] is None and cols["i32b"][r] is None
               for r in range(C.N))


def test_oracle_spot_values():
    """The oracle against hand-computed answers of the rule table."""
    sch = {"x": dtypes.int32, "y": dtypes.int32, "u": dtypes.float64,
           "v": dtypes.float64, "b": dtypes.int8}

    def ev(e, **row):
        return O.evaluate(e, row, sch)

    x, y, u, v, b = (Col(n) for n in "xyuvb")
    assert ev(Cmp(">", x + y, Literal(0)), x=2 ** 31 - 1, y=1) is False
    assert ev(Arith("%", x, y), x=-7, y=2) == -1
    assert ev(Arith("%", x, y), x=-2 ** 31, y=-1) == 0
    assert ev(Arith("%", x, y), x=5, y=0) is None
    assert ev(Arith("%", u, v), u=-5.5, v=2.0) == -1.5
    assert ev(Arith("%", u, v), u=5.5, v=-0.0) is None
    assert ev(u / v, u=1.0, v=-0.0) is None
    assert ev((b + b) / Literal(2), b=100) == -28.0
    assert ev(Cast(u, dtypes.int32), u=3e9) == 2 ** 31 - 1
    assert ev(Cast(u, dtypes.int32), u=-3e9) == -2 ** 31
    assert ev(Cast(u, dtypes.int16), u=3e9) == -1
    assert ev(Cast(u, dtypes.int8), u=-3e9) == 0
    assert ev(Cast(u, dtypes.int16), u=70000.9) == 70000 - 65536
    assert ev(Cast(u, dtypes.int64), u=1e19) == 2 ** 63 - 1
    assert ev(Cast(u, dtypes.int64), u=-1.9) == -1
    assert ev(Cast(u, dtypes.int64), u=math.nan) == 0
    dec = dtypes.decimal64(7, 2)
    assert ev(Cast(u, dec), u=0.125) == 12 and ev(Cast(u, dec), u=0.375) == 38
    assert ev(Cast(u, dec), u=-0.125) == -12
    assert ev(Cast(u, dec), u=math.inf) is None
    assert ev(Cmp("==", u, v), u=math.nan, v=math.nan) is True
    assert ev(Cmp(">", u, v), u=math.nan, v=math.inf) is True
    assert ev(Cmp("<=", u, v), u=math.nan, v=math.inf) is False
    assert ev(Cmp("==", u, v), u=-0.0, v=0.0) is True
    assert ev(InList(x, [1, None]), x=2) is False
    assert ev(InList(x, [1, None]), x=None) is None


# ------------------------------------------------------- eval vs the oracle
@pytest.fixture(scope="module")
def eval_results():
    rb = C.batch("cpu")
    with eval_scope(rb):
        return {nm: e.eval(rb) for nm, e in C.battery()}


@pytest.mark.parametrize("name", [nm for nm, _ in C.battery()])
def test_eval_matches_oracle(eval_results, name):
    C.check_all(eval_results, [name])


# ------------------------------------------------------- compiler structure
def _instrs(prog):
    return prog.instr_np.view(fused._INSTR_DTYPE)


def test_battery_compiles_except_float_mod():
    exprs = [e for _, e in C.battery()]
    names = [nm for nm, _ in C.battery()]
    progs = fused.compile_all(exprs, C.SCHEMA)
    covered = sorted(i for p in progs for i in p.expr_idx)
    assert [names[i] for i in range(len(names)) if i not in covered] \
        == sorted(C.EVAL_ONLY)
    assert len(progs) > 6
    for p in progs:
        assert len(p.out_dtypes) <= 8 and len(p.colnames) <= 16
        assert p.max_depth <= 30 and len(_instrs(p)) <= 192
    # every opcode the compiler can emit (it never emits ISNOTNULL)
    ops = set()
    for p in progs:
        ops |= set(_instrs(p)["op"].tolist())
    assert ops == set(range(40)) - {fused.ISNOTNULL}


def test_narrow_operators_are_followed_by_trunc():
    sch = {"a": dtypes.int32, "b": dtypes.int32, "h": dtypes.int8,
           "l": dtypes.int64}
    prog = fused.compile_exprs(
        [Cmp(">", Col("a") + Col("b"), Literal(0)),
         Col("h") * Col("h"), Col("l") - Col("l")], sch)
    ins = _instrs(prog)
    seq = [(int(o), int(i)) for o, i in zip(ins["op"], ins["imm"])]
    assert seq[seq.index((fused.ADDI, 0)) + 1] == (fused.TRUNC_I, 32)
    assert seq[seq.index((fused.MULI, 0)) + 1] == (fused.TRUNC_I, 8)
    assert seq[seq.index((fused.SUBI, 0)) + 1][0] == fused.OUT
    # float -> int carries its saturation width
    prog = fused.compile_exprs([Cast(Col("f"), dtypes.int16),
                                Cast(Col("f"), dtypes.int64)],
                               {"f": dtypes.float64})
    seq = [(int(o), int(i)) for o, i in zip(*(_instrs(prog)[k]
                                              for k in ("op", "imm")))]
    assert (fused.D2I_TRUNC, 32) in seq and (fused.D2I_TRUNC, 64) in seq
    assert seq[seq.index((fused.D2I_TRUNC, 32)) + 1] == (fused.TRUNC_I, 16)


@pytest.mark.parametrize("expr", [
    Cast(Col("ts"), dtypes.int64),
    Cast(Col("f"), dtypes.timestamp),
    Cast(Col("i"), dtypes.timestamp),
    Coalesce([Col("ts"), Literal(0)]),
    Cmp("<", Col("ts"), Col("i")),
    Cast(Col("ts"), dtypes.date32),
], ids=["ts_i64", "f_ts", "i32_ts", "coalesce_ts", "cmp_ts_i32", "ts_date"])
def test_timestamp_casts_fall_back(expr):
    sch = {"ts": dtypes.timestamp, "f": dtypes.float64, "i": dtypes.int32}
    assert fused.compile_exprs([expr], sch) is None
    prog = fused.compile_exprs([Col("i") + Literal(1), expr,
                                Col("f") * Literal(2.0)], sch)
    assert prog.expr_idx == [0, 2] and prog.colnames == ["i", "f"]


def test_timestamp_arithmetic_still_compiles():
    """A timestamp is a plain 64-bit slot: ts - ts and ts + ts need no
    cast and no TRUNC_I, so they stay in the kernel."""
    sch = {"t": dtypes.timestamp, "u": dtypes.timestamp}
    prog = fused.compile_exprs([Col("t") - Col("u"), Col("t") + Col("u"),
                                Cmp("<", Col("t"), Col("u"))], sch)
    assert prog.expr_idx == [0, 1, 2]
    assert [dt.code for dt in prog.out_dtypes] == [
        dtypes.TIMESTAMP, dtypes.TIMESTAMP, dtypes.BOOL]
    assert fused.TRUNC_I not in _instrs(prog)["op"].tolist()


def test_float32_column_falls_back():
    sch = {"x": dtypes.float32, "i": dtypes.int32}
    assert fused.compile_exprs([Col("x") + Literal(1.0)], sch) is None
    assert fused.compile_exprs([Cast(Col("i"), dtypes.float32)], sch) is None
    prog = fused.compile_exprs([Col("x") * Col("x"), Col("i") + Col("i")],
                               sch)
    assert prog.expr_idx == [1] and prog.colnames == ["i"]


def test_depth_limit():
    sch = {f"c{k}": dtypes.int64 for k in range(16)}
    prog = fused.compile_exprs([C.right_nested_sum(30)], sch)
    assert prog is not None and prog.max_depth == 30
    assert len(prog.colnames) == 16
    assert fused.compile_exprs([C.right_nested_sum(31)], sch) is None


def test_nine_expressions_split_8_and_1():
    exprs = [Col("i32a") + Literal(k) for k in range(9)]
    progs = fused.compile_all(exprs, C.SCHEMA)
    assert [p.expr_idx for p in progs] == [list(range(8)), [8]]


def _sum_of(names):
    e = Col(names[0])
    for nm in names[1:]:
        e = e + Col(nm)
    return e


def test_column_limit():
    sch = {f"c{k}": dtypes.int64 for k in range(40)}
    wide17 = _sum_of([f"c{k}" for k in range(17)])
    wide16 = _sum_of([f"c{k}" for k in range(20, 36)])
    assert fused.compile_exprs([wide17], sch) is None
    prog = fused.compile_exprs([wide17, wide16], sch)
    assert prog.expr_idx == [1]
    assert prog.colnames == [f"c{k}" for k in range(20, 36)]
    ins = _instrs(prog)
    push = ins["a"][ins["op"] == fused.PUSH_COL].tolist()
    assert push == list(range(16))


def test_column_table_after_a_failed_expression():
    sch = {"a": dtypes.int64, "x": dtypes.int64, "y": dtypes.int64,
           "u": dtypes.float64}
    # float % is refused only after x, y and u entered the column table
    exprs = [Col("a") + Literal(1),
             Arith("%", Col("x") + Col("y"), Col("u")),
             Col("y") - Col("x")]
    prog = fused.compile_exprs(exprs, sch)
    assert prog.expr_idx == [0, 2]
    assert prog.colnames == ["a", "y", "x"]
    ins = _instrs(prog)
    assert ins["a"][ins["op"] == fused.PUSH_COL].tolist() == [0, 1, 2]
    assert ins["a"][ins["op"] == fused.OUT].tolist() == [0, 1]
    assert prog.max_depth == 2


def test_instruction_limit():
    sch = {"a": dtypes.int64, "b": dtypes.int64}
    long_in = InList(Col("a"), list(range(60)))        # 4 instrs per value
    ok_in = InList(Col("a"), list(range(40)))
    assert fused.compile_exprs([long_in], sch) is None
    prog = fused.compile_exprs([Col("a") + Col("b"), long_in,
                                Col("b") * Literal(2)], sch)
    assert prog.expr_idx == [0, 2]
    assert len(_instrs(prog)) == 8
    assert fused.compile_exprs([ok_in], sch).expr_idx == [0]
    # two that fit alone but not together: the second stays interpreted
    progs = fused.compile_all([ok_in, InList(Col("b"), list(range(40)))],
                              sch)
    assert progs is not None and progs[0].expr_idx == [0]
