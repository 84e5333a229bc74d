"""k_expr_exec and eval-on-device against the independent oracle
(expr_oracle.py): the whole battery of expr_cases.py on the 777-row edge
batch, then the kernel's limits -- stack depth 30 (the largest dynamic-LDS
launch), null-mask bit 29, 16 input columns and 8 outputs of every output
dtype, the split into several programs, the grid stride beyond 2048 blocks
-- and the executor's Project/Filter with fusion on and off.

Never one path against the other: a rule both paths get wrong (narrow
integer wrap, NaN order, cast saturation) passes such a comparison.
float64 is compared bit for bit; test_expr_semantics.py says why.
"""
import random

import pytest
import torch

import expr_cases as C
import expr_oracle as O
from auron_amd import dtypes, fused
from auron_amd.column import Column, RecordBatch
from auron_amd.exprs import (Aliased, BoolOp, Cast, Coalesce, Col, IsNull,
                             Not, eval_scope)

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def gpu_batch():
    from auron_amd import native

    native.require()
    return C.batch(DEV)


def test_fused_matches_oracle(gpu_batch):
    """Whole battery through compile_all: more than 6 programs, outputs
    scattered by expr_idx, every expression still its own."""
    names = [nm for nm, _ in C.battery()]
    got, progs = C.run_fused([e for _, e in C.battery()], gpu_batch)
    torch.cuda.synchronize()
    assert len(progs) > 6
    assert [nm for nm, g in zip(names, got) if g is None] \
        == sorted(C.EVAL_ONLY)
    C.check_all({nm: g for nm, g in zip(names, got) if g is not None})


@pytest.fixture(scope="module")
def device_eval_results(gpu_batch):
    with eval_scope(gpu_batch):
        got = {nm: e.eval(gpu_batch) for nm, e in C.battery()}
    torch.cuda.synchronize()
    return got


@pytest.mark.parametrize("name", [nm for nm, _ in C.battery()])
def test_eval_on_device_matches_oracle(device_eval_results, name):
    C.check_all(device_eval_results, [name])


def test_depth_30_and_null_bit_29():
    """30 operands deep: 30 * 256 * 8 = 61,440 B of dynamic LDS, and the
    deepest operand's null flag lives in bit 29 of the mask."""
    n = 300
    rng = random.Random(30)
    names = [f"c{k}" for k in range(16)]
    schema = {nm: dtypes.int64 for nm in names}
    cols = {nm: [rng.randint(-2 ** 62, 2 ** 62) for _ in range(n)]
            for nm in names}
    for r in range(n):
        kind = r % 4
        if kind == 1:
            cols["c15"][r] = None            # only the deepest operand
        elif kind == 2:
            cols["c0"][r] = None             # only the first
        elif kind == 3:
            cols[names[rng.randrange(16)]][r] = None
    rb = RecordBatch(names, [Column.from_pylist(cols[nm], dtypes.int64)
                             for nm in names]).to(DEV)
    expr = C.right_nested_sum(30)
    prog = fused.compile_exprs([expr], schema)
    assert prog.max_depth == 30
    out = fused.run(prog, rb)[0]
    torch.cuda.synchronize()
    dt, want = O.eval_column(expr, cols, schema)
    assert sum(v is None for v in want) >= n // 2
    assert sum(v is not None for v in want) >= n // 4
    msg = C.mismatch(out, dt, *C.expected_tensors(dt, want), "depth30")
    assert msg is None, msg


def test_grid_stride(gpu_batch):
    """2048 * 256 + 300 rows: the smallest shape at which the grid is
    capped and a thread takes a second row."""
    n = 2048 * 256 + 300
    idx = torch.arange(n, device=DEV) % C.N
    big = RecordBatch(gpu_batch.names, [
        Column(c.dtype, c.data[idx],
               None if c.validity is None else c.validity[idx])
        for c in gpu_batch.columns])
    pick = ["wrap_mul_cast", "f_div", "kleene_or", "cast_f_i16"]
    exprs = dict(C.battery())
    got, progs = C.run_fused([exprs[nm] for nm in pick], big)
    torch.cuda.synchronize()
    assert len(progs) == 1 and len(progs[0].out_dtypes) == 4
    C.check_all(dict(zip(pick, got)), tile=idx.cpu())


def test_limits_16_columns_8_output_dtypes(gpu_batch):
    """One program at both limits; an output of every dtype the kernel can
    store, int8 and int16 included."""
    c = C.c
    exprs = [
        ("o_bool", BoolOp("or", [c("flag"), c("flag2"),
                                 Not(IsNull(c("nul")))])),
        ("o_i8", c("i8") + Cast(c("i16"), dtypes.int8)),
        ("o_i16", c("i16") - c("i8")),
        ("o_i32", c("i32a") * c("i32b")),
        ("o_date", Coalesce([c("d"), c("d2")])),
        ("o_i64", c("i64a") - c("i64b")),
        ("o_dec", c("p") + c("q")),
        ("o_f64", c("f") * c("g") + Cast(c("p4"), dtypes.float64)),
    ]
    prog = fused.compile_exprs([e for _, e in exprs], C.SCHEMA)
    assert len(prog.colnames) == 16 and len(prog.out_dtypes) == 8
    assert [dt.code for dt in prog.out_dtypes] == [
        dtypes.BOOL, dtypes.INT8, dtypes.INT16, dtypes.INT32, dtypes.DATE32,
        dtypes.INT64, dtypes.DECIMAL64, dtypes.FLOAT64]
    outs = fused.run(prog, gpu_batch)
    torch.cuda.synchronize()
    cols = C.columns()
    errors = []
    for (nm, e), out in zip(exprs, outs):
        dt, want = O.eval_column(e, cols, C.SCHEMA)
        assert any(v is None for v in want)
        assert sum(v is not None for v in want) >= C.N // 4
        msg = C.mismatch(out, dt, *C.expected_tensors(dt, want), nm)
        if msg:
            errors.append(msg)
    assert not errors, "\n".join(errors)


@pytest.mark.parametrize("fusion", ["1", "0"])
def test_executor_project_filter(gpu_batch, monkeypatch, fusion):
    """Project over Filter through the executor, fusion on and off, each
    against the oracle. The predicate is NULL on some rows (they drop) and
    wraps in int32 on others; one projection (float %) always stays on the
    eval path, so a fused run mixes both."""
    from auron_amd import AuronSession
    from auron_amd.plan import nodes as P

    exprs = dict(C.battery())
    pred = "wrap_add_gt"
    proj = ["wrap_mul_cast", "mod_f", "cast_f_i32", "f_ge", "cast_f_dec",
            "case_nullcond_else", "mod_i64"]
    plan = P.Project(
        P.Filter(P.MemoryScan([gpu_batch]), exprs[pred]),
        [Aliased(exprs[nm], nm) for nm in proj] + [Aliased(Col("i8"), "i8")])
    monkeypatch.setenv("AURON_EXPR_FUSION", fusion)
    launched = []
    real_run = fused.run

    def counting_run(prog, b):
        launched.append(list(prog.expr_idx))
        return real_run(prog, b)

    monkeypatch.setattr(fused, "run", counting_run)
    out = AuronSession(device=DEV).collect(plan).to("cpu")
    if fusion == "1":
        # the filter's program, then the projection's: every non-trivial
        # projection but float % (index 1) came out of k_expr_exec
        assert launched == [[0], [0, 2, 3, 4, 5, 6]]
    else:
        assert launched == []

    exp = C.expected()
    mask = exp[pred][1]
    assert None in mask and True in mask and False in mask
    keep = torch.tensor([r for r in range(C.N) if mask[r] is True])
    assert out.num_rows == keep.numel()
    C.check_all({nm: out.column(nm) for nm in proj}, tile=keep)
    i8 = C.columns()["i8"]
    msg = C.mismatch(out.column("i8"), dtypes.int8,
                     *C.expected_tensors(dtypes.int8,
                                         [i8[r] for r in keep.tolist()]),
                     "i8")
    assert msg is None, msg
