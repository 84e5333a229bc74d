"""The k_dec128_* kernels against their Python-integer references on the
device, bit for bit (limbs and validity), at the wave and block edges and one
row past the grid's thread capacity; and decimal128 plans on the GPU against
their CPU runs, with the native switch on and off."""
import random

import pytest
import torch

from auron_amd import AuronSession, dtypes, native, ops
from auron_amd.column import Column, RecordBatch
from auron_amd.exprs import Aliased, Arith, Cmp, Col
from auron_amd.plan import nodes as P

from test_dec128_arith import EDGE, P38, dec_values, limbs

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SIZES = [0, 1, 63, 64, 65, 255, 256, 257, 4097]
CMP_OPS = ["==", "!=", "<", "<=", ">", ">="]


def _pairs(n, seed, la=37, lb=37):
    """n (a, b) pairs: the edge block first, then random magnitudes of up to
    la / lb decimal digits."""
    rng = random.Random(seed)
    out = list(EDGE[:n])
    while len(out) < n:
        da, db = rng.randint(0, la), rng.randint(0, lb)
        out.append((rng.randint(-10 ** da, 10 ** da),
                    rng.randint(-10 ** db, 10 ** db)))
    return out


def _operands(n, seed, la=37, lb=37):
    pairs = _pairs(n, seed, la, lb)
    return limbs([a for a, _ in pairs]), limbs([b for _, b in pairs])


def _narrow(x):
    """The int64 [n] form: the low limb, read as a signed 64-bit value."""
    return x[:, 0].contiguous()


def _mask(n, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, generator=g) < 0.8


def _same(got, want):
    """(data, valid) pairs equal bit for bit; `got` lives on the device."""
    gd, gv = got
    wd, wv = want
    assert gd.device.type == "cuda" and gv.device.type == "cuda"
    assert gd.dtype == wd.dtype and gd.shape == wd.shape
    assert gv.dtype == torch.bool
    assert torch.equal(gv.cpu(), wv)
    assert torch.equal(gd.cpu(), wd)


def _dev(*ts):
    return [None if t is None else t.to(DEV) for t in ts]


@pytest.fixture(autouse=True)
def _need_native():
    native.require()


@pytest.mark.parametrize("n", SIZES)
def test_add_sub_kernels(n):
    a, b = _operands(n, 1)
    va, vb = _mask(n, 2), _mask(n, 3)
    da, db, dva, dvb = _dev(a, b, va, vb)
    for ka, kb, d, p in [(0, 0, 0, 38), (2, 0, 1, 38), (0, 0, 1, 20),
                         (0, 1, 38, 38), (38, 0, 38, 38)]:
        for fn, ref in ((ops.dec128_add, ops.dec128_add_ref),
                        (ops.dec128_sub, ops.dec128_sub_ref)):
            _same(fn(da, db, ka, kb, d, p, dva, dvb),
                  ref(a, b, ka, kb, d, p, va, vb))
    # int64 [n] operands on either side, no validity
    na, nb = _narrow(a), _narrow(b)
    dna, dnb = _dev(na, nb)
    _same(ops.dec128_add(dna, db, 4, 0, 0, 38),
          ops.dec128_add_ref(na, b, 4, 0, 0, 38))
    _same(ops.dec128_sub(da, dnb, 0, 2, 1, 38),
          ops.dec128_sub_ref(a, nb, 0, 2, 1, 38))
    _same(ops.dec128_add(dna, dnb, 0, 0, 0, 38),
          ops.dec128_add_ref(na, nb, 0, 0, 0, 38))


@pytest.mark.parametrize("n", SIZES)
def test_mul_kernel(n):
    a, b = _operands(n, 4, 24, 24)
    va = _mask(n, 5)
    da, db, dva = _dev(a, b, va)
    for d, p in [(0, 38), (1, 38), (38, 38), (4, 20)]:
        _same(ops.dec128_mul(da, db, d, p, dva, None),
              ops.dec128_mul_ref(a, b, d, p, va, None))
    nb = _narrow(b)
    _same(ops.dec128_mul(da, nb.to(DEV), 2, 38),
          ops.dec128_mul_ref(a, nb, 2, 38))
    _same(ops.dec128_mul(nb.to(DEV), da, 0, 38),
          ops.dec128_mul_ref(nb, a, 0, 38))


@pytest.mark.parametrize("n", SIZES)
def test_div_kernel(n):
    a, b = _operands(n, 6, 30, 20)
    vb = _mask(n, 7)
    da, db, dvb = _dev(a, b, vb)
    for k, p in [(0, 38), (1, 38), (6, 38), (38, 38), (0, 20)]:
        _same(ops.dec128_div(da, db, k, p, None, dvb),
              ops.dec128_div_ref(a, b, k, p, None, vb))
    na, nb = _narrow(a), _narrow(b)
    _same(ops.dec128_div(da, nb.to(DEV), 6, 38),
          ops.dec128_div_ref(a, nb, 6, 38))
    _same(ops.dec128_div(na.to(DEV), db, 38, 38),
          ops.dec128_div_ref(na, b, 38, 38))


@pytest.mark.parametrize("n", SIZES)
def test_cmp_kernel(n):
    a, b = _operands(n, 8)
    if n > 8:  # equal values at different scales
        a[-4:] = limbs([7, -7, 0, P38 // 10 ** 6])
        b[-4:] = limbs([7 * 10 ** 6, -7 * 10 ** 6, 0,
                        P38 // 10 ** 6 * 10 ** 6])
    da, db = _dev(a, b)
    na = _narrow(a)
    for op in CMP_OPS:
        for ka, kb in [(0, 0), (6, 0), (0, 38), (38, 0)]:
            got = ops.dec128_cmp(da, db, ka, kb, op)
            assert got.device.type == "cuda" and got.dtype == torch.bool
            assert torch.equal(got.cpu(), ops.dec128_cmp_ref(a, b, ka, kb, op))
        assert torch.equal(ops.dec128_cmp(na.to(DEV), db, 2, 0, op).cpu(),
                           ops.dec128_cmp_ref(na, b, 2, 0, op))


@pytest.mark.parametrize("n", SIZES)
def test_rescale_kernel(n):
    x, _ = _operands(n, 9, 38, 1)
    if n > 8:
        x[-3:] = torch.tensor([[0, -(1 << 63)], [-1, (1 << 63) - 1],
                               [-(1 << 63), -1]])  # -2^127, 2^127-1, -2^63
    vx = _mask(n, 10)
    dx, dvx = _dev(x, vx)
    for k, p in [(0, 38), (0, 20), (1, 38), (38, 38), (-1, 38), (-38, 38),
                 (-2, 10)]:
        _same(ops.dec128_rescale(dx, k, p, dvx),
              ops.dec128_rescale_ref(x, k, p, vx))
    for kw in ({"abs_": True}, {"negate": True}, {"truncate": True}):
        _same(ops.dec128_rescale(dx, -1, 38, **kw),
              ops.dec128_rescale_ref(x, -1, 38, **kw))
    # the cast shapes: into int64 / int32 ranges, and decimal64 out
    for bound in (1 << 63, 1 << 31):
        kw = dict(bound=bound, truncate=True, asym=True, narrow_out=True)
        _same(ops.dec128_rescale(dx, -2, None, dvx, **kw),
              ops.dec128_rescale_ref(x, -2, None, vx, **kw))
    _same(ops.dec128_rescale(dx, -4, 18, narrow_out=True),
          ops.dec128_rescale_ref(x, -4, 18, narrow_out=True))
    nx = _narrow(x)
    _same(ops.dec128_rescale(nx.to(DEV), 19, 38),
          ops.dec128_rescale_ref(nx, 19, 38))
    _same(ops.dec128_rescale(nx.to(DEV), -3, 18, narrow_out=True),
          ops.dec128_rescale_ref(nx, -3, 18, narrow_out=True))


def test_misaligned_operand_views():
    """[n,2] views that start 8 bytes into an allocation: the wrappers
    realign them for the kernels' 16-byte loads."""
    n = 257
    a, b = _operands(n, 11)

    def shifted(t):
        base = torch.empty(2 * n + 1, dtype=torch.int64, device=DEV)
        v = base[1:].view(n, 2)
        v.copy_(t)
        assert v.data_ptr() % 16 == 8
        return v

    sa, sb = shifted(a), shifted(b)
    _same(ops.dec128_add(sa, sb, 2, 0, 1, 38),
          ops.dec128_add_ref(a, b, 2, 0, 1, 38))
    _same(ops.dec128_mul(sa, b.to(DEV), 38, 38),
          ops.dec128_mul_ref(a, b, 38, 38))
    _same(ops.dec128_div(a.to(DEV), sb, 6, 38),
          ops.dec128_div_ref(a, b, 6, 38))
    assert torch.equal(ops.dec128_cmp(sa, sb, 0, 6, "<").cpu(),
                       ops.dec128_cmp_ref(a, b, 0, 6, "<"))
    _same(ops.dec128_rescale(sa, -2, 38), ops.dec128_rescale_ref(a, -2, 38))


@pytest.fixture(scope="module")
def wrapped():
    """One row more than the grid has threads, with the add and cmp
    references computed once."""
    n = ops.dec128_grid_threads() + 1
    g = torch.Generator().manual_seed(12)
    a = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), generator=g,
                      dtype=torch.int64)
    b = torch.randint(-(1 << 63), (1 << 63) - 1, (n, 2), generator=g,
                      dtype=torch.int64)
    # |value| < 2^104 ~ 2e31: sums at scale shift 2 stay inside 38 digits
    a[:, 1] = torch.randint(-(1 << 40), 1 << 40, (n,), generator=g)
    b[:, 1] = torch.randint(-(1 << 40), 1 << 40, (n,), generator=g)
    b[::5] = a[::5]  # equal rows for the comparison
    a[-1] = torch.tensor([-1, (1 << 40) - 1])  # the row past the grid
    return {"n": n, "a": a, "b": b,
            "add": ops.dec128_add_ref(a, b, 2, 0, 1, 38),
            "cmp": ops.dec128_cmp_ref(a, b, 0, 0, "<=")}


def test_add_grid_stride_wrap(wrapped):
    da, db = _dev(wrapped["a"], wrapped["b"])
    assert bool(wrapped["add"][1][-1])
    _same(ops.dec128_add(da, db, 2, 0, 1, 38), wrapped["add"])


def test_cmp_grid_stride_wrap(wrapped):
    da, db = _dev(wrapped["a"], wrapped["b"])
    got = ops.dec128_cmp(da, db, 0, 0, "<=")
    assert torch.equal(got.cpu(), wrapped["cmp"])


# ---------------------------------------------------------------------- plans
def _plan_batch(n=3000, seed=13):
    rng = random.Random(seed)
    d1 = [rng.randint(-10 ** 30, 10 ** 30) for _ in range(n)]
    d2 = [rng.randint(-10 ** 22, 10 ** 22) for _ in range(n)]
    d1[:3] = [P38, -P38, 0]
    d2[:3] = [1, -1, 0]
    e = [rng.randint(-10 ** 7 + 1, 10 ** 7 - 1) for _ in range(n)]
    i = [rng.randint(-1000, 1000) for _ in range(n)]
    g = torch.Generator().manual_seed(seed)
    cols = [Column(dtypes.decimal128(38, 2), limbs(d1),
                   torch.rand(n, generator=g) < 0.9),
            Column(dtypes.decimal128(30, 6), limbs(d2),
                   torch.rand(n, generator=g) < 0.9),
            Column(dtypes.decimal64(7, 2), torch.tensor(e)),
            Column(dtypes.int32, torch.tensor(i, dtype=torch.int32))]
    return RecordBatch(["d1", "d2", "e", "i"], cols)


def _plan(batch):
    proj = [Aliased(Arith("+", Col("d1"), Col("d2")), "s"),
            Aliased(Arith("-", Col("d1"), Col("e")), "m"),
            Aliased(Arith("*", Col("d2"), Col("i")), "p"),
            Aliased(Arith("/", Col("d1"), Col("d2")), "q"),
            Aliased(Arith("/", Col("e"), Col("d1")), "r")]
    return P.Project(P.Filter(P.MemoryScan([batch]),
                              Cmp(">", Col("d1"), Col("d2"))), proj)


def _result(out):
    out = out.to("cpu")
    return {nm: (out.column(nm).dtype, dec_values(out.column(nm)))
            for nm in out.names}


@pytest.fixture(scope="module")
def cpu_plan_result():
    return _result(AuronSession().collect(_plan(_plan_batch())))


def test_plan_gpu_matches_cpu(cpu_plan_result):
    got = _result(AuronSession(device=DEV).collect(
        _plan(_plan_batch().to(DEV))))
    assert got == cpu_plan_result
    rows = len(cpu_plan_result["s"][1])
    assert 500 < rows < 3000
    for nm in "smpqr":
        assert sum(v is not None for v in cpu_plan_result[nm][1]) > rows // 2


def test_device_path_never_syncs():
    """Overflow and x / 0 stay on the device: evaluating the expression
    nodes under torch's sync debug mode raises on any host synchronisation."""
    from auron_amd import functions
    from auron_amd.exprs import Abs, Cast

    b = _plan_batch(n=513).to(DEV)
    nodes = [Arith(op, Col(l), Col(r)) for op in "+-*/"
             for l, r in (("d1", "d2"), ("d1", "e"), ("i", "d2"))]
    nodes += [Cmp("<=", Col("d1"), Col("d2")), Cmp("==", Col("e"), Col("d1")),
              Abs(Col("d1")), Cast(Col("d1"), dtypes.decimal128(38, 6)),
              Cast(Col("d2"), dtypes.decimal64(18, 2)),
              Cast(Col("d2"), dtypes.int64),
              Cast(Col("i"), dtypes.decimal128(38, 20)),
              functions.CheckOverflow(Col("d1"), 20, 2)]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        outs = [e.eval(b) for e in nodes]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert all(o.data.device.type == "cuda" for o in outs)
    assert all(len(o) == 513 for o in outs)


def test_plan_switch_off_matches_on(cpu_plan_result, monkeypatch):
    monkeypatch.setenv("AURON_DECIMAL128_NATIVE_ARITH", "0")
    assert not ops._dec128_native(torch.device(DEV), 0)
    got = _result(AuronSession(device=DEV).collect(
        _plan(_plan_batch().to(DEV))))
    assert got == cpu_plan_result
