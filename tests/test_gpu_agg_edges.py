"""k_agg_scatter, k_agg_scatter_lds, k_agg_multi and k_agg_count against
the independent oracle (agg_oracle.py), never against another kernel: every
kernel path, row counts around one wave, gid patterns inside a wave, all
value dtypes with and without validity, special values, null layouts,
the partial -> final merge, and run-to-run determinism of NaN MIN/MAX.

Float sums: inputs k/8 with |k| <= 2**20 sum exactly in any order and are
compared with ==; general inputs are compared with math.fsum under the
recursive-summation bound 1.01 (m-1) 2**-53 sum|v| per group of m rows,
which holds for every order (float32 inputs widen exactly to float64)."""
import functools

import pytest
import torch

from auron_amd import ops

import agg_cases as C
import agg_oracle as O
from test_agg_semantics import merge_partials, result_dtype, run_case

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BIG_N = 2048 * 256 + 65  # the grid-stride loop runs a second, partial round

# (n, ngroups, path): au_agg_scatter stages in LDS when the accumulators and
# counts fit 64 KiB (ngroups * 2 * 8) and n >= 16 * ngroups
PATH_SHAPES = [(16, 1, "lds"), (65536, 4096, "lds"), (4096, 8, "lds"),
               (65552, 4097, "seg"), (127, 8, "seg")]
SEG_ROWS = [(1, 1), (63, 8), (64, 8), (65, 8), (257, 17)]


def lds_path(n, ngroups):
    return ngroups * 2 * 8 <= (64 << 10) and n >= 16 * ngroups


@functools.lru_cache(maxsize=None)
def case_for(kind, n, ngroups, pattern, with_validity, flavour="exact", unused_end=0):
    return C.agg_case(f"{kind}-{n}x{ngroups}-{pattern}-{'v' if with_validity else 'nv'}",
                      kind, n, ngroups, pattern, with_validity, flavour,
                      unused_end, seed=n + ngroups)


def test_shapes_take_the_intended_path():
    for n, ngroups, path in PATH_SHAPES:
        assert lds_path(n, ngroups) == (path == "lds"), (n, ngroups)
    for n, ngroups in SEG_ROWS + [(BIG_N, 4097)]:
        assert not lds_path(n, ngroups), (n, ngroups)
    assert lds_path(4096, 8) and (4096 + 255) // 256 == 16  # 16 blocks flush


@pytest.mark.parametrize("kind", C.VALUE_KINDS)
@pytest.mark.parametrize("with_validity", [True, False])
@pytest.mark.parametrize("n,ngroups", [(16, 1), (4096, 8), (127, 8)] + SEG_ROWS)
def test_agg_scatter_small_shapes(kind, with_validity, n, ngroups):
    for k, pattern in enumerate(("runs", "random")):
        run_case(case_for(kind, n, ngroups, pattern, with_validity,
                          unused_end=(n + k) % 2), DEV)


@pytest.mark.parametrize("kind", ["float64", "float32", "int64", "int32"])
@pytest.mark.parametrize("with_validity", [True, False])
@pytest.mark.parametrize("n,ngroups", [(65536, 4096), (65552, 4097)])
def test_agg_scatter_path_boundary(kind, with_validity, n, ngroups):
    run_case(case_for(kind, n, ngroups, "runs", with_validity,
                      unused_end=int(with_validity)), DEV)


@pytest.mark.parametrize("kind", ["float64", "int64"])
def test_agg_scatter_second_grid_round(kind):
    run_case(case_for(kind, BIG_N, 4097, "runs", True), DEV)


@pytest.mark.parametrize("kind", C.FLOAT_KINDS)
@pytest.mark.parametrize("n,ngroups", [(127, 8), (4096, 8), (2000, 100), (65552, 4097)])
def test_agg_scatter_general_floats(kind, n, ngroups):
    """+-max, the smallest subnormal and arbitrary values."""
    case = case_for(kind, n, ngroups, "runs", True, "general")
    gids, col = case.gids_t(DEV), case.column(DEV)
    for fn in ("sum", "min", "max"):
        acc, cnt = ops.agg_scatter(gids, ngroups, col, fn)
        O.check_agg(acc.cpu().tolist(), cnt.cpu().tolist(), case.want(fn),
                    f"{case.name} {fn}")


WAVE_SPOTS = [(0,), (63,), (64, 67), (127, 128), (191,), tuple(range(168, 192)),
              (64, 65, 67, 70)]


@pytest.mark.parametrize("kind", ["float64", "float32", "int64", "int32", "int8"])
def test_agg_wave_patterns(kind):
    """One run of 64, A A B A recurrences, a run across lanes 63 -> 0, a run
    that ends at the last row; NaN (or the int extremes) first, last, alone
    and as the whole group."""
    for spots in WAVE_SPOTS:
        run_case(C.wave_pattern_case(kind, spots, with_validity=len(spots) == 2), DEV)


@pytest.mark.parametrize("kind", C.FLOAT_KINDS)
def test_nan_min_max_is_deterministic(kind):
    cases = [C.wave_pattern_case(kind, s) for s in WAVE_SPOTS]
    cases += [case_for(kind, 4096, 8, "random", True),
              case_for(kind, 2000, 100, "random", False)]
    for _ in range(3):
        for case in cases:
            run_case(case, DEV)


# ------------------------------------------------------------------- count
@pytest.mark.parametrize("n,ngroups", SEG_ROWS + [(127, 8), (4096, 8), (65552, 4097),
                                                  (BIG_N, 4097)])
def test_agg_count(n, ngroups):
    case = case_for("int64", n, ngroups, "runs", True)
    gids = case.gids_t(DEV)
    got = ops.agg_count_star(gids, ngroups)
    assert got.dtype == torch.int64 and got.cpu().tolist() == case.row_counts()
    _, cnt = ops.agg_scatter(gids, ngroups, case.column(DEV), "count")
    assert cnt.cpu().tolist() == case.want("count")[1]
    nv = case_for("int64", n, ngroups, "runs", False)
    _, cnt = ops.agg_scatter(nv.gids_t(DEV), ngroups, nv.column(DEV), "count")
    assert cnt.cpu().tolist() == nv.row_counts()


# ------------------------------------------------------------------- multi
def multi_items(n, ngroups, how_many, flavour="exact"):
    """Descriptors over one gid vector: differing validity, one column
    under two ops, f64 / f32 / i64 / i32 mixed."""
    base = case_for("float64", n, ngroups, "runs", True, flavour)
    specs = [("int64", True, "min"), ("float32", True, "min"),
             ("int32", False, "sum"), ("float64", False, "min")]
    items = [(base, "sum"), (base, "max")]
    for k, (kind, with_validity, fn) in enumerate(specs[:how_many - 2]):
        items.append((C.agg_case(f"multi-{kind}-{n}", kind, n, ngroups, "runs",
                                 with_validity, flavour, seed=101 + k,
                                 gids=base.gids), fn))
    return base, items


@pytest.mark.parametrize("n,ngroups,how_many",
                         [(1, 1, 2), (63, 8, 6), (64, 8, 3), (65, 8, 6), (257, 17, 4),
                          (127, 8, 5), (4096, 8, 6), (65552, 4097, 6), (BIG_N, 4097, 2)])
def test_agg_scatter_multi(n, ngroups, how_many):
    base, items = multi_items(n, ngroups, how_many)
    gids = base.gids_t(DEV)
    cols = {id(c): c.column(DEV) for c, _ in items}
    out = ops.agg_scatter_multi(gids, ngroups, [(cols[id(c)], fn) for c, fn in items])
    assert len(out) == len(items)
    for (case, fn), (acc, cnt) in zip(items, out):
        assert acc.dtype == result_dtype(case.kind, fn), (case.name, fn)
        O.check_agg(acc.cpu().tolist(), cnt.cpu().tolist(), case.want(fn),
                    f"multi {case.name} {fn}", exact=True)


def test_agg_scatter_multi_general_floats_and_narrow_ints():
    base, items = multi_items(2000, 100, 4, "general")
    narrow = [C.agg_case(f"multi-{k}", k, 2000, 100, "runs", True, seed=7, gids=base.gids)
              for k in ("int8", "int16", "bool")]
    items = items + [(narrow[0], "min"), (narrow[1], "max"), (narrow[2], "max"),
                     (narrow[0], "sum"), (narrow[2], "sum")]
    out = ops.agg_scatter_multi(base.gids_t(DEV), 100,
                                [(c.column(DEV), fn) for c, fn in items])
    for (case, fn), (acc, cnt) in zip(items, out):
        assert acc.dtype == result_dtype(case.kind, fn), (case.name, fn)
        O.check_agg(acc.cpu().tolist(), cnt.cpu().tolist(), case.want(fn),
                    f"multi {case.name} {fn}")


def test_agg_scatter_multi_wave_patterns():
    for spots in WAVE_SPOTS:
        cases = [C.wave_pattern_case(k, spots, with_validity=v)
                 for k, v in (("float64", False), ("float32", True), ("int64", True))]
        items = [(cases[0], "min"), (cases[0], "max"), (cases[1], "max"),
                 (cases[1], "min"), (cases[2], "min"), (cases[0], "sum")]
        out = ops.agg_scatter_multi(cases[0].gids_t(DEV), 6,
                                    [(c.column(DEV), fn) for c, fn in items])
        for (case, fn), (acc, cnt) in zip(items, out):
            O.check_agg(acc.cpu().tolist(), cnt.cpu().tolist(), case.want(fn),
                        f"multi {case.name} {fn}", exact=True)


# ------------------------------------------------------ partial -> final
@pytest.mark.parametrize("kind", ["float64", "float32", "int64", "int16", "bool"])
@pytest.mark.parametrize("n,ngroups", [(4096, 8), (300, 17), (2000, 100)])
def test_partial_final_merge(kind, n, ngroups):
    case = case_for(kind, n, ngroups, "runs", True)
    for fn in C.ops_for(kind):
        acc, cnt = merge_partials(case, fn, DEV)
        O.check_agg(acc.cpu().tolist(), cnt.cpu().tolist(), case.want(fn),
                    f"merge {case.name} {fn}", exact=True)
