"""ops.range_bucket / range_bucket_ref: range bucket of string and
decimal128 keys with torch.searchsorted semantics, checked against Python
bisect over UTF-8 bytes / big ints.

The adversarial generators here are shared with test_gpu_range_bucket.py
and test_external_sort_wide_keys.py."""
import random
from bisect import bisect_left, bisect_right

import pytest
import torch

from auron_amd import dtypes, ops
from auron_amd.column import Column

M64 = (1 << 64) - 1
D128 = dtypes.decimal128(38, 2)
BOUND_COUNTS = (0, 1, 2, 7, 64)


# ------------------------------------------------------------------ strings
def string_pool():
    """Strings that break a careless comparator: empty, proper prefixes,
    first difference right around the 8-byte word boundaries and past a
    256-byte pad, and bytes >= 0x80 (wrong under a signed compare)."""
    pool = ["", "a", "ab", "abc", "spark", "sparkle", "sparkles",
            "é", "z", "中", "\x7f", "zé", "z\x7f", "中文", "éa", "ée",
            "\x7f\x7f", "zz", "~", "中a"]
    filler = "pqrstuvw" * 40
    for p in (7, 8, 9, 15, 16, 17, 300):
        base = filler[:p]
        # base is a proper prefix of the rest; the others first differ at
        # byte p, one of them in a non-ASCII byte
        pool += [base, base + "a", base + "b", base + "é", base + "a" * 9]
    return pool


def random_words(rng, k):
    return ["".join(rng.choice("abcdefghijklmnopqrstuvwxyz")
                    for _ in range(rng.randint(1, 20))) for _ in range(k)]


def string_values(n, seed, null_frac=0.05, distinct=None):
    """n python values (None = null) over the pool plus random words."""
    rng = random.Random(seed)
    pool = string_pool()
    words = pool + random_words(rng, max(0, (distinct or 2 * len(pool))
                                         - len(pool)))
    return [None if rng.random() < null_frac else rng.choice(words)
            for _ in range(n)]


def string_bounds(values, nb, seed):
    """nb ascending bounds drawn from the rows (so bounds equal rows),
    with a forced duplicate."""
    rng = random.Random(seed)
    cand = [v for v in values if v is not None] or [""]
    bs = [rng.choice(cand) for _ in range(nb)]
    if nb >= 2:
        bs[1] = bs[0]
    return sorted(bs, key=lambda s: s.encode("utf-8"))


def string_expected(values, bounds, right):
    bb = [b.encode("utf-8") for b in bounds]
    f = bisect_right if right else bisect_left
    return [f(bb, (v or "").encode("utf-8")) for v in values]


def slice_view(c: Column, start: int, stop: int) -> Column:
    """Zero-copy row slice: for strings offsets[0] stays non-zero and the
    byte buffer is the parent's."""
    val = None if c.validity is None else c.validity[start:stop]
    if c.dtype.uses_offsets:
        return Column(c.dtype, c.data, val, c.offsets[start:stop + 1])
    return Column(c.dtype, c.data[start:stop], val)


# --------------------------------------------------------------- decimal128
def i128_column(ints, valid=None, device="cpu") -> Column:
    limbs = []
    for v in ints:
        lo = v & M64
        limbs.append((lo - (1 << 64) if lo >= (1 << 63) else lo, v >> 64))
    data = torch.tensor(limbs, dtype=torch.int64).reshape(-1, 2)
    validity = None if valid is None else torch.tensor(valid, dtype=torch.bool)
    return Column(D128, data, validity).to(device)


def i128_pool():
    """Negative values, low limbs with the top bit set, equal high limbs
    with different low limbs, magnitudes beyond 18 digits."""
    pool = [0, 1, -1, 10**18, -10**18, 10**30 + 7, -(10**30) - 7,
            10**37, -(10**37), (1 << 63), (1 << 63) - 1, (1 << 63) + 1,
            -(1 << 63), M64, M64 + 1, -(M64 + 1)]
    for hi in (-3, -1, 0, 5):
        for lo in (0, 1, (1 << 63) - 1, 1 << 63, (1 << 63) + 12345, M64):
            pool.append((hi << 64) | lo)
    return pool


def i128_values(n, seed, null_frac=0.05):
    rng = random.Random(seed)
    pool = i128_pool()
    vals, valid = [], []
    for _ in range(n):
        if rng.random() < 0.5:
            v = rng.choice(pool)
        else:
            v = rng.randint(-10**37, 10**37)
        vals.append(v)
        valid.append(rng.random() >= null_frac)
    return vals, valid


def i128_bounds(vals, nb, seed):
    rng = random.Random(seed)
    bs = [rng.choice(vals) for _ in range(nb)]
    if nb >= 2:
        bs[1] = bs[0]
    return sorted(bs)


def i128_expected(vals, bounds, right):
    f = bisect_right if right else bisect_left
    return [f(bounds, v) for v in vals]


# -------------------------------------------------------------------- tests
@pytest.fixture(scope="module")
def str_case():
    values = string_values(600, seed=11)
    return values, Column.from_pylist(values, dtypes.string)


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("nb", BOUND_COUNTS)
def test_string_ref_matches_bisect(str_case, nb, right):
    values, key = str_case
    bounds = string_bounds(values, nb, seed=nb)
    bcol = Column.from_pylist(bounds, dtypes.string)
    got = ops.range_bucket_ref(key, bcol, right)
    assert got.dtype == torch.int64
    assert got.tolist() == string_expected(values, bounds, right)
    # the public entry point dispatches to the reference on CPU
    assert torch.equal(ops.range_bucket(key, bcol, right), got)


@pytest.mark.parametrize("right", [False, True])
def test_string_every_pool_value_as_bound(right):
    """All pool strings as rows and as bounds: every pair of adversarial
    strings is ordered against each other."""
    pool = string_pool()
    bounds = sorted(set(pool), key=lambda s: s.encode("utf-8"))
    key = Column.from_pylist(pool, dtypes.string)
    got = ops.range_bucket_ref(key, Column.from_pylist(bounds, dtypes.string),
                               right)
    assert got.tolist() == string_expected(pool, bounds, right)


@pytest.mark.parametrize("right", [False, True])
def test_string_sliced_key(str_case, right):
    values, key = str_case
    m = len(values) - 5
    sl = slice_view(key, 3, m)
    assert int(sl.offsets[0]) != 0 and len(sl) == m - 3
    bounds = string_bounds(values, 7, seed=5)
    got = ops.range_bucket(sl, Column.from_pylist(bounds, dtypes.string), right)
    assert got.tolist() == string_expected(values[3:m], bounds, right)


def test_string_empty_key_and_null_bounds_rejected():
    empty = Column.from_pylist([], dtypes.string)
    b = Column.from_pylist(["a", "b"], dtypes.string)
    assert ops.range_bucket(empty, b).numel() == 0
    with pytest.raises(AssertionError):
        ops.range_bucket(b, Column.from_pylist(["a", None], dtypes.string))


@pytest.mark.parametrize("right", [False, True])
@pytest.mark.parametrize("nb", BOUND_COUNTS)
def test_decimal128_ref_matches_bigint_bisect(nb, right):
    vals, valid = i128_values(500, seed=23)
    key = i128_column(vals, valid)
    bounds = i128_bounds(vals, nb, seed=nb)
    bcol = i128_column(bounds)
    got = ops.range_bucket_ref(key, bcol, right)
    assert got.tolist() == i128_expected(vals, bounds, right)
    assert torch.equal(ops.range_bucket(key, bcol, right), got)
    sl = slice_view(key, 3, 400)
    assert ops.range_bucket(sl, bcol, right).tolist() == \
        i128_expected(vals[3:400], bounds, right)


@pytest.mark.parametrize("right", [False, True])
def test_int64_is_searchsorted(right):
    g = torch.Generator().manual_seed(4)
    k = torch.randint(-50, 50, (1000,), generator=g)
    b = torch.randint(-50, 50, (9,), generator=g).sort().values
    got = ops.range_bucket(Column(dtypes.int64, k), Column(dtypes.int64, b),
                           right)
    assert torch.equal(got, torch.searchsorted(b, k, right=right))
