"""The Window operator (window_exec.rs processors): the input is sorted once
by (partition, ORDER BY); partitions, peer groups and the node's frame are
derived once per node and shared by its functions (`_FUNCTIONS`)."""
from __future__ import annotations

from functools import cached_property
from typing import List

import torch

from .. import dtypes, ops
from ..column import Column, RecordBatch, adjacent_equal, compact_validity
from ..exprs import AggFunc, Col, Literal, WindowFunc, _cast_col, \
    dec128_to_float64
from ..plan import nodes as P
from .agg import _finalize_agg, _state_dtype, _sum128_scatter, \
    _sum_needs_128, _sum_split_128


class _Peers:
    """Peer groups (runs of equal ORDER BY keys inside a partition), from
    the mask of their first rows."""

    def __init__(self, lay: "_Layout", first: torch.Tensor):
        self.lay, self.first = lay, first

    @cached_property
    def group(self) -> torch.Tensor:
        """Per row: running index of its peer group."""
        return torch.cumsum(self.first.to(torch.int64), 0) - 1

    @cached_property
    def start(self) -> torch.Tensor:
        """Per row: index of its first peer."""
        idx = self.lay.idx
        return torch.cummax(
            torch.where(self.first, idx, torch.full_like(idx, -1)), 0).values

    @cached_property
    def end(self) -> torch.Tensor:
        """Per row: index of its last peer."""
        pstart = torch.nonzero(self.first, as_tuple=False).flatten()
        return torch.cat([pstart[1:] - 1, self.lay.tail])[self.group]


class _Layout:
    """The node's input sorted by (partition, ORDER BY): `sb`, and over its
    `n` rows the dense partition id `seg` (`nseg` partitions starting at
    `seg_start`), per row the index of its partition's `first` and `last`
    row and its `pos_in_seg`. Well defined for n == 0: every per-row and
    per-partition tensor is then empty."""

    def __init__(self, ex, node: P.Window, b: RecordBatch):
        device = b.device
        self.n = n = b.num_rows
        self.order_by = list(node.order_by)
        self.idx = torch.arange(n, dtype=torch.int64, device=device)
        self.tail = self.idx[n - 1:]  # [n - 1], or nothing when n == 0
        # first row of each partition
        starts = torch.zeros(n, dtype=torch.bool, device=device)
        starts[:1] = True
        if node.partition_by:
            # partition membership only needs GROUPING, not lexicographic
            # order: map partition keys (often several strings) to hash
            # group ids once and sort by the integer id — avoids per-pass
            # host string-rank sorts that dominated q47/q57/q67
            pcols = [k.eval(b) for k in node.partition_by]
            gids0, _ = ops.group_ids(pcols)
            tmp = RecordBatch(list(b.names) + ["__wgid"],
                              list(b.columns) + [Column(dtypes.int64, gids0)])
            perm = ex._sort_permutation(
                tmp, [(Col("__wgid"), True)] + self.order_by)
            gids = gids0[perm]
            starts[1:] = gids[1:] != gids[:-1]
        else:
            perm = (ex._sort_permutation(b, self.order_by)
                    if self.order_by else self.idx)
        self.sb = b.gather(perm)
        self.sb._eval_memo = {}  # CSE scope; sb is operator-local, dies with it
        self.starts = starts
        # normalize arbitrary hash ids to dense segment ids over the
        # sorted rows
        self.seg = torch.cumsum(starts.to(torch.int64), 0) - 1
        self.seg_start = torch.nonzero(starts, as_tuple=False).flatten()
        self.nseg = self.seg_start.numel()
        self.first = self.seg_start[self.seg]
        self.pos_in_seg = self.idx - self.first
        self._peers = {}

    @cached_property
    def seg_last(self) -> torch.Tensor:
        return torch.cat([self.seg_start[1:] - 1, self.tail])

    @cached_property
    def last(self) -> torch.Tensor:
        return self.seg_last[self.seg]

    @cached_property
    def seg_len(self) -> torch.Tensor:
        return self.last - self.first + 1

    @cached_property
    def order_keys(self) -> List[Column]:
        return [k.eval(self.sb) for k, _ in self.order_by]

    def peers(self, nan_equal: bool = False) -> _Peers:
        """Peer groups over all ORDER BY keys; without ORDER BY a whole
        partition is one group. NULL keys are peers of each other, NaN keys
        only when `nan_equal`."""
        # fewer than two rows have no neighbours to compare: skip the keys
        keys = self.order_keys if self.n > 1 else []
        flavour = nan_equal and any(c.dtype.is_float for c in keys)
        if flavour not in self._peers:
            first = self.starts
            if keys:
                same = None
                for c in keys:
                    eq = adjacent_equal(c, nan_equal=flavour)
                    same = eq if same is None else same & eq
                first = first.clone()
                first[1:].logical_or_(~same)
            self._peers[flavour] = _Peers(self, first)
        return self._peers[flavour]


class _Window:
    """One Window node being executed: its layout and its frame, resolved
    once. `kind` is "partition" (no ORDER BY: the whole partition),
    "running" (the default frame with ORDER BY; ROWS: up to the current
    row, RANGE: up to its last peer), "rows" (explicit ROWS bounds) or
    "value" (explicit RANGE bounds)."""

    def __init__(self, ex, node: P.Window, b: RecordBatch):
        self.ex, self.node = ex, node
        self.lay = _Layout(ex, node, b)
        explicit = not (node.frame_lo is None and node.frame_hi == 0)
        self.range_key = None
        if node.frame == "range" and explicit:
            self.kind = "value"
            self.range_key = self._check_value_frame()
        elif node.frame == "rows" and explicit:
            self.kind = "rows"
        else:
            self.kind = "running" if node.order_by else "partition"
        if self.lay.n == 0:
            # no rows, no frames: every kind degenerates to the (empty)
            # whole partition, and no frame kernel runs over zero rows
            self.kind = "partition"
        elif self.range_key is not None:
            self.bump("window.range_frame_rows")

    def bump(self, key: str):
        m = self.ex.ctx.metrics
        m[key] = m.get(key, 0) + self.lay.n

    def _check_value_frame(self):
        """Validate an explicit RANGE frame; -> the single ORDER BY key if a
        bound is a value offset, else None."""
        node = self.node
        lo, hi = node.frame_lo, node.frame_hi
        if not ((lo is not None and lo != 0) or (hi != "U" and hi != 0)):
            return None
        if len(node.order_by) != 1:
            raise ValueError(
                "a RANGE frame with a value offset needs exactly one "
                f"ORDER BY key, got {len(node.order_by)}")
        key = self.lay.order_keys[0]
        kdt = key.dtype
        if not (kdt.is_integer or kdt.is_float or kdt.code in (
                dtypes.DATE32, dtypes.TIMESTAMP, dtypes.DECIMAL64)):
            raise NotImplementedError(
                f"RANGE frame value offsets over a {kdt.name} key")
        want = float if kdt.is_float else int
        for v in (lo, hi):
            if v is not None and v != "U" and (
                    isinstance(v, bool) or not isinstance(v, (int, float))
                    or (want is int and not isinstance(v, int))):
                raise ValueError(
                    f"RANGE frame bound {v!r} does not fit a {kdt.name} key")
        return key

    @cached_property
    def bounds(self):
        """The node's frame as per-row inclusive (a, b, empty) over the
        sorted rows, whatever its kind."""
        L, lo, hi = self.lay, self.node.frame_lo, self.node.frame_hi
        if self.kind == "value":
            a, b = self._value_frame_bounds()
        elif self.kind == "rows":
            # row offsets (None / "U" unbounded), clamped to the partition
            a = L.first if lo is None else torch.maximum(L.idx + int(lo),
                                                         L.first)
            b = L.last if hi == "U" else torch.minimum(L.idx + int(hi), L.last)
        elif self.kind == "running":
            a = L.first
            b = L.peers().end if self.node.frame == "range" else L.idx
        else:
            a, b = L.first, L.last
        return a, b, a > b

    def _value_frame_bounds(self):
        """RANGE BETWEEN <lo> AND <hi> with explicit bounds (Spark's
        semantics) -> per-row inclusive frame (a, b) over the sorted rows.

        CURRENT ROW is the whole peer group; a value offset compares the
        single ORDER BY key (k+lo <= key <= k+hi ascending, k-lo >= key >=
        k-hi descending; integer k±offset saturates). Rows whose key is
        NULL — or NaN for float keys — are special: their offset/current
        bounds resolve to their own peer group, and an ordinary row's offset
        bound never reaches them. Unbounded is the partition edge."""
        L, lo, hi = self.lay, self.node.frame_lo, self.node.frame_hi
        # peer groups (NaN keys are peers of each other, as NULLs are)
        peers = L.peers(nan_equal=True)
        a = L.first if lo is None else peers.start
        b = L.last if hi == "U" else peers.end
        key = self.range_key
        if key is None:
            return a, b
        if key.dtype.is_float:
            kd = key.data.to(torch.float64)
            special = torch.isnan(kd)
        else:
            kd = key.data.to(torch.int64)
            special = torch.zeros_like(L.starts)
        if key.validity is not None:
            special = special | ~key.validity
        # ordinary keys sit contiguously inside each partition (NULLs
        # and NaNs sort to its ends): per-partition window [slo, shi]
        ordinary = ~special
        slo = torch.full_like(L.seg_start, L.n)
        shi = torch.full_like(L.seg_start, -1)
        slo.scatter_reduce_(0, L.seg[ordinary], L.idx[ordinary], "amin")
        shi.scatter_reduce_(0, L.seg[ordinary], L.idx[ordinary], "amax")
        # (a partition without ordinary keys keeps the empty [n, -1])
        ka, kb = ops.window_range_bounds(
            kd, slo[L.seg], shi[L.seg], lo, hi,
            descending=not self.node.order_by[0][1])
        if lo is not None:
            a = torch.where(special, a, ka)
        if hi != "U":
            b = torch.where(special, b, kb)
        return a, b


# ------------------------------------------------------------- aggregates
def _prefix_range(pre, a, b, empty):
    """pre[b] - (a > 0 ? pre[a-1] : 0) of an inclusive prefix array, zero
    for an empty frame."""
    hi_v = pre[b.clamp(min=0)]
    lo_i = a - 1
    lo_v = torch.where(lo_i >= 0, pre[lo_i.clamp(min=0)],
                       torch.zeros((), dtype=pre.dtype, device=pre.device))
    out = hi_v - lo_v
    return torch.where(empty, torch.zeros_like(out), out)


def _valid_mask(w: _Window, val: Column) -> torch.Tensor:
    return val.validity if val.validity is not None else \
        torch.ones_like(w.lay.starts)


def _nulls_to_identity(work, valid, fn: str):
    """`work` (int64 or float64) with NULLs replaced by the identity of
    `fn` (min or max)."""
    if work.dtype == torch.int64:
        info = torch.iinfo(torch.int64)
        fill = info.max if fn == "min" else info.min
    else:
        fill = float("inf") if fn == "min" else float("-inf")
    return torch.where(valid, work, torch.full_like(work, fill))


def _frame_aggregate_i128(fn: str, val: Column, a: torch.Tensor,
                          b: torch.Tensor, empty: torch.Tensor) -> Column:
    """sum/avg/min/max of a DECIMAL128 column over per-row inclusive
    frames [a, b], exact: sums are differences of one unsegmented
    128-bit prefix sum (wrapped prefixes cancel), min/max come from the
    128-bit frame primitive. Nulls are skipped; a frame with no valid
    value gives NULL. sum/min/max keep the argument's type, avg is
    float64."""
    assert val.dtype.code == dtypes.DECIMAL128, val.dtype
    valid = val.validity
    if valid is None:
        cnt = torch.where(empty, torch.zeros_like(a), b - a + 1)
    else:
        cnt = _prefix_range(torch.cumsum(valid.to(torch.int64), 0),
                            a, b, empty)
    validity = compact_validity(cnt > 0)
    if fn in ("sum", "avg"):
        s = ops.window_frame_sum_i128(
            ops.prefix_sum_i128(val.data, valid), a, b)
        if fn == "sum":
            return Column(val.dtype, s, validity)
        data = dec128_to_float64(s, val.dtype.scale) \
            / cnt.clamp(min=1).to(torch.float64)
        return Column(dtypes.float64, data, validity)
    assert fn in ("min", "max"), fn
    x = val.data
    if valid is not None:
        ident = torch.tensor(
            ops._I128_MAX if fn == "min" else ops._I128_MIN,
            dtype=torch.int64, device=a.device)
        x = torch.where(valid.unsqueeze(1), x, ident)
    # an empty frame (a > b) yields the identity; cnt == 0 makes it NULL
    m = ops.window_frame_minmax_i128(x, a, b, fn)
    return Column(val.dtype, m, validity)


def _frame_aggregate(w: _Window, fn: str, val: Column) -> Column:
    """sum/avg/count/min/max over the node's per-row inclusive frames
    [a, b] (`empty` marks a > b): prefix-sum differences for
    sum/avg/count, the frame min/max primitive for min/max. Nulls are
    skipped; a frame with no valid value gives NULL (count 0)."""
    a, b, empty = w.bounds
    valid = _valid_mask(w, val)
    cnt = _prefix_range(torch.cumsum(valid.to(torch.int64), 0), a, b, empty)
    if fn == "count":
        return Column(dtypes.int64, cnt)
    validity = compact_validity(cnt > 0)
    if fn in ("sum", "avg"):
        vd = val.data
        if vd.dtype not in (torch.float64, torch.float32):
            vd = vd.to(torch.int64)
        x = torch.where(valid, vd, torch.zeros_like(vd))
        s = _prefix_range(torch.cumsum(x, 0), a, b, empty)
        if fn == "avg":
            data = s.to(torch.float64) / cnt.clamp(min=1).to(torch.float64)
            if val.dtype.code == dtypes.DECIMAL64:
                data = data / (10.0 ** val.dtype.scale)
            return Column(dtypes.float64, data, validity)
        out_dt = val.dtype if val.dtype.code == dtypes.DECIMAL64 else (
            dtypes.float64 if val.dtype.is_float else dtypes.int64)
        return Column(out_dt, s.to(out_dt.torch_dtype), validity)
    assert fn in ("min", "max"), fn
    vd = val.data
    x = _nulls_to_identity(vd.to(torch.float64 if vd.dtype.is_floating_point
                                 else torch.int64), valid, fn)
    # an empty frame (a > b) yields the identity; cnt == 0 makes it NULL
    m = ops.window_frame_minmax(x, a, b, fn)
    w.bump("window.frame_minmax_rows")
    return Column(val.dtype, m.to(vd.dtype), validity)


def _short_span_minmax(w: _Window, fn: str, val: Column) -> Column:
    """min/max over explicit ROWS bounds with a short bounded span
    (window_exec.rs frame processors): a chain of shifted comparisons."""
    L, lo, hi = w.lay, w.node.frame_lo, w.node.frame_hi
    valid = _valid_mask(w, val)
    cmp = torch.minimum if fn == "min" else torch.maximum
    acc = None
    for off in range(lo, hi + 1):
        j = (L.idx + off).clamp(0, max(L.n - 1, 0))
        ok = (L.idx + off >= L.first) & (L.idx + off <= L.last) & valid[j]
        v = val.data[j]
        if acc is None:
            acc, acc_ok = v.clone(), ok.clone()
        else:
            acc = torch.where(ok & ~acc_ok, v, acc)
            acc = torch.where(ok & acc_ok, cmp(acc, v), acc)
            acc_ok = acc_ok | ok
    return Column(val.dtype, acc, compact_validity(acc_ok))


def _running_aggregate(w: _Window, fn: str, val: Column) -> Column:
    """Cumulative frame within partitions (nulls skipped)."""
    L = w.lay
    v = val.data
    if v.dtype in (torch.int8, torch.int16, torch.int32):
        v = v.to(torch.int64)
    elif v.dtype == torch.float32:
        v = v.to(torch.float64)
    valid = _valid_mask(w, val)
    cum_valid = torch.cumsum(valid.to(torch.int64), 0)
    run_count = cum_valid - (cum_valid[L.first]
                             - valid[L.first].to(torch.int64))
    if fn == "count":
        return Column(dtypes.int64, run_count)
    validity = compact_validity(run_count > 0)
    if fn in ("sum", "avg"):
        z = torch.where(valid, v, torch.zeros_like(v))
        cs = torch.cumsum(z, 0)
        run = cs - (cs[L.first] - z[L.first])
        if fn == "avg":
            return Column(dtypes.float64,
                          run.to(torch.float64)
                          / run_count.clamp(min=1).to(torch.float64),
                          validity)
        dt = val.dtype if val.dtype.code == dtypes.DECIMAL64 else (
            dtypes.float64 if run.dtype == torch.float64 else dtypes.int64)
        return Column(dt, run, validity)
    # running min/max: exact segmented scan in the VALUE domain (int64
    # for int/decimal, float64 for floats) via log2(maxseglen) doubling
    # steps — never routed through shifted floats, so int64/decimal
    # values beyond 2^53 stay exact (advisor finding r1).
    run = _nulls_to_identity(
        v if v.dtype == torch.int64 else v.to(torch.float64), valid, fn)
    combine = torch.minimum if fn == "min" else torch.maximum
    maxlen = int((L.seg_last - L.seg_start).max().item()) + 1
    off = 1
    while off < maxlen:
        cand = torch.empty_like(run)
        cand[off:] = run[:-off]
        ok = (L.idx - off) >= L.first
        run = torch.where(ok, combine(run, cand), run)
        off <<= 1
    dt = val.dtype if val.dtype.code == dtypes.DECIMAL64 else (
        dtypes.int64 if val.dtype.is_integer else dtypes.float64)
    return Column(dt, run, validity)


def _aggregate(w: _Window, wf: WindowFunc, name: str) -> Column:
    node, L, fn = w.node, w.lay, wf.fn
    val = wf.arg.eval(L.sb)
    wide = val.dtype.code == dtypes.DECIMAL128
    if wide or (fn == "sum" and _sum_needs_128(val.dtype)):
        if fn == "sum" and not (node.order_by and L.n):
            # whole-partition sum promoted to decimal128:
            # exact limb accumulation (q12/q20/q98 ratios)
            scatter = _sum128_scatter if wide else _sum_split_128
            data, cnt = scatter(L.seg, max(L.nseg, 1), val)
            out_dt = val.dtype if wide else _state_dtype(
                AggFunc("sum", None, name=name), val.dtype)
            return Column(out_dt, data,
                          compact_validity(cnt > 0)).gather(L.seg)
        if wide and fn != "count":
            # every other decimal128 frame: exact 128-bit
            # prefix / pyramid over the per-row frame (a, b)
            w.bump("window.frame_i128_rows")
            return _frame_aggregate_i128(fn, val, *w.bounds)
        # decimal64 sums wide enough to need 128 bits (and
        # count over decimal128): float64 accumulator
        val = _cast_col(val, dtypes.float64)
    if w.kind == "rows" and fn in ("min", "max") and isinstance(
            node.frame_lo, int) and isinstance(node.frame_hi, int) \
            and node.frame_hi - node.frame_lo < 1024:
        return _short_span_minmax(w, fn, val)
    if w.kind in ("value", "rows"):
        return _frame_aggregate(w, fn, val)
    if w.kind == "running":
        # Spark's default frame with ORDER BY: unbounded
        # preceding .. current row (running aggregate)
        out = _running_aggregate(w, fn, val)
        if node.frame == "range":
            # RANGE frame: peer rows (equal order keys within the
            # partition) share the value at the LAST peer row
            out = out.gather(L.peers().end)
        return out
    # whole-partition aggregate (no ORDER BY, no frame): the GROUP BY
    # kernels, so float MIN/MAX follow the aggregate rule (NaN the greatest
    # value: MIN skips NaN unless all are NaN), whereas the frame and running
    # paths above keep "NaN propagates" into both MIN and MAX
    acc, cnt = ops.agg_scatter(L.seg, max(L.nseg, 1), val, fn)
    return _finalize_agg(AggFunc(fn, None, name=name), val.dtype, acc,
                            cnt).gather(L.seg)


# ------------------------------------------------- ranking, offset, value
def _row_number(w, wf, name):
    return Column(dtypes.int64, w.lay.pos_in_seg + 1)


def _rank(w, wf, name):
    """SQL rank(): 1 + index distance from the partition's first row to the
    row's first peer."""
    return Column(dtypes.int64, w.lay.peers().start - w.lay.first + 1)


def _dense_rank(w, wf, name):
    group = w.lay.peers().group
    return Column(dtypes.int64, group - group[w.lay.first] + 1)


def _percent_rank(w, wf, name):
    denom = (w.lay.seg_len - 1).clamp(min=1).to(torch.float64)
    return Column(dtypes.float64,
                  (_rank(w, wf, name).data - 1).to(torch.float64) / denom)


def _cume_dist(w, wf, name):
    L = w.lay
    # without ORDER BY every row counts as its own peer group here
    pend = L.peers().end if L.order_by else L.idx
    return Column(dtypes.float64, (pend - L.first + 1).to(torch.float64)
                  / L.seg_len.to(torch.float64))


def _ntile(w, wf, name):
    # ntile(k): first (len%k) buckets get one extra row
    L = w.lay
    k = wf.offset if wf.offset else 1
    base = torch.div(L.seg_len, k, rounding_mode="floor")
    rem = L.seg_len - base * k
    cut = rem * (base + 1)
    lo = torch.div(L.pos_in_seg, (base + 1).clamp(min=1),
                   rounding_mode="floor") + 1
    hi = rem + torch.div((L.pos_in_seg - cut), base.clamp(min=1),
                         rounding_mode="floor") + 1
    return Column(dtypes.int64, torch.where(L.pos_in_seg < cut, lo, hi))


def _lead_lag(w, wf, name):
    L = w.lay
    val = wf.arg.eval(L.sb)
    k = wf.offset if wf.offset else 1
    idx = L.idx - (-k if wf.fn == "lead" else k)
    idx_c = idx.clamp(0, max(L.n - 1, 0))
    ok = (idx >= 0) & (idx < L.n) & (L.seg[idx_c] == L.seg)
    gi = torch.where(ok, idx_c, torch.full_like(idx_c, -1))
    out = val.gather(gi, may_have_negative=True)
    if wf.default is not None and out.validity is not None:
        dcol = Literal(wf.default, val.dtype).eval(L.sb)
        esc = ~out.validity
        # only frame-escapes get the default; genuine nulls stay
        if val.validity is not None:
            esc = esc & ~torch.where(gi >= 0, ~val.validity[gi.clamp(min=0)],
                                     torch.zeros_like(esc))
        out = Column(out.dtype, torch.where(esc, dcol.data, out.data),
                     compact_validity(out.validity | esc))
    return out


def _value_at(val: Column, at: torch.Tensor, miss: torch.Tensor) -> Column:
    """val[at], NULL where `miss`."""
    return val.gather(torch.where(miss, torch.full_like(at, -1), at),
                      may_have_negative=True)


def _first_last_value(w, wf, name):
    L = w.lay
    val = wf.arg.eval(L.sb)
    if w.kind == "value":
        a, b, empty = w.bounds
        return _value_at(val, a if wf.fn == "first_value" else b, empty)
    if wf.fn == "first_value":
        return val.gather(L.first)
    # frame unbounded preceding..current: ROWS -> current row;
    # RANGE -> last peer row
    if w.kind == "running" and w.node.frame == "range":
        return val.gather(L.peers().end)
    return val


def _nth_value(w, wf, name):
    L = w.lay
    k = wf.offset if wf.offset else 1
    return _value_at(wf.arg.eval(L.sb), L.first + (k - 1),
                     L.pos_in_seg < (k - 1))


_FUNCTIONS = {
    "row_number": _row_number, "rank": _rank, "dense_rank": _dense_rank,
    "percent_rank": _percent_rank, "cume_dist": _cume_dist, "ntile": _ntile,
    "sum": _aggregate, "avg": _aggregate, "count": _aggregate,
    "min": _aggregate, "max": _aggregate,
    "lead": _lead_lag, "lag": _lead_lag,
    "first_value": _first_last_value, "last_value": _first_last_value,
    "nth_value": _nth_value,
}


def exec_window(ex, node: P.Window, b: RecordBatch) -> List[RecordBatch]:
    """Run `node` over its concatenated input `b` for the executor `ex`:
    the child's columns in sorted order, followed by one column per
    function."""
    w = _Window(ex, node, b)
    names, cols = list(w.lay.sb.names), list(w.lay.sb.columns)
    for al in node.functions:
        if al.expr.fn not in _FUNCTIONS:
            raise NotImplementedError(f"window fn {al.expr.fn}")
        names.append(al.name)
        cols.append(_FUNCTIONS[al.expr.fn](w, al.expr, al.name))
    return [RecordBatch(names, cols)]
