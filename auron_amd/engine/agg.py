"""The HashAgg operator (agg_exec.rs / agg_table.rs analogue): rows are
grouped once per batch, every aggregate folds into a (value, count) state
pair, and states with equal keys combine through ONE function
(`_combine_states`) whether the streaming table re-merges itself or the
final stage finishes. The helpers that only need tensors are module
functions; the window operator imports the sum and finalize rules from here."""
from __future__ import annotations

import itertools
from typing import List, Optional

import torch

from .. import dtypes, ops
from ..column import Column, RecordBatch, compact_validity
from ..config import AGG_STREAMING, PARTIAL_AGG_SKIPPING_RATIO, \
    STREAM_PEEK_FACTOR, AuronConf
from ..dtypes import DataType
from ..exprs import AggFunc, Col, dec64_to_dec128, eval_scope
from ..plan import nodes as P

# the state of these IS the count: never null, never finalized
_COUNT_FNS = ("count", "count_star", "count_distinct")

# how rows fold into a state, and how two states of one aggregate combine
_COMBINER = {"sum": "sum", "avg": "sum", "min": "min", "max": "max",
             "first": "first", "first_ignores_null": "first"}

# agg fns whose state is mergeable across chunks (everything _combine_states
# can combine); count_distinct / collect_* need the whole group resident
_SPLITTABLE_AGGS = frozenset(_COMBINER) | {"count", "count_star"}


def _state_names(i: int):
    """Partial-state columns of aggregate i: (value state, valid count)."""
    return f"__agg{i}_0", f"__agg{i}_1"


def _concat(batches: List[RecordBatch]) -> RecordBatch:
    from .executor import _concat as concat  # (the executor imports us)

    return concat(batches)


def exec_hash_agg(ex, node: P.HashAgg) -> List[RecordBatch]:
    stream_ok = (AuronConf().get(AGG_STREAMING)
                 and ex._est_input_bytes(node.child)
                 > ex._stream_bytes_threshold())
    if node.mode == "partial" and stream_ok:
        # streaming partial agg (agg_table.rs analogue): inputs are
        # consumed chunk-by-chunk, states re-merged when they shrink,
        # and the accumulated state registers with the memmgr so it
        # can spill under pressure — the whole input never has to be
        # resident at once
        return _partial_chunked(ex, node)
    if (node.mode == "complete" and stream_ok
            and all(a.fn in _SPLITTABLE_AGGS for a in node.aggs)
            and (node.keys or ex.ctx.world_size == 1)):
        # (keyless complete at W>1 keeps the one-shot path: its
        # emit-null-row-only-on-rank-0 rule lives in _hash_agg_body)
        # W=1 collapses partial+exchange+final towers to one complete
        # agg (see _rewrite) — stream it when the input is large:
        # chunk the child into partial states, then run ONE final pass
        # over the merged states (the distributed composition), so a
        # rollup over a SF>=100 fact join never materializes. Small
        # inputs (peeked below one chunk) keep the one-pass grouping.
        buf, rest = _peek_stream(ex, ex.execute_iter(node.child))
        if rest is None:
            return _body_scoped(ex, node, _concat(buf))
        part = P.HashAgg(node.child, node.keys, node.aggs, mode="partial")
        states = _concat(_partial_chunked(
            ex, part, batches=itertools.chain(buf, rest)))
        fin = P.HashAgg(node.child, node.keys, node.aggs, mode="final")
        return _body_scoped(ex, fin, states)
    return _body_scoped(ex, node, ex.collect(node.child))


def _body_scoped(ex, node: P.HashAgg, b: RecordBatch) -> List[RecordBatch]:
    with eval_scope(b):
        return _hash_agg_body(ex, node, b)


def _peek_stream(ex, it, threshold: Optional[int] = None):
    """Pull from a batch iterator until `threshold` rows are buffered.
    Returns (buffered, rest_iterator) — rest is None when the stream
    was exhausted under the threshold (small input: the caller should
    take the cheaper one-shot path; the chunk/merge machinery only
    pays for itself when the input is genuinely large)."""
    if threshold is None:
        threshold = AuronConf().get(STREAM_PEEK_FACTOR) * ex.ctx.batch_rows
    buf: List[RecordBatch] = []
    rows = 0
    for b in it:
        buf.append(b)
        rows += b.num_rows
        if rows > threshold:
            return buf, it
    return buf, None


def _partial_chunked(ex, node: P.HashAgg, batches=None) -> List[RecordBatch]:
    if batches is None:
        buf, rest = _peek_stream(ex, ex.execute_iter(node.child))
        if rest is None:
            return _body_scoped(ex, node, _concat(buf))
        batches = itertools.chain(buf, rest)
    schema_batch: Optional[RecordBatch] = None
    limit = ex.ctx.batch_rows
    memmgr = ex.ctx.memmgr
    acc: List[RecordBatch] = []
    acc_rows = 0
    merge_worthwhile = True
    holder = memmgr.register("agg-partial-state", acc)

    def flush_merge():
        nonlocal acc, acc_rows, merge_worthwhile, holder
        cur = holder.batches()
        merged = _merge_states(node, _concat(cur)) if cur else None
        holder.release()
        if merged is not None:
            if merged.num_rows > 0.8 * acc_rows:
                # low-reduction keys: stop paying for re-merges; the
                # post-exchange final agg regroups anyway
                merge_worthwhile = False
            acc = [merged]
            acc_rows = merged.num_rows
        else:
            acc = []
            acc_rows = 0
        holder = memmgr.register("agg-partial-state", acc)

    for b in batches:
        if schema_batch is None:
            schema_batch = b.slice(0, 0)
        for lo in range(0, max(b.num_rows, 1), limit):
            chunk = b if b.num_rows <= limit else \
                b.slice(lo, min(limit, b.num_rows - lo))
            out = _body_scoped(ex, node, chunk)
            cur = holder.batches()
            cur.extend(out)
            acc_rows += sum(x.num_rows for x in out)
            holder.refresh()
            if b.num_rows <= limit:
                break
        if merge_worthwhile and acc_rows > 2 * limit:
            flush_merge()
    result = holder.batches()
    holder.release()
    if not result:
        # preserve the empty-input partial schema (the child stream is
        # consumed; a 0-row slice of its first batch carries the schema)
        assert schema_batch is not None, "child stream yielded no batches"
        return _body_scoped(ex, node, schema_batch)
    return result


def group_rows(key_cols: List[Column], n: int, device):
    """-> (gid per row, number of groups, key columns one row per group).
    Without keys every row is in group 0 and ONE group is reported: whether
    an empty keyless input still has that group is the caller's rule."""
    if key_cols:
        gids, reps = ops.group_ids(key_cols)
        return gids, int(reps.numel()), [c.gather(reps) for c in key_cols]
    return torch.zeros(n, dtype=torch.int64, device=device), 1, []


def _combine_states(gids, ngroups, fn: str, sv: Column, sc: Column, n: int):
    """Combine the state rows (value state `sv`, count state `sc`, `n` of
    them) that share a group -> (combined value state, merged count). The
    value state comes back as a Column where its validity or layout is its
    own (first, decimal128 limbs), else as the raw accumulator: a state is
    null exactly where its merged count is 0."""
    merged_cnt, _ = ops.agg_scatter(gids, ngroups, sc, "sum")
    if fn in ("count", "count_star"):
        return merged_cnt, merged_cnt
    comb = _COMBINER[fn]  # (count_distinct and collect_* have no state)
    if comb == "first":
        acc, _ = _agg_first(gids, ngroups, sv)
    elif comb == "sum" and sv.dtype.code == dtypes.DECIMAL128:
        data, cnt = _sum128_scatter(gids, ngroups, sv)
        acc = Column(sv.dtype, data, compact_validity(cnt > 0))
    elif comb == "sum" and _decimal_sum_unsafe(sv, n):
        acc, _ = _sum_split_exact(gids, ngroups, sv)
    else:
        acc, _ = ops.agg_scatter(gids, ngroups, sv, comb)
    return acc, merged_cnt


def _merge_states(node: P.HashAgg, b: RecordBatch) -> RecordBatch:
    """Combine partial-state rows with equal keys into one state row
    (state schema in, state schema out — the pre-exchange self-merge
    of the reference's in-memory agg table)."""
    n = b.num_rows
    key_cols = [Col(a.name).eval(b) for a in node.keys]
    gids, ngroups, out_keys = group_rows(key_cols, n, b.device)
    if not key_cols and n == 0:
        ngroups = 0
    names = [a.name for a in node.keys]
    cols = list(out_keys)
    for i, agg in enumerate(node.aggs):
        s0, s1 = _state_names(i)
        sv = b.column(s0)
        acc, cnt = _combine_states(gids, ngroups, agg.fn, sv, b.column(s1), n)
        if agg.fn in _COUNT_FNS:
            acc = Column(dtypes.int64, cnt)
        elif not isinstance(acc, Column):
            acc = Column(sv.dtype, acc, compact_validity(cnt > 0))
        cols += [acc, Column(dtypes.int64, cnt)]
        names += [s0, s1]
    return RecordBatch(names, cols)


def _fusable(agg: AggFunc, val: Optional[Column], n: int) -> bool:
    """Plain sum/avg/min/max that k_agg_multi can take."""
    if agg.fn not in ("sum", "avg", "min", "max") or val is None:
        return False
    if val.dtype.code == dtypes.DECIMAL128:
        return False  # two-limb path
    if agg.fn == "sum" and _sum_needs_128(val.dtype):
        return False  # decimal128 result path
    if agg.fn in ("sum", "avg") and _decimal_sum_unsafe(val, n):
        return False  # exact split path
    return True


def _accumulate(node: P.HashAgg, agg: AggFunc, val: Optional[Column], fused,
                key_cols, gids, ngroups, n: int):
    """Fold the rows of each group into one aggregate -> (acc, valid count,
    value dtype); acc is a Column where the state has its own validity or
    layout, else the raw accumulator. `fused` is this aggregate's
    k_agg_multi result, if it took part."""
    device = gids.device
    if agg.fn == "count_star":
        cnt = ops.agg_count_star(gids, ngroups)
        return cnt, cnt, dtypes.int64
    if agg.fn == "count_distinct":
        assert node.mode == "complete", "count_distinct needs complete mode (pre-exchanged)"
        _, d_reps = ops.group_ids(key_cols + [val])
        og = gids[d_reps]
        if val.validity is not None:
            og = og[val.validity[d_reps]]
        cnt = torch.zeros(ngroups, dtype=torch.int64, device=device)
        if og.numel():
            cnt.scatter_add_(0, og, torch.ones(og.numel(), dtype=torch.int64, device=device))
        return cnt, cnt, dtypes.int64
    if agg.fn in ("collect_list", "collect_set"):
        assert node.mode == "complete", \
            "collect_* needs complete mode (pre-exchanged)"
        acc = _agg_collect(gids, ngroups, val, dedupe=agg.fn == "collect_set",
                           key_cols=key_cols)
        return acc, ops.agg_scatter(gids, ngroups, val, "count")[1], acc.dtype
    if agg.fn in ("first", "first_ignores_null"):
        return (*_agg_first(gids, ngroups, val), val.dtype)
    if fused is not None:
        return (*fused, val.dtype)
    if agg.fn == "sum" and _sum_needs_128(val.dtype):
        # declared result exceeds the 64-bit backing: exact
        # 128-bit limbs (state schema is static -> SPMD-safe)
        scatter = _sum128_scatter if val.dtype.code == dtypes.DECIMAL128 \
            else _sum_split_128
        data, vcnt = scatter(gids, ngroups, val)
        acc = Column(_state_dtype(agg, val.dtype), data,
                     compact_validity(vcnt > 0))
        return acc, vcnt, val.dtype
    if agg.fn in ("sum", "avg") and _decimal_sum_unsafe(val, n):
        return (*_sum_split_exact(gids, ngroups, val), val.dtype)
    fn = "count" if agg.fn == "count" else _COMBINER[agg.fn]
    return (*ops.agg_scatter(gids, ngroups, val, fn), val.dtype)


def _hash_agg_body(ex, node: P.HashAgg, b: RecordBatch) -> List[RecordBatch]:
    n = b.num_rows
    final = node.mode == "final"
    key_cols = [(Col(a.name) if final else a.expr).eval(b) for a in node.keys]
    if key_cols and node.mode == "partial" and _partial_skip(key_cols, n):
        return [_partial_passthrough(node, b, key_cols)]
    gids, ngroups, out_keys = group_rows(key_cols, n, b.device)
    # a keyless (global) agg over an empty input yields one null row
    # in SQL — but distributed, only the rank holding the gathered
    # rows (rank 0 after an Exchange "single") may emit it, else
    # every rank would contribute a duplicate
    if not key_cols and n == 0 and node.mode in ("final", "complete") \
            and ex.ctx.rank != 0:
        ngroups = 0
    names = [a.name for a in node.keys]
    cols = list(out_keys)
    if final:
        for i, agg in enumerate(node.aggs):
            s0, s1 = _state_names(i)
            sv = b.column(s0)
            acc, cnt = _combine_states(gids, ngroups, agg.fn, sv,
                                       b.column(s1), n)
            cols.append(Column(dtypes.int64, cnt) if agg.fn in _COUNT_FNS
                        else _finalize_agg(agg, sv.dtype, acc, cnt, widen=False))
            names.append(agg.name)
        return [RecordBatch(names, cols)]
    vals = [a.expr.eval(b) if a.expr is not None else None for a in node.aggs]
    # fuse plain sum/avg/min/max aggregates into ONE kernel pass
    # (k_agg_multi): gids are read once, head flags computed once
    fused = {}
    if ngroups > 0:
        fuse_idx = [i for i, (a, v) in enumerate(zip(node.aggs, vals))
                    if _fusable(a, v, n)]
        if len(fuse_idx) > 1:
            fused = dict(zip(fuse_idx, ops.agg_scatter_multi(
                gids, ngroups, [(vals[i], node.aggs[i].fn) for i in fuse_idx])))
    for i, (agg, val) in enumerate(zip(node.aggs, vals)):
        acc, vcnt, vdt = _accumulate(node, agg, val, fused.get(i), key_cols,
                                     gids, ngroups, n)
        if node.mode == "partial":
            if not isinstance(acc, Column):
                acc = Column(_state_dtype(agg, vdt), acc,
                             None if agg.fn in _COUNT_FNS else vcnt > 0)
            cols += [acc, Column(dtypes.int64, vcnt)]
            names += _state_names(i)
        else:  # complete
            cols.append(Column(dtypes.int64, acc) if agg.fn in _COUNT_FNS
                        else _finalize_agg(agg, vdt, acc, vcnt))
            names.append(agg.name)
    return [RecordBatch(names, cols)]


def _decimal_sum_unsafe(val: Column, nrows: int) -> bool:
    """True when a plain int64 scatter-sum of this decimal column could
    wrap (advisor finding r1: n*maxabs must fit int64)."""
    if val.dtype.code != dtypes.DECIMAL64 or nrows == 0:
        return False
    m = int(val.data.abs().max().item())
    return m > 0 and nrows * m >= (1 << 62)


def _sum_split_raw(gids, ngroups, val: Column):
    """Split int64 addends into 32-bit digit accumulators (exact for
    <2^31 rows): returns (h, rem, cnt) with group total = h*2^32+rem."""
    device = gids.device
    n = gids.numel()
    assert n < (1 << 31), "batch too large for split accumulation"
    valid = val.validity if val.validity is not None else \
        torch.ones(n, dtype=torch.bool, device=device)
    x = torch.where(valid, val.data, torch.zeros_like(val.data))
    lo = x & 0xFFFFFFFF
    hi = x >> 32
    sum_lo = torch.zeros(ngroups, dtype=torch.int64, device=device)
    sum_hi = torch.zeros(ngroups, dtype=torch.int64, device=device)
    cnt = torch.zeros(ngroups, dtype=torch.int64, device=device)
    if n:
        sum_lo.scatter_add_(0, gids, lo)
        sum_hi.scatter_add_(0, gids, hi)
        cnt.scatter_add_(0, gids, valid.to(torch.int64))
    carry = sum_lo >> 32
    rem = sum_lo & 0xFFFFFFFF
    h = sum_hi + carry
    return h, rem, cnt


def _sum_split_exact(gids, ngroups, val: Column):
    """Exact decimal sum via hi/lo 32-bit split accumulators: each
    int64 addend is split into (v>>32, v&0xffffffff); both partial
    sums stay far from int64 range for <2^31 rows, and the recombine
    detects true overflow of the mathematical result instead of
    silently wrapping (sum(decimal) with p+10>18 routes to the
    decimal128 path instead of this one)."""
    h, rem, cnt = _sum_split_raw(gids, ngroups, val)
    if bool(((h < -(1 << 31)) | (h > (1 << 31) - 1)).any()):
        raise ArithmeticError(
            "decimal sum overflow: group total exceeds 18 significant "
            "digits (decimal64 backing); rescale or cast to double")
    return h * (1 << 32) + rem, cnt


def _sum_split_128(gids, ngroups, val: Column):
    """Exact sum of decimal64 addends into decimal128 limbs.

    total = h*2^32 + rem with rem in [0,2^32); two's-complement
    128-bit limbs are lo = (h<<32)+rem (bit pattern) and
    hi = h>>32 (arithmetic = floor(h/2^32))."""
    h, rem, cnt = _sum_split_raw(gids, ngroups, val)
    lo = (h << 32) + rem
    hi = h >> 32
    return torch.stack([lo, hi], dim=1), cnt


def _sum_needs_128(vdt: DataType) -> bool:
    return (vdt.code == dtypes.DECIMAL64 and vdt.precision + 10 > 18) \
        or vdt.code == dtypes.DECIMAL128


def _sum128_scatter(gids, ngroups, col: Column):
    """Exact group sum of a decimal128 [n,2] column: the 128-bit value
    is split into four 32-bit digits (top digit signed), each digit
    scatter-summed in int64, then recomposed with carry propagation —
    no digit sum can overflow below 2^31 rows."""
    device = gids.device
    n = gids.numel()
    assert n < (1 << 31), "batch too large for split accumulation"
    valid = col.validity if col.validity is not None else \
        torch.ones(n, dtype=torch.bool, device=device)
    z = torch.zeros((), dtype=torch.int64, device=device)
    lo = torch.where(valid, col.data[:, 0], z)
    hi = torch.where(valid, col.data[:, 1], z)
    m = 0xFFFFFFFF
    digs = [lo & m, (lo >> 32) & m, hi & m, hi >> 32]
    sums = []
    cnt = torch.zeros(ngroups, dtype=torch.int64, device=device)
    for d in digs:
        sd = torch.zeros(ngroups, dtype=torch.int64, device=device)
        if n:
            sd.scatter_add_(0, gids, d)
        sums.append(sd)
    if n:
        cnt.scatter_add_(0, gids, valid.to(torch.int64))
    c = sums[0] >> 32
    r0 = sums[0] & m
    t1 = sums[1] + c
    r1 = t1 & m
    t2 = sums[2] + (t1 >> 32)
    r2 = t2 & m
    t3 = sums[3] + (t2 >> 32)
    out_lo = (r1 << 32) | r0
    out_hi = (t3 << 32) | r2
    return torch.stack([out_lo, out_hi], dim=1), cnt


def _partial_skip(key_cols, n: int) -> bool:
    """Partial-agg skipping (conf.rs:39-42): sample the reduction
    ratio; when grouping barely reduces rows, skip the hash table and
    emit singleton states — the post-exchange final agg regroups."""
    if n < (1 << 14):
        return False
    ratio = AuronConf().get(PARTIAL_AGG_SKIPPING_RATIO)
    if ratio >= 1.0:
        return False
    sn = min(n, 1 << 16)
    idx = torch.arange(sn, dtype=torch.int64, device=key_cols[0].device)
    sample = [c.gather(idx) for c in key_cols]
    _, reps = ops.group_ids(sample)
    return int(reps.numel()) > ratio * sn


def _partial_passthrough(node: P.HashAgg, b: RecordBatch,
                         key_cols) -> RecordBatch:
    """Each row becomes its own group: states carry the raw value and
    a 0/1 count. Schema-identical to the grouped partial output."""
    n = b.num_rows
    device = b.device
    names = [a.name for a in node.keys]
    cols = list(key_cols)
    for i, agg in enumerate(node.aggs):
        names += _state_names(i)
        if agg.fn == "count_star":
            ones = torch.ones(n, dtype=torch.int64, device=device)
            cols += [Column(dtypes.int64, ones), Column(dtypes.int64, ones)]
            continue
        val = agg.expr.eval(b)
        valid = val.validity if val.validity is not None else \
            torch.ones(n, dtype=torch.bool, device=device)
        cnt = valid.to(torch.int64)
        if agg.fn == "count":
            cols += [Column(dtypes.int64, cnt), Column(dtypes.int64, cnt)]
            continue
        state_dt = _state_dtype(agg, val.dtype)
        data = val.data
        if (state_dt.code == dtypes.DECIMAL128
                and val.dtype.code == dtypes.DECIMAL64):
            data = dec64_to_dec128(data)
        elif data.dtype != state_dt.torch_dtype and not state_dt.uses_offsets:
            data = data.to(state_dt.torch_dtype)
        cols += [Column(state_dt, data, val.validity, val.offsets),
                 Column(dtypes.int64, cnt)]
    return RecordBatch(names, cols)


def _agg_first(gids, ngroups, val: Column):
    """first value per group, skipping nulls (the reference's
    first_ignores_null; plain `first` maps here too — order is
    engine-dependent in Spark anyway)."""
    device = gids.device
    n = gids.numel()
    order = torch.arange(n, dtype=torch.int64, device=device)
    valid = val.validity
    g, o = (gids, order) if valid is None else (gids[valid], order[valid])
    first_row = torch.full((ngroups,), n, dtype=torch.int64, device=device)
    cnt = torch.zeros(ngroups, dtype=torch.int64, device=device)
    if g.numel():
        first_row.scatter_reduce_(0, g, o, reduce="amin", include_self=True)
        cnt.scatter_add_(0, g, torch.ones_like(g))
    safe = first_row.clamp(max=max(n - 1, 0))
    col = val.gather(safe)
    v = (cnt > 0)
    if col.validity is not None:
        v = v & col.validity
    return Column(val.dtype, col.data, v, col.offsets), cnt


def _state_dtype(agg: AggFunc, vdt: DataType) -> DataType:
    if agg.fn in _COUNT_FNS:
        return dtypes.int64
    if agg.fn in ("sum", "avg"):
        if vdt.code == dtypes.DECIMAL128:
            return dtypes.decimal128(38, vdt.scale)
        if vdt.code == dtypes.DECIMAL64:
            if agg.fn == "sum" and vdt.precision + 10 > 18:
                # exceeds the 64-bit backing: two-limb accumulator
                return dtypes.decimal128(vdt.precision + 10, vdt.scale)
            return dtypes.decimal64(min(vdt.precision + 10, 38), vdt.scale)
        if vdt.is_integer or vdt.code == dtypes.BOOL:
            return dtypes.int64
        return dtypes.float64
    return vdt  # min/max/first keep input type


def _agg_collect(gids, ngroups, val: Column, dedupe: bool,
                 key_cols) -> Column:
    """collect_list / collect_set -> LIST column, one row per group
    (agg/collect.rs analogue). Null inputs excluded; a group with no
    collected values yields an EMPTY list (Spark semantics). Order
    within a list is unspecified (as in Spark)."""
    device = gids.device
    assert not val.dtype.uses_offsets, \
        "collect over string/list children: round 2"
    keep = val.validity if val.validity is not None else \
        torch.ones(len(val), dtype=torch.bool, device=device)
    if dedupe:
        base = key_cols if key_cols else [Column(dtypes.int64, gids)]
        _, d_reps = ops.group_ids(base + [val])
        sel = torch.zeros(len(val), dtype=torch.bool, device=device)
        sel[d_reps] = True
        keep = keep & sel
    idx = torch.nonzero(keep, as_tuple=False).flatten()
    g = gids[idx]
    order = torch.argsort(g, stable=True)
    rows = idx[order]
    lens = torch.bincount(g[order], minlength=ngroups)
    offsets = torch.zeros(ngroups + 1, dtype=torch.int64, device=device)
    torch.cumsum(lens, 0, out=offsets[1:])
    return Column(dtypes.list_of(val.dtype), val.data[rows], None,
                  offsets.to(torch.int64))


def _finalize_agg(agg: AggFunc, vdt: DataType, acc, cnt: torch.Tensor,
                  widen: bool = True) -> Column:
    if agg.fn in ("collect_list", "collect_set"):
        return acc  # empty groups stay empty lists, not null
    validity = compact_validity(cnt > 0)
    if isinstance(acc, Column):
        v = acc.validity
        if validity is not None:
            v = validity if v is None else (v & validity)
        return Column(acc.dtype, acc.data, v, acc.offsets)
    if agg.fn == "avg":
        if vdt.code == dtypes.DECIMAL64:
            # Spark: avg(decimal(p,s)) -> decimal(p+4, s+4), HALF_UP;
            # exact integer long division (advisor finding r1)
            cnt_ = cnt.clamp(min=1)
            sign = torch.sign(acc)
            a = acc.abs()
            q = torch.div(a, cnt_, rounding_mode="floor")
            r = a - q * cnt_
            frac = torch.div(r * 20000 + cnt_, cnt_ * 2,
                             rounding_mode="floor")
            data = sign * (q * 10000 + frac)
            out_dt = dtypes.decimal64(min(vdt.precision + 4, 18),
                                      vdt.scale + 4)
            return Column(out_dt, data, validity)
        data = acc.to(torch.float64) / cnt.clamp(min=1).to(torch.float64)
        return Column(dtypes.float64, data, validity)
    # widen=False: vdt is ALREADY the state dtype (final mode) — a
    # second _state_dtype pass would double-promote sum(decimal)
    out_dt = _state_dtype(agg, vdt) if widen else vdt
    return Column(out_dt, acc, validity)
