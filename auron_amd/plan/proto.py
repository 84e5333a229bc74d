"""TaskDefinition protobuf serde (plan/auron.proto over plan/pbwire).

Role parity: auron-planner's prost encode + planner.rs decode
(create_plan :122 / create_expr :941): a host engine serializes a
TaskDefinition with any protobuf binding generated from plan/auron.proto
and the engine decodes it here into executable PhysicalPlanNodes.
"""
from __future__ import annotations

import dataclasses
import importlib
from typing import List, Optional

import msgpack
import torch

from .. import dtypes as _dt
from ..dtypes import DataType
from ..exchange import pack_batch, unpack_batch
from ..exprs import (AggFunc, Aliased, Arith, BoolOp, CaseWhen, Cast, Cmp,
                     Col, Expr, InList, IsNull, Like, Literal, Not, TryCast,
                     WindowFunc)
from . import nodes as P
from .pbwire import (decode_fields, write_double, write_int, write_len,
                     write_str)

# --------------------------------------------------------------- helpers

_ARITH_OPS = {"+", "-", "*", "/", "%"}
_CMP_OPS = {"==", "!=", "<", "<=", ">", ">="}


def _msg(fn):
    """Build a sub-message payload with a local bytearray."""
    out = bytearray()
    fn(out)
    return bytes(out)


def _enc_dtype(dt: DataType) -> bytes:
    def build(o):
        write_int(o, 1, dt.code)
        if dt.precision:
            write_int(o, 2, dt.precision)
        if dt.scale:
            write_int(o, 3, dt.scale)

    return _msg(build)


def _dec_dtype(buf: bytes) -> DataType:
    f = decode_fields(buf)
    return DataType(f[1][-1] if 1 in f else 0,
                    f[2][-1] if 2 in f else 0,
                    f[3][-1] if 3 in f else 0)


def _enc_scalar(value, dtype: Optional[DataType]) -> bytes:
    def build(o):
        if value is None:
            write_int(o, 1, 1)
        if dtype is not None:
            write_len(o, 2, _enc_dtype(dtype))
            write_int(o, 7, 1)
        if isinstance(value, bool):
            write_int(o, 6, int(value))
        elif isinstance(value, int):
            write_int(o, 3, value)
        elif isinstance(value, float):
            write_double(o, 4, value)
        elif isinstance(value, str):
            write_str(o, 5, value)

    return _msg(build)


def _dec_scalar(buf: bytes):
    f = decode_fields(buf)
    dtype = _dec_dtype(f[2][-1]) if f.get(7, [0])[-1] else None
    if f.get(1, [0])[-1]:
        return None, dtype
    if 6 in f:
        return bool(f[6][-1]), dtype
    if 3 in f:
        return f[3][-1], dtype
    if 4 in f:
        return f[4][-1], dtype
    if 5 in f:
        return f[5][-1].decode("utf-8"), dtype
    return None, dtype


# ------------------------------------------------------------ expressions
def encode_expr(e: Expr) -> bytes:
    def build(o):
        if isinstance(e, Col):
            write_len(o, 1, _msg(lambda m: write_str(m, 1, e.name)))
        elif isinstance(e, Literal):
            write_len(o, 2, _enc_scalar(e.value, e.dtype))
        elif isinstance(e, (Arith, Cmp)):
            def m(b):
                write_len(b, 1, encode_expr(e.left))
                write_len(b, 2, encode_expr(e.right))
                write_str(b, 3, e.op)

            write_len(o, 4, _msg(m))
        elif isinstance(e, IsNull):
            write_len(o, 6, _msg(lambda m: write_len(m, 1, encode_expr(e.child))))
        elif isinstance(e, Not):
            write_len(o, 8, _msg(lambda m: write_len(m, 1, encode_expr(e.child))))
        elif isinstance(e, CaseWhen):
            def m(b):
                for c, v in e.branches:
                    write_len(b, 1, encode_expr(c))
                    write_len(b, 2, encode_expr(v))
                if e.otherwise is not None:
                    write_len(b, 3, encode_expr(e.otherwise))
                    write_int(b, 4, 1)

            write_len(o, 9, _msg(m))
        elif isinstance(e, TryCast):  # before Cast: TryCast subclasses? no, both leafs
            def m(b):
                write_len(b, 1, encode_expr(e.child))
                write_len(b, 2, _enc_dtype(e.to))

            write_len(o, 15, _msg(m))
        elif isinstance(e, Cast):
            def m(b):
                write_len(b, 1, encode_expr(e.child))
                write_len(b, 2, _enc_dtype(e.to))

            write_len(o, 10, _msg(m))
        elif isinstance(e, InList):
            def m(b):
                write_len(b, 1, encode_expr(e.child))
                for v in e.values:
                    write_len(b, 2, _enc_scalar(v, None))

            write_len(o, 13, _msg(m))
        elif isinstance(e, BoolOp):
            def m(b):
                write_str(b, 1, e.op)
                for a in e.args:
                    write_len(b, 2, encode_expr(a))

            write_len(o, 16, _msg(m))
        elif isinstance(e, Like):
            def m(b):
                write_len(b, 1, encode_expr(e.child))
                write_str(b, 2, e.pattern)

            write_len(o, 20, _msg(m))
        elif isinstance(e, WindowFunc):
            def m(b):
                write_str(b, 1, e.fn)
                if e.arg is not None:
                    write_len(b, 2, encode_expr(e.arg))
                    write_int(b, 3, 1)
                write_int(b, 4, e.offset)
                if e.default is not None:
                    write_len(b, 5, _enc_scalar(e.default, None))
                    write_int(b, 6, 1)

            write_len(o, 21, _msg(m))
        else:
            write_len(o, 14, _enc_function(e))

    return _msg(build)


def _enc_function(e: Expr) -> bytes:
    """Generic function-expr carrier: class name + reflected fields."""
    assert dataclasses.is_dataclass(e), f"cannot encode {type(e)}"

    def build(o):
        write_str(o, 1, type(e).__name__)
        for f in dataclasses.fields(e):
            v = getattr(e, f.name)
            write_len(o, 2, _enc_field(f.name, v))

    return _msg(build)


def _enc_field(name: str, v) -> bytes:
    def build(o):
        write_str(o, 1, name)
        if v is None:
            write_int(o, 9, 7)
        elif isinstance(v, Expr):
            write_len(o, 2, encode_expr(v))
            write_int(o, 9, 0)
        elif isinstance(v, bool):
            write_int(o, 8, int(v))
            write_int(o, 9, 6)
        elif isinstance(v, int):
            write_int(o, 3, v)
            write_int(o, 9, 1)
        elif isinstance(v, str):
            write_str(o, 4, v)
            write_int(o, 9, 2)
        elif isinstance(v, float):
            write_double(o, 5, v)
            write_int(o, 9, 3)
        elif isinstance(v, DataType):
            write_len(o, 6, _enc_dtype(v))
            write_int(o, 9, 4)
        elif isinstance(v, (list, tuple)) and all(isinstance(x, Expr) for x in v):
            for x in v:
                write_len(o, 7, encode_expr(x))
            write_int(o, 9, 5)
        else:
            raise TypeError(f"unsupported function field {name}={v!r}")

    return _msg(build)


_FUNC_REGISTRY = {}
for _mod in ("auron_amd.exprs", "auron_amd.functions"):
    _m = importlib.import_module(_mod)
    for _n in dir(_m):
        _c = getattr(_m, _n)
        if isinstance(_c, type) and dataclasses.is_dataclass(_c):
            _FUNC_REGISTRY[_n] = _c


def _dec_function(buf: bytes) -> Expr:
    f = decode_fields(buf)
    name = f[1][-1].decode("utf-8")
    cls = _FUNC_REGISTRY.get(name)
    if cls is None:
        raise ValueError(f"unknown function expr {name}")
    kwargs = {}
    for fb in f.get(2, []):
        ff = decode_fields(fb)
        fname = ff[1][-1].decode("utf-8")
        kind = ff.get(9, [0])[-1]
        if kind == 7:
            kwargs[fname] = None
        elif kind == 0:
            kwargs[fname] = decode_expr(ff[2][-1])
        elif kind == 1:
            kwargs[fname] = ff[3][-1]
        elif kind == 2:
            kwargs[fname] = ff[4][-1].decode("utf-8")
        elif kind == 3:
            kwargs[fname] = ff[5][-1]
        elif kind == 4:
            kwargs[fname] = _dec_dtype(ff[6][-1])
        elif kind == 5:
            kwargs[fname] = [decode_expr(x) for x in ff.get(7, [])]
        elif kind == 6:
            kwargs[fname] = bool(ff[8][-1])
    return cls(**kwargs)


def decode_expr(buf: bytes) -> Expr:
    f = decode_fields(buf)
    if 1 in f:
        m = decode_fields(f[1][-1])
        return Col(m[1][-1].decode("utf-8"))
    if 2 in f:
        v, dt = _dec_scalar(f[2][-1])
        return Literal(v, dt)
    if 4 in f:
        m = decode_fields(f[4][-1])
        op = m[3][-1].decode("utf-8")
        l = decode_expr(m[1][-1])
        r = decode_expr(m[2][-1])
        return Arith(op, l, r) if op in _ARITH_OPS else Cmp(op, l, r)
    if 6 in f:
        m = decode_fields(f[6][-1])
        return IsNull(decode_expr(m[1][-1]))
    if 8 in f:
        m = decode_fields(f[8][-1])
        return Not(decode_expr(m[1][-1]))
    if 9 in f:
        m = decode_fields(f[9][-1])
        whens = [decode_expr(x) for x in m.get(1, [])]
        thens = [decode_expr(x) for x in m.get(2, [])]
        otherwise = decode_expr(m[3][-1]) if m.get(4, [0])[-1] else None
        return CaseWhen(list(zip(whens, thens)), otherwise)
    if 10 in f:
        m = decode_fields(f[10][-1])
        return Cast(decode_expr(m[1][-1]), _dec_dtype(m[2][-1]))
    if 15 in f:
        m = decode_fields(f[15][-1])
        return TryCast(decode_expr(m[1][-1]), _dec_dtype(m[2][-1]))
    if 13 in f:
        m = decode_fields(f[13][-1])
        vals = [_dec_scalar(x)[0] for x in m.get(2, [])]
        return InList(decode_expr(m[1][-1]), vals)
    if 16 in f:
        m = decode_fields(f[16][-1])
        return BoolOp(m[1][-1].decode("utf-8"),
                      [decode_expr(x) for x in m.get(2, [])])
    if 20 in f:
        m = decode_fields(f[20][-1])
        return Like(decode_expr(m[1][-1]), m[2][-1].decode("utf-8"))
    if 21 in f:
        m = decode_fields(f[21][-1])
        arg = decode_expr(m[2][-1]) if m.get(3, [0])[-1] else None
        default = _dec_scalar(m[5][-1])[0] if m.get(6, [0])[-1] else None
        return WindowFunc(m[1][-1].decode("utf-8"), arg,
                          m.get(4, [1])[-1], default)
    if 14 in f:
        return _dec_function(f[14][-1])
    raise ValueError("empty PhysicalExprNode")


def _enc_aliased(a: Aliased) -> bytes:
    return _msg(lambda o: (write_len(o, 1, encode_expr(a.expr)),
                           write_str(o, 2, a.name)))


def _dec_aliased(buf: bytes) -> Aliased:
    f = decode_fields(buf)
    return Aliased(decode_expr(f[1][-1]), f[2][-1].decode("utf-8"))


def _enc_sortkey(e: Expr, asc: bool) -> bytes:
    return _msg(lambda o: (write_len(o, 1, encode_expr(e)),
                           write_int(o, 2, int(asc))))


def _dec_sortkey(buf: bytes):
    f = decode_fields(buf)
    return decode_expr(f[1][-1]), bool(f.get(2, [1])[-1])


def _enc_aggfn(a: AggFunc) -> bytes:
    def build(o):
        write_str(o, 1, a.fn)
        if a.expr is not None:
            write_len(o, 2, encode_expr(a.expr))
            write_int(o, 3, 1)
        if a.distinct:
            write_int(o, 4, 1)
        write_str(o, 5, a.name)

    return _msg(build)


def _dec_aggfn(buf: bytes) -> AggFunc:
    f = decode_fields(buf)
    expr = decode_expr(f[2][-1]) if f.get(3, [0])[-1] else None
    return AggFunc(f[1][-1].decode("utf-8"), expr,
                   bool(f.get(4, [0])[-1]), f[5][-1].decode("utf-8"))


# --------------------------------------------------------------- plan
def encode_plan(node: P.PlanNode) -> bytes:
    def child(o, tag, payload):
        write_len(o, tag, payload)

    def build(o):
        if isinstance(node, P.Debug):
            child(o, 1, _msg(lambda m: (write_len(m, 1, encode_plan(node.child)),
                                        write_str(m, 2, node.label))))
        elif isinstance(node, P.Exchange):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                write_str(b, 2, node.kind)
                for k in node.keys:
                    write_len(b, 3, encode_expr(k))
                if node.persist:
                    write_int(b, 4, 1)

            child(o, 2, _msg(m))
        elif isinstance(node, P.ParquetScan):
            assert node.filters is None, "scan filters ride Filter nodes"

            def m(b):
                for p in node.paths:
                    write_str(b, 1, p)
                if node.columns is not None:
                    write_int(b, 2, 1)
                    for c in node.columns:
                        write_str(b, 3, c)

            child(o, 5, _msg(m))
        elif isinstance(node, P.Project):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                for a in node.exprs:
                    write_len(b, 2, _enc_aliased(a))

            child(o, 6, _msg(m))
        elif isinstance(node, P.Sort):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                for e, asc in node.keys:
                    write_len(b, 2, _enc_sortkey(e, asc))
                if node.limit is not None:
                    write_int(b, 3, 1)
                    write_int(b, 4, node.limit)

            child(o, 7, _msg(m))
        elif isinstance(node, P.Filter):
            child(o, 8, _msg(lambda m: (write_len(m, 1, encode_plan(node.child)),
                                        write_len(m, 2, encode_expr(node.predicate)))))
        elif isinstance(node, P.Union):
            def m(b):
                for c in node.inputs:
                    write_len(b, 1, encode_plan(c))

            child(o, 9, _msg(m))
        elif isinstance(node, P.SortMergeJoin):
            def m(b):
                write_len(b, 1, encode_plan(node.left))
                write_len(b, 2, encode_plan(node.right))
                for k in node.left_keys:
                    write_len(b, 3, encode_expr(k))
                for k in node.right_keys:
                    write_len(b, 4, encode_expr(k))
                write_str(b, 5, node.how)
                write_str(b, 6, node.existence_col)
                if node.residual is not None:
                    write_len(b, 7, encode_expr(node.residual))
                    write_int(b, 8, 1)

            child(o, 10, _msg(m))
        elif isinstance(node, P.HashJoin):
            def m(b):
                write_len(b, 1, encode_plan(node.left))
                write_len(b, 2, encode_plan(node.right))
                for k in node.left_keys:
                    write_len(b, 3, encode_expr(k))
                for k in node.right_keys:
                    write_len(b, 4, encode_expr(k))
                write_str(b, 5, node.how)
                write_str(b, 6, node.build_side)
                if node.broadcast:
                    write_int(b, 7, 1)
                write_str(b, 8, node.existence_col)
                if node.residual is not None:
                    write_len(b, 9, encode_expr(node.residual))
                    write_int(b, 10, 1)

            child(o, 11, _msg(m))
        elif isinstance(node, P.Broadcast):
            child(o, 13, _msg(lambda m: write_len(m, 1, encode_plan(node.child))))
        elif isinstance(node, P.RenameColumns):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                for n in node.names:
                    write_str(b, 2, n)

            child(o, 14, _msg(m))
        elif isinstance(node, P.EmptyPartitions):
            def m(b):
                for n in node.names:
                    write_str(b, 1, n)

            child(o, 15, _msg(m))
        elif isinstance(node, P.HashAgg):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                for a in node.keys:
                    write_len(b, 2, _enc_aliased(a))
                for a in node.aggs:
                    write_len(b, 3, _enc_aggfn(a))
                write_str(b, 4, node.mode)

            child(o, 16, _msg(m))
        elif isinstance(node, P.Limit):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                write_int(b, 2, node.n)
                if node.offset:
                    write_int(b, 3, node.offset)

            child(o, 17, _msg(m))
        elif isinstance(node, P.MemoryScan):
            def m(b):
                for batch in node.batches:
                    meta, buf = pack_batch(batch.to("cpu"), "cpu")
                    payload = msgpack.packb(
                        {"meta": meta, "buf": buf.numpy().tobytes()},
                        use_bin_type=True)
                    write_len(b, 1, payload)

            child(o, 18, _msg(m))
        elif isinstance(node, P.CoalesceBatches):
            child(o, 19, _msg(lambda m: (write_len(m, 1, encode_plan(node.child)),
                                         write_int(m, 2, node.target_rows))))
        elif isinstance(node, P.Expand):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                for proj in node.projections:
                    write_len(b, 2, _msg(lambda pm, proj=proj: [
                        write_len(pm, 1, _enc_aliased(a)) for a in proj]))

            child(o, 20, _msg(m))
        elif isinstance(node, P.Window):
            def m(b):
                write_len(b, 1, encode_plan(node.child))
                for e in node.partition_by:
                    write_len(b, 2, encode_expr(e))
                for e, asc in node.order_by:
                    write_len(b, 3, _enc_sortkey(e, asc))
                for a in node.functions:
                    write_len(b, 4, _enc_aliased(a))
                write_str(b, 5, node.frame)
                # bounds only when they differ from the default frame, so
                # default-frame plans keep their encoding
                if not (node.frame_lo is None and node.frame_hi == 0):
                    _enc_frame_bound(b, 6, node.frame_lo)
                    _enc_frame_bound(b, 9, node.frame_hi)

            child(o, 22, _msg(m))
        elif isinstance(node, P.Generate):
            assert node.udtf is None, "UDTF callbacks are process-local"

            def m(b):
                write_len(b, 1, encode_plan(node.child))
                write_str(b, 2, node.generator)
                for a in node.args:
                    write_len(b, 3, encode_expr(a))

            child(o, 23, _msg(m))
        elif isinstance(node, P.ParquetSink):
            child(o, 24, _msg(lambda m: (write_len(m, 1, encode_plan(node.child)),
                                         write_str(m, 2, node.path))))
        elif isinstance(node, P.OrcScan):
            def m(b):
                for p in node.paths:
                    write_str(b, 1, p)
                if node.columns is not None:
                    write_int(b, 2, 1)
                    for c in node.columns:
                        write_str(b, 3, c)

            child(o, 25, _msg(m))
        elif isinstance(node, P.OrcSink):
            child(o, 27, _msg(lambda m: (write_len(m, 1, encode_plan(node.child)),
                                         write_str(m, 2, node.path))))
        else:
            raise TypeError(f"cannot proto-encode {type(node).__name__}")

    return _msg(build)


def decode_plan(buf: bytes) -> P.PlanNode:
    f = decode_fields(buf)
    tag = next(iter(f))
    m = decode_fields(f[tag][-1])

    def plan(t=1):
        return decode_plan(m[t][-1])

    def strv(t, default=""):
        return m[t][-1].decode("utf-8") if t in m else default

    if tag == 1:
        return P.Debug(plan(), strv(2))
    if tag == 2:
        return P.Exchange(plan(), strv(2, "hash"),
                          [decode_expr(x) for x in m.get(3, [])],
                          bool(m.get(4, [0])[-1]))
    if tag == 5:
        cols = [x.decode("utf-8") for x in m.get(3, [])] if m.get(2, [0])[-1] else None
        return P.ParquetScan([x.decode("utf-8") for x in m.get(1, [])], cols)
    if tag == 6:
        return P.Project(plan(), [_dec_aliased(x) for x in m.get(2, [])])
    if tag == 7:
        limit = m[4][-1] if m.get(3, [0])[-1] else None
        return P.Sort(plan(), [_dec_sortkey(x) for x in m.get(2, [])], limit)
    if tag == 8:
        return P.Filter(plan(), decode_expr(m[2][-1]))
    if tag == 9:
        return P.Union([decode_plan(x) for x in m.get(1, [])])
    if tag == 10:
        residual = decode_expr(m[7][-1]) if m.get(8, [0])[-1] else None
        return P.SortMergeJoin(decode_plan(m[1][-1]), decode_plan(m[2][-1]),
                               [decode_expr(x) for x in m.get(3, [])],
                               [decode_expr(x) for x in m.get(4, [])],
                               strv(5, "inner"), strv(6, "exists"), residual)
    if tag == 11:
        residual = decode_expr(m[9][-1]) if m.get(10, [0])[-1] else None
        return P.HashJoin(decode_plan(m[1][-1]), decode_plan(m[2][-1]),
                          [decode_expr(x) for x in m.get(3, [])],
                          [decode_expr(x) for x in m.get(4, [])],
                          strv(5, "inner"), strv(6, "right"),
                          bool(m.get(7, [0])[-1]), strv(8, "exists"), residual)
    if tag == 13:
        return P.Broadcast(plan())
    if tag == 14:
        return P.RenameColumns(plan(), [x.decode("utf-8") for x in m.get(2, [])])
    if tag == 15:
        return P.EmptyPartitions([x.decode("utf-8") for x in m.get(1, [])])
    if tag == 16:
        return P.HashAgg(plan(), [_dec_aliased(x) for x in m.get(2, [])],
                         [_dec_aggfn(x) for x in m.get(3, [])],
                         strv(4, "complete"))
    if tag == 17:
        return P.Limit(plan(), m[2][-1], m.get(3, [0])[-1])
    if tag == 18:
        batches = []
        for payload in m.get(1, []):
            d = msgpack.unpackb(payload, raw=False, strict_map_key=False)
            buf2 = torch.frombuffer(bytearray(d["buf"]), dtype=torch.uint8)
            batches.append(unpack_batch(d["meta"], buf2))
        return P.MemoryScan(batches)
    if tag == 19:
        return P.CoalesceBatches(plan(), m[2][-1])
    if tag == 20:
        projections = []
        for pbuf in m.get(2, []):
            pf = decode_fields(pbuf)
            projections.append([_dec_aliased(x) for x in pf.get(1, [])])
        return P.Expand(plan(), projections)
    if tag == 22:
        return P.Window(plan(), [decode_expr(x) for x in m.get(2, [])],
                        [_dec_sortkey(x) for x in m.get(3, [])],
                        [_dec_aliased(x) for x in m.get(4, [])],
                        strv(5, "range"),
                        _dec_frame_bound(m, 6, None),
                        _dec_frame_bound(m, 9, 0))
    if tag == 23:
        return P.Generate(plan(), strv(2),
                          [decode_expr(x) for x in m.get(3, [])])
    if tag == 24:
        return P.ParquetSink(plan(), strv(2))
    if tag == 25:
        cols = [x.decode("utf-8") for x in m.get(3, [])] if m.get(2, [0])[-1] else None
        return P.OrcScan([x.decode("utf-8") for x in m.get(1, [])], cols)
    if tag == 27:
        return P.OrcSink(plan(), strv(2))
    raise ValueError(f"unknown PhysicalPlanNode tag {tag}")


# FrameBoundKind (auron.proto); fields kind, int value, double value sit at
# consecutive tags
_FB_UNBOUNDED_PRECEDING, _FB_UNBOUNDED_FOLLOWING = 1, 2
_FB_OFFSET_INT, _FB_OFFSET_DOUBLE = 3, 4


def _enc_frame_bound(b: bytearray, tag: int, bound):
    if bound is None:
        write_int(b, tag, _FB_UNBOUNDED_PRECEDING)
    elif isinstance(bound, str):
        assert bound == "U", bound
        write_int(b, tag, _FB_UNBOUNDED_FOLLOWING)
    elif isinstance(bound, float):
        write_int(b, tag, _FB_OFFSET_DOUBLE)
        write_double(b, tag + 2, bound)
    else:
        write_int(b, tag, _FB_OFFSET_INT)
        write_int(b, tag + 1, int(bound))


def _dec_frame_bound(m, tag: int, default):
    kind = m.get(tag, [0])[-1]
    if kind == 0:
        return default
    if kind == _FB_UNBOUNDED_PRECEDING:
        return None
    if kind == _FB_UNBOUNDED_FOLLOWING:
        return "U"
    if kind == _FB_OFFSET_INT:
        return m.get(tag + 1, [0])[-1]
    if kind == _FB_OFFSET_DOUBLE:
        return m.get(tag + 2, [0.0])[-1]
    raise ValueError(f"unknown FrameBoundKind {kind}")


# ----------------------------------------------------------- task defs
def serialize_task_pb(task_id: str, stage_id: int, partition: int,
                      plan: P.PlanNode) -> bytes:
    out = bytearray()
    write_str(out, 1, task_id)
    write_int(out, 2, stage_id)
    write_int(out, 3, partition)
    write_len(out, 4, encode_plan(plan))
    return bytes(out)


def deserialize_task_pb(data: bytes):
    f = decode_fields(data)
    return (f[1][-1].decode("utf-8"), f.get(2, [0])[-1], f.get(3, [0])[-1],
            decode_plan(f[4][-1]))
