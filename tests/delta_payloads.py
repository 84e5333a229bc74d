"""Shared helper for the DELTA_BINARY_PACKED tests (not collected): a
pure-Python encoder that follows the parquet spec, and the payload set
both the CPU and the GPU tests decode.

pyarrow writes only one layout (block 256, 4 miniblocks), so the other
layouts, the junk bit widths of unused miniblocks and the exact bit
widths come from this encoder."""
import random

INT64_MIN = -(1 << 63)
INT64_MAX = (1 << 63) - 1
INT32_MIN = -(1 << 31)
INT32_MAX = (1 << 31) - 1

COUNTS = [0, 1, 2, 33, 64, 65, 129, 257, 1000]
LAYOUTS = [(128, 4), (256, 4), (128, 1), (512, 4)]
BIT_WIDTHS = [0, 1, 7, 8, 31, 32, 33, 57, 58, 63, 64]


def wrap(v: int, esize: int) -> int:
    """Two's-complement wrap of v to a signed esize-byte integer."""
    bits = 8 * esize
    v &= (1 << bits) - 1
    return v - (1 << bits) if v >> (bits - 1) else v


def _uvarint(v: int) -> bytes:
    out = bytearray()
    while True:
        b = v & 0x7F
        v >>= 7
        if v:
            out.append(b | 0x80)
        else:
            out.append(b)
            return bytes(out)


def _zigzag(v: int, esize: int) -> int:
    bits = 8 * esize
    return ((v << 1) ^ (v >> (bits - 1))) & ((1 << bits) - 1)


def _pack(vals, bw: int) -> bytes:
    acc = 0
    for i, v in enumerate(vals):
        acc |= v << (i * bw)
    return acc.to_bytes((len(vals) * bw + 7) // 8, "little")


def encode(values, block: int, minis: int, esize: int,
           junk_unused: bool = False) -> bytes:
    """DELTA_BINARY_PACKED stream of `values` (signed esize-byte ints):
    header <block size> <miniblocks per block> <total> <zigzag first>,
    then per block <zigzag min delta> <bit widths> <miniblocks>. Deltas
    wrap at the value width. The last miniblock that holds values is
    padded to its full size; miniblocks after it carry no data, and their
    bit-width bytes are 0, or junk (> 64 included) with `junk_unused`."""
    assert block % minis == 0 and (block // minis) % 32 == 0
    per = block // minis
    mask = (1 << (8 * esize)) - 1
    out = bytearray()
    out += _uvarint(block) + _uvarint(minis) + _uvarint(len(values))
    out += _uvarint(_zigzag(values[0], esize) if values else 0)
    deltas = [wrap(b - a, esize) for a, b in zip(values, values[1:])]
    for b0 in range(0, len(deltas), block):
        blk = deltas[b0:b0 + block]
        mn = min(blk)
        adj = [(d - mn) & mask for d in blk]
        out += _uvarint(_zigzag(mn, esize))
        widths = bytearray()
        body = bytearray()
        for m in range(minis):
            part = adj[m * per:(m + 1) * per]
            if not part:
                widths.append((0x41 + 61 * m) & 0xFF if junk_unused else 0)
                continue
            bw = max(part).bit_length()
            widths.append(bw)
            body += _pack(part + [0] * (per - len(part)), bw)
        out += widths + body
    return bytes(out)


def values_with_width(count: int, bw: int, esize: int, seed: int):
    """`count` values whose deltas are drawn uniformly below 2**bw and
    which are the wrapping cumulative sum of those deltas. Every run of 32
    deltas holds the smallest and the largest delta of that width, so each
    miniblock is packed at exactly `bw` bits."""
    rng = random.Random(seed)
    bits = 8 * esize
    assert bw <= bits
    deltas = [rng.randrange(1 << bw) for _ in range(max(count - 1, 0))]
    for i in range(0, len(deltas) - 1, 32):
        if bw == bits:  # full width: most negative and most positive delta
            deltas[i], deltas[i + 1] = 1 << (bits - 1), (1 << (bits - 1)) - 1
        else:
            deltas[i], deltas[i + 1] = 0, (1 << bw) - 1
    vals = []
    v = wrap(rng.randrange(1 << bits), esize)
    for i in range(count):
        vals.append(v)
        if i < len(deltas):
            v = wrap(v + deltas[i], esize)
    return vals


def _plain(count: int, esize: int, seed: int):
    rng = random.Random(seed)
    lim = 10 ** 6
    return [rng.randint(-lim, lim) for _ in range(count)]


def payload_set():
    """[(name, values, esize, bytes)] — the smallest shapes where the
    decode can go wrong: every count around the 32/64-value miniblock and
    wave edges, every layout, junk widths on unused miniblocks, every
    delta bit width that changes how many words a value straddles,
    negative min_delta, and full-range wrap."""
    out = []

    def add(name, vals, esize, block, minis, junk=False):
        vals = [wrap(v, esize) for v in vals]
        out.append((name, vals, esize,
                    encode(vals, block, minis, esize, junk)))

    seed = 0
    for esize in (8, 4):
        for count in COUNTS:
            for (block, minis) in LAYOUTS:
                for junk in (False, True):
                    seed += 1
                    add(f"n{count}-{block}x{minis}-j{int(junk)}-e{esize}",
                        _plain(count, esize, seed), esize, block, minis, junk)
        for bw in BIT_WIDTHS:
            if bw > 8 * esize:
                continue
            for (block, minis) in ((128, 4), (256, 4)):
                seed += 1
                add(f"bw{bw}-{block}x{minis}-e{esize}",
                    values_with_width(257, bw, esize, seed), esize, block,
                    minis)
        seed += 1
        rng = random.Random(seed)
        v, dec = 5000, []
        for _ in range(300):  # falling values: min_delta is negative
            dec.append(v)
            v -= rng.randint(0, 1000)
        add(f"negmin-e{esize}", dec, esize, 128, 4)
    add("extremes-e8", [INT64_MIN, INT64_MAX] * 100 + [0, -1, 1], 8, 256, 4)
    add("extremes-128x4-e8", [INT64_MIN, INT64_MAX] * 100 + [0, -1, 1], 8,
        128, 4, True)
    add("extremes-e4", [INT32_MIN, INT32_MAX] * 100 + [0, -1, 1], 4, 256, 4)
    add("extremes-128x4-e4", [INT32_MIN, INT32_MAX] * 100 + [0, -1, 1], 4,
        128, 4, True)
    return out


def multi_page_chunks():
    """[(name, esize, [(values, bytes)])]: several payloads as the pages
    of one chunk, a total-0 and a total-1 page between ordinary ones."""
    chunks = []
    for esize in (8, 4):
        pages = []
        specs = [(257, 128, 4, False), (0, 256, 4, False), (1000, 256, 4, True),
                 (1, 128, 1, True), (65, 512, 4, True), (1, 256, 4, False),
                 (0, 128, 4, True), (129, 128, 1, False)]
        for i, (count, block, minis, junk) in enumerate(specs):
            vals = values_with_width(count, (13 * i + 5) % (8 * esize + 1),
                                     esize, 1000 + i)
            pages.append((vals, encode(vals, block, minis, esize, junk)))
        chunks.append((f"pages-e{esize}", esize, pages))
    return chunks


# ------------------------------------------------------ pyarrow-written files
INT_COLS = ["i32", "i64", "d", "dec"]
N_ROWS = 5000


def delta_table():
    """5000 rows, ~15% NULL: INT32, INT64, date32, an integer-stored
    decimal and a string column. Written with row_group_size=3000 and
    write_batch_size=256, the last page of row group 0 (rows 2816..2999)
    holds only NULL strings and the last page of row group 1 (rows
    4792..4999) only empty strings."""
    import decimal

    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(17)
    n = N_ROWS
    null = lambda: rng.random(n) < 0.15  # noqa: E731
    words = ["", "a", "héllo wörld", "日本語のテキスト", "x" * 300, "delta",
             "length-byte-array", "🙂🙃"]
    s = [words[i] + str(i) * (i % 3) for i in rng.integers(0, len(words), n)]
    s[7], s[8], s[9] = "", "x" * 300, "日本語"
    smask = null()
    s = [None if m else v for v, m in zip(s, smask)]
    s[2816:3000] = [None] * 184
    s[4792:5000] = [""] * 208
    dec = [decimal.Decimal(int(v)).scaleb(-2)
           for v in rng.integers(-10 ** 8, 10 ** 8, n)]
    return pa.table({
        "i32": pa.array(rng.integers(-2 ** 31, 2 ** 31, n).astype(np.int32),
                        mask=null()),
        "i64": pa.array(np.cumsum(rng.integers(-50, 10 ** 6, n)), mask=null()),
        "d": pa.array(rng.integers(0, 20000, n).astype(np.int32),
                      mask=null()).cast(pa.date32()),
        "dec": pa.array(dec, pa.decimal128(9, 2), mask=null()),
        "s": pa.array(s, pa.string()),
    })


def write_delta_file(table, path: str, pv: str, codec: str) -> None:
    import pyarrow.parquet as pq

    enc = {c: "DELTA_BINARY_PACKED" for c in INT_COLS}
    enc["s"] = "DELTA_LENGTH_BYTE_ARRAY"
    pq.write_table(table, path, use_dictionary=False, compression=codec,
                   column_encoding=enc, data_page_version=pv,
                   store_decimal_as_integer=True, row_group_size=3000,
                   data_page_size=2048, write_batch_size=256)
