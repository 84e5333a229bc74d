"""Shared helper for the DELTA_BYTE_ARRAY tests (not collected): a
pure-Python encoder on top of delta_payloads.encode, and the payload set
both the CPU and the GPU tests decode.

pyarrow always writes the longest common prefix; the encoder here takes
explicit prefix lengths, so non-maximal prefixes, prefixes that cut a
UTF-8 character and a nonzero first prefix on a later page can be built."""
import random

import delta_payloads as dp

COUNTS = [0, 1, 2, 63, 64, 65, 257]


def max_prefixes(strings):
    """Longest common prefix with the previous string (0 for the first)."""
    out, prev = [], b""
    for s in strings:
        k = 0
        while k < min(len(s), len(prev)) and s[k] == prev[k]:
            k += 1
        out.append(k)
        prev = s
    return out


def encode_raw(prefix_lens, suffix_lens, suffix_bytes: bytes,
               block: int = 128, minis: int = 4) -> bytes:
    """A page from its three parts as given, sane or not."""
    return (dp.encode(list(prefix_lens), block, minis, 4)
            + dp.encode(list(suffix_lens), block, minis, 4) + suffix_bytes)


def encode(strings, prefixes=None, prev: bytes = b"", block: int = 128,
           minis: int = 4) -> bytes:
    """DELTA_BYTE_ARRAY page of `strings` (bytes): DELTA_BINARY_PACKED
    prefix lengths, DELTA_BINARY_PACKED suffix lengths, suffix bytes.
    `prefixes` defaults to the longest ones; any shorter prefix is valid
    too. `prev` is the value before the page, for pages whose first prefix
    is not 0 (old parquet-mr files)."""
    if prefixes is None:
        prefixes = max_prefixes([prev] + list(strings))[1:]
    last = prev
    for s, p in zip(strings, prefixes):
        assert p <= len(last) and s[:p] == last[:p], (s, p, last)
        last = s
    suffixes = [s[p:] for s, p in zip(strings, prefixes)]
    return encode_raw(prefixes, [len(x) for x in suffixes],
                      b"".join(suffixes), block, minis)


def sorted_strings(count: int, seed: int, stem: bytes = b"k/"):
    """Sorted, prefix-heavy keys with duplicates and a few empty strings."""
    rng = random.Random(seed)
    out = []
    for _ in range(count):
        r = rng.random()
        if r < 0.05:
            out.append(b"")
        elif r < 0.15 and out:
            out.append(out[-1])
        else:
            depth = rng.randint(1, 4)
            out.append(stem + b"/".join(
                b"%03d" % rng.randrange(12) for _ in range(depth)))
    return sorted(out)


def _tile_edge_strings(T: int):
    """Lengths T-1, T, T+1, 2T+5, with prefixes that end on, one before and
    one after a tile edge."""
    rng = random.Random(99)
    body = bytes(rng.randrange(256) for _ in range(2 * T + 5))
    strings, prefixes = [], []
    prev = b""
    for ln in (2 * T + 5, T - 1, T, T + 1, 2 * T + 5, T + 1, 2 * T + 5,
               T, 2 * T + 5, T - 1):
        for p in (T - 1, T, T + 1, 2 * T - 1, 2 * T, 2 * T + 1, 0):
            p = min(p, len(prev), ln)
            tail = bytes(rng.randrange(256) for _ in range(ln - p))
            s = prev[:p] + tail
            strings.append(s)
            prefixes.append(p)
            prev = s
    return strings, prefixes


def payload_set(T: int):
    """[(name, strings, [page bytes])] for tile size T; a payload with more
    than one page is one chunk."""
    out = []

    def add(name, strings, prefixes=None):
        out.append((name, list(strings), [encode(strings, prefixes)]))

    for n in COUNTS:
        add(f"sorted-n{n}", sorted_strings(n, 10 + n))
    rng = random.Random(5)
    rnd = [bytes(rng.randrange(256) for _ in range(rng.randrange(40)))
           for _ in range(130)]
    add("all-prefix-0", rnd, [0] * len(rnd))
    add("identical", [b"the same string every time"] * 200)
    add("identical-long", [b"x" * (T + 7)] * 70)
    inter = []
    for i, s in enumerate(sorted_strings(120, 3)):
        inter += [s, b""] if i % 3 else [s]
    add("empty-interleaved", inter)
    add("only-empty", [b""] * 100)
    strings, prefixes = _tile_edge_strings(T)
    add("tile-edges", strings, prefixes)
    # staircases: the prefix falls by one per row (walking forward, then
    # walking back), so a wave that starts on the stairs collects one byte
    # from each of many predecessors, across a tile edge
    base = bytes(rng.randrange(256) for _ in range(T + 90))
    stair, sp, prev = [base], [0], base
    for k in range(len(base) - 1, 0, -1):
        prev = prev[:k] + bytes([prev[k] ^ 0x55])
        stair.append(prev)
        sp.append(k)
    add("staircase-down", stair, sp)
    stair, sp, prev = [], [], b""
    for k in range(T + 90):
        prev = prev + bytes([rng.randrange(256)])
        stair.append(prev)
        sp.append(k)
    stair += [prev] * 5  # the whole staircase under one full prefix
    sp += [len(prev)] * 5
    add("staircase-up", stair, sp)
    srt = sorted_strings(200, 8)
    add("non-maximal", srt, [p // 2 for p in max_prefixes(srt)])
    utf = sorted(("日本語のテキスト%d" % (i % 17)).encode() +
                 ("é" * (i % 5)).encode() for i in range(150))
    add("utf8-cut", utf, [max(p - 1, 0) for p in max_prefixes(utf)])
    a = sorted_strings(100, 21)
    b = [s for s in sorted_strings(90, 22) if s]
    out.append(("two-pages-restart", a + b, [encode(a), encode(b)]))
    assert max_prefixes([a[-1], b[0]])[1] > 0
    out.append(("two-pages-carry", a + b, [encode(a), encode(b, prev=a[-1])]))
    return out


def chunk(pages):
    """(raw bytes, [(off, len, n_rows)]) of pages laid end to end; n_rows is
    read back from the page's own header total."""
    raw, descs = b"", []
    for pg in pages:
        descs.append((len(raw), len(pg), _total(pg)))
        raw += pg
    return raw, descs


def _total(page: bytes) -> int:
    pos, vals = 0, []
    for _ in range(3):
        v, shift = 0, 0
        while True:
            b = page[pos]
            pos += 1
            v |= (b & 0x7F) << shift
            shift += 7
            if not b & 0x80:
                break
        vals.append(v)
    return vals[2]


# ------------------------------------------------------ pyarrow-written files
N_ROWS = 5000


def dba_table():
    """5000 rows of one string column "s", ~15% NULL, sorted so that
    prefixes are long. Written with row_group_size=3000 and
    write_batch_size=256, the last page of row group 0 (rows 2816..2999)
    holds only NULLs and the last page of row group 1 (rows 4792..4999) only
    empty strings."""
    import numpy as np
    import pyarrow as pa

    rng = np.random.default_rng(29)
    n = N_ROWS
    words = ["", "a", "héllo wörld", "日本語のテキスト", "x" * 300,
             "https://example.org/path/", "delta-byte-array", "🙂🙃"]
    # a 12-character random tail keeps every 256-row batch above the
    # 2048-byte page size, so a page ends at each batch
    tails = rng.integers(0, 1 << 48, n)
    s = sorted(words[i] + str(j % 97) * (j % 3) + "/%012x" % tails[j]
               for j, i in enumerate(rng.integers(0, len(words), n)))
    mask = rng.random(n) < 0.15
    s = [None if m else v for v, m in zip(s, mask)]
    s[2816:3000] = [None] * 184
    s[4792:5000] = [""] * 208
    return pa.table({"s": pa.array(s, pa.string())})


def write_dba_file(table, path: str, pv: str, codec: str) -> None:
    import pyarrow.parquet as pq

    pq.write_table(table, path, use_dictionary=False, compression=codec,
                   column_encoding={"s": "DELTA_BYTE_ARRAY"},
                   data_page_version=pv, row_group_size=3000,
                   data_page_size=2048, write_batch_size=256)
