"""Fixtures for the gzip tests, made with the standard library's zlib/gzip: a
BGZF writer, the BGZF end-of-file member, a bit writer for raw deflate blocks
assembled by hand, and the decode and error cases the CPU and GPU tests share.
A helper, not a test."""
import functools
import gzip
import os
import random
import struct
import zlib

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN_FQ = os.path.join(HERE, "golden", "fq", "input.fasta")

# the 28-byte empty member bgzip writes at the end of a file
BGZF_EOF = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")

# reasons (include/kgx.h)
BLOCK_TYPE, STORED_LEN, OVERSUBSCRIBED, INCOMPLETE, REPEAT_FIRST, REPEAT_OVERRUN, NO_EOB, BAD_SYMBOL = range(1, 9)
TOO_MANY_CODES, BAD_CODE, DISTANCE, INPUT_END, OUTPUT_FULL, OUTPUT_SHORT, CRC = range(9, 16)
GZ_NOT_GZIP, GZ_METHOD, GZ_RESERVED_FLAG, GZ_TRUNCATED, GZ_BSIZE, GZ_BLOCKED_ISIZE, GZ_HEADER_CRC = range(32, 39)


def raw_deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
    return c.compress(data) + c.flush()


def bgzf_member(raw, data=None, crc=None, isize=None, bsize=None):
    """One blocked member around the raw deflate bytes `raw`; crc and isize
    default to those of `data`, bsize to the member's size - 1."""
    crc = zlib.crc32(data) if crc is None else crc
    isize = len(data) if isize is None else isize
    bsize = len(raw) + 25 if bsize is None else bsize
    head = struct.pack("<4BI2BH2BHH", 0x1F, 0x8B, 8, 4, 0, 0, 0xFF, 6, 0x42, 0x43, 2, bsize)
    return head + raw + struct.pack("<II", crc & 0xFFFFFFFF, isize)


def bgzf(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, chunk=65280, eof=True):
    out = []
    for at in range(0, len(data), chunk):
        part = data[at:at + chunk]
        out.append(bgzf_member(raw_deflate(part, level, strategy), part))
    if eof:
        out.append(BGZF_EOF)
    return b"".join(out)


class BitWriter:
    """Raw deflate assembled by hand: bits least significant first, Huffman
    codes most significant bit first (RFC 1951 3.1.1)."""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):
        self.acc |= (value & ((1 << count) - 1)) << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8
        return self

    def code(self, value, count):
        for i in range(count - 1, -1, -1):
            self.bits((value >> i) & 1, 1)
        return self

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)
        return self

    def stored(self, data, last, nlen=None):
        self.bits(last, 1).bits(0, 2).align()
        self.bits(len(data), 16).bits((len(data) ^ 0xFFFF) if nlen is None else nlen, 16)
        self.out += data
        return self

    def fixed_literal(self, v):
        return self.code(0x30 + v, 8) if v < 144 else self.code(0x190 + v - 144, 9)

    def fixed_symbol(self, s):
        """literal/length symbol 256..287 of the fixed code"""
        return self.code(s - 256, 7) if s < 280 else self.code(0xC0 + s - 280, 8)

    def bytes(self):
        return bytes(self.align().out)


_LBASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227,
          258]
_LEXT = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
_DBASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097,
          6145, 8193, 12289, 16385, 24577]
_DEXT = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]


def fixed_match(w, length, dist):
    """one match in a fixed-Huffman block"""
    ls = max(i for i in range(29) if _LBASE[i] <= length)
    if length == 258:
        ls = 28
    w.fixed_symbol(257 + ls).bits(length - _LBASE[ls], _LEXT[ls])
    ds = max(i for i in range(30) if _DBASE[i] <= dist)
    w.code(ds, 5).bits(dist - _DBASE[ds], _DEXT[ds])
    return w


@functools.lru_cache(maxsize=None)
def golden():
    with open(GOLDEN_FQ, "rb") as f:
        return f.read()


def fibonacci_text():
    """22 letters with Fibonacci frequencies (46,367 bytes), shuffled: zlib's
    Z_HUFFMAN_ONLY gives 15-bit literal codes (zlib cuts the text into two blocks,
    so the depth depends on which rare letters fall into the first: this shuffle
    reaches 15, as the tests assert through the statistics)"""
    fib, parts = [1, 1], []
    while len(fib) < 22:
        fib.append(fib[-1] + fib[-2])
    for i, f in enumerate(fib):
        parts.append(bytes([ord("a") + i]) * f)
    data = bytearray(b"".join(parts))
    random.Random(1).shuffle(data)
    return bytes(data)


def window_member():
    """one stored block of 32,768 bytes, then a fixed block with one match of
    length 258 at distance 32,768"""
    first = random.Random(11).randbytes(32768)
    w = BitWriter().stored(first, 0)
    w.bits(1, 1).bits(1, 2)
    fixed_match(w, 258, 32768).fixed_symbol(256)
    data = first + first[:258]
    return bgzf_member(w.bytes(), data), data


def flush_member(mode):
    a, b = golden()[:9000], golden()[9000:15000]
    c = zlib.compressobj(6, zlib.DEFLATED, -15)
    raw = c.compress(a) + c.flush(mode) + c.compress(b) + c.flush()
    return bgzf_member(raw, a + b), a + b


def literal_then_match(dist):
    """fixed block: `dist` literals directly followed by a match of 40 bytes at
    that distance"""
    lit = b"ACGT"[:dist]
    w = BitWriter().bits(1, 1).bits(1, 2)
    for v in lit:
        w.fixed_literal(v)
    fixed_match(w, 40, dist).fixed_symbol(256)
    data = (lit * 44)[:dist + 40]
    return bgzf_member(w.bytes(), data), data


@functools.lru_cache(maxsize=None)
def decode_cases():
    """name -> (gzip bytes, the text, what the statistics must show).  The
    blocked ones hold only blocked members."""
    g = golden()
    cases = {}
    for name, level, strategy, key in (("l0", 0, zlib.Z_DEFAULT_STRATEGY, "stored_blocks"),
                                       ("l1", 1, zlib.Z_DEFAULT_STRATEGY, "dynamic_blocks"),
                                       ("l6", 6, zlib.Z_DEFAULT_STRATEGY, "dynamic_blocks"),
                                       ("l9", 9, zlib.Z_DEFAULT_STRATEGY, "dynamic_blocks"),
                                       ("fixed", 6, zlib.Z_FIXED, "fixed_blocks")):
        for chunk in (65280, 1000, 37):
            for eof in (True, False):
                n = -(-len(g) // chunk)
                # a small chunk may compress best as another block type: the type is pinned where
                # zlib's choice is known, the whole text in one member (and level 0 is always stored)
                want = {"members": n + (1 if eof else 0)}
                if chunk == 65280 or level == 0:
                    want[key] = ("ge", n)
                cases[f"golden_{name}_c{chunk}_{'eof' if eof else 'noeof'}"] = (
                    bgzf(g, level, strategy, chunk, eof), g, want)
    cases["empty"] = (BGZF_EOF, b"", {"members": 1, "fixed_blocks": ("ge", 1)})
    cases["isize0_between"] = (bgzf(g[:500], eof=False) + BGZF_EOF + bgzf(g[500:900], eof=False), g[:900],
                               {"members": 3})
    run = b"I" * 60000
    cases["overlap_d1"] = (bgzf(run, eof=False), run, {"overlap": 1, "max_length": 258, "max_distance": 1})
    p3 = b"ACG" * 3000
    cases["overlap_period3"] = (bgzf(p3, eof=False), p3, {"overlap": 1, "max_distance": 3})
    for d in (1, 2, 3, 4):
        m, data = literal_then_match(d)
        cases[f"literal_match_d{d}"] = (m, data, {"overlap": 1, "max_distance": d, "max_length": 40,
                                                   "fixed_blocks": 1})
    m, data = window_member()
    cases["window_32768"] = (m, data, {"max_distance": 32768, "max_length": 258, "stored_blocks": 1,
                                       "fixed_blocks": 1})
    fibt = fibonacci_text()
    cases["codelen15"] = (bgzf(fibt, 6, zlib.Z_HUFFMAN_ONLY, eof=False), fibt, {"max_code_len": 15})
    one = b"A" * 3000
    cases["one_symbol"] = (bgzf(one, 6, zlib.Z_HUFFMAN_ONLY, eof=False), one, {"dynamic_blocks": ("ge", 1)})
    for nm, mode in (("sync_flush", zlib.Z_SYNC_FLUSH), ("full_flush", zlib.Z_FULL_FLUSH)):
        m, data = flush_member(mode)
        cases[nm] = (m, data, {"dynamic_blocks": 2, "stored_blocks": 1})
    noise = random.Random(3).randbytes(65280)
    stored = bgzf(noise, 0, eof=False)
    assert len(stored) == 65316
    cases["stored_65280"] = (stored, noise, {"stored_blocks": ("ge", 1), "members": 1})
    for n in (1, 3, 64, 65, 257):
        data = g[:n * 61]
        cases[f"members_{n}"] = (bgzf(data, chunk=61, eof=False), data, {"members": n})
    return cases


def plain_cases():
    """name -> (gzip bytes, the text): bodies with plain (non-blocked) members"""
    g = golden()
    named = bytearray(gzip.compress(g[:3000]))
    # FLG = FHCRC | FNAME | FCOMMENT, then the name, the comment and the header's CRC16
    head = bytes(named[:3]) + bytes([2 | 8 | 16]) + bytes(named[4:10]) + b"reads.fastq\0a comment\0"
    head += struct.pack("<H", zlib.crc32(head) & 0xFFFF)
    return {
        "plain": (gzip.compress(g), g),
        "plain_two": (gzip.compress(g[:7000]) + gzip.compress(g[7000:]), g),
        "plain_then_blocked": (gzip.compress(g[:7000]) + bgzf(g[7000:], chunk=1000), g),
        "blocked_then_plain": (bgzf(g[:7000], chunk=1000, eof=False) + gzip.compress(g[7000:]), g),
        "plain_named": (head + bytes(named[10:]), g[:3000]),
        "plain_trailing": (gzip.compress(g[:3000]) + b"\0\0not gzip at all", g[:3000]),
    }


def _dynamic_header(w, hlit, hdist, cl_lens):
    """BTYPE 2 header with the 19 code-length code lengths in cl_lens (by symbol)"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w.bits(1, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(19 - 4, 4)
    for s in order:
        w.bits(cl_lens.get(s, 0), 3)
    return w


@functools.lru_cache(maxsize=None)
def error_cases():
    """name -> (one blocked member, the reason it must fail with).  Every one
    fails in the decoder or in the trailer checks, not in the framing."""
    g = golden()[:200]
    good_raw = raw_deflate(g)
    cases = {}
    cases["block_type_3"] = (bgzf_member(BitWriter().bits(1, 1).bits(3, 2).bytes(), b""), BLOCK_TYPE)
    cases["len_nlen"] = (bgzf_member(BitWriter().stored(b"abcd", 1, nlen=0x1234).bytes(), b"abcd"), STORED_LEN)
    # code-length code: three codes of length 1
    w = _dynamic_header(BitWriter(), 257, 1, {0: 1, 1: 1, 2: 1})
    cases["oversubscribed"] = (bgzf_member(w.bytes(), b""), OVERSUBSCRIBED)
    # a match at distance 4 after one literal
    w = BitWriter().bits(1, 1).bits(1, 2).fixed_literal(65)
    fixed_match(w, 10, 4).fixed_symbol(256)
    cases["distance_before_start"] = (bgzf_member(w.bytes(), b"A" * 11), DISTANCE)
    cases["input_ends_mid_symbol"] = (bgzf_member(good_raw[:len(good_raw) // 2], g), INPUT_END)
    cases["output_one_longer"] = (bgzf_member(raw_deflate(g + b"x"), g), OUTPUT_FULL)
    cases["output_one_shorter"] = (bgzf_member(raw_deflate(g[:-1]), g), OUTPUT_SHORT)
    cases["crc_bit"] = (bgzf_member(good_raw, g, crc=zlib.crc32(g) ^ 0x400), CRC)
    # code 16 first
    w = _dynamic_header(BitWriter(), 257, 1, {16: 1, 0: 1})
    w.code(1, 1)  # symbols in code order: 0 -> '0', 16 -> '1'
    cases["repeat_first"] = (bgzf_member(w.bytes(), b""), REPEAT_FIRST)
    # fixed block with length symbol 286
    w = BitWriter().bits(1, 1).bits(1, 2).fixed_literal(65).fixed_symbol(286)
    cases["length_symbol_286"] = (bgzf_member(w.bytes(), b"A"), BAD_SYMBOL)
    # fixed block with distance symbol 30
    w = BitWriter().bits(1, 1).bits(1, 2).fixed_literal(65).fixed_symbol(257).code(30, 5)
    cases["distance_symbol_30"] = (bgzf_member(w.bytes(), b"AAAA"), BAD_SYMBOL)
    return cases


def framing_error_cases():
    """name -> (body, finished, reason): refused by the framing walk"""
    g = golden()[:200]
    good = bgzf_member(raw_deflate(g), g)
    return {
        "bsize_past_input": (bgzf_member(raw_deflate(g), g, bsize=len(good) + 40), GZ_TRUNCATED),
        "isize_65537": (bgzf_member(raw_deflate(g), g, isize=65537), GZ_BLOCKED_ISIZE),
        "bsize_too_small": (bgzf_member(raw_deflate(g), g, bsize=20), GZ_BSIZE),
        "reserved_flag": (good[:3] + bytes([good[3] | 0x20]) + good[4:], GZ_RESERVED_FLAG),
    }


def member_200():
    """a blocked member of exactly 200 bytes, for the truncation sweep"""
    rng = random.Random(5)
    for n in range(300, 1200):
        data = bytes(rng.choice(b"ACGTN") for _ in range(n))
        m = bgzf_member(raw_deflate(data), data)
        if len(m) == 200:
            return m, data
    raise AssertionError("no 200-byte member found")
