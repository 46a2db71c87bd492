"""Fixtures for the gzip tests, made with the standard library's zlib/gzip: a
BGZF writer, the BGZF end-of-file member, a bit writer for raw deflate blocks
assembled by hand, and the decode and error cases the CPU and GPU tests share.

Hand-assembled with the bit writer: dynamic blocks from code lengths
(canonical_codes, dynamic_block), so that every decoder reason 1..15 has a
named error case (ZLIB_MESSAGES: what zlib says to the same stream) and the
two legal incomplete distance sets (none, one code of length 1) have decode
cases of their own; the match geometry grid (geometry_members: literals
pending x distance x length around the 64-lane passes), the stored geometry
(stored_members) and the output sizes around the CRC slices (size_members),
each one body of decode_cases().  mutated_corpus(): seeded raw deflate
streams over every zlib strategy, small windows and memLevels, most of them
bit-flipped or cut, each with zlib's verdict (zlib_inflate: libz through
ctypes, for the bytes zlib produced before an error, which the zlib module
throws away).  gzip_header_variants(): single members with every optional
header field, for the framing differential against zlib.

A helper, not a test."""
import ctypes
import ctypes.util
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
    # the two legal incomplete distance sets, kept legal: no distance code and no match; one 1-bit
    # distance code and its bit
    cases["no_distance_code"] = (bgzf_member(incomplete_distance_block([0], [("eob",)]), b"AAA"), b"AAA",
                                 {"dynamic_blocks": 1, "matches": 0, "max_code_len": 2, "max_distance": 0})
    cases["single_distance_code"] = (
        bgzf_member(incomplete_distance_block([1], [("len",), ("bit", 0), ("eob",)]), b"AAAAAA"), b"AAAAAA",
        {"dynamic_blocks": 1, "matches": 1, "max_code_len": 2, "max_distance": 1, "max_length": 3, "overlap": 1})
    # literals alone: what the kernel's literal registers hold (63, 0 after a flush of 64, 1) when the
    # last end of block comes
    for n in (63, 64, 65):
        data = bytes(literal_value(i) for i in range(n))
        w = BitWriter().bits(1, 1).bits(1, 2)
        for v in data:
            w.fixed_literal(v)
        cases[f"literals_only_{n}"] = (bgzf_member(w.fixed_symbol(256).bytes(), data), data,
                                       {"fixed_blocks": 1, "matches": 0, "members": 1})
    geo = geometry_members()
    cases["geometry"] = (b"".join(m for *_, m, _ in geo), b"".join(t for *_, t in geo),
                         {"members": len(geo), "fixed_blocks": len(geo), "matches": len(geo), "max_distance": 259,
                          "max_length": 258, "overlap": 1, "dynamic_blocks": 0, "stored_blocks": 0})
    sto = stored_members()
    cases["stored_geometry"] = (b"".join(m for *_, m, _ in sto), b"".join(t for *_, t in sto),
                                {"members": len(sto), "fixed_blocks": 2 * len(sto), "stored_blocks": len(sto),
                                 "matches": len(sto), "max_distance": 4095 + 65, "max_length": 70, "overlap": 1})
    siz = size_members()
    cases["sizes"] = (b"".join(m for _, m, _ in siz), b"".join(t for *_, t in siz), {"members": len(siz)})
    return cases


# the decode cases this list names are the ones made of members with per-member expectations
MEMBER_SETS = ("geometry", "stored_geometry", "sizes")


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


def _dynamic_header(w, hlit, hdist, cl_lens, last=1):
    """BTYPE 2 header with the 19 code-length code lengths in cl_lens (by symbol)"""
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    w.bits(last, 1).bits(2, 2).bits(hlit - 257, 5).bits(hdist - 1, 5).bits(19 - 4, 4)
    for s in order:
        w.bits(cl_lens.get(s, 0), 3)
    return w


def canonical_codes(lens):
    """code lengths by symbol -> {symbol: (code, length)}, the canonical code
    of RFC 1951 3.2.2 (also for an incomplete set)"""
    count = [0] * 16
    for n in lens:
        count[n] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for n in range(1, 16):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    codes = {}
    for s, n in enumerate(lens):
        if n:
            codes[s] = (nxt[n], n)
            nxt[n] += 1
    return codes


def dynamic_block(w, last, ll_lens, d_lens):
    """a BTYPE 2 header for the literal/length lengths ll_lens (257..286 of
    them) and the distance lengths d_lens (1..30), every length sent as itself
    through a code-length code of sixteen 4-bit codes; returns the two codes"""
    _dynamic_header(w, len(ll_lens), len(d_lens), {s: 4 for s in range(16)}, last)
    for n in list(ll_lens) + list(d_lens):
        w.code(n, 4)  # sixteen codes of length 4: symbol n is code n
    return canonical_codes(ll_lens), canonical_codes(d_lens)


def _ll_lens(lengths, n=257):
    """a literal/length length list from {symbol: length}"""
    lens = [0] * max(n, max(lengths) + 1)
    for s, v in lengths.items():
        lens[s] = v
    return lens


# a complete literal/length set: 'A' in 1 bit, end of block and length symbol 257 (3 bytes) in 2
_A_EOB_L3 = {65: 1, 256: 2, 257: 2}


def incomplete_distance_block(d_lens, tail, pad=b""):
    """a final dynamic block over _A_EOB_L3 and the distance lengths d_lens:
    "AAA", then `tail`: a list of ("eob",), ("len",) and ("bit", v)"""
    w = BitWriter()
    ll, _ = dynamic_block(w, 1, _ll_lens(_A_EOB_L3, 258), d_lens)
    for _ in range(3):
        w.code(*ll[65])
    for t in tail:
        if t[0] == "eob":
            w.code(*ll[256])
        elif t[0] == "len":
            w.code(*ll[257])
        else:
            w.bits(t[1], 1)
    return w.bytes() + pad


def literal_value(i):
    """the i-th literal of the geometry members: a multiplicative hash, so no
    two places a wrong source index could point to hold equal runs"""
    return ((i * 2654435761 & 0xFFFFFFFF) >> 13) & 0xFF


GEOMETRY_P = (0, 1, 62, 63, 64, 65, 127, 128, 129)
GEOMETRY_DIST = (1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 66, 127, 128, 129, 257, 258, 259)
GEOMETRY_LEN = (3, 4, 63, 64, 65, 128, 129, 257, 258)


def _match_text(text, length, dist):
    for _ in range(length):
        text.append(text[-dist])


@functools.lru_cache(maxsize=None)
def geometry_members():
    """[(P, dist, len, member, text)]: fixed blocks of max(P, dist) literals,
    one match (len, dist), one literal, end of block: every branch of the
    kernel's match() (dist >= len, dist == 1, i % dist) with the match and the
    literals pending in front of it on both sides of every 64-lane pass"""
    out = []
    for p in GEOMETRY_P:
        for dist in GEOMETRY_DIST:
            for length in GEOMETRY_LEN:
                n = max(p, dist)
                text = bytearray(literal_value(i) for i in range(n))
                w = BitWriter().bits(1, 1).bits(1, 2)
                for v in text:
                    w.fixed_literal(v)
                fixed_match(w, length, dist)
                _match_text(text, length, dist)
                text.append(literal_value(n + length))
                w.fixed_literal(text[-1]).fixed_symbol(256)
                out.append((p, dist, length, bgzf_member(w.bytes(), bytes(text)), bytes(text)))
    return out


STORED_P = (1, 62, 63, 64, 65, 129)
STORED_S = (0, 1, 63, 64, 65, 4095)


@functools.lru_cache(maxsize=None)
def stored_members():
    """[(P, S, dist, len, member, text)]: a fixed block of P literals (left
    pending in the kernel's registers at its end of block), a stored block of
    S bytes, and a final fixed block whose match starts in the literals and
    runs across the stored bytes"""
    out = []
    for p in STORED_P:
        for s in STORED_S:
            text = bytearray(literal_value(i) for i in range(p))
            w = BitWriter().bits(0, 1).bits(1, 2)
            for v in text:
                w.fixed_literal(v)
            w.fixed_symbol(256)
            body = bytes(literal_value(1000 + i) for i in range(s))
            w.stored(body, 0)
            text += body
            dist, length = s + (p + 1) // 2, 70
            w.bits(1, 1).bits(1, 2)
            fixed_match(w, length, dist)
            _match_text(text, length, dist)
            w.fixed_symbol(256)
            out.append((p, s, dist, length, bgzf_member(w.bytes(), bytes(text)), bytes(text)))
    return out


SIZES = (1, 2, 63, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65535, 65536)


@functools.lru_cache(maxsize=None)
def size_members():
    """[(ISIZE, member, text)]: single members around the 64 CRC slices and up
    to the largest blocked member; random bytes stored and FASTQ text
    compressed by turns (the two largest are text: stored they would not fit
    BSIZE)"""
    out = []
    for i, n in enumerate(SIZES):
        if i % 2 and n < 65000:
            text = random.Random(n).randbytes(n)
            out.append((n, bgzf_member(raw_deflate(text, 0), text), text))
        else:
            text = (golden() * 4)[:n]
            out.append((n, bgzf_member(raw_deflate(text), text), text))
    return out


# ---- zlib's verdict on a raw deflate stream ---------------------------------------


class _ZStream(ctypes.Structure):
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_uint), ("total_in", ctypes.c_ulong),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_uint), ("total_out", ctypes.c_ulong),
                ("msg", ctypes.c_char_p), ("state", ctypes.c_void_p), ("zalloc", ctypes.c_void_p),
                ("zfree", ctypes.c_void_p), ("opaque", ctypes.c_void_p), ("data_type", ctypes.c_int),
                ("adler", ctypes.c_ulong), ("reserved", ctypes.c_ulong)]


@functools.lru_cache(maxsize=None)
def _libz():
    z = ctypes.CDLL(ctypes.util.find_library("z") or "libz.so.1")
    z.zlibVersion.restype = ctypes.c_char_p
    return z


ZLIB_ROOM = 1 << 20


def zlib_inflate(raw, room=ZLIB_ROOM):
    """libz's inflate (the library under the zlib module) over one raw deflate
    stream: (accepted, the bytes it produced -- on a failure those before it,
    which zlib.decompressobj discards --, input bytes consumed, its message).
    The accept verdict, the text and the input consumed are checked against
    zlib.decompressobj(-15) here, so that module stays the reference."""
    z, s = _libz(), _ZStream()
    src, dst = ctypes.create_string_buffer(bytes(raw), max(len(raw), 1)), ctypes.create_string_buffer(room)
    assert z.inflateInit2_(ctypes.byref(s), -15, z.zlibVersion(), ctypes.sizeof(s)) == 0
    s.next_in, s.avail_in = ctypes.addressof(src), len(raw)
    s.next_out, s.avail_out = ctypes.addressof(dst), room
    rc = z.inflate(ctypes.byref(s), 2)  # Z_SYNC_FLUSH: as far as the input goes
    out, used, msg = dst.raw[:s.total_out], int(s.total_in), (s.msg or b"").decode()
    z.inflateEnd(ctypes.byref(s))
    if s.total_out == room and rc != 1:
        raise OverflowError("zlib_inflate: the room is too small for this stream")
    d = zlib.decompressobj(-15)
    try:
        text = d.decompress(bytes(raw))
        module = (True, text, len(raw) - len(d.unused_data)) if d.eof else (False, None, None)
    except zlib.error as e:
        module = (False, None, None)
        assert rc == -3 and msg and msg in str(e), (rc, msg, str(e))
    assert module[0] == (rc == 1), (module[0], rc)
    if module[0]:
        assert (module[1], module[2]) == (out, used)
    return rc == 1, out, used, msg


CORPUS_SEED, CORPUS_N = 1951, 3000
CORPUS_REJECT_ROOM = 4096  # the room a stream zlib rejects is decoded into


def mutated_corpus(seed, n):
    """n raw deflate streams and zlib's verdict on each:
    [(stream, accepted, zlib's output, input bytes zlib consumed)].  Data of
    four kinds (FASTQ text, random bytes, periodic, one byte repeated), 0 to
    6,000 bytes; every level, all five strategies, windows of 512, 4 Ki and
    32 Ki bytes, memLevel 1, 8 and 9 (1: many short dynamic blocks).  A quarter
    of the streams are as zlib wrote them; the others have 1 to 5 bits
    flipped, for half of them within the first 48 bytes, where the block
    headers are, and a third of the flipped ones are then cut short."""
    rng = random.Random(seed)
    g = golden()
    strategies = (zlib.Z_DEFAULT_STRATEGY, zlib.Z_FILTERED, zlib.Z_HUFFMAN_ONLY, zlib.Z_RLE, zlib.Z_FIXED)
    out = []
    while len(out) < n:
        size = rng.choice((0, 1, 2, 3, rng.randrange(64), rng.randrange(700), rng.randrange(6001),
                           rng.randrange(6001)))
        kind = rng.randrange(4)
        if kind == 0:
            at = rng.randrange(len(g) - size)
            data = g[at:at + size]
        elif kind == 1:
            data = rng.randbytes(size)
        elif kind == 2:
            period = rng.randbytes(rng.choice((1, 2, 3, 5, 63, 64, 65, 130, 300)))
            data = (period * (size // len(period) + 1))[:size]
        else:
            data = bytes([rng.randrange(256)]) * size
        c = zlib.compressobj(rng.randrange(10), zlib.DEFLATED, rng.choice((-9, -12, -15)), rng.choice((1, 8, 9)),
                             rng.choice(strategies))
        raw = bytearray(c.compress(data) + c.flush())
        if rng.randrange(4):
            head = rng.randrange(2)
            for _ in range(rng.randrange(1, 6)):
                bit = rng.randrange(8 * (min(len(raw), 48) if head else len(raw)))
                raw[bit >> 3] ^= 1 << (bit & 7)
            if rng.randrange(3) == 0:
                del raw[rng.randrange(len(raw)):]
        try:
            ok, text, used, _ = zlib_inflate(bytes(raw))
        except OverflowError:
            continue
        if len(text) > 65536:  # more than a blocked member's slot may hold
            continue
        out.append((bytes(raw), ok, text, used))
    return out


@functools.lru_cache(maxsize=None)
def corpus():
    """the corpus the native, host-ABI and GPU tests share: the same bytes and
    the same rooms (corpus_room) in all of them"""
    return mutated_corpus(CORPUS_SEED, CORPUS_N)


def corpus_room(ok, text):
    return len(text) if ok else CORPUS_REJECT_ROOM


def corpus_verdicts_are_balanced(c):
    """at least a quarter accepted and a quarter rejected, by zlib alone"""
    ok = sum(1 for _, a, _, _ in c if a)
    return 4 * ok >= len(c) and 4 * (len(c) - ok) >= len(c), ok


# ---- gzip header variants ------------------------------------------------------------


def gzip_member(data, flg=0, extra=None, name=None, comment=None, hcrc=None, mtime=0, xfl=0, os_=255, level=6):
    """one gzip member with the optional header fields given (RFC 1952 2.3);
    name and comment as given, zero byte included or not; hcrc: None = none,
    True = right, an int = XORed onto the right one"""
    flg |= (4 if extra is not None else 0) | (8 if name is not None else 0) | (16 if comment is not None else 0) | \
        (2 if hcrc is not None else 0)
    head = struct.pack("<4BI2B", 0x1F, 0x8B, 8, flg, mtime, xfl, os_)
    if extra is not None:
        head += struct.pack("<H", len(extra)) + extra
    head += (name or b"") + (comment or b"")
    if hcrc is not None:
        head += struct.pack("<H", (zlib.crc32(head) & 0xFFFF) ^ (0 if hcrc is True else hcrc))
    return head + raw_deflate(data, level) + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def gzip_header_variants():
    """name -> (body, blocked): single members; `blocked` says whether the
    framing walk must take the member as a blocked one"""
    g = golden()[:3000]
    raw = raw_deflate(g)

    def bc(front=b"", behind=b"", fhcrc=False):  # the BC subfield's BSIZE covers the whole member
        n = 10 + 2 + len(front) + 6 + len(behind) + (2 if fhcrc else 0) + len(raw) + 8
        return front + b"BC" + struct.pack("<HH", 2, n - 1) + behind

    v = {
        "extra_foreign_then_bc": (gzip_member(g, extra=bc(b"XY" + struct.pack("<H", 5) + b"hello")), True),
        "extra_bc_then_foreign": (gzip_member(g, extra=bc(behind=b"Zz" + struct.pack("<H", 0))), True),
        "extra_without_bc": (gzip_member(g, extra=b"XY" + struct.pack("<H", 3) + b"abc"), False),
        "extra_bc_of_length_3": (gzip_member(g, extra=b"BC" + struct.pack("<H", 3) + b"abc"), False),
        "extra_empty": (gzip_member(g, extra=b""), False),
        "fname_unterminated": (gzip_member(g, name=b"reads.fastq")[:21], False),
        "fcomment_unterminated": (gzip_member(g, name=b"reads.fastq\0", comment=b"no end")[:28], False),
        "fname_and_fcomment": (gzip_member(g, name=b"reads.fastq\0", comment=b"a comment\0"), False),
        "fhcrc_right": (gzip_member(g, hcrc=True), False),
        "fhcrc_wrong_low_byte": (gzip_member(g, hcrc=0x0001), False),
        "fhcrc_wrong_high_byte": (gzip_member(g, hcrc=0x8000), False),
        "fhcrc_after_all_fields": (gzip_member(g, flg=1, extra=b"XY" + struct.pack("<H", 1) + b"q", name=b"n\0",
                                               comment=b"c\0", hcrc=True, mtime=0x12345678, xfl=2, os_=3), False),
        "fhcrc_blocked": (gzip_member(g, extra=bc(fhcrc=True), hcrc=True), True),
        "ftext": (gzip_member(g, flg=1), False),
        "mtime_xfl_os": (gzip_member(g, mtime=0xFFFFFFFF, xfl=4, os_=0), False),
        "xfl_os_other": (gzip_member(g, mtime=1, xfl=0xFF, os_=13), False),
    }
    return v


def zlib_gunzip(body):
    """zlib's reading of one gzip member: the text, or None when it refuses it
    or finds it incomplete"""
    d = zlib.decompressobj(31)
    try:
        text = d.decompress(body)
    except zlib.error:
        return None
    return text if d.eof else None


# what zlib says to the raw deflate data of an error case (None: zlib takes the
# stream; the member fails in its trailer or at the end of its input)
ZLIB_MESSAGES = {
    "block_type_3": "invalid block type",
    "len_nlen": "invalid stored block lengths",
    "oversubscribed": "invalid code lengths set",
    "distance_before_start": "invalid distance too far back",
    "input_ends_mid_symbol": None,
    "output_one_longer": None,
    "output_one_shorter": None,
    "crc_bit": None,
    "repeat_first": "invalid bit length repeat",
    "length_symbol_286": "invalid literal/length code",
    "distance_symbol_30": "invalid distance code",
    "hlit_287": "too many length or distance symbols",
    "hdist_31": "too many length or distance symbols",
    "repeat_overrun_by_one": "invalid bit length repeat",
    "repeat_overrun_two_full_runs": "invalid bit length repeat",
    "no_end_of_block_code": "invalid code -- missing end-of-block",
    "incomplete_code_length_code": "invalid code lengths set",
    "incomplete_literal_set": "invalid literal/lengths set",
    "incomplete_distance_set": "invalid distances set",
    "length_with_no_distance_code": "invalid distance code",
    "other_bit_of_single_distance_code": "invalid distance code",
    "bad_distance_bit_at_the_end": "invalid distance code",
    "hand_output_longer": None,
    "hand_output_shorter": None,
    "hand_crc": None,
    "literals_63_then_distance": "invalid distance too far back",
    "literals_64_then_distance": "invalid distance too far back",
    "literals_65_then_distance": "invalid distance too far back",
}

# every hand-made stream is followed by this much padding, so that its reason
# does not depend on where the input ends
PAD = b"\0\0\0\0"


@functools.lru_cache(maxsize=None)
def error_cases():
    """name -> (one blocked member, the reason it must fail with).  Every one
    fails in the decoder or in the trailer checks, not in the framing.  Every
    reason 1..15 has at least one member assembled by hand with BitWriter."""
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

    def hand(name, w, reason, text=b"", **kw):
        raw = w if isinstance(w, bytes) else w.bytes() + PAD
        cases[name] = (bgzf_member(raw, text, **kw), reason)

    # 9: HLIT = 287 (HDIST legal), HDIST = 31 (HLIT legal)
    hand("hlit_287", _dynamic_header(BitWriter(), 287, 1, {0: 1, 1: 1}), TOO_MANY_CODES)
    hand("hdist_31", _dynamic_header(BitWriter(), 257, 31, {0: 1, 1: 1}), TOO_MANY_CODES)
    # 6: HLIT + HDIST = 258 lengths; code 18 ('1' of the code-length code {0, 18}) for 138 zeros, then
    # for 121: one too many; and twice 138
    w = _dynamic_header(BitWriter(), 257, 1, {0: 1, 18: 1})
    hand("repeat_overrun_by_one", w.code(1, 1).bits(127, 7).code(1, 1).bits(121 - 11, 7), REPEAT_OVERRUN)
    w = _dynamic_header(BitWriter(), 257, 1, {0: 1, 18: 1})
    hand("repeat_overrun_two_full_runs", w.code(1, 1).bits(127, 7).code(1, 1).bits(127, 7), REPEAT_OVERRUN)
    # 7: 138 + 120 zeros fill the 258 lengths exactly, and lens[256] is 0
    w = _dynamic_header(BitWriter(), 257, 1, {0: 1, 18: 1})
    hand("no_end_of_block_code", w.code(1, 1).bits(127, 7).code(1, 1).bits(120 - 11, 7), NO_EOB)
    # 4: a code-length code of one 2-bit code; a literal/length set whose only code is 256 in 2 bits; a
    # distance set of one 2-bit code under a complete literal/length set
    hand("incomplete_code_length_code", _dynamic_header(BitWriter(), 257, 1, {0: 2}), INCOMPLETE)
    w = BitWriter()
    dynamic_block(w, 1, _ll_lens({256: 2}), [0])
    hand("incomplete_literal_set", w, INCOMPLETE)
    w = BitWriter()
    dynamic_block(w, 1, _ll_lens(_A_EOB_L3, 258), [2])
    hand("incomplete_distance_set", w, INCOMPLETE)
    # 10: the two legal incomplete distance sets, and input that is no code of them: a length symbol
    # where there is no distance code at all; the other bit of the single 1-bit distance code
    hand("length_with_no_distance_code", incomplete_distance_block([0], [("len",)], PAD), BAD_CODE, b"AAA")
    hand("other_bit_of_single_distance_code", incomplete_distance_block([1], [("len",), ("bit", 1)], PAD),
         BAD_CODE, b"AAA")
    # 12 for 10: the same impossible distance bit as the member's last data bit: fewer than 15 bits are
    # left, and the decoder reports the end of the input (include/kgx.h); zlib names the code
    hand("bad_distance_bit_at_the_end", incomplete_distance_block([1], [("len",), ("bit", 1)]), INPUT_END, b"AAA")
    # 13, 14, 15 by hand: one literal and a 10-byte run of it against ISIZE 10; "AB" against ISIZE 3;
    # "AB" with another text's CRC
    w = BitWriter().bits(1, 1).bits(1, 2).fixed_literal(65)
    hand("hand_output_longer", fixed_match(w, 10, 1).fixed_symbol(256), OUTPUT_FULL, b"A" * 10)
    w = BitWriter().bits(1, 1).bits(1, 2).fixed_literal(65).fixed_literal(66).fixed_symbol(256)
    hand("hand_output_shorter", w, OUTPUT_SHORT, b"ABC")
    w = BitWriter().bits(1, 1).bits(1, 2).fixed_literal(65).fixed_literal(66).fixed_symbol(256)
    hand("hand_crc", w, CRC, b"AC")
    # 11 with 63, 64 and 65 literals in front: what the kernel still holds in registers when the
    # failure comes is stored, and counted in out_len
    for n in (63, 64, 65):
        w = BitWriter().bits(1, 1).bits(1, 2)
        for i in range(n):
            w.fixed_literal(literal_value(i))
        hand(f"literals_{n}_then_distance", fixed_match(w, 5, n + 1).fixed_symbol(256), DISTANCE,
             bytes(literal_value(i) for i in range(n + 5)))
    assert set(cases) == set(ZLIB_MESSAGES)
    return cases


def error_case_prefixes():
    """name -> the bytes a failing member of error_cases() produces before its
    failure, where the case defines them"""
    p = {f"literals_{n}_then_distance": bytes(literal_value(i) for i in range(n)) for n in (63, 64, 65)}
    for name in ("length_with_no_distance_code", "other_bit_of_single_distance_code", "bad_distance_bit_at_the_end"):
        p[name] = b"AAA"
    p["hand_output_longer"] = b"A"
    return p


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
