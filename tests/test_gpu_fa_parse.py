"""The FASTA parser on the device (kgx_fa_parse, kgx_fa_parse_device;
csrc/kgx_fa_parse.hip) against the CPU restatement tests/fa_restate.py:
records, records without an id, consumed bytes, newline counts and the error,
lenient, lenient finished and strict finished, at the lengths and positions
where a lane, a tile or a scan round ends."""
import ctypes

import numpy as np
import pytest

import fa_restate
from helpers import synthetic_table

pytestmark = pytest.mark.gpu

TILE = 4096
STRICT_FINISHED = 3


@pytest.fixture(scope="module")
def ctx(gpu):
    _, table = synthetic_table(20000)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as c:
        yield c


def _records(ctx, r):
    h = ctx.fa_seqs_to_host(r)
    if not r.n_seqs and not r.seq_offsets:
        assert (r.n_residues, r.n_id_bytes, r.n_seqs_no_id) == (0, 0, 0)
        return []
    so, io = h["seq_offsets"].astype(np.int64), h["id_offsets"].astype(np.int64)
    assert so[0] == 0 and io[0] == 0 and so[-1] == r.n_residues and io[-1] == r.n_id_bytes
    assert np.all(np.diff(so) >= 0) and np.all(np.diff(io) >= 0)
    assert r.n_seqs_no_id == int(np.sum(np.diff(io) == 0))
    b, i = h["residues"].tobytes(), h["ids"].tobytes()
    return [(i[io[k]:io[k + 1]], b[so[k]:so[k + 1]]) for k in range(r.n_seqs)]


def _error_of(r):
    return (r.error_pos, r.error, r.error_byte, r.error_newlines) if r.error else None


def _check(ctx, text: bytes, parse=None):
    """All three modes of one text, and the carried-tail invariant."""
    parse = parse or (lambda flags: ctx.fa_parse(text, flags))
    first = fa_restate.first_error(text)
    for finished in (False, True):
        want, consumed, newlines, error = fa_restate.lenient(text, finished)
        r = parse(2 if finished else 0)
        assert _records(ctx, r) == want
        assert (r.consumed, r.newlines, _error_of(r)) == (consumed, newlines, error)
        assert r.n_seqs_no_id == sum(1 for i, _ in want if not i)
        if not finished and want:
            # text[:consumed] holds those records and no more; what follows holds no complete one
            assert text[consumed:consumed + 1] == b">"
            assert _records(ctx, ctx.fa_parse(text[:consumed], 2)) == want
            assert ctx.fa_parse(text[consumed:], 0).n_seqs == 0
        elif not finished:
            assert consumed == 0
    want, error = fa_restate.parse(text, stop_at_error=True)
    r = parse(STRICT_FINISHED)
    got = _records(ctx, r)
    assert got == want
    assert (r.consumed, r.newlines, _error_of(r)) == (len(text), text.count(b"\n"), first)
    if error is not None:
        assert (r.error_text(), 1 + r.error_newlines, got[-1][0]) == error
        assert text[r.error_pos] == r.error_byte
        # STRICT without FINISHED and an error: the same cut
        r1 = parse(1)
        assert _records(ctx, r1) == want and (r1.consumed, _error_of(r1)) == (len(text), first)
    else:
        # STRICT without an error is the lenient result
        r1, r0 = parse(1), fa_restate.lenient(text, False)
        assert _records(ctx, r1) == r0[0] and (r1.consumed, r1.newlines, r1.error) == (r0[1], r0[2], 0)
    return r


def _fasta(records, width=60, eol=b"\n") -> bytes:
    out = []
    for rid, seq in records:
        out.append(b">" + rid + eol)
        for k in range(0, len(seq), width):
            out.append(seq[k:k + width] + eol)
    return b"".join(out)


def _proteins(rng, n, lo=0, hi=200):
    a = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    return [(b"p%d" % k, bytes(a[rng.integers(0, 20, int(rng.integers(lo, hi + 1)))])) for k in range(n)]


def test_lengths(ctx):
    """Text lengths around a lane, a wave's 1024 bytes and a tile."""
    base = _fasta(_proteins(np.random.default_rng(1), 60, 20, 200), width=23)
    assert len(base) > TILE + 1
    for n in (0, 1, 15, 16, 17, 1023, 1024, 1025, 4095, 4096, 4097):
        _check(ctx, base[:n])


def test_record_end_on_every_lane_and_tile_edge(ctx):
    """A first record whose id length takes 48 consecutive values puts the '>'
    that ends it, and every byte of the records after it, on the last and the
    first byte of a lane and of a tile."""
    body = b">b c\nAC*\nDE\n>\nFG\n> only def\nHI\n\n>last\nKL"
    seen = set()
    for shift in range(48):
        lead = b">" + b"F" * (TILE - 24 + shift - len(b">\nACDE\n")) + b"\nACDE\n"
        text = lead + body
        assert text[len(lead)] == ord(">")
        seen.add(len(lead))
        r = _check(ctx, text)
        assert r.n_seqs == 5
    assert {TILE - 1, TILE, TILE - 17, TILE - 16, TILE + 15, TILE + 16} <= seen


def test_spans_over_a_tile_edge(ctx):
    """An id, a definition line and a sequence line that each cross byte 4096;
    sequences longer than a tile."""
    pad = lambda k: _fasta([(b"pad", b"A" * (k - len(b">pad\n\n")))], width=1 << 20)
    for text in (
        pad(TILE - 10) + b">" + b"i" * 40 + b" def\nACDE\n>n\nFG\n",
        pad(TILE - 10) + b">id " + b"definition > * " * 4 + b"\nACDE\n>n\nFG\n",
        pad(TILE - 10) + b">id\n" + b"ACDEFGHIKLMNPQRSTVWY" * 2 + b"\nAC\n>n\nFG\n",
        pad(TILE - 2) + b">id\r\nAC\r\nDE\r\n>n\r\nFG\r\n",
    ):
        assert len(text) > TILE + 8
        r = _check(ctx, text)
        assert r.error == 0 and r.n_seqs == 3
    rng = np.random.default_rng(2)
    long_seq = bytes(rng.choice(np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8), 5000))
    for width in (1 << 20, 60):
        text = _fasta([(b"first", b"ACDE"), (b"long", long_seq), (b"last", b"FG")], width=width)
        r = _check(ctx, text)
        assert r.error == 0 and _records(ctx, r)[1] == (b"long", long_seq)


def test_hand_cases(ctx):
    """'\\r\\n' line ends, blank lines, empty ids, '*' in data and first on a
    later line, '>' straight after a header, no leading '>', texts that end
    inside an id, a definition line or a data line, bytes >= 0x80: alone, and
    pushed so that they straddle the first tile's edge."""
    lead = _fasta([(b"lead", b"ACDEFGHIKL" * 400)], width=70)
    assert len(lead) < TILE - 9
    for case in fa_restate.HAND_CASES:
        _check(ctx, case)
    for case in fa_restate.HAND_CASES:
        if not case.startswith(b">"):
            continue
        for back in (1, 4, 9):
            text = lead + b"\n" * (TILE - back - len(lead)) + case  # blank lines up to the case's '>'
            assert text[TILE - back] == ord(">")
            _check(ctx, text)
    r = ctx.fa_parse(b">a\nAC\r\n*DE\n>b\n", STRICT_FINISHED)
    assert (r.error, r.error_byte, r.error_pos, r.error_newlines, r.n_seqs) == (3, ord("*"), 7, 2, 1)
    assert r.error_text() == "Bad id or data character '*'"
    r = ctx.fa_parse(b">a\n>b\nAC\n", 2)
    assert (r.error, r.error_byte, r.error_pos) == (2, ord(">"), 3) and _records(ctx, r) == [(b"a", b"bAC")]


def test_random_texts(ctx):
    for text in fa_restate.random_texts():
        _check(ctx, text)


@pytest.fixture(scope="module")
def big():
    """Just over 1 MiB of well-formed FASTA: about 4,000 records whose id
    lengths vary, so that line starts fall on every lane offset."""
    rng = np.random.default_rng(0xB16)
    a = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    recs = []
    for k in range(4000):
        rid = b"prot%d" % k + b"x" * (k % 17)
        recs.append((rid + (b" definition %d" % k if k % 3 == 0 else b""), bytes(a[rng.integers(0, 20, 240 + k % 53)])))
    text = _fasta(recs)
    assert 257 * TILE < len(text) < 2 * (1 << 20)
    assert {text.index(b"\n", p) % 16 for p in range(0, len(text), 997)} == set(range(16))
    return text


def test_big_against_oracle(gpu, ctx, big, oracle_lib):
    r = ctx.fa_parse(big, 2)
    assert (r.n_seqs, r.error, r.consumed, r.newlines, r.n_seqs_no_id) == (4000, 0, len(big), big.count(b"\n"), 0)
    assert r.parse_ms > 0 and r.upload_ms > 0
    got = _records(ctx, r)
    lines = "".join(f"{i.decode('latin-1')}\t{s.decode('latin-1')}\n" for i, s in got)
    assert lines == oracle_lib.fasta_parse(big)
    r = ctx.fa_parse(big, 0)
    assert (r.n_seqs, r.consumed) == (3999, big.rindex(b">")) and _records(ctx, r) == got[:-1]


def test_device_text(gpu, ctx, big):
    """kgx_fa_parse_device over device copies of exactly n bytes."""
    lib = gpu.lib()
    noisy = fa_restate.random_texts(6, 9000, seed=5)
    for text in [big[:TILE - 1], big[:TILE], big[:TILE + 1], big] + [t for t in noisy if t]:
        d = ctypes.c_void_p()
        gpu.check(lib.kgx_device_alloc(0, len(text), ctypes.byref(d)), "alloc")
        try:
            gpu.check(lib.kgx_memcpy_h2d(d, text, len(text)), "h2d")
            if text is big:
                r = ctx.fa_parse_device(d.value, len(text), 2)
                assert (r.n_seqs, r.error, r.consumed, r.upload_ms) == (4000, 0, len(big), 0)
                assert _records(ctx, r) == fa_restate.lenient(big, True)[0]
            else:
                _check(ctx, text, lambda flags: ctx.fa_parse_device(d.value, len(text), flags))
        finally:
            lib.kgx_device_free(d)


def test_arguments_and_empty(gpu, ctx):
    r = ctx.fa_parse(b"", 0)
    assert (r.n_seqs, r.consumed, r.newlines, r.error, r.n_residues, r.residues, r.seq_offsets) == (0, 0, 0, 0, 0, None, None)
    for flags in (2, 3):
        r = ctx.fa_parse(b"", flags)
        assert (r.n_seqs, r.n_seqs_no_id, r.consumed, r.error, r.n_residues, r.n_id_bytes) == (1, 1, 0, 0, 0, 0)
        h = ctx.fa_seqs_to_host(r)
        assert h["seq_offsets"].tolist() == [0, 0] and h["id_offsets"].tolist() == [0, 0]
        r = ctx.fa_parse_device(None, 0, flags)
        assert (r.n_seqs, r.n_seqs_no_id) == (1, 1) and ctx.fa_seqs_to_host(r)["id_offsets"].tolist() == [0, 0]
    out = gpu.FaSeqs()
    lib = gpu.lib()
    assert lib.kgx_fa_parse(ctx.handle, b">", 1, 4, ctypes.byref(out)) == gpu.KGX_EINVAL
    assert "KGX_FA_STRICT" in gpu.last_error()
    assert lib.kgx_fa_parse(ctx.handle, None, 1, 0, ctypes.byref(out)) == gpu.KGX_EINVAL
    assert lib.kgx_fa_parse(ctx.handle, b">", 1, 0, None) == gpu.KGX_EINVAL
    assert lib.kgx_fa_parse(None, b">", 1, 0, ctypes.byref(out)) == gpu.KGX_EINVAL
    assert lib.kgx_fa_parse(ctx.handle, b">", gpu.FA_PARSE_MAX + 1, 0, ctypes.byref(out)) == gpu.KGX_ERANGE
    assert "KGX_FA_PARSE_MAX" in gpu.last_error()
    assert lib.kgx_fa_parse_device(ctx.handle, 0x1008, gpu.FA_PARSE_MAX + 1, 0, ctypes.byref(out)) == gpu.KGX_ERANGE
    assert lib.kgx_fa_parse_device(ctx.handle, 0x1008, 64, 0, ctypes.byref(out)) == gpu.KGX_EINVAL
    assert "aligned" in gpu.last_error()


def test_fq_results_survive_a_fasta_parse(gpu, ctx):
    """The FASTA outputs are buffers of their own: an fq parse's reads are
    still there after a FASTA parse, and the other way round."""
    fq = b"@r1\nACGTACGT\n+\nIIIIIIII\n@r2\nTTTT\n+\nIIII\n"
    rq = ctx.fq_parse(fq, 0)
    ra = ctx.fa_parse(b">a\nACDE\n>b\nFG\n", 2)
    hq = ctx.fq_reads_to_host(rq)
    assert hq["bases"].tobytes() == b"ACGTACGTTTTT" and hq["ids"].tobytes() == b"r1r2"
    ctx.fq_parse(fq, 0)
    assert _records(ctx, ra) == [(b"a", b"ACDE"), (b"b", b"FG")]


def _stream(ctx, whole: bytes, block: int):
    """Blocks of `block` bytes through strict parses, the tail carried:
    (records, None or (message, line, id))."""
    records, lines, tail, error = [], 0, b"", None
    for at in range(0, len(whole), block):
        text = tail + whole[at:at + block]
        r = ctx.fa_parse(text, 1)
        records += _records(ctx, r)
        if r.error:
            error = (r.error_text(), 1 + lines + r.error_newlines, records[-1][0])
            break
        lines += r.newlines
        tail = text[r.consumed:]
    if error is None:
        r = ctx.fa_parse(tail, STRICT_FINISHED)
        records += _records(ctx, r)
        if r.error:
            error = (r.error_text(), 1 + lines + r.error_newlines, records[-1][0])
    return records, error


def test_block_cut_stream(ctx):
    rng = np.random.default_rng(9)
    good = _fasta(_proteins(rng, 40, 0, 300), width=60)
    texts = [good, good.replace(b"\n", b"\r\n"), good + b">bad\nAC-DE\n>after\nAC\n", good + b">z\nAC\n*\n",
             b"x" + good, good[:-1], good + b">end in id", b""]
    assert len(good) > 4096 + 1000
    for whole in texts:
        want = fa_restate.parse(whole, stop_at_error=True)
        for block in (37, 1000, 4096):
            assert _stream(ctx, whole, block) == want, (whole[-30:], block)
