"""The FASTQ parser on the device (kgx_fq_parse, kgx_fq_parse_device,
kgx_fq_proteins_device; csrc/kgx_fq_parse.hip) against the CPU restatement
tests/f2p_restate.py: records, consumed bytes, newline counts and the error,
lenient and strict, with every byte of a record on a lane edge and on a tile
edge, state-dependent bytes, lines longer than tiles, cuts and degenerate
texts."""
import ctypes

import numpy as np
import pytest

import f2p_restate
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
    h = ctx.fq_reads_to_host(r)
    ro, io = h["read_offsets"].astype(np.int64), h["id_offsets"].astype(np.int64)
    assert ro[0] == 0 and io[0] == 0 and ro[-1] == r.n_bases and io[-1] == r.n_id_bytes
    assert np.all(np.diff(ro) >= 0) and np.all(np.diff(io) >= 0)
    assert r.n_reads_no_id == int(np.sum(np.diff(io) == 0))
    b, i = h["bases"].tobytes(), h["ids"].tobytes()
    return [(i[io[k]:io[k + 1]], b[ro[k]:ro[k + 1]]) for k in range(r.n_reads)]


def _want_strict(text: bytes):
    """The restatement under STRICT | FINISHED: parse_complete hands the record
    in progress over only if it has an id (an error hands it over as it stands)."""
    records, error = f2p_restate.parse(text)
    if error is None and not records[-1][0]:
        records = records[:-1]
    return records, error


def _check_lenient(ctx, text: bytes, error_expected=True):
    want, error = f2p_restate.parse(text, stop_at_error=False)
    r = ctx.fq_parse(text, 0)
    assert _records(ctx, r) == want
    if want:
        # consumed is the end of the last record: a quality newline, the records before it, none after it
        assert text[r.consumed - 1:r.consumed] == b"\n"
        assert f2p_restate.parse(text[:r.consumed], False)[0] == want
        assert f2p_restate.parse(text[r.consumed:], False)[0] == []
    else:
        assert r.consumed == 0
    assert r.newlines == text[:r.consumed].count(b"\n")
    if error is not None and error_expected:
        assert r.error and r.error_text() == error[0] and 1 + r.error_newlines == error[1]
        assert text[r.error_pos] == r.error_byte and r.error_pos < r.consumed
        assert r.error_newlines == text[:r.error_pos + 1].count(b"\n")
    elif error is None:
        assert r.error == 0
    return r


def _check_strict(ctx, text: bytes):
    want, error = _want_strict(text)
    r = ctx.fq_parse(text, STRICT_FINISHED)
    got = _records(ctx, r)
    assert got == want
    assert r.consumed == len(text)
    if error is None:
        assert r.error == 0 and r.newlines == text.count(b"\n")
    else:
        rid = got[-1][0]
        line = 1 + r.error_newlines
        assert f"Error found: {r.error_text()} at line {line} id='{rid.decode('latin-1')}'" == \
            f2p_restate.error_report(error)
        assert text[r.error_pos] == r.error_byte
    return r


def _rec(rid: bytes, bases: bytes, defline: bytes = b"", plus: bytes = b"", qual=None) -> bytes:
    return b"@" + rid + defline + b"\n" + bases + b"\n+" + plus + b"\n" + \
        (b"I" * len(bases) if qual is None else qual) + b"\n"


def _short_records(rng, n):
    """Ids of 1-3 bytes, some with a tab or space definition, 11-13 bases, '+id' on some plus lines."""
    out = []
    for k in range(n):
        rid = bytes(rng.choice(np.frombuffer(b"abcxyz019", np.uint8), 1 + k % 3))
        bases = bytes(rng.choice(np.frombuffer(b"ACGTacgtNn", np.uint8), 11 + (k // 3) % 3))
        defline = (b"", b"\tdef 1", b" d")[(k // 2) % 3]
        out.append(_rec(rid, bases, defline, rid if k % 4 == 1 else b""))
    return b"".join(out)


def _state_records():
    """Bytes whose meaning depends on the state."""
    b = b"ACGTACGTACGT"
    return b"".join([
        _rec(b"q1", b, qual=b"@IIIIIIIIIII"), _rec(b"q2", b, qual=b"+IIIIIIIIIII"), _rec(b"q3", b, qual=b"@+@+@+@+@+@+"),
        _rec(b"a@b+c>d", b, b" def @+> @x\t+y"), _rec(b"", b), _rec(b"", b, b" only a definition"),
        _rec(b"x", b, b"\t"), _rec(b">gt", b, plus=b"+@>"), _rec(b"@at", b, qual=b"@@@@@@@@@@@@"),
        _rec(b"e", b"", qual=b""), _rec(b"+p", b, qual=b"+\t+ +@+@+@+@"),
    ])


def _sweep(ctx, body: bytes):
    """A first record whose id length takes 48 consecutive values puts every
    byte of the body's first records on a lane edge and on the tile edge."""
    other = len(_rec(b"", b"ACGTACGTACGT"))
    for shift in range(48):
        text = _rec(b"F" * (TILE - other - 24 + shift), b"ACGTACGTACGT") + body
        _check_lenient(ctx, text)
        _check_strict(ctx, text)


@pytest.fixture(scope="module")
def many():
    """20,000 reads of 150 bases: the text and the restatement's records (parsed once)."""
    rng = np.random.default_rng(0xF0)
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (20000, 150))]
    records = [(b"read%d" % i, bytes(b[i])) for i in range(len(b))]
    text = f2p_restate.fastq_of(records)
    want, error = f2p_restate.parse(text, stop_at_error=False)
    assert error is None and want == records
    return text, want


def test_well_formed(gpu, ctx, many):
    text, want = many
    r = ctx.fq_parse(text, 0)
    assert (r.n_reads, r.error, r.consumed, r.newlines) == (len(want), 0, len(text), 4 * len(want))
    assert r.n_reads_no_id == 0 and r.parse_ms > 0 and r.upload_ms > 0
    assert _records(ctx, r) == want
    d = ctypes.c_void_p()
    gpu.check(gpu.lib().kgx_device_alloc(0, len(text), ctypes.byref(d)), "alloc")
    try:
        gpu.check(gpu.lib().kgx_memcpy_h2d(d, text, len(text)), "h2d")
        for flags in (0, gpu.FQ_STRICT, STRICT_FINISHED):
            r = ctx.fq_parse_device(d.value, len(text), flags)
            assert (r.n_reads, r.error, r.consumed, r.newlines) == (len(want), 0, len(text), 4 * len(want))
            assert _records(ctx, r) == want
    finally:
        gpu.lib().kgx_device_free(d)


def test_every_byte_on_lane_and_tile_edges(ctx):
    _sweep(ctx, _short_records(np.random.default_rng(1), 60))


def test_state_dependent_bytes(ctx):
    _sweep(ctx, _state_records() + _short_records(np.random.default_rng(2), 8))


def test_long_lines(ctx):
    rng = np.random.default_rng(3)
    long_read = bytes(rng.choice(np.frombuffer(b"ACGTN", np.uint8), 70000))
    text = b"".join([
        _rec(b"first", b"ACGTACGT"), _rec(b"long", long_read, qual=b"I" * 10),
        _rec(b"i" * 5000, b"ACGTAC"), _rec(b"d", b"ACGTACG", b" " + b"definition @+> " * 600),
        _rec(b"q", b"ACGT", qual=b"@" * 70000), _rec(b"last", b"TTTT"),
    ])
    r = _check_lenient(ctx, text)
    assert r.n_reads == 6 and r.consumed == len(text)
    _check_strict(ctx, text)


BAD_PIECES = {
    # name: (bytes in front of the offending byte, the offending byte and what follows)
    "leading_gt": (b"", b">" + _rec(b"g", b"ACGTACGTACGT")),
    "garbage": (b"", b"garbage\n" + _rec(b"g", b"ACGTACGTACGT")),
    "blank_lines": (b"", b"\n\n" + _rec(b"b", b"ACGTACGTACGT")),
    "dash": (b"@d\nACGT", b"-ACGT\n+\nIIIIIIII\n"),
    "star": (b"@s\nACGT", b"*ACGT\n+\nIIIIIIII\n"),
    "digit": (b"@n\nACGT", b"5ACGT\n+\nIIIIIIII\n"),
    "cr": (b"@c\nACGTACGT", b"\r\n+\nIIIIIIII\n"),
    "high_byte": (b"@h\nACGT", b"\xc3ACGT\n+\nIIIIIIII\n"),
    "missing_plus": (b"@m\nACGTACGT\n", b"IIIIIIII\n" + _rec(b"m2", b"ACGT")),
    "empty_id_cut": (b"@\nAC", b"-GT\n+\nIIII\n"),
}


def _bad_texts():
    """Each offending byte before, on and after the tile edge (byte 4095, 4096, 4097)."""
    good = _short_records(np.random.default_rng(4), 10)
    other = len(_rec(b"", b"ACGT"))
    for name, (front, back) in BAD_PIECES.items():
        for at in (TILE - 1, TILE, TILE + 1):
            lead = _rec(b"L" * (at - len(front) - other), b"ACGT")
            text = lead + front + back + good
            assert len(lead + front) == at
            yield name, at, text


def _two_errors():
    good = _short_records(np.random.default_rng(5), 120)  # more than a tile
    return _rec(b"t0", b"ACGT") + b"@e1\nAC-GT\n+\nIIII\n" + good + b"@e2\nAC*GT\n+\nIIII\n" + good


def test_lenient_malformed(ctx):
    for name, at, text in _bad_texts():
        r = _check_lenient(ctx, text)
        assert r.error_pos == at, (name, at)
    text = _two_errors()
    r = _check_lenient(ctx, text)
    assert r.error_byte == ord("-") and text.index(b"*") // TILE > r.error_pos // TILE


def test_strict(ctx):
    for name, at, text in _bad_texts():
        r = _check_strict(ctx, text)
        assert r.error_pos == at and r.error, (name, at)
        if name == "empty_id_cut":
            assert _records(ctx, r)[-1] == (b"", b"AC") and r.n_reads_no_id == 1
    text = _two_errors()
    r = _check_strict(ctx, text)
    assert r.error_byte == ord("-") and r.n_reads == 2
    # STRICT without FINISHED and an error: the same cut
    r2 = ctx.fq_parse(text, 1)
    assert (r2.n_reads, r2.error_pos, r2.consumed) == (2, r.error_pos, len(text))


def test_cuts(ctx):
    body = _short_records(np.random.default_rng(6), 50)
    last = _rec(b"last", b"ACGTACGTACGTACGTACGTACGT")
    whole = body + last
    want_whole = f2p_restate.parse(whole, False)[0]
    data_line_end = len(b"@last\n") + 24 + 1
    cuts = [len(body) + k for k in range(1, 49)] + [len(whole) - k for k in (4, 3, 2, 1)]
    assert len(body) + data_line_end in cuts and len(whole) - 1 in cuts and len(last) > 52
    for cut in cuts:
        text = whole[:cut]
        for flags in (0, 1):
            r = ctx.fq_parse(text, flags)
            first = _records(ctx, r)
            assert first == want_whole[:-1] and r.consumed == len(body) and r.error == 0
            assert r.newlines == body.count(b"\n")
        r = ctx.fq_parse(text[r.consumed:] + whole[cut:], 0)
        assert first + _records(ctx, r) == want_whole and r.consumed == len(last)
        r = _check_strict(ctx, text)
        # once a byte of the id is there the record is emitted with what it has
        assert r.n_reads == len(want_whole) - (cut == len(body) + 1) and r.error == 0


def test_degenerate(gpu, ctx):
    r = ctx.fq_parse(b"", STRICT_FINISHED)
    assert (r.n_reads, r.consumed, r.newlines, r.error, r.n_bases, r.bases) == (0, 0, 0, 0, 0, None)
    t = ctx.fq_proteins_device(r)
    assert (t.n_reads, t.n_fragments, t.n_bytes) == (0, 0, 0)
    for text in (b"@", b"@abc def ACGT", b"@id", b"\n\n\n\n\n", b"\n", _rec(b"one", b"ACGTACGT"), b"x", b">",
                 b"@a\nAC", b"@a\nAC\n", b"@a\nAC\n+", b"@a\nAC\n+\nII"):
        _check_lenient(ctx, text, error_expected=False)
        _check_strict(ctx, text)
    r = ctx.fq_parse(b"\n\n\n", 0)
    assert (r.n_reads, r.consumed, r.error) == (0, 0, 0)  # nothing consumed: nothing reported yet
    r = ctx.fq_parse(b"\n\n\n", 1)
    assert (r.n_reads, r.n_reads_no_id, r.error, r.error_byte, r.error_newlines, r.consumed) == (1, 1, 2, 10, 1, 3)
    r = ctx.fq_parse(_rec(b"one", b"ACGTACGT"), 0)
    assert _records(ctx, r) == [(b"one", b"ACGTACGT")] and r.newlines == 4
    # arguments
    out = gpu.FqReads()
    lib = gpu.lib()
    assert lib.kgx_fq_parse(ctx.handle, b"@", 1, 4, ctypes.byref(out)) == gpu.KGX_EINVAL
    assert lib.kgx_fq_parse(ctx.handle, None, 1, 0, ctypes.byref(out)) == gpu.KGX_EINVAL
    assert lib.kgx_fq_parse(ctx.handle, b"@", 1, 0, None) == gpu.KGX_EINVAL
    assert lib.kgx_fq_parse(ctx.handle, b"@", gpu.FQ_PARSE_MAX + 1, 0, ctypes.byref(out)) == gpu.KGX_ERANGE
    assert "KGX_FQ_PARSE_MAX" in gpu.last_error()
    assert lib.kgx_fq_parse_device(ctx.handle, 0x1008, 64, 0, ctypes.byref(out)) == gpu.KGX_EINVAL
    assert "aligned" in gpu.last_error()


def test_bounds_and_proteins_device(gpu, ctx, oracle_lib):
    """Text buffers of exactly n bytes around the tile size; the slack past the
    reads poisoned before kgx_fq_proteins_device reads them."""
    rng = np.random.default_rng(7)
    recs = [(b"r%d" % k, bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 90 + k % 60))) for k in range(40)]
    base = f2p_restate.fastq_of(recs)
    assert len(base) > TILE + 200
    lib = gpu.lib()
    for n in (TILE - 1, TILE, TILE + 1):
        text = base[:n]
        want, _ = _want_strict(text)
        d = ctypes.c_void_p()
        gpu.check(lib.kgx_device_alloc(0, n, ctypes.byref(d)), "alloc")
        try:
            gpu.check(lib.kgx_memcpy_h2d(d, text, n), "h2d")
            for poison in (0x00, 0xFF, ord("A")):
                # without FINISHED the record in progress is no read: its bytes lie past n_bases
                for flags, expect in ((STRICT_FINISHED, want), (0, f2p_restate.parse(text, False)[0])):
                    r = ctx.fq_parse_device(d.value, n, flags)
                    assert _records(ctx, r) == expect
                    fill = bytes([poison]) * 16
                    gpu.check(lib.kgx_memcpy_h2d(r.bases + r.n_bases, fill, 16), "h2d")
                    gpu.check(lib.kgx_memcpy_h2d(r.ids + r.n_id_bytes, fill, 16), "h2d")
                    t = ctx.fq_proteins_device(r)
                    got = bytes(ctx.fq_text_to_host(t)["text"])
                    assert got == f2p_restate.records_text(expect, oracle_lib.translate11)
                    assert t.n_reads == len(expect) and got.count(b">") == t.n_fragments > 0
        finally:
            lib.kgx_device_free(d)
    # reads that are not this context's last parse are refused
    r = ctx.fq_parse(base, 0)
    stale = gpu.FqReads.from_buffer_copy(r)
    stale.bases = r.bases + 16
    t = gpu.FqText()
    assert lib.kgx_fq_proteins_device(ctx.handle, ctypes.byref(stale), ctypes.byref(t)) == gpu.KGX_EINVAL
