"""kgx_inflate_host, kgx_gunzip_scan and the host side of kgx_gunzip (no
context: blocked members on host threads, plain members on the caller's)
through abi.py: the decode and error cases of bgzf_util (every decoder reason
by a hand-made member, the legal incomplete distance sets, the geometry,
stored-geometry and size members, these also one by one with their
statistics), the first 512 streams of the mutated corpus against zlib's
verdicts, raw and wrapped as blocked members, and single members with every
optional header field against zlib.decompressobj(31).  No GPU."""
import zlib

import pytest

import bgzf_util as bz
from test_inflate_native import check_corpus_stream, check_stats


@pytest.fixture(scope="module")
def abi(kgx):
    return kgx


def test_new_symbols_are_exported_and_listed(abi):
    for name in ("kgx_inflate_host", "kgx_gunzip_scan", "kgx_gunzip", "kgx_gunzip_device"):
        assert name in abi.SIGNATURES and name in abi.header_symbols()
        assert getattr(abi.lib(), name)


def test_inflate_host_decodes_and_reports(abi):
    g = bz.golden()
    for level in (0, 1, 6, 9):
        raw = bz.raw_deflate(g, level)
        rc, out, used, st, reason, bit = abi.inflate_host(raw + b"tail", len(g))
        assert (rc, reason) == (0, 0) and out == g and used == len(raw)
        assert st["stored_blocks" if level == 0 else "dynamic_blocks"] >= 1
    raw = bz.raw_deflate(g, 6, zlib.Z_FIXED)
    rc, out, used, st, reason, bit = abi.inflate_host(raw, len(g))
    assert rc == 0 and out == g and st["fixed_blocks"] == 1 and st["dynamic_blocks"] == 0
    # no room: nothing past cap, and the bytes before it are the text's
    rc, out, used, st, reason, bit = abi.inflate_host(raw, 100)
    assert rc == abi.KGX_EFORMAT and reason == bz.OUTPUT_FULL and out == g[:len(out)] and len(out) <= 100
    assert "reason 13" in abi.last_error()
    rc, out, used, st, reason, bit = abi.inflate_host(b"", 10)
    assert rc == abi.KGX_EFORMAT and reason == bz.INPUT_END and bit == 0


def test_inflate_host_error_reasons(abi):
    for name, (member, reason) in bz.error_cases().items():
        if reason in (bz.OUTPUT_SHORT, bz.CRC):
            continue  # trailer checks: the gzip layer's (test_gunzip_error_cases)
        raw, isize = member[18:-8], int.from_bytes(member[-4:], "little")
        rc, out, used, st, got, bit = abi.inflate_host(raw, isize)
        assert rc == abi.KGX_EFORMAT and got == reason, (name, got)
        assert bit <= 8 * len(raw)


def test_scan(abi):
    g = bz.golden()
    b = bz.bgzf(g, chunk=1000)
    assert abi.gunzip_scan(b) == {"members": 21, "blocked": 21, "out_bytes": len(g), "consumed": len(b)}
    # a member that is not complete yet stays unconsumed
    first = int.from_bytes(b[16:18], "little") + 1
    s = abi.gunzip_scan(b[:first + 30], finished=False)
    assert s["blocked"] == 1 and s["consumed"] == first and s["out_bytes"] == 1000
    with pytest.raises(abi.KgxError) as e:
        abi.gunzip_scan(b[:first + 30], finished=True)
    assert e.value.code == abi.KGX_EFORMAT and "member 1" in str(e.value) and "cut short" in str(e.value)
    # stops at a plain member's header, and counts it
    p = bz.plain_cases()["blocked_then_plain"][0]
    s = abi.gunzip_scan(p)
    assert s["members"] == s["blocked"] + 1 and s["blocked"] == 7 and s["out_bytes"] == 7000
    # trailing garbage after a member is consumed
    s = abi.gunzip_scan(b + b"\0\0junk")
    assert s["consumed"] == len(b) + 6 and s["blocked"] == 21
    for name, (body, reason) in bz.framing_error_cases().items():
        with pytest.raises(abi.KgxError) as e:
            abi.gunzip_scan(body)
        assert e.value.code == abi.KGX_EFORMAT and f"reason {reason}" in str(e.value), name
    with pytest.raises(abi.KgxError):
        abi.gunzip_scan(b"@read1\nACGT\n+\nIIII\n")
    assert abi.gunzip_scan(b"") == {"members": 0, "blocked": 0, "out_bytes": 0, "consumed": 0}


def test_gunzip_host_threads_decode_cases(abi):
    for name, (gz, text, want) in bz.decode_cases().items():
        out, consumed, st = abi.gunzip(None, gz)
        assert out == text and consumed == len(gz), name
        assert st["host_blocked_members"] == st["members"] and st["device_members"] == 0, name
        check_stats(st, want, name)


def test_gunzip_plain_members(abi):
    for name, (gz, text) in bz.plain_cases().items():
        out, consumed, st = abi.gunzip(None, gz, cap=len(text))
        assert out == text and consumed == len(gz), name
        assert st["plain_members"] >= 1, name
        # too little room: KGX_ERANGE
        with pytest.raises(abi.KgxError) as e:
            abi.gunzip(None, gz, cap=len(text) - 1)
        assert e.value.code == abi.KGX_ERANGE, name
    # every member is decoded, not only the first (RFC 1952 2.2)
    gz, text = bz.plain_cases()["plain_two"]
    assert abi.gunzip(None, gz, cap=len(text))[2]["members"] == 2
    # a plain member waits for `finished`
    out, consumed, st = abi.gunzip(None, bz.plain_cases()["plain"][0], finished=False, cap=30000)
    assert (out, consumed, st["members"]) == (b"", 0, 0)


def test_gunzip_error_cases(abi):
    for name, (member, reason) in bz.error_cases().items():
        body = bz.bgzf(b"first\n", eof=False) + member + bz.bgzf(b"last\n", eof=False)
        with pytest.raises(abi.KgxError) as e:
            abi.gunzip(None, body)
        assert e.value.code == abi.KGX_EFORMAT, name
        assert "member 1:" in str(e.value) and f"reason {reason}" in str(e.value), (name, str(e.value))
    # a plain member cut short, and one with a wrong CRC
    gz, text = bz.plain_cases()["plain"]
    with pytest.raises(abi.KgxError) as e:
        abi.gunzip(None, gz[:-9], cap=len(text))
    assert e.value.code == abi.KGX_EFORMAT and "cut short" in str(e.value)
    bad = gz[:-8] + bytes([gz[-8] ^ 1]) + gz[-7:]
    with pytest.raises(abi.KgxError) as e:
        abi.gunzip(None, bad, cap=len(text))
    assert e.value.code == abi.KGX_EFORMAT and f"reason {bz.CRC}" in str(e.value)


def test_member_sets_member_by_member(abi):
    """the geometry, stored-geometry and size members one by one through
    kgx_inflate_host in a room of exactly the text: the text, the input used
    and the statistics of the member's one match"""
    for p, dist, length, m, text in bz.geometry_members():
        rc, out, used, st, reason, bit = abi.inflate_host(m[18:-8], len(text))
        assert (rc, reason, out, used) == (0, 0, text, len(m) - 26), (p, dist, length)
        assert (st["matches"], st["max_distance"], st["max_length"], st["overlap"]) == \
            (1, dist, length, int(dist < length)), (p, dist, length, st)
    for p, s, dist, length, m, text in bz.stored_members():
        rc, out, used, st, reason, bit = abi.inflate_host(m[18:-8], len(text))
        assert (rc, reason, out, used) == (0, 0, text, len(m) - 26), (p, s)
        assert (st["matches"], st["max_distance"], st["max_length"], st["stored_blocks"], st["fixed_blocks"]) == \
            (1, dist, length, 1, 2), (p, s, st)
    for n, m, text in bz.size_members():
        rc, out, used, st, reason, bit = abi.inflate_host(m[18:-8], n)
        assert (rc, reason, out, used) == (0, 0, text, len(m) - 26), n
        # one byte less room: refused, and what was produced is the text's beginning
        rc, out, used, st, reason, bit = abi.inflate_host(m[18:-8], n - 1)
        assert (rc, reason) == (abi.KGX_EFORMAT, bz.OUTPUT_FULL) and out == text[:len(out)], n


def test_error_case_prefixes(abi):
    """what a failing stream produced before it failed is there and counted"""
    for name, prefix in bz.error_case_prefixes().items():
        m = bz.error_cases()[name][0]
        rc, out, used, st, reason, bit = abi.inflate_host(m[18:-8], int.from_bytes(m[-4:], "little"))
        assert rc == abi.KGX_EFORMAT and out == prefix, (name, out)


CORPUS_SLICE = 512  # of bz.corpus(): the streams the GPU test gives to the kernel


def test_corpus_slice_through_the_library(abi):
    """the first 512 streams of the corpus through kgx_inflate_host, with the
    rooms and the requirements of test_inflate_native.test_mutated_corpus_against_zlib"""
    for i, entry in enumerate(bz.corpus()[:CORPUS_SLICE]):
        raw, ok, text, _ = entry
        rc, out, used, st, reason, bit = abi.inflate_host(raw, bz.corpus_room(ok, text))
        assert (rc == 0) == (reason == 0) and used == (bit + 7) // 8
        check_corpus_stream(i, entry, dict(reason=reason, out_len=len(out), bit=bit), out)
        if reason:
            assert f"reason {reason})" in abi.last_error() and f"at bit {bit}" in abi.last_error(), i


def test_corpus_slice_as_blocked_members(abi):
    """the same streams wrapped as blocked members through kgx_gunzip without a
    context: those zlib accepts as one body, whose text is zlib's; every one
    it rejects in the middle of accepted ones, where the error names its index
    and the reason kgx_inflate_host gave for the stream"""
    part = bz.corpus()[:CORPUS_SLICE]
    good = [(bz.bgzf_member(raw, text), text) for raw, ok, text, _ in part if ok]
    assert len(good) >= CORPUS_SLICE // 4
    body, text = b"".join(m for m, _ in good), b"".join(t for _, t in good)
    out, consumed, st = abi.gunzip(None, body)
    assert out == text and consumed == len(body) and st["host_blocked_members"] == len(good)
    front, back = b"".join(m for m, _ in good[:5]), b"".join(m for m, _ in good[5:8])
    rejected = 0
    for raw, ok, text, _ in part:
        if ok:
            continue
        room = bz.corpus_room(ok, text)
        reason = abi.inflate_host(raw, room)[4]
        with pytest.raises(abi.KgxError) as e:
            abi.gunzip(None, front + bz.bgzf_member(raw, b"", crc=0x12345678, isize=room) + back)
        assert e.value.code == abi.KGX_EFORMAT and "member 5:" in str(e.value) and \
            f"(reason {reason})" in str(e.value), (rejected, str(e.value))
        assert "member 5:" in abi.last_error() and f"(reason {reason})" in abi.last_error()
        rejected += 1
    assert rejected >= CORPUS_SLICE // 4


def test_header_variants_against_zlib(abi):
    """single members with every optional header field (RFC 1952 2.3) against
    zlib.decompressobj(31): the same verdict and the same text; the framing
    walk's `blocked` says which it took as blocked members (a BC subfield of
    length 2 anywhere in the extra field)"""
    g = bz.golden()[:3000]
    for name, (body, blocked) in bz.gzip_header_variants().items():
        want = bz.zlib_gunzip(body)
        try:
            out, consumed, st = abi.gunzip(None, body, cap=len(g))
        except abi.KgxError as e:
            assert e.code == abi.KGX_EFORMAT, name
            out = None
            assert "member 0:" in str(e), (name, str(e))
            assert ("reason 38" if "fhcrc" in name else "reason 35") in str(e), (name, str(e))
        assert out == want, name
        if want is not None:
            assert want == g and consumed == len(body), name
            assert (st["host_blocked_members"], st["plain_members"]) == ((1, 0) if blocked else (0, 1)), name
            assert abi.gunzip_scan(body) == {"members": 1, "blocked": int(blocked),
                                            "out_bytes": len(g) if blocked else 0,
                                            "consumed": len(body) if blocked else 0}, name
        else:
            assert not blocked
            with pytest.raises(abi.KgxError):
                abi.gunzip_scan(body)


@pytest.mark.parametrize("step", (1, 17, 4096))
def test_gunzip_streaming_never_splits_a_member(abi, step):
    g = bz.golden()
    gz = bz.bgzf(g, chunk=1000)
    ends, at = set(), 0
    while at < len(gz):
        at += int.from_bytes(gz[at + 16:at + 18], "little") + 1
        ends.add(at)
    tail, out, taken = b"", [], 0
    for at in range(0, len(gz), step):
        tail += gz[at:at + step]
        last = at + step >= len(gz)
        text, consumed, _ = abi.gunzip(None, tail, finished=last, cap=len(g))
        taken += consumed
        assert consumed == 0 or taken in ends
        out.append(text)
        tail = tail[consumed:]
    assert b"".join(out) == g and tail == b"" and taken == len(gz)
