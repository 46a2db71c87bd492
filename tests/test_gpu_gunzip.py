"""inflate_members_kernel (csrc/kgx_inflate.hip) through kgx_gunzip and
kgx_gunzip_device: the decode cases of tests/bgzf_util.py byte for byte, with
the statistics that show each hit its target, on the device and on the host
threads (option gunzip_device 1 and 0); the error cases as status codes, with
the other members' text intact and the sentinel bytes around every slot
untouched.  Among the cases: a hand-made member for every decoder reason, the
two legal incomplete distance sets, and the member sets with per-member
expectations (match geometry, stored geometry, sizes: one launch each).  And
the kernel against the host decoder against zlib, member by member, over 512
streams of the mutated corpus, half of them corrupt.  The same bytes pass
tests/test_inflate_native.py on the CPU, plain and under ASan/UBSan, before
they are given to the kernel here."""
import ctypes
import zlib

import numpy as np
import pytest

import bgzf_util as bz
from helpers import synthetic_table
from test_inflate_native import check_stats

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def world(gpu):
    spec, table = synthetic_table(2000)
    img = gpu.Image.from_table(table)
    ctx = gpu.Context(img)
    yield gpu, ctx
    ctx.close()
    img.close()


def member_table(abi, gz, gap=0):
    """the framing walk in Python: the kernel's member table for a body of
    blocked members, every slot followed by `gap` bytes nobody may write"""
    rows, at, out = [], 0, 0
    while at < len(gz):
        assert gz[at:at + 4] == b"\x1f\x8b\x08\x04" and gz[at + 12:at + 16] == b"BC\x02\x00"
        total = int.from_bytes(gz[at + 16:at + 18], "little") + 1
        crc, isize = int.from_bytes(gz[at + total - 8:at + total - 4], "little"), \
            int.from_bytes(gz[at + total - 4:at + total], "little")
        rows.append((at + 18, out, total - 26, isize, crc, 0))
        out += isize + gap
        at += total
    return np.array(rows, dtype=abi.GZ_MEMBER_DTYPE), out


class DeviceBytes:
    def __init__(self, abi, data: bytes):
        self.abi, self.n = abi, max(len(data), 1)
        p = ctypes.c_void_p()
        abi.check(abi.lib().kgx_device_alloc(0, self.n, ctypes.byref(p)), "kgx_device_alloc")
        self.p = p.value
        if data:
            abi.check(abi.lib().kgx_memcpy_h2d(self.p, data, len(data)), "kgx_memcpy_h2d")

    def read(self) -> bytes:
        buf = ctypes.create_string_buffer(self.n)
        self.abi.check(self.abi.lib().kgx_memcpy_d2h(buf, self.p, self.n), "kgx_memcpy_d2h")
        return buf.raw

    def free(self):
        self.abi.lib().kgx_device_free(self.p)


def run_kernel(abi, ctx, gz, gap=16):
    """the body's members through kgx_gunzip_device into a sentinel-filled
    buffer: (rc, status, stats, members, the buffer after the kernel)"""
    members, room = member_table(abi, gz, gap)
    members["out_off"] += gap  # a gap in front of the first slot too
    d_gz, d_out = DeviceBytes(abi, gz), DeviceBytes(abi, b"\xa5" * (room + gap))
    try:
        rc, status, stats, ms = abi.gunzip_device(ctx, d_gz.p, members, d_out.p)
        return rc, status, stats, members, d_out.read()
    finally:
        d_gz.free()
        d_out.free()


def sentinels_intact(members, buf, gap, skip=()):
    at = 0
    for i, m in enumerate(members):
        off, n = int(m["out_off"]), int(m["out_len"])
        assert buf[at:off] == b"\xa5" * (off - at), f"bytes in front of member {i}'s slot were written"
        at = off + n
    assert buf[at:] == b"\xa5" * (len(buf) - at), "bytes behind the last slot were written"


def test_decode_cases_device_and_host_threads(world):
    abi, ctx = world
    for device in (1, 0):
        ctx.set_option("gunzip_device", device)
        for name, (gz, text, want) in bz.decode_cases().items():
            out, consumed, st = abi.gunzip(ctx, gz)
            assert out == text and consumed == len(gz), (name, device)
            assert st["device_members" if device else "host_blocked_members"] == st["members"], (name, device)
            check_stats(st, want, (name, device))
            assert st["bytes_in"] == len(gz) and st["bytes_out"] == len(text)
    ctx.set_option("gunzip_device", 0)


def test_kernel_alone_with_sentinels(world):
    """kgx_gunzip_device: every slot holds its member's text, and no byte
    between the slots, in front of the first or behind the last was written"""
    abi, ctx = world
    for name in ("golden_l6_c1000_eof", "golden_l0_c37_noeof", "overlap_d1", "literal_match_d1", "literal_match_d3",
                 "window_32768", "codelen15", "sync_flush", "stored_65280", "members_64", "members_65", "members_257",
                 "members_1", "members_3", "isize0_between", "empty", "no_distance_code", "single_distance_code",
                 "literals_only_63", "literals_only_64", "literals_only_65"):
        gz, text, want = bz.decode_cases()[name]
        rc, status, stats, members, buf = run_kernel(abi, ctx, gz)
        assert rc == 0 and not status["reason"].any(), (name, abi.last_error())
        assert (status["out_len"] == members["out_len"]).all(), name
        got = b"".join(buf[int(m["out_off"]):int(m["out_off"]) + int(m["out_len"])] for m in members)
        assert got == text, name
        sentinels_intact(members, buf, 16)
        total = {k: (int(stats[k].max()) if k.startswith("max_") or k == "overlap" else int(stats[k].sum()))
                 for k in stats.dtype.names}
        total["members"] = len(members)
        check_stats(total, want, name)


def member_stats(stats, i):
    return {k: int(stats[k][i]) for k in stats.dtype.names}


def test_member_sets_on_the_device(world):
    """one launch each over the match geometry (1,377 members: the literals
    pending, the distance and the length of one match on both sides of every
    64-lane pass, through all three index rules of WaveIO::match), the stored
    geometry (36: pending literals flushed by a stored block, a match across
    it) and the sizes (13: the CRC slices around 64 bytes and up to 65,536):
    every member's text in its slot, its status, the statistics of its one
    match, and the sentinels"""
    abi, ctx = world
    sets = {
        "geometry": [(m, t, dict(matches=1, max_distance=d, max_length=n, overlap=int(d < n), fixed_blocks=1,
                                 stored_blocks=0, dynamic_blocks=0)) for p, d, n, m, t in bz.geometry_members()],
        "stored_geometry": [(m, t, dict(matches=1, max_distance=d, max_length=n, overlap=int(d < n), fixed_blocks=2,
                                        stored_blocks=1, dynamic_blocks=0))
                            for p, s, d, n, m, t in bz.stored_members()],
        "sizes": [(m, t, {}) for n, m, t in bz.size_members()],
    }
    assert set(sets) == set(bz.MEMBER_SETS)
    for name, rows in sets.items():
        gz, text, want = bz.decode_cases()[name]
        assert gz == b"".join(m for m, _, _ in rows)
        rc, status, stats, members, buf = run_kernel(abi, ctx, gz)
        assert rc == 0 and not status["reason"].any(), (name, abi.last_error())
        assert len(members) == len(rows) and (status["out_len"] == members["out_len"]).all(), name
        sentinels_intact(members, buf, 16)
        for i, (m, t, st) in enumerate(rows):
            off = int(members["out_off"][i])
            assert buf[off:off + len(t)] == t and int(members["out_len"][i]) == len(t), (name, i)
            assert int(status["bit_pos"][i] + 7) // 8 == len(m) - 26, (name, i)
            check_stats(member_stats(stats, i), st, (name, i))


def corpus_members(abi, part):
    """the kernel's table for streams of bz.corpus(), back to back in one
    buffer: every member's slot is the stream's room (bz.corpus_room), with 16
    sentinel bytes in front and behind; the CRC is the text's for a stream
    zlib accepts (every 16th of them gets another, for reason 15) and
    arbitrary for the others"""
    rows, gz, out, accepted = [], bytearray(), 16, 0
    for raw, ok, text, _ in part:
        room, crc = bz.corpus_room(ok, text), 0x12345678
        if ok:
            crc = zlib.crc32(text) ^ (0x00010000 if accepted % 16 == 15 else 0)
            accepted += 1
        rows.append((len(gz), out, len(raw), room, crc, 0))
        gz += raw
        out += room + 16
    return np.array(rows, dtype=abi.GZ_MEMBER_DTYPE), bytes(gz), out


def test_device_against_host_against_zlib(world):
    """One launch over the first 512 streams of the mutated corpus, about half
    of which zlib rejects: one decoder under two policies, so for every member
    the kernel's reason, out_len, bit position and all eight statistics are
    what kgx_inflate_host returns for the same bytes and room -- but for
    reasons 14 and 15, which the kernel adds from the trailer where the stream
    itself is sound.  A slot zlib accepts holds zlib's text; another holds what
    the host produced before it failed and nothing behind it; no sentinel
    changed.  These are exactly the bytes and rooms that
    tests/test_inflate_native.py ran on the CPU, plain and under ASan/UBSan
    (its first 512 corpus streams; tests/test_gunzip_host.py runs the same
    through the library): that passes before this is given to the kernel.
    This test shows rejection; it is not here to find a fault."""
    abi, ctx = world
    part = bz.corpus()[:512]
    members, gz, room = corpus_members(abi, part)
    d_gz, d_out = DeviceBytes(abi, gz), DeviceBytes(abi, b"\xa5" * room)
    try:
        rc, status, stats, ms = abi.gunzip_device(ctx, d_gz.p, members, d_out.p)
        buf = d_out.read()
    finally:
        d_gz.free()
        d_out.free()
    assert rc == abi.KGX_EFORMAT
    sentinels_intact(members, buf, 16)
    seen = set()
    for i, (raw, ok, text, _) in enumerate(part):
        off, n = int(members["out_off"][i]), int(members["out_len"][i])
        h_rc, h_out, h_used, h_st, h_reason, h_bit = abi.inflate_host(raw, n)
        assert (h_reason == 0) == ok, i
        want = h_reason
        if h_reason == 0 and len(h_out) != n:
            want = bz.OUTPUT_SHORT
        elif h_reason == 0 and zlib.crc32(h_out) != int(members["crc"][i]):
            want = bz.CRC
        got = (int(status["reason"][i]), int(status["out_len"][i]), int(status["bit_pos"][i]))
        assert got == (want, len(h_out), h_bit), (i, got, (want, len(h_out), h_bit))
        assert member_stats(stats, i) == h_st, (i, member_stats(stats, i), h_st)
        assert buf[off:off + len(h_out)] == h_out, i
        assert buf[off + len(h_out):off + n] == b"\xa5" * (n - len(h_out)), i
        if ok:
            assert h_out == text, i
        seen.add(want)
    print(f"device against host: {len(part)} members, reasons {sorted(seen)}")
    # accepted, refused by the trailer alone, and refused by the stream
    assert {0, bz.CRC} <= seen and seen - {0, bz.OUTPUT_SHORT, bz.CRC}, seen


def test_error_cases_on_the_device(world):
    """a failing member between two good ones: its reason and index, the
    neighbours' text, what it produced before it failed, and nothing outside
    the slots"""
    abi, ctx = world
    first, last = b"first member\n", b"last member\n"
    prefixes = bz.error_case_prefixes()
    for name, (member, reason) in bz.error_cases().items():
        body = bz.bgzf(first, eof=False) + member + bz.bgzf(last, eof=False)
        rc, status, stats, members, buf = run_kernel(abi, ctx, body)
        assert rc == abi.KGX_EFORMAT, name
        assert list(status["reason"]) == [0, reason, 0], (name, list(status["reason"]))
        assert "member 1:" in abi.last_error() and f"reason {reason}" in abi.last_error(), name
        assert int(status["bit_pos"][1]) <= 8 * int(members["in_len"][1]), name
        assert buf[int(members["out_off"][0]):][:len(first)] == first, name
        assert buf[int(members["out_off"][2]):][:len(last)] == last, name
        if name in prefixes:
            assert int(status["out_len"][1]) == len(prefixes[name]), (name, int(status["out_len"][1]))
            assert buf[int(members["out_off"][1]):][:len(prefixes[name])] == prefixes[name], name
        sentinels_intact(members, buf, 16)
        for device in (1, 0):
            ctx.set_option("gunzip_device", device)
            with pytest.raises(abi.KgxError) as e:
                abi.gunzip(ctx, body)
            assert e.value.code == abi.KGX_EFORMAT and "member 1:" in str(e.value) and \
                f"reason {reason}" in str(e.value), (name, device)
    ctx.set_option("gunzip_device", 0)
    for name, (body, reason) in bz.framing_error_cases().items():
        with pytest.raises(abi.KgxError) as e:
            abi.gunzip(ctx, body)
        assert e.value.code == abi.KGX_EFORMAT and f"reason {reason}" in str(e.value), name


def test_every_truncation_of_a_200_byte_member_on_the_device(world):
    """174 members in one launch, member k holding the first k bytes of the
    deflate data: every one fails, none writes outside its slot"""
    abi, ctx = world
    m, data = bz.member_200()
    raw, n = m[18:-8], len(data)
    rows = [(0, 16 + k * (n + 16), k, n, zlib.crc32(data), 0) for k in range(len(raw))]
    members = np.array(rows, dtype=abi.GZ_MEMBER_DTYPE)
    d_gz, d_out = DeviceBytes(abi, raw), DeviceBytes(abi, b"\xa5" * (16 + len(raw) * (n + 16)))
    try:
        rc, status, stats, ms = abi.gunzip_device(ctx, d_gz.p, members, d_out.p)
        buf = d_out.read()
    finally:
        d_gz.free()
        d_out.free()
    assert rc == abi.KGX_EFORMAT and status["reason"].all()
    assert (status["bit_pos"] <= 8 * members["in_len"]).all()
    sentinels_intact(members, buf, 16)
    for k in range(len(raw)):  # what a member wrote before it failed is the text's beginning
        got = buf[rows[k][1]:rows[k][1] + int(status["out_len"][k])]
        assert got == data[:len(got)], k


def test_plain_members_and_room(world):
    abi, ctx = world
    ctx.set_option("gunzip_device", 1)
    for name, (gz, text) in bz.plain_cases().items():
        out, consumed, st = abi.gunzip(ctx, gz, cap=len(text))
        assert out == text and consumed == len(gz) and st["plain_members"] >= 1, name
    gz, text, _ = bz.decode_cases()["golden_l6_c1000_eof"]
    with pytest.raises(abi.KgxError) as e:
        abi.gunzip(ctx, gz, cap=len(text) - 1)
    assert e.value.code == abi.KGX_ERANGE


@pytest.mark.parametrize("step", (1, 17, 4096))
def test_streaming_equals_one_block(world, step):
    abi, ctx = world
    ctx.set_option("gunzip_device", 1)
    g = bz.golden()
    gz = bz.bgzf(g, chunk=1000)
    if step == 1:  # a member and a half of single bytes, then the rest in one block
        first = int.from_bytes(gz[16:18], "little") + 1
        blocks = [gz[i:i + 1] for i in range(first + first // 2)] + [gz[first + first // 2:]]
    else:
        blocks = [gz[i:i + step] for i in range(0, len(gz), step)]
    ends, at = {0}, 0
    while at < len(gz):
        at += int.from_bytes(gz[at + 16:at + 18], "little") + 1
        ends.add(at)
    tail, out, taken = b"", [], 0
    for i, blk in enumerate(blocks):
        tail += blk
        text, consumed, _ = abi.gunzip(ctx, tail, finished=i == len(blocks) - 1, cap=len(g))
        taken += consumed
        assert taken in ends
        out.append(text)
        tail = tail[consumed:]
    assert b"".join(out) == g and taken == len(gz)
