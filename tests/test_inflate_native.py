"""The DEFLATE decoder and the gzip framing (csrc/kgx_inflate.h, kgx_gzip.h) on
the host, through tests/native/inflate_check.cpp: every decode case byte for
byte with the statistics that show it hit its target, every error case with
its reason (every reason 1..15 by a member assembled by hand, with the message
zlib has for the same stream), the sliced CRC against zlib.crc32 at sizes
around the 64 slices, every truncation of a 200-byte member, the match and
stored geometry member by member with the statistics of each one's match, and
3,000 seeded streams, most of them corrupted, against zlib's verdict, bytes
and input consumed (the checker's `pack` mode: many streams from one file).
The program is built twice, plain and with
-fsanitize=address,undefined, and both runs must say the same; inputs and
outputs live in heap blocks of exactly their size, so a step outside them is a
sanitizer report.  These cases pass here before the GPU tests hand the same
bytes to the kernel.  No GPU."""
import collections
import os
import struct
import subprocess
import zlib

import pytest

import bgzf_util as bz
from close_kmers_amd import build as kbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "inflate_check.cpp")
BUILD = os.path.join(HERE, "native", "_build")
STATS = ("stored_blocks", "fixed_blocks", "dynamic_blocks", "max_code_len", "max_distance", "max_length", "overlap",
         "matches")


def _build(name, flags):
    out = os.path.join(BUILD, name)
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_inflate.h"), os.path.join(kbuild.CSRC, "kgx_gzip.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(BUILD, exist_ok=True)
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-g", *flags, f"-I{kbuild.CSRC}", SRC, "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return out


def check_stats(got, want, name):
    """want: field -> value, or ("ge", value)"""
    for k, v in want.items():
        if isinstance(v, tuple):
            assert got[k] >= v[1], (name, k, got[k], v)
        else:
            assert got[k] == v, (name, k, got[k], v)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every case through both builds: {build: {case: (fields, output bytes)}}"""
    d = tmp_path_factory.mktemp("inflate")
    lines, names = [], []

    def add(mode, name, data, cap=0):
        with open(d / f"{name}.in", "wb") as f:
            f.write(data)
        lines.append(f"{mode} {d / (name + '.in')} {d / (name + '.out')} {cap}")
        names.append(name)

    for name, (gz, text, _) in bz.decode_cases().items():
        add("gz", name, gz)
    for name, (gz, text) in bz.plain_cases().items():
        add("gz", name, gz, len(text))
    for name, (gz, _) in bz.error_cases().items():
        add("gz", "err_" + name, bz.bgzf(b"first member\n", eof=False) + gz + bz.bgzf(b"last member\n", eof=False))
    for name, (gz, _) in bz.framing_error_cases().items():
        add("gz", "frame_" + name, gz)
    add("raw", "raw_golden", bz.raw_deflate(bz.golden()), len(bz.golden()))
    add("raw", "raw_golden_tight", bz.raw_deflate(bz.golden()), len(bz.golden()) - 1)
    add("crc", "crc_golden", bz.golden())
    add("crc", "crc_empty", b"")
    add("crc", "crc_63", bz.golden()[:63])
    add("crc", "crc_65536", (bz.golden() * 4)[:65536])
    for n in CRC_SIZES:
        add("crc", f"crc_n{n}", crc_text(n))
    add("trunc", "trunc_200", bz.member_200()[0])
    add("pack", "pack_corpus", pack((raw, bz.corpus_room(ok, text)) for raw, ok, text, _ in bz.corpus()))
    add("pack", "pack_geometry", pack((m[18:-8], len(t)) for *_, m, t in bz.geometry_members()))
    add("pack", "pack_errors", pack((m[18:-8], int.from_bytes(m[-4:], "little")) for m, _ in bz.error_cases().values()))
    add("pack", "pack_stored", pack((m[18:-8], len(t)) for *_, m, t in bz.stored_members()))
    with open(d / "cases.txt", "w") as f:
        f.write("\n".join(lines) + "\n")
    out = {}
    for build, flags in (("plain", ["-O2"]), ("sanitized", ["-O1", "-fsanitize=address,undefined",
                                                           "-fno-sanitize-recover=all"])):
        exe = _build("inflate_check" + ("" if build == "plain" else "_san"), flags)
        r = subprocess.run([exe, str(d / "cases.txt")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (build, r.stdout[-2000:], r.stderr[-4000:])
        assert r.stderr == "", (build, r.stderr[-4000:])
        got = r.stdout.splitlines()
        assert len(got) == len(names), (build, r.stdout[-2000:])
        res = {}
        for name, line in zip(names, got):
            p = d / f"{name}.out"
            res[name] = (line.split(), p.read_bytes() if p.exists() else b"")
            if p.exists():
                p.unlink()
        out[build] = res
    return out


CRC_SIZES = (1, 2, 62, 64, 65, 127, 128, 129, 4095, 4096, 4097, 65535)


def crc_text(n):
    return bytes(bz.literal_value(i) for i in range(n))


def pack(streams):
    """the checker's `pack` input: {u32 length, u32 room, bytes} per stream"""
    return b"".join(struct.pack("<II", len(raw), room) + raw for raw, room in streams)


def unpack(blob):
    """the checker's `pack` output: [(fields, the bytes produced)]"""
    out, at = [], 0
    while at < len(blob):
        v = struct.unpack_from("<IIQ8I", blob, at)
        at += 48
        out.append((dict(reason=v[0], out_len=v[1], bit=v[2], **dict(zip(STATS, v[3:]))), blob[at:at + v[1]]))
        at += v[1]
    return out


def _gz_fields(f):
    assert f[0] == "gz"
    v = [int(x) for x in f[1:]]
    return dict(reason=v[0], member=v[1], bit=v[2], out_len=v[3], members=v[4], blocked=v[5],
                **dict(zip(STATS, v[6:])))


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_decode_cases(runs, build):
    for name, (gz, text, want) in bz.decode_cases().items():
        f, out = runs[build][name]
        got = _gz_fields(f)
        assert got["reason"] == 0, (name, got)
        assert out == text, name
        assert got["blocked"] == got["members"], name
        check_stats(got, want, name)


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_plain_members(runs, build):
    for name, (gz, text) in bz.plain_cases().items():
        f, out = runs[build][name]
        got = _gz_fields(f)
        assert got["reason"] == 0 and out == text, (name, got)
        assert got["blocked"] < got["members"], name


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_error_cases(runs, build):
    """the failing member is the middle one of three: its reason and index are
    reported and the two others' text is intact"""
    for name, (gz, reason) in bz.error_cases().items():
        f, out = runs[build]["err_" + name]
        got = _gz_fields(f)
        assert (got["reason"], got["member"]) == (reason, 1), (name, got)
        assert out.startswith(b"first member\n") and out.endswith(b"last member\n"), name
        middle = out[len(b"first member\n"):len(out) - len(b"last member\n")]
        assert middle == b"\xa5" * len(middle), name
    for name, (gz, reason) in bz.framing_error_cases().items():
        got = _gz_fields(runs[build]["frame_" + name][0])
        assert (got["reason"], got["member"]) == (reason, 0), (name, got)
    # the deflate data alone in a room of ISIZE: the stream's reason (none where the trailer fails), the
    # bit position inside the data, and the bytes produced before the failure
    alone = unpack(runs[build]["pack_errors"][1])
    assert len(alone) == len(bz.error_cases())
    for (name, (gz, reason)), (g, out) in zip(bz.error_cases().items(), alone):
        assert g["reason"] == (0 if reason in (bz.OUTPUT_SHORT, bz.CRC) else reason), (name, g)
        assert g["bit"] <= 8 * (len(gz) - 26), (name, g)
        if name in bz.error_case_prefixes():
            assert out == bz.error_case_prefixes()[name], (name, out)


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_raw_stream_and_room(runs, build):
    f, out = runs[build]["raw_golden"]
    raw = bz.raw_deflate(bz.golden())
    assert f[0] == "raw" and int(f[1]) == 0 and out == bz.golden()
    assert int(f[4]) == len(raw) and int(f[2]) <= 8 * len(raw)
    f, out = runs[build]["raw_golden_tight"]
    assert int(f[1]) == bz.OUTPUT_FULL and out == bz.golden()[:len(out)] and len(out) <= len(bz.golden()) - 1


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_sliced_crc_is_zlib_crc32(runs, build):
    for name, data in (("crc_golden", bz.golden()), ("crc_empty", b""), ("crc_63", bz.golden()[:63]),
                       ("crc_65536", (bz.golden() * 4)[:65536]), *((f"crc_n{n}", crc_text(n)) for n in CRC_SIZES)):
        f, _ = runs[build][name]
        assert f[0] == "crc"
        assert int(f[1], 16) == zlib.crc32(data), name
        assert int(f[2], 16) == zlib.crc32(data), name


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_every_truncation_of_a_200_byte_member(runs, build):
    m, data = bz.member_200()
    assert len(m) == 200
    f, _ = runs[build]["trunc_200"]
    assert f[0] == "trunc" and int(f[1]) == 200 - 26
    assert int(f[2]) == int(f[1]) and int(f[3]) == 0


def check_corpus_stream(i, entry, got, out):
    """what is required of every stream of the corpus: `got` and `out` are the
    decoder's result and bytes for entry i of bz.corpus() in its room"""
    raw, ok, text, used = entry
    room = bz.corpus_room(ok, text)
    assert (got["reason"] == 0) == ok, (i, got, ok)
    assert got["out_len"] == len(out) <= room and got["bit"] <= 8 * len(raw), (i, got)
    if ok:
        assert out == text and (got["bit"] + 7) // 8 == used, (i, got, used)
    else:
        assert out == text[:len(out)], (i, got, len(text))


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_mutated_corpus_against_zlib(runs, build):
    """3,000 seeded streams, most of them bit-flipped or cut (bgzf_util.
    mutated_corpus): accepted iff zlib accepts; then zlib's bytes and zlib's
    input consumed; else no more than the room, no bit position past the input,
    and a prefix of what zlib produced before it failed.  The corpus is kept
    honest on zlib's verdicts: a quarter at least on either side, and six
    decoder reasons at least reached by mutation alone."""
    corpus = bz.corpus()
    f, blob = runs[build]["pack_corpus"]
    got = unpack(blob)
    assert f == ["pack", str(len(corpus)), str(sum(1 for c in corpus if c[1])), str(sum(1 for c in corpus if not c[1]))]
    assert len(got) == len(corpus) == bz.CORPUS_N
    balanced, accepted = bz.corpus_verdicts_are_balanced(corpus)
    reasons = collections.Counter(g["reason"] for g, _ in got)
    print(f"corpus: {len(corpus)} streams, zlib accepts {accepted} ({100 * accepted // len(corpus)}%), "
          f"decoder reasons {dict(sorted(reasons.items()))}")
    assert balanced, accepted
    for i, (entry, (g, out)) in enumerate(zip(corpus, got)):
        check_corpus_stream(i, entry, g, out)
    assert len([r for r in reasons if r]) >= 6, reasons


@pytest.mark.parametrize("build", ("plain", "sanitized"))
def test_member_sets_member_by_member(runs, build):
    """every member of the match and stored geometry alone in a room of its
    text's size: the text, and the statistics of its one match"""
    got = unpack(runs[build]["pack_geometry"][1])
    geo = bz.geometry_members()
    assert len(got) == len(geo) == 1377
    for (p, dist, length, m, text), (g, out) in zip(geo, got):
        assert g["reason"] == 0 and out == text, (p, dist, length, g)
        assert (g["matches"], g["max_distance"], g["max_length"], g["overlap"], g["fixed_blocks"]) == \
            (1, dist, length, int(dist < length), 1), (p, dist, length, g)
        assert (g["bit"] + 7) // 8 == len(m) - 26
    got = unpack(runs[build]["pack_stored"][1])
    sto = bz.stored_members()
    assert len(got) == len(sto) == 36
    for (p, s, dist, length, m, text), (g, out) in zip(sto, got):
        assert g["reason"] == 0 and out == text, (p, s, g)
        assert (g["matches"], g["max_distance"], g["max_length"], g["stored_blocks"], g["fixed_blocks"]) == \
            (1, dist, length, 1, 2), (p, s, g)


def test_both_builds_say_the_same(runs):
    """the sanitized run's lines and bytes are the plain run's"""
    assert runs["plain"].keys() == runs["sanitized"].keys()
    for name, plain in runs["plain"].items():
        assert plain == runs["sanitized"][name], name


def test_fixtures_are_what_their_names_say():
    """zlib's own reading of the fixtures: gzip.decompress takes the BGZF
    writer's output, and the first member's block-type bits are 0 / 2 / 2 / 2 / 1;
    zlib decodes every decode case to its text (the member sets member by
    member), refuses the deflate data of every error case with the message
    recorded for it, or takes it where the failure is the trailer's or the
    input's end, and produces before a failure what error_case_prefixes says"""
    import gzip
    g = bz.golden()
    assert len(g) == 19261
    for level, strategy, btype in ((0, zlib.Z_DEFAULT_STRATEGY, 0), (1, zlib.Z_DEFAULT_STRATEGY, 2),
                                   (6, zlib.Z_DEFAULT_STRATEGY, 2), (9, zlib.Z_DEFAULT_STRATEGY, 2),
                                   (6, zlib.Z_FIXED, 1)):
        b = bz.bgzf(g, level, strategy)
        assert gzip.decompress(b) == g
        assert (b[18] >> 1) & 3 == btype
    assert gzip.decompress(bz.BGZF_EOF) == b"" and len(bz.BGZF_EOF) == 28
    for name, (gz, text, _) in bz.decode_cases().items():
        assert gzip.decompress(gz) == text, name
    for name, (gz, text) in bz.plain_cases().items():
        if name != "plain_trailing":
            assert gzip.decompress(gz) == text, name
    for *_, m, text in list(bz.geometry_members()) + list(bz.stored_members()) + list(bz.size_members()):
        assert len(m) <= 65536 and gzip.decompress(m) == text
        assert bz.zlib_inflate(m[18:-8]) == (True, text, len(m) - 26, "")
    assert [len(t) for _, _, t in bz.size_members()] == list(bz.SIZES)
    assert set(bz.error_cases()) == set(bz.ZLIB_MESSAGES)
    assert {r for _, r in bz.error_cases().values()} == set(range(1, 16))
    for name, (m, reason) in bz.error_cases().items():
        raw, isize, message = m[18:-8], int.from_bytes(m[-4:], "little"), bz.ZLIB_MESSAGES[name]
        ok, out, used, msg = bz.zlib_inflate(raw)
        if message is None:  # zlib has no complaint: the trailer does not fit, or the input ends
            assert msg == "" and (ok or reason == bz.INPUT_END), name
            if ok:
                assert len(out) != isize or zlib.crc32(out) != int.from_bytes(m[-8:-4], "little"), name
        else:
            assert not ok and message in msg, (name, msg)
        if name in bz.error_case_prefixes() and not ok:
            assert out == bz.error_case_prefixes()[name], name
    # the hand-made failing streams do not end where they fail (but for the one that must)
    for name in bz.ZLIB_MESSAGES:
        if bz.ZLIB_MESSAGES[name] and name not in ("bad_distance_bit_at_the_end", "block_type_3", "len_nlen",
                                                   "oversubscribed", "distance_before_start", "repeat_first",
                                                   "length_symbol_286", "distance_symbol_30"):
            raw = bz.error_cases()[name][0][18:-8]
            assert len(raw) - bz.zlib_inflate(raw)[2] >= 2, name
    for name, (body, blocked) in bz.gzip_header_variants().items():
        sound = "unterminated" not in name and "wrong" not in name
        assert (bz.zlib_gunzip(body) == bz.golden()[:3000]) == sound, name
