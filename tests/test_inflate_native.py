"""The DEFLATE decoder and the gzip framing (csrc/kgx_inflate.h, kgx_gzip.h) on
the host, through tests/native/inflate_check.cpp: every decode case byte for
byte with the statistics that show it hit its target, every error case with
its reason, the sliced CRC against zlib.crc32, and every truncation of a
200-byte member.  The program is built twice, plain and with
-fsanitize=address,undefined, and both runs must say the same; inputs and
outputs live in heap blocks of exactly their size, so a step outside them is a
sanitizer report.  These cases pass here before the GPU tests hand the same
bytes to the kernel.  No GPU."""
import os
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
    add("trunc", "trunc_200", bz.member_200()[0])
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
                       ("crc_65536", (bz.golden() * 4)[:65536])):
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


def test_fixtures_are_what_their_names_say():
    """zlib's own reading of the fixtures: gzip.decompress takes the BGZF
    writer's output, and the first member's block-type bits are 0 / 2 / 2 / 2 / 1"""
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
