"""fastq_to_protein on the CPU: the restatement (tests/f2p_restate.py) against
the oracle's fragments, the stop-at-error FASTQ parser (csrc/kgx_fq_parse.h)
against the restatement through tests/native/fq_parse_check.cpp -- built with
the address and undefined-behaviour sanitizers and run directly -- the fq
handler's parser on the same malformed inputs, the text-or-gzip sniff of
csrc/kgx_gzip.h through the same program, and the command line.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import f2p_restate
from tests_golden_codons import back_translate, revcomp

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fq_parse_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "fq_parse_check")

A11, B11 = "MKTAYIAKQRQ", "GSHMLEDPVRW"  # 11 residues each

# translation -> the indices of its records (DESIGN.md §8.11's rules, worked)
WORKED = [(A11, [1]), ("*" + A11, [2]), ("***" + A11, [2]), (A11 + "**" + B11 + "*", [1, 2]),
          ("MKT*" + B11, [2]), ("*", []), ("", [])]


def _random_reads(rng, n):
    """The alphabet of tests/test_gpu_fq.py::_random_reads."""
    alphabet = np.frombuffer(b"ACGTACGTACGTacgtNnUuRYKMSWBDHVX.-", np.uint8)
    reads = []
    for i in range(n):
        L = int(rng.integers(0, 320)) if i % 7 else int(rng.integers(0, 12))
        pool = alphabet if i % 3 == 0 else np.frombuffer(b"ACGT", np.uint8)
        reads.append(bytes(pool[rng.integers(0, len(pool), L)]))
    return reads


def test_restatement_matches_oracle_fragments(oracle_lib):
    """Per read the restatement's kept (frame, token) list is the oracle's
    fq_fragments, and each frame's indices ascend."""
    rng = np.random.default_rng(5)
    n = 0
    for dna in _random_reads(rng, 400):
        k = f2p_restate.kept(dna, oracle_lib.translate11)
        assert [(f, t) for f, _, t in k] == oracle_lib.fq_fragments(dna)
        for f in f2p_restate.FRAMES:
            idx = [i for g, i, _ in k if g == f]
            assert idx == sorted(set(idx))
        n += len(k)
    assert n > 300


@pytest.mark.parametrize("frame", [1, 3, -1, -2])
def test_restatement_worked_cases(oracle_lib, frame):
    rng = np.random.default_rng(6)
    for prot, want in WORKED:
        dna = "ACGT"[:abs(frame) - 1] + back_translate(prot, rng)
        dna = dna if frame > 0 else revcomp(dna)
        k = [x for x in f2p_restate.kept(dna.encode(), oracle_lib.translate11) if x[0] == frame]
        assert [i for _, i, _ in k] == want, (prot, frame)
        assert [(f, t) for f, _, t in f2p_restate.kept(dna.encode(), oracle_lib.translate11)] == \
            oracle_lib.fq_fragments(dna.encode())
    assert f2p_restate.read_text(b"r1", back_translate("*" + A11, rng).encode(), oracle_lib.translate11) \
        .startswith(b">r1:1:2\n" + A11.encode() + b"\n")


def _build_check():
    from close_kmers_amd import build as kbuild
    deps = [SRC] + [os.path.join(kbuild.CSRC, h) for h in ("kgx_fq_parse.h", "kgx_gzip.h", "kgx_inflate.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return OUT


def _run_check(tmp_path, text: bytes, block: int, mode: str):
    p = tmp_path / "in.fq"
    p.write_bytes(text)
    r = subprocess.run([_build_check(), str(p), str(block), mode], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    records, error = [], None
    for line in r.stdout.split(b"\n")[:-1]:
        f = line.split(b"\t")
        if f[0] == b"R":
            records.append((f[1], f[2]))
        else:
            error = (int(f[1]), f[2], b"\t".join(f[3:]).decode("latin-1"))
    return records, error


_GOOD = [(b"r1", b"ACGTACGTAC"), (b"r2", b"TTGACCA"), (b"r3", b"GGGCCCAAATTT"), (b"r4", b"ACGT"), (b"r5", b"TTTT")]
_WELL = f2p_restate.fastq_of(_GOOD)
PARSER_INPUTS = {
    "well_formed": _WELL,
    "no_final_newline": _WELL[:-1],
    "no_final_newline_in_bases": _WELL[:_WELL.rindex(b"\n+")],
    "crlf": _WELL.replace(b"\n", b"\r\n"),
    "fasta_first": b">r1\nACGT\n" + _WELL,
    "missing_plus": f2p_restate.fastq_of(_GOOD[:2]) + b"@r3\nGGGCCC\nIIIIII\n" + f2p_restate.fastq_of(_GOOD[3:]),
    "bad_character_in_third": f2p_restate.fastq_of(_GOOD[:2]) + b"@r3\nGGGC-CAAATTT\n+\nIIIIIIIIIIII\n" +
    f2p_restate.fastq_of(_GOOD[3:]),
    "blank_first_in_header": f2p_restate.fastq_of(_GOOD[:1]) + b"@ r2 after a blank\nTTGACCA\n+\nIIIIIII\n" +
    f2p_restate.fastq_of(_GOOD[2:]),
    "id_with_description": b"@r1 len=10 x\tz\nACGTACGTAC\n+r1 again\nIIIIIIIIII\n" + f2p_restate.fastq_of(_GOOD[1:]),
    "blank_line_between_records": f2p_restate.fastq_of(_GOOD[:2]) + b"\n" + f2p_restate.fastq_of(_GOOD[2:]),
    "empty": b"",
}


@pytest.mark.parametrize("name", sorted(PARSER_INPUTS))
def test_strict_parser_matches_restatement(tmp_path, name):
    """The records the tool translates (ids not empty) and the error, in
    blocks of 1, 7 and 4096 bytes."""
    text = PARSER_INPUTS[name]
    want_records, want_error = f2p_restate.parse(text)
    want = [r for r in want_records if r[0]]
    for block in (1, 7, 4096):
        records, error = _run_check(tmp_path, text, block, "strict")
        assert [r for r in records if r[0]] == want, (name, block)
        if want_error is None:
            assert error is None, (name, block)
        else:
            assert error == (want_error[1], want_error[2], f2p_restate.error_report(want_error)), (name, block)
    # what each input is there for
    ids = [r[0] for r in want]
    expect = {"well_formed": ([b"r1", b"r2", b"r3", b"r4", b"r5"], None),
              "no_final_newline": ([b"r1", b"r2", b"r3", b"r4", b"r5"], None),
              "no_final_newline_in_bases": ([b"r1", b"r2", b"r3", b"r4", b"r5"], None),
              "crlf": ([b"r1\r"], 2), "fasta_first": ([], 1), "missing_plus": ([b"r1", b"r2", b"r3"], 11),
              "bad_character_in_third": ([b"r1", b"r2", b"r3"], 10),
              "blank_first_in_header": ([b"r1", b"r3", b"r4", b"r5"], None),
              "id_with_description": ([b"r1", b"r2", b"r3", b"r4", b"r5"], None),
              "blank_line_between_records": ([b"r1", b"r2"], 10), "empty": ([], None)}[name]
    assert ids == expect[0] and (want_error[1] if want_error else None) == expect[1]
    if name == "bad_character_in_third":
        assert want[2] == (b"r3", b"GGGC")
    if name == "no_final_newline_in_bases":
        assert want[4] == (b"r5", b"TTTT")


@pytest.mark.parametrize("name", sorted(PARSER_INPUTS))
def test_handler_parser_still_parses_past_errors(tmp_path, name):
    """fq_parse as FqRequest drives it: an offending byte is dropped and the
    parse goes on; only records ended by their quality line are emitted."""
    text = PARSER_INPUTS[name]
    want, _ = f2p_restate.parse(text, stop_at_error=False)
    for block in (1, 7, 4096):
        records, error = _run_check(tmp_path, text, block, "handler")
        assert records == want and error is None, (name, block)
    if name in ("bad_character_in_third", "blank_line_between_records"):
        assert [r[0] for r in want][-2:] == [b"r4", b"r5"]  # the records after the error are still there
    if name == "missing_plus":  # r3 waits for a '+': r4's, whose quality line then ends r3
        assert [r[0] for r in want] == [b"r1", b"r2", b"r3", b"r5"]
    if name == "bad_character_in_third":
        assert want[2] == (b"r3", b"GGGCCAAATTT")


_GZ = bytes([0x1f, 0x8b, 0x08])
# (the body's first bytes, finished, fresh) -> the sniff's decision, by the
# rules of the fq handler and fastq_to_protein: a first byte other than 1f, an
# empty body or a parser not at a fresh start is text; 1f 8b 08 is gzip, but
# with fewer than gzip's 10 header bytes it is held while more may come; fewer
# than 3 bytes starting with 1f are held while more may come, text otherwise
SNIFF_CASES = [
    (b"", 0, 1, "TEXT"), (b"", 1, 1, "TEXT"),
    (b"\x1f", 0, 1, "HELD"), (b"\x1f", 1, 1, "TEXT"),
    (b"\x1f\x8b", 0, 1, "HELD"), (b"\x1f\x8b", 1, 1, "TEXT"),
    (b"\x1f\x8c", 0, 1, "HELD"), (b"\x1f\x8c", 1, 1, "TEXT"),
    (_GZ, 0, 1, "HELD"), (_GZ, 1, 1, "GZIP"),
    (_GZ + bytes(1), 0, 1, "HELD"), (_GZ + bytes(1), 1, 1, "GZIP"),
    (_GZ + bytes(2), 0, 1, "HELD"), (_GZ + bytes(2), 1, 1, "GZIP"),
    (_GZ + bytes(3), 0, 1, "HELD"), (_GZ + bytes(3), 1, 1, "GZIP"),
    (_GZ + bytes(4), 0, 1, "HELD"), (_GZ + bytes(4), 1, 1, "GZIP"),
    (_GZ + bytes(5), 0, 1, "HELD"), (_GZ + bytes(5), 1, 1, "GZIP"),
    (_GZ + bytes(6), 0, 1, "HELD"), (_GZ + bytes(6), 1, 1, "GZIP"),
    (_GZ + bytes(7), 0, 1, "GZIP"), (_GZ + bytes(7), 1, 1, "GZIP"),
    (_GZ + bytes(9), 0, 1, "GZIP"), (_GZ + bytes(9), 1, 1, "GZIP"),
    (b"\x1f\x8b\x07", 0, 1, "TEXT"), (b"\x1f\x8b\x07", 1, 1, "TEXT"),
    (b"\x1f\x8b\x07" + bytes(7), 0, 1, "TEXT"), (b"\x1f\x8c\x08" + bytes(7), 1, 1, "TEXT"),
    (b"@r1\nACGT\n+\nIIII\n", 0, 1, "TEXT"), (b"@", 0, 1, "TEXT"), (b"@r1\nACGT\n+\nIIII\n", 1, 1, "TEXT"),
    (b"\x1f", 0, 0, "TEXT"), (_GZ, 0, 0, "TEXT"), (_GZ + bytes(7), 0, 0, "TEXT"), (_GZ + bytes(7), 1, 0, "TEXT"),
]


def test_gzip_sniff_decisions():
    """gzip_sniff (csrc/kgx_gzip.h), the one sniff of the fq handler and
    fastq_to_protein: the table above, with the bytes split between the held
    start and the new block at every position."""
    args, want = [], []
    for data, finished, fresh, decision in SNIFF_CASES:
        for cut in range(len(data) + 1):
            args += [data[:cut].hex() or "-", data[cut:].hex() or "-", str(finished), str(fresh)]
            want.append(decision)
    r = subprocess.run([_build_check(), "sniff"] + args, capture_output=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.decode().split() == want
    assert {"HELD", "TEXT", "GZIP"} == set(want)


def test_command_line_parsing():
    from close_kmers_amd import fastq_to_protein as f2p
    a = f2p.parse_args(["reads.fq"])
    assert (a.fastq, a.output, a.device, a.data, a.part_bytes) == ("reads.fq", None, 0, None, 0)
    a = f2p.parse_args(["-o", "out.faa", "reads.fq.gz", "--device", "3", "--data", "/d", "--part-bytes", "4096"])
    assert (a.fastq, a.output, a.device, a.data, a.part_bytes) == ("reads.fq.gz", "out.faa", 3, "/d", 4096)
    assert f2p.parse_args(["--output-file", "o", "x"]).output == "o"
    for bad in ([], ["a", "b"], ["a", "--part-bytes", "-1"], ["a", "--device", "x"]):
        with pytest.raises(SystemExit):
            f2p.parse_args(bad)
