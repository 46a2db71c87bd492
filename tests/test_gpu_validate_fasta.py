"""close_kmers_amd.validate_fasta against the restatement of validate_fasta.cc
(tests/fa_restate.py): stdout and the "Error found" line on stderr, byte for
byte, at block sizes that carry tails and put the error in a later block; and
unique_prots --parse-device with its reader, fasta_device.read_records."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fa_restate
from close_kmers_amd import synth
from helpers import data_dir_for, synthetic_table

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _fasta(rng, lengths, eol=b"\n"):
    a = np.frombuffer(b"ACDEFGHIKLMNPQRSTVWY", np.uint8)
    out = []
    for k, n in enumerate(lengths):
        seq = bytes(a[rng.integers(0, 20, n)])
        out.append(b">p%d def %d" % (k, k) + eol + b"".join(seq[i:i + 60] + eol for i in range(0, n, 60)))
    return b"".join(out)


def cases():
    rng = np.random.default_rng(43)
    valid = _fasta(rng, [int(x) for x in rng.integers(0, 400, 120)])
    good = _fasta(rng, [50, 60, 70, 130])
    return {
        "valid": valid,
        "empty": b"",
        "single": _fasta(rng, [151]),
        "crlf": _fasta(rng, [50, 61, 120], eol=b"\r\n"),
        "no_final_newline": valid[:-1],
        "missing_gt": b"junk\n" + good,                              # line 1
        "bad_data": good + b">bd\nACDE\nAC-DE\n" + good,             # the third line after good
        "bad_id_or_data": good + b">bi\nACDE\n*ACDE\n" + good,
        "gt_after_header": good + b">h1\n>h2\nACDE\n" + good,
        "error_in_last_record": valid + b">last\nACDE\nFG HI\n",
        "error_in_record_without_id": good + b"> noid\nAC1DE\n",
        "without_ids": good + b">\nACDE\n> only a definition\nFGHI\n" + good,
    }


CASES = cases()
GOOD_LINES = 4 + 1 + 1 + 2 + 3  # the four records of `good`: headers and 60-column lines


def test_the_cases_are_what_they_are_meant_to_be():
    V = lambda name: fa_restate.validate_fasta(CASES[name])
    assert V("empty") == ("valid\t1\nn_seqs\t0\n", "")
    assert V("single")[0].endswith("stddev\t0.00\n") and V("single")[0].startswith("valid\t1\nn_seqs\t1\n")
    assert V("valid")[0].startswith("valid\t1\nn_seqs\t120\n") and V("valid") == V("no_final_newline")
    assert V("crlf")[0].startswith("valid\t1\nn_seqs\t3\ntotal_size\t231\n")
    assert V("without_ids")[0].startswith("valid\t1\nn_seqs\t8\n")
    assert V("missing_gt") == ("valid\t0\nn_seqs\t0\nerror_message\tMissing >\nerror_line\t1\n",
                               "Error found: Missing > at line 1 id=''\n")
    assert V("bad_data") == ("valid\t0\nn_seqs\t5\nerror_message\tBad data character '-'\nerror_line\t%d\n"
                             % (GOOD_LINES + 3), "Error found: Bad data character '-' at line %d id='bd'\n" % (GOOD_LINES + 3))
    assert V("bad_id_or_data")[1] == "Error found: Bad id or data character '*' at line %d id='bi'\n" % (GOOD_LINES + 3)
    assert V("gt_after_header")[1] == "Error found: Bad data character '>' at line %d id='h1'\n" % (GOOD_LINES + 2)
    assert "n_seqs\t121\nerror_message\tBad data character ' '\n" in V("error_in_last_record")[0]
    assert "n_seqs\t4\n" in V("error_in_record_without_id")[0] and V("error_in_record_without_id")[1].endswith("id=''\n")


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_validate_fasta(gpu, tmp_path, capfdbinary, name):
    from close_kmers_amd import validate_fasta
    data = CASES[name]
    p = tmp_path / (name + ".fa")
    p.write_bytes(data)
    want = tuple(s.encode("latin-1") for s in fa_restate.validate_fasta(data))
    for block in (["--block-bytes", "64"], ["--block-bytes", "4096"], []):
        capfdbinary.readouterr()
        assert validate_fasta.main([str(p)] + block) == 0
        got = capfdbinary.readouterr()
        assert (got.out, got.err) == want, block


@pytest.mark.gpu
def test_command_line_stdin(gpu):
    data = CASES["bad_data"]
    r = subprocess.run([sys.executable, "-m", "close_kmers_amd.validate_fasta", "-", "--block-bytes", "1000"], input=data,
                       capture_output=True, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert (r.stdout, r.stderr) == tuple(s.encode("latin-1") for s in fa_restate.validate_fasta(data))


@pytest.mark.gpu
def test_read_records_and_unique_prots(gpu, oracle_lib, tmp_path):
    from close_kmers_amd import fasta_device, unique_prots
    spec, table = synthetic_table(20000)
    # where the host reader and the reference's parser differ
    odd = b">a one\r\nACDE\r\nFG*HI\r\n> x\r\nKLMN\r\n>b\r\nPQ\r\n\r\nRS\r\n>c"
    p = tmp_path / "odd.fa"
    p.write_bytes(odd)
    want = [tuple(f.encode("latin-1") for f in ln.split("\t")) for ln in oracle_lib.fasta_parse(odd).splitlines()]
    assert want == [(b"a", b"ACDEFG*HI"), (b"", b"KLMN"), (b"b", b"PQRS"), (b"c", b"")]
    res, off = synth.make_queries(spec, 60)
    recs = [(b"prot%d" % k, res[int(off[k]):int(off[k + 1])].tobytes()) for k in range(60)]
    recs += recs[3:9]  # proteins with the same k-mer set: groups of more than one
    well = b"".join(b">" + i + b"x%d\n" % n + b"".join(s[k:k + 60] + b"\n" for k in range(0, len(s), 60))
                    for n, (i, s) in enumerate(recs))
    q = tmp_path / "well.fa"
    q.write_bytes(well)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        for block in (7, 64, 1 << 20):
            assert fasta_device.read_records(ctx, str(p), block) == want
        got = fasta_device.read_records(ctx, str(q), 1000)
        assert got == [(i + b"x%d" % n, s) for n, (i, s) in enumerate(recs)]
    data = data_dir_for(str(tmp_path / "data"), table)
    outs = [str(tmp_path / "host.txt"), str(tmp_path / "device.txt")]
    assert unique_prots.main([data, str(q), "--output", outs[0]]) == 0
    assert unique_prots.main([data, str(q), "--output", outs[1], "--parse-device"]) == 0
    host, device = (open(o, "rb").read() for o in outs)
    assert host == device and host.count(b"\t") == len(recs) and 0 < host.count(b"\n") < len(recs)
