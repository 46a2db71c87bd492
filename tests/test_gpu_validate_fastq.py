"""python -m close_kmers_amd.validate_fastq as a subprocess against a
restatement of validate_fastq.cc (:14-107) over tests/f2p_restate.py's parser:
stdout and the "Error found" line on stderr, byte for byte."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import f2p_restate

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def restate(fastq: bytes):
    """(stdout, stderr) of validate_fastq.cc for the file's bytes: the callback
    counts the records that have an id; an error ends the parse and the record
    in progress is handed over (parse_complete), so it counts if it has an id."""
    records, error = f2p_restate.parse(fastq)
    sizes = [len(seq) for rid, seq in records if rid]
    if error is not None:
        out = "valid\t0\nn_seqs\t%d\nerror_message\t%s\nerror_line\t%d\n" % (len(sizes), error[0], error[1])
        return out.encode("latin-1"), (f2p_restate.error_report(error) + "\n").encode("latin-1")
    out = "valid\t1\nn_seqs\t%d\n" % len(sizes)
    if sizes:
        n, total = float(len(sizes)), sum(sizes)
        mean = float(total) / n
        accum = 0.0
        for s in sizes:
            accum += (float(s) - mean) * (float(s) - mean)
        stddev = math.sqrt(accum / (n - 1.0)) if len(sizes) > 1 else 0.0
        out += "total_size\t%d\nmean\t%.2f\nstddev\t%.2f\n" % (total, mean, stddev)
    return out.encode("latin-1"), b""


def _reads(rng, lengths):
    acgt = np.frombuffer(b"ACGT", np.uint8)
    return [(b"r%d" % k, bytes(acgt[rng.integers(0, 4, L)])) for k, L in enumerate(lengths)]


def cases():
    rng = np.random.default_rng(41)
    mixed = f2p_restate.fastq_of(_reads(rng, [int(x) for x in rng.integers(0, 400, 300)]))
    good = f2p_restate.fastq_of(_reads(rng, [50, 60, 70]))
    out = {
        "mixed_lengths": mixed,
        "one_read": f2p_restate.fastq_of(_reads(rng, [151])),
        "empty": b"",
        "read_without_id": good + b"@\nACGTACGT\n+\nIIIIIIII\n" + good,
        "no_final_newline": mixed[:-1],
        "fasta": b">seq\nACGT\n",
        "missing_at": good + b"garbage\n" + good,
        "blank_line": good + b"\n" + good,
        "bad_data": good + b"@cut\nACGT-ACGT\n+\nIIIIIIIII\n" + good,
        "crlf": good.replace(b"\n", b"\r\n"),
        "high_byte": good + b"@hb\nAC\xc3GT\n+\nIIIII\n",
        "missing_plus": good + b"@mp\nACGT\nIIII\n" + good,
        "cut_record_without_id": good + b"@\nAC*GT\n+\nIIIII\n",
    }
    return out


CASES = cases()


def _run(args, data=None):
    env = dict(os.environ, PYTHONPATH=ROOT)
    return subprocess.run([sys.executable, "-m", "close_kmers_amd.validate_fastq"] + args, input=data,
                          capture_output=True, cwd=ROOT, env=env, timeout=300)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_command_line(gpu, tmp_path, name):
    """Blocks of 1000 bytes, so that tails are carried and an error falls in a later block."""
    data = CASES[name]
    p = tmp_path / (name + ".fq")
    p.write_bytes(data)
    r = _run([str(p), "--block-bytes", "1000"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert (r.stdout, r.stderr) == restate(data)


def test_the_cases_are_what_they_are_meant_to_be():
    assert restate(CASES["one_read"])[0].endswith(b"stddev\t0.00\n")
    assert restate(CASES["empty"])[0] == b"valid\t1\nn_seqs\t0\n"
    assert b"valid\t1\nn_seqs\t6\n" in restate(CASES["read_without_id"])[0]
    assert b"n_seqs\t4\n" in restate(CASES["bad_data"])[0]  # the cut record has an id: counted
    assert b"n_seqs\t3\n" in restate(CASES["cut_record_without_id"])[0]
    for name in ("fasta", "missing_at", "blank_line", "bad_data", "crlf", "high_byte", "missing_plus"):
        assert restate(CASES[name])[0].startswith(b"valid\t0\n"), name


@pytest.mark.gpu
def test_stdin(gpu):
    data = CASES["mixed_lengths"]
    r = _run(["-"], data)
    assert r.returncode == 0 and (r.stdout, r.stderr) == restate(data)
