"""validate_fastq on the CPU: report() (close_kmers_amd/validate_fastq.py)
against the restatement of validate_fastq.cc in tests/test_gpu_validate_fastq.py,
its two decimals against the C library's own "%.2f" where the value lies
exactly between two of them, and the new calls' presence in libkgx.so and in
the header.  No GPU."""
import ctypes

import numpy as np

import f2p_restate
from close_kmers_amd import validate_fastq
from test_gpu_validate_fastq import CASES, restate


def _report_of(fastq: bytes) -> bytes:
    records, error = f2p_restate.parse(fastq)
    lengths = np.array([len(seq) for rid, seq in records if rid], np.int64)
    return validate_fastq.report(lengths, error[:2] if error else None).encode("latin-1")


def test_report_matches_the_restatement():
    for name, data in CASES.items():
        assert _report_of(data) == restate(data)[0], name
    assert validate_fastq.report([], None) == "valid\t1\nn_seqs\t0\n"
    assert validate_fastq.report([7], None) == "valid\t1\nn_seqs\t1\ntotal_size\t7\nmean\t7.00\nstddev\t0.00\n"
    assert validate_fastq.report([5, 9], ("Missing +", 12)) == \
        "valid\t0\nn_seqs\t2\nerror_message\tMissing +\nerror_line\t12\n"


def _c_fixed2(x: float) -> str:
    buf = ctypes.create_string_buffer(64)
    libc = ctypes.CDLL(None)
    libc.snprintf.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_char_p, ctypes.c_double]
    libc.snprintf(buf, 64, b"%.2f", ctypes.c_double(x))
    return buf.value.decode()


def test_two_decimals_on_ties():
    """One read of k bases among n - 1 empty ones: mean k / n and deviation
    k / sqrt(n), exact in binary for n a power of four, so with n = 8 or 64 and
    k = 1 or 3 they end in ...5 at the third decimal.  std::fixed with
    setprecision(2) rounds such a value to the even neighbour, as printf does."""
    want = {(8, 1): ("0.12", None), (8, 3): ("0.38", None), (64, 1): ("0.02", "0.12"), (64, 3): ("0.05", "0.38"),
            (64, 5): ("0.08", "0.62")}
    for (n, k), (mean, stddev) in want.items():
        lines = validate_fastq.report([k] + [0] * (n - 1), None).split("\n")
        assert lines[1] == f"n_seqs\t{n}" and lines[2] == f"total_size\t{k}"
        assert lines[3] == "mean\t" + mean == "mean\t" + _c_fixed2(k / n)
        if stddev:
            assert lines[4] == "stddev\t" + stddev == "stddev\t" + _c_fixed2(k / 8.0)


def test_new_symbols_are_exported_and_listed(kgx):
    for name in ("kgx_fq_parse", "kgx_fq_parse_device", "kgx_fq_proteins_device"):
        assert name in kgx.SIGNATURES and name in kgx.header_symbols()
        assert getattr(kgx.lib(), name)
    assert ctypes.sizeof(kgx.FqReads) == 104
    assert (kgx.FQ_STRICT, kgx.FQ_FINISHED, kgx.FQ_PARSE_MAX) == (1, 2, 0xFFFFF000)
