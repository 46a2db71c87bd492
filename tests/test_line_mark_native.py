"""line_mark (csrc/kgx_line_home.h), the overflow mark of a key in the line
index, run on the host by tests/native/line_mark_check.cpp against a
restatement in Python; the spread the marks exist for: the 40 keys around one
7-mer, which share a home line under the minimizer home, take most of the 16
values; and the home word, which carries the marks bit beside the shift and
the home mode (checked inside the native program).  No GPU."""
import os
import subprocess

import numpy as np

from close_kmers_amd import build as kbuild
from test_line_home_native import CORE, M32, _keys, mix32

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "line_mark_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "line_mark_check")


def line_mark(key: int) -> int:
    return mix32((((key & M32) ^ 0x27D4EB2F) + (key >> 32) * 0xC2B2AE35) & M32) >> 28


def _native(keys, n_lines=1777777779):
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_line_home.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([OUT, str(n_lines)], input="\n".join(str(k) for k in keys) + "\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr  # 1: the home word or a home bucket is off
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def test_line_mark_host_equals_python_restatement_and_home_word_round_trips():
    keys = _keys()
    for n_lines in (1, 7, 1777777779):
        got = _native(keys, n_lines)
        assert len(got) == len(keys)
        for k, (g, rec, bit) in zip(keys, got):
            assert g == line_mark(k), k
            assert (rec, bit) == (g >> 2, 28 + (g & 3)), k  # bit 60 + (g & 3) of the record's second word
    # every value occurs, about evenly: 3032 keys over 16 values, +- 5 sigma
    counts = np.bincount([g for g, _, _ in got], minlength=16)
    assert counts.min() > 190 - 67 and counts.max() < 190 + 67, counts


def test_the_40_keys_around_one_7mer_spread_over_the_marks():
    """X extended by each of the 20 residues on either side: under the
    minimizer home these share a line when X is their minimizer, so their
    marks are what tells them apart on it.  At least 12 of 16 values each
    (40 uniform draws from 16 values leave fewer than 12 one time in 800, so
    20 cores would fail an ideal hash one time in 40; these pass)."""
    rng = np.random.default_rng(11)
    cores = [0, 1, CORE - 1, 7 * (CORE - 1) // 19] + [int(x) for x in rng.integers(0, CORE, 16)]
    for x in cores:
        keys = [r * CORE + x for r in range(20)] + [x * 20 + r for r in range(20)]
        marks = {g for g, _, _ in _native(keys)}
        assert marks == {line_mark(k) for k in keys}
        assert len(marks) >= 12, (x, sorted(marks))
