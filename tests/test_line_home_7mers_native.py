"""The home of a key from the two 7-mers the probe's encode already holds
(seven_mers and line_home_7mers, csrc/kgx_line_home.h), run on the host by
tests/native/line_home_7mers_check.cpp: the 7-mers from the eight residue
codes equal key / 20 and key mod 20^7, and the home from them equals
line_home of the key under both modes, up to the largest line count the
aligned probe takes.  And line_index_aligned, which tables that probe takes,
at its edges.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

from close_kmers_amd import build as kbuild
from test_line_home_native import CORE, _keys, line_home

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "line_home_7mers_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "line_home_7mers_check")
MOST_LINES = 2 ** 32 - 3


@pytest.fixture(scope="module")
def exe():
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_line_home.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return OUT


@pytest.fixture(scope="module")
def keys():
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 20, 6008)
    windows = []
    for i in range(len(codes) - 7):
        k = 0
        for c in codes[i:i + 8]:
            k = k * 20 + int(c)
        windows.append(k)
    return _keys() + windows


@pytest.mark.parametrize("n_lines", (1, 3, 7, 1001, 1777777779, MOST_LINES))
def test_home_from_the_7mers_equals_line_home(exe, keys, n_lines):
    r = subprocess.run([exe, str(n_lines)], input="\n".join(str(k) for k in keys) + "\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr  # 1: the check's own comparison with line_home failed
    got = [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]
    assert len(got) == len(keys)
    for k, (a, b, h0, h1) in zip(keys, got):
        assert a == k // 20 and b == k % CORE, k
        assert a < 2 ** 31 and b < 2 ** 31
        assert h0 == line_home(k, n_lines, 0), (k, n_lines)
        assert h1 == line_home(k, n_lines, 1), (k, n_lines)


def _aligned(exe, num_sigs, shift=2, mode=1, marks=1):
    r = subprocess.run([exe, "aligned", str(num_sigs), str(shift), str(mode), str(marks)],
                       capture_output=True, text=True, timeout=30)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip() == "1"


def test_the_aligned_probe_is_taken_exactly_where_it_holds(exe):
    assert _aligned(exe, 4 * MOST_LINES)  # n_lines + 2 still fits 32 bits
    assert not _aligned(exe, 4 * (MOST_LINES + 1))
    assert not _aligned(exe, 4 * 2 ** 32)
    for mode in (0, 1):
        assert _aligned(exe, 4, mode=mode) and _aligned(exe, 4 * 1777777779, mode=mode)
        for num_sigs in (4 * 1777777779 + 1, 4 * 1777777779 + 2, 7, 5):  # not whole lines
            assert not _aligned(exe, num_sigs, mode=mode)
        for shift in (0, 1, 3):  # not the index's 4-record lines
            assert not _aligned(exe, 4 * 1001, shift=shift, mode=mode)
        assert not _aligned(exe, 4 * 1001, mode=mode, marks=0)  # no marks: the generic kernel
    assert not _aligned(exe, 0)
