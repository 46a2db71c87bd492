"""The homes of the line index's pairs layout (HOME_PAIRS_BIT,
csrc/kgx_line_home.h), run on the host by tests/native/line_pairs_check.cpp:
a key's two homes are its 7-mers' homes in their roles (line 2k + 1 of the
7-mer's block for a key's first seven residues, line 2k for its last seven),
they differ and lie below 2 * (n_lines >> 1); windows g (even) and g + 1 of one
sequence start at lines 2k and 2k + 1 of one block; the minimizer home is one
of the two; without the bit every function returns what it returned.  No GPU."""
import os
import subprocess

import pytest

from close_kmers_amd import build as kbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "line_pairs_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "line_pairs_check")


@pytest.fixture(scope="module")
def exe():
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_line_home.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return OUT


@pytest.mark.parametrize("n_lines", (3, 7, 1001, 1777777779, 2 ** 32 - 3))
def test_pairs_homes(exe, n_lines):
    r = subprocess.run([exe, str(n_lines)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 2_000_000


def test_fewer_than_three_lines_is_refused(exe):
    """an index of 1 line has no block: the builder keeps pairs off there, and the check says so"""
    assert subprocess.run([exe, "1"], capture_output=True, text=True, timeout=120).returncode == 2
