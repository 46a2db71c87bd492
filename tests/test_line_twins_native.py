"""The homes behind the line index's twin records (seven_mer_home, twin_home
and pair_home, csrc/kgx_line_home.h), run on the host by
tests/native/line_twins_check.cpp: minimizer_home returns what it returned
before it was split; a key's minimizer and twin homes are the homes of its two
7-mers; pair_home is the last 7-mer's home at an even window index and the
first's at an odd one, so windows g (even) and g + 1 of one sequence always
share it.  No GPU."""
import os
import subprocess

import pytest

from close_kmers_amd import build as kbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "line_twins_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "line_twins_check")


@pytest.fixture(scope="module")
def exe():
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_line_home.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return OUT


@pytest.mark.parametrize("n_lines", (1, 3, 7, 1001, 1777777779, 2 ** 32 - 3))
def test_pair_home_and_the_split_minimizer_home(exe, n_lines):
    r = subprocess.run([exe, str(n_lines)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr
    last = r.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 2_000_000
