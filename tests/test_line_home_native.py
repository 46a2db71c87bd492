"""line_home (csrc/kgx_line_home.h), the home line of a key in the line index,
run on the host by tests/native/line_home_check.cpp against a restatement in
Python, under both home modes; and the property the minimizer home exists for:
two windows that share their minimizer share their line.  No GPU."""
import os
import subprocess

import numpy as np

from close_kmers_amd import build as kbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "line_home_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "line_home_check")
CORE = 20 ** 7
M32 = 0xFFFFFFFF


def mix32(x: int) -> int:
    x = (x + 0x9E3779B9) & M32
    x ^= x >> 16
    x = x * 0x7FEB352D & M32
    x ^= x >> 15
    x = x * 0x846CA68B & M32
    x ^= x >> 16
    return x


def minimizer(key: int) -> int:
    a, b = key // 20, key % CORE
    return a if mix32(a) <= mix32(b) else b


def line_home(key: int, n_lines: int, mode: int) -> int:
    if mode == 0:
        return key % n_lines
    m = minimizer(key)
    hm = min(mix32(key // 20), mix32(key % CORE))
    return (mix32(m ^ 0x85EBCA6B) << 3 | (hm & 7)) % n_lines


def _native(keys, n_lines):
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_line_home.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([OUT, str(n_lines)], input="\n".join(str(k) for k in keys) + "\n",
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-500:] + r.stderr
    return [tuple(int(x) for x in line.split()) for line in r.stdout.splitlines()]


def _keys():
    rng = np.random.default_rng(7)
    keys = [0, 1, 19, 20, CORE - 1, CORE, CORE + 1, 20 ** 8 - 1, 20 ** 8 - 20, 2 ** 31, 2 ** 32, 2 ** 34]
    keys += [r * (20 ** 8 - 1) // 19 for r in range(20)]  # homopolymers: both 7-mers equal
    keys += [int(k) for k in rng.integers(0, 20 ** 8, 3000)]
    return keys


def test_line_home_host_equals_python_restatement():
    keys = _keys()
    # 1, tiny, the benchmark's line count, and past 2^32 lines (the hashed home has 35 bits)
    for n_lines in (1, 3, 1001, 1777777779, 2 ** 33 + 1, 2 ** 35 - 1):
        got = _native(keys, n_lines)
        assert len(got) == len(keys)
        for k, (h0, h1) in zip(keys, got):
            assert h0 == line_home(k, n_lines, 0), (k, n_lines)
            assert h1 == line_home(k, n_lines, 1), (k, n_lines)


def test_windows_sharing_their_minimizer_share_a_line():
    """Consecutive windows of a sequence: window i's last seven residues are
    window i + 1's first seven.  Where that 7-mer is the minimizer of both, the
    native homes are equal; it happens for about a third of the pairs, and
    never for three windows in a row (except inside a homopolymer)."""
    rng = np.random.default_rng(3)
    codes = rng.integers(0, 20, 6008)
    keys = []
    for i in range(len(codes) - 7):
        k = 0
        for c in codes[i:i + 8]:
            k = k * 20 + int(c)
        keys.append(k)
    n_lines = 1777777779
    home = [h1 for _, h1 in _native(keys, n_lines)]
    shared = 0
    for i in range(len(keys) - 1):
        common = keys[i] % CORE
        assert common == keys[i + 1] // 20
        if minimizer(keys[i]) == common and minimizer(keys[i + 1]) == common:
            assert home[i] == home[i + 1], i
            shared += 1
    # the shared 7-mer has the smallest hash of three: 1/3 of 6000 pairs, +- 5 sigma
    assert 2000 - 190 < shared < 2000 + 190, shared
    runs3 = sum(home[i] == home[i + 1] == home[i + 2] for i in range(len(keys) - 2))
    assert runs3 == 0
    # a homopolymer's windows are one key, so one line
    hp = [7 * (20 ** 8 - 1) // 19] * 3
    assert len({h1 for _, h1 in _native(hp, n_lines)}) == 1
