"""The parts of a request's blocks when the device frames them
(csrc/kgx_fq_body.h: a block's last part runs whether full or not, the text
behind the last complete record is carried, a gzip body's parts end at member
boundaries, and a record longer than one parse takes sends the rest of its
block to the host parser) through tests/native/fq_body_check.cpp, built plain
and with the address and undefined-behaviour sanitizers and run directly,
against a byte-wise model of the lenient parse.  The limit is a stand-in of
512 or 1,000 bytes for KGX_FQ_PARSE_MAX, which no GPU test reaches.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fq_body_check.cpp")
FLAGS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


def _build_check(kind):
    from close_kmers_amd import build as kbuild
    out = os.path.join(HERE, "native", "_build", "fq_body_check_" + kind)
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_fq_body.h"), os.path.join(kbuild.CSRC, "kgx_fq_parts.h")]
    if not os.path.exists(out) or any(os.path.getmtime(d) > os.path.getmtime(out) for d in deps):
        os.makedirs(os.path.dirname(out), exist_ok=True)
        r = subprocess.run(["g++", "-std=c++17", "-Wall"] + FLAGS[kind] + [f"-I{kbuild.CSRC}", SRC, "-o", out],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return out


@pytest.mark.parametrize("kind,seed", [("plain", 1), ("sanitized", 2)])
def test_parts_of_blocks_against_the_model(kind, seed):
    r = subprocess.run([_build_check(kind), str(seed), "12"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 1000 and int(words[3]) > 10000 and int(words[5]) > 100, r.stdout


def test_header_needs_no_hip():
    from close_kmers_amd import build as kbuild
    text = open(os.path.join(kbuild.CSRC, "kgx_fq_body.h")).read()
    code = text.split("#pragma once")[1]
    assert "hip" not in code.lower()
    assert [l for l in code.splitlines() if l.startswith('#include "')] == ['#include "kgx_fq_parts.h"']
