"""The part and tail arithmetic of the device-parsed fastq_to_protein
(csrc/kgx_fq_parts.h: how much text a part takes, what is carried, the line
count across parts, growth of a part that holds no complete record) through
tests/native/fq_parts_check.cpp, built with the address and undefined-behaviour
sanitizers and run directly: texts of many lengths in blocks of 1 byte to 1 MB
and parts of 1 byte to 64 KB, parts smaller than a record among them, against
a byte-wise model of the strict parse over the whole text.  No GPU."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "fq_parts_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "fq_parts_check")


def _build_check():
    from close_kmers_amd import build as kbuild
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_fq_parts.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                            "-fno-sanitize-recover=all", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    return OUT


@pytest.mark.parametrize("seed", [1, 2])
def test_parts_carry_lines_and_growth(seed):
    r = subprocess.run([_build_check(), str(seed), "40"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    words = r.stdout.split()
    assert words[0] == "ok" and int(words[1]) > 10000 and int(words[3]) > 100, r.stdout


def test_header_needs_no_hip():
    """The header compiles alone with the host compiler."""
    from close_kmers_amd import build as kbuild
    text = open(os.path.join(kbuild.CSRC, "kgx_fq_parts.h")).read()
    assert "hip" not in text.split("#pragma once")[1].lower()
    assert "#include \"" not in text
