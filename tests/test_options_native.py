"""kgx_ctx_set_option's table (csrc/kgx_options.h): the 43 names, their
defaults, accepted values and error texts against a hand-written record,
checked on the CPU by tests/native/options_check.cpp.  No GPU."""
import os
import subprocess

from close_kmers_amd import build as kbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "options_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "options_check")


def test_option_table_matches_the_record():
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_options.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{kbuild.CSRC}", SRC, "-o", OUT],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([OUT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
