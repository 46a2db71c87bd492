"""The host planner of signature selection in key-range passes
(csrc/kgx_sig_plan.h): greedy packing of 1,600-bin counts into passes of at
most B tuples, refinement of a bin above B two letters deeper, KGX_ERANGE for
a single k-mer above B, the letter ranks and the automatic budget -- checked
over small corpora on the CPU by tests/native/sig_plan_check.cpp.  No GPU."""
import os
import subprocess

from close_kmers_amd import build as kbuild

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "sig_plan_check.cpp")
OUT = os.path.join(HERE, "native", "_build", "sig_plan_check")


def test_planner_packs_refines_and_refuses():
    deps = [SRC, os.path.join(kbuild.CSRC, "kgx_sig_plan.h"), os.path.join(kbuild.INCLUDE, "kgx.h")]
    if not os.path.exists(OUT) or any(os.path.getmtime(d) > os.path.getmtime(OUT) for d in deps):
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", f"-I{kbuild.CSRC}", f"-I{kbuild.INCLUDE}", SRC,
                            "-o", OUT], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
    r = subprocess.run([OUT], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip().splitlines()[-1].startswith("ok "), r.stdout + r.stderr
    assert r.stdout.count("# ") == 4  # the four corpora
