"""Build-time guard for the lane scorers (kgx_score.hip): the lean kernel that
launch_score picks for calls without OTU output under order_constraint 0
(score_lean_kernel<PK, SB, PACK>, option score_lean) holds at most 64 VGPRs
and uses no scratch memory in its PACKED16 instantiations -- 64 registers are
one probe wave's worth, so a scorer wave takes one probe wave's place on a
SIMD and not three.  The kernel carries amdgpu_waves_per_eu(8, 8), which makes
the compiler stay within 64 registers whatever it costs, so the assertion
that carries the weight is the one on scratch: a body that no longer fits
shows up as spills, not as a 65th register.  The general kernel
(score_kernel<PK, SB>) holds no more than it did before the lean one was
split off (133 / 96 registers for PACKED16 at 8 / 2 records per batch, 136 /
99 for the planes).  Compiles the
file for gfx950 with the compiler's resource remarks and reads nothing else.
No GPU."""
import os
import re
import subprocess

from close_kmers_amd import build as kbuild


def test_lean_lane_scorer_holds_64_vgprs_and_the_general_one_no_more_than_before(tmp_path):
    src = os.path.join(kbuild.CSRC, "kgx_score.hip")
    cmd = [kbuild.HIPCC, "-O3", "-std=c++17", f"--offload-arch={kbuild.ARCH}", f"-I{kbuild.INCLUDE}",
           f"-I{kbuild.CSRC}", "-x", "hip", "-c", src, "-o", str(tmp_path / "s.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    kernels = {}
    name = None
    for ln in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            kernels[name] = {}
        m = re.search(r"(VGPRs|ScratchSize \[bytes/lane\]): (\d+)", ln)
        if m and name:
            kernels[name][m.group(1).split()[0]] = int(m.group(2))

    def pick(pattern):
        return {k: v for k, v in kernels.items() if re.search(pattern, k)}

    # score_lean_kernel<PK = true, SB, PACK> (Itanium mangling): the batch depths
    # launch_score uses (the long-sequence depth and 2 for short sequences), with
    # and without packing; bench.py's C2 batch runs the deeper one without PACK
    # (score_lean 1, the default)
    lean = pick(r"score_lean_kernelILb1ELi\d+ELb[01]EEE")
    assert len(lean) == 4, sorted(kernels)
    assert len(pick(r"score_lean_kernelILb1ELi2ELb[01]EEE")) == 2, sorted(lean)
    for k, v in lean.items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs"] <= 64, (k, v)
    # the planes instantiations need not meet 64, but must not spill
    for k, v in pick(r"score_lean_kernelILb0ELi\d+ELb[01]EEE").items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
    # score_kernel<PK, SB>
    before = {r"score_kernelILb1ELi8EEE": 133, r"score_kernelILb1ELi2EEE": 96,
              r"score_kernelILb0ELi8EEE": 136, r"score_kernelILb0ELi2EEE": 99}
    for pattern, bound in before.items():
        got = pick(pattern)
        assert len(got) == 1, (pattern, sorted(kernels))
        for k, v in got.items():
            print(k, v)
            assert v["ScratchSize"] == 0, (k, v)
            assert v["VGPRs"] <= bound, (k, v, bound)
