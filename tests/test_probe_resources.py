"""Build-time guard: the line probe over an index with marks
(probe_line_kernel<J, 4, DNA, MARKS = true, TWINS, DEFER> in kgx_probe.hip)
at the default tile of 128 windows (J = 2) holds at most 64 VGPRs and uses no
scratch memory, in both forms of its aligned body (KGX_PROBE_DEFER), with and
without twin records, for proteins and for DNA: 64 registers are 8 waves per
SIMD, and it is the other resident waves that cover a chain's dependent
round trips.  Compiles the file for gfx950 with the compiler's resource
remarks.  No GPU."""
import os
import re
import subprocess

from close_kmers_amd import build as kbuild


def test_line_probe_with_marks_at_j2_holds_64_vgprs_and_no_scratch(tmp_path):
    src = os.path.join(kbuild.CSRC, "kgx_probe.hip")
    cmd = [kbuild.HIPCC, "-O3", "-std=c++17", f"--offload-arch={kbuild.ARCH}", f"-I{kbuild.INCLUDE}",
           f"-I{kbuild.CSRC}", "-x", "hip", "-c", src, "-o", str(tmp_path / "p.o"),
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
    # J = 2, G = 4, DNA either, MARKS true, TWINS either, DEFER either (Itanium mangling of the template arguments)
    marks_j2 = {k: v for k, v in kernels.items()
                if re.search(r"probe_line_kernelILi2ELi4ELb[01]ELb1ELb[01]ELb[01]EEE", k)}
    assert len(marks_j2) == 8, sorted(kernels)
    for k, v in marks_j2.items():
        print(k, v)
        assert v["ScratchSize"] == 0, (k, v)
        assert v["VGPRs"] <= 64, (k, v)
