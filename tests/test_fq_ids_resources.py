"""Build-time guard: the kernels of kgx_fq_read_ids (csrc/kgx_fq_ids.hip) use no
scratch memory, spill nothing and keep to 64 VGPRs, so they can run beside the
probe.  Compiles the file for gfx950 with the compiler's resource remarks; the
figures are recorded in DESIGN.md §8.14.  No GPU."""
import os
import re
import subprocess

from close_kmers_amd import build as kbuild

KERNELS = ("fq_ids_len_kernel", "fq_ids_sums_kernel", "fq_ids_copy_kernel")


def test_fq_ids_kernel_resources(tmp_path):
    src = os.path.join(kbuild.CSRC, "kgx_fq_ids.hip")
    cmd = [kbuild.HIPCC, "-O3", "-std=c++17", f"--offload-arch={kbuild.ARCH}", f"-I{kbuild.INCLUDE}",
           f"-I{kbuild.CSRC}", "-x", "hip", "-c", src, "-o", str(tmp_path / "i.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    blocks = re.split(r"remark: [^\n]*Function Name: ", r.stderr)[1:]
    seen = {}
    for b in blocks:
        name = b.split()[0]
        get = lambda what: int(re.search(re.escape(what) + r": (\d+)", b).group(1))
        seen[name] = {"vgprs": get("VGPRs"), "scratch": get("ScratchSize [bytes/lane]"), "spill": get("VGPRs Spill"),
                      "sgpr_spill": get("SGPRs Spill"), "lds": get("LDS Size [bytes/block]"),
                      "occupancy": get("Occupancy [waves/SIMD]")}
    print(seen)
    for k in KERNELS:
        assert any(k in name for name in seen), (k, sorted(seen))
    assert len(seen) == len(KERNELS), sorted(seen)
    for name, v in seen.items():
        assert v["scratch"] == 0 and v["spill"] == 0 and v["sgpr_spill"] == 0, (name, v)
        assert v["vgprs"] <= 64, (name, v)
