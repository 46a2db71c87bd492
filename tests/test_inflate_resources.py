"""Build-time guard: inflate_members_kernel (csrc/kgx_inflate.hip) uses no
scratch memory, keeps at least 6 waves per SIMD (it is bound by the latency of
one member's serial symbol chain, so waves in flight are its throughput) and a
workgroup's LDS stays under 16 KiB (four waves' code tables and the CRC
table).  Compiles the file for gfx950 with the compiler's resource remarks.
No GPU."""
import os
import re
import subprocess

from close_kmers_amd import build as kbuild


def test_inflate_kernel_resources(tmp_path):
    src = os.path.join(kbuild.CSRC, "kgx_inflate.hip")
    cmd = [kbuild.HIPCC, "-O3", "-std=c++17", f"--offload-arch={kbuild.ARCH}", f"-I{kbuild.INCLUDE}",
           f"-I{kbuild.CSRC}", "-x", "hip", "-c", src, "-o", str(tmp_path / "i.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    text = r.stderr[r.stderr.index("inflate_members_kernel"):]
    get = lambda what: int(re.search(re.escape(what) + r": (\d+)", text).group(1))
    assert get("ScratchSize [bytes/lane]") == 0
    assert get("VGPRs Spill") == 0
    assert get("Occupancy [waves/SIMD]") >= 6
    assert get("LDS Size [bytes/block]") <= 16384
