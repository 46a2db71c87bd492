"""Build-time guard: every kernel of the device FASTA parser
(csrc/kgx_fa_parse.hip) uses no scratch memory and spills no register, and the
library and the header carry its entry points.  Compiles the file for gfx950
with the compiler's resource remarks; the VGPR, LDS and occupancy figures are
recorded in DESIGN.md §8.13, not asserted.  No GPU."""
import os
import re
import subprocess

from close_kmers_amd import build as kbuild

KERNELS = ("fa_parse_map_kernel", "fa_parse_state_kernel", "fa_parse_count_kernel", "fa_parse_sums_kernel",
           "fa_parse_write_kernel", "fa_parse_no_id_kernel")


def test_fa_parse_kernel_resources(tmp_path):
    src = os.path.join(kbuild.CSRC, "kgx_fa_parse.hip")
    cmd = [kbuild.HIPCC, "-O3", "-std=c++17", f"--offload-arch={kbuild.ARCH}", f"-I{kbuild.INCLUDE}",
           f"-I{kbuild.CSRC}", "-x", "hip", "-c", src, "-o", str(tmp_path / "p.o"),
           "-Rpass-analysis=kernel-resource-usage"]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    # one block of remarks per kernel, begun by "Function Name: <mangled name>"
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


def test_fa_parse_symbols(kgx):
    import ctypes
    lib = ctypes.CDLL(kbuild.LIB)
    for name in ("kgx_fa_parse", "kgx_fa_parse_device"):
        assert hasattr(lib, name), name
    header = open(os.path.join(kbuild.INCLUDE, "kgx.h")).read()
    for word in ("KGX_FA_STRICT 1u", "KGX_FA_FINISHED 2u", "KGX_FA_PARSE_MAX 0xFFFFF000ull", "typedef struct kgx_fa_seqs",
                 "int kgx_fa_parse_device(kgx_ctx *", "int kgx_fa_parse(kgx_ctx *"):
        assert word in header, word
    assert ctypes.sizeof(kgx.FaSeqs) == 104
    assert (kgx.FA_STRICT, kgx.FA_FINISHED, kgx.FA_PARSE_MAX) == (1, 2, 0xFFFFF000)
    assert kgx.FA_ERROR_TEXT[1:] == ("Missing >", "Bad data character '", "Bad id or data character '")
    r = kgx.FaSeqs()
    r.error, r.error_byte = 3, ord("*")
    assert r.error_text() == "Bad id or data character '*'"
    r.error = 1
    assert r.error_text() == "Missing >"
