"""Host side of the grouping by k-mer set (close_kmers_amd/unique_prots.py,
csrc/kgx_uniq.hip): the C ABI's symbols, the text, and the restatement
(tests/uniq_restate.py) on the oracle's hits.  No device needed.
"""
import ctypes
import os
import re

import numpy as np

import uniq_restate
from close_kmers_amd import build as kbuild
from helpers import DesignedImage, encode, pack

NAMES = ["kgx_uniq_run", "kgx_uniq_stats_get", "kgx_uniq_groups", "kgx_uniq_group_of", "kgx_uniq_sets",
         "kgx_uniq_destroy"]


def test_symbols_are_declared_bound_and_exported(kgx):
    header = open(os.path.join(kbuild.INCLUDE, "kgx.h")).read()
    for n in NAMES:
        assert n in kgx.SIGNATURES and n in kgx.header_symbols() and hasattr(kgx.lib(), n), n
    assert re.search(r"#define KGX_UNIQ_STAGES 5\b", header)
    assert kgx.UNIQ_STAGES == ("upload", "pass", "sets", "group", "download")
    assert "kgx_uniq.hip" in kbuild.LIB_SOURCES


def test_the_stats_struct_has_the_headers_size(kgx):
    # kgx_uniq_stats: 7 u64, 2 u32, 5 floats = 84 bytes, padded to the u64's 8
    header = open(os.path.join(kbuild.INCLUDE, "kgx.h")).read()
    body = re.search(r"typedef struct kgx_uniq_stats \{(.*?)\} kgx_uniq_stats;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    size = {"uint64_t": 8, "uint32_t": 4, "float": 4}
    total, names = 0, []
    for typ, decl in re.findall(r"(uint64_t|uint32_t|float)\s+([^;]+);", body):
        for d in decl.split(","):
            m = re.fullmatch(r"\s*(\w+)(?:\[(\w+)\])?\s*", d)
            count = 1 if not m.group(2) else 5 if m.group(2) == "KGX_UNIQ_STAGES" else int(m.group(2))
            assert total % size[typ] == 0  # no padding inside
            total += size[typ] * count
            names.append(m.group(1))
    assert names == [f for f, _ in kgx.UniqStats._fields_]
    assert ctypes.sizeof(kgx.UniqStats) == (total + 7) // 8 * 8 == 88
    assert kgx.UniqStats.n_pieces.offset == 56 and kgx.UniqStats.stage_ms.offset == 64


def test_null_arguments_are_einval_without_a_device(kgx):
    out = ctypes.c_void_p()
    off = np.zeros(1, np.uint64)
    lib = kgx.lib()
    assert lib.kgx_uniq_run(None, None, off.ctypes.data, 0, 0, 64, ctypes.byref(out)) == kgx.KGX_EINVAL
    assert lib.kgx_uniq_run(None, None, None, 0, 0, 64, None) == kgx.KGX_EINVAL
    assert lib.kgx_uniq_run(None, None, off.ctypes.data, 0, 0, 65, ctypes.byref(out)) == kgx.KGX_EINVAL
    assert b"digest_bits" in kgx.lib().kgx_last_error()
    assert out.value is None
    assert lib.kgx_uniq_stats_get(None, None) == kgx.KGX_EINVAL
    p, n = ctypes.c_void_p(), ctypes.c_uint64()
    assert lib.kgx_uniq_groups(None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(n)) == kgx.KGX_EINVAL
    assert lib.kgx_uniq_group_of(None, ctypes.byref(p), ctypes.byref(n)) == kgx.KGX_EINVAL
    assert lib.kgx_uniq_sets(None, ctypes.byref(p), ctypes.byref(p), ctypes.byref(n)) == kgx.KGX_EINVAL
    assert lib.kgx_uniq_destroy(None) == kgx.KGX_OK


def test_format_groups_byte_for_byte():
    from close_kmers_amd import unique_prots
    ids = [b"fig|1.peg.1", b"", b"b", b"c|x"]
    # groups {1, 3}, {0}, {2}: a trailing tab per id, the empty id a bare tab
    got = unique_prots.format_groups(ids, np.array([0, 2, 3, 4], np.uint64), np.array([1, 3, 0, 2], np.uint32))
    assert got == b"\tc|x\t\nfig|1.peg.1\t\nb\t\n"
    assert got == uniq_restate.text(ids, [[1, 3], [0], [2]])
    assert unique_prots.format_groups(ids, np.array([0, 4], np.uint64), np.arange(4, dtype=np.uint32)) == \
        b"fig|1.peg.1\t\tb\tc|x\t\n"
    assert unique_prots.format_groups([], np.array([0], np.uint64), np.zeros(0, np.uint32)) == b""


def test_the_restatement_on_the_oracles_hits(oracle_lib):
    k1, k2, k3 = "ACDEFGHI", "CDEFGHIK", "WWWWWWWW"
    K1, K2, K3 = encode(k1), encode(k2), encode(k3)
    assert K1 < K2 < K3
    d = DesignedImage()
    for f, k in enumerate((k1, k2, k3)):
        d.add(k, f)
    table = d.table()
    seqs = [k3 + "MM",                  # {K3}
            k1 + "MM" + k2 + "MM",      # {K1, K2}
            k1 + "MM",                  # {K1}: a proper prefix of the one above
            "MMMMMMMMMMMM",             # no hit
            k2 + "MM" + k1 + k1 + "MM",  # {K1, K2} again: other order, a repeat
            "",                         # empty
            k1[:7]]                     # 7 residues
    res, off = pack([(str(i), s) for i, s in enumerate(seqs)])
    r = oracle_lib.process_batch(table, res, off, want=1)
    groups, keys = uniq_restate.groups(r.hit_offsets, r.hits["which_kmer"])
    assert keys == [(), (K1,), (K1, K2), (K3,)]   # the empty set first, the prefix before its extension
    assert groups == [[3, 5, 6], [2], [1, 4], [0]]
    by_size = sorted(keys, key=lambda k: (len(k), k))
    assert by_size != keys and by_size == [(), (K1,), (K3,), (K1, K2)]
    assert uniq_restate.group_of(groups, len(seqs)).tolist() == [3, 2, 1, 0, 2, 0, 0]
    assert uniq_restate.pieces_by_rule(off, 0) == 1 and uniq_restate.pieces_by_rule(off, 1) == len(seqs)
