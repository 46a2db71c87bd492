"""Host side of the recall (close_kmers_amd/recall.py): labels, the two files,
the validation line, the C ABI's symbols.  No device needed.

The expected bytes under tests/golden/recall/ were written by hand: seven
records in two files, kinds 0 to 3, the kind-2 name order ("gamma ?? Alpha":
the lexically larger name first), scores 12, 0.5, 1e6 and 1234567 as an ostream
prints a float (1e+06, 1.23457e+06), a definition outside the index, an id
without a definition, and a definition that is itself a composite, whose New
row is skipped although the sequence counts as changed.
"""
import ctypes
import os
import re

import numpy as np

from close_kmers_amd import build as kbuild
from close_kmers_amd import recall
from helpers import GOLDEN

FUNCTIONS = [b"Alpha", b"beta", b"gamma"]


def test_labels_are_three_valued():
    id_function = {b"a": b"beta", b"b": b"not kept", b"c": b"", b"e": b"Alpha"}
    records = [[(b"a", b"AC"), (b"b", b"AC")], [], [(b"c", b""), (b"d", b"AC"), (b"e", b"AC")]]
    lab = recall.labels(id_function, records, FUNCTIONS)
    assert lab.dtype == np.int32
    assert lab.tolist() == [1, recall.LABEL_OTHER, recall.LABEL_NONE, recall.LABEL_NONE, 0]
    assert (recall.LABEL_OTHER, recall.LABEL_NONE) == (-1, -2)
    res, off = recall.pack(records)
    assert off.tolist() == [0, 2, 4, 4, 6, 8] and res.tobytes() == b"ACACACAC"


def test_write_recall_matches_the_hand_written_files(kgx, tmp_path):
    best = np.zeros(7, kgx.BEST_DTYPE)
    best["fi0"] = best["fi1"] = -1
    #            kind fi0 fi1 score     weighted   offset
    rows = [(1, 0, -1, 12.0, 0.5, 12.0),          # a1 Alpha, as defined
            (1, 1, -1, 1e6, 1234567.0, 9.0),      # a2 beta, defined Alpha
            (2, 0, 2, 7.0, 0.0, 1.0),             # a3 Alpha | gamma -> "gamma ?? Alpha"
            (2, 2, 1, 9.0, 3.25, 6.0),            # a4 gamma | beta, defined as that composite
            (0, -1, -1, 0.0, 0.0, 0.0),           # a5 no calls, no definition
            (3, 1, 2, 0.0, 0.0, 2.0),             # a6 no call, defined beta
            (0, -1, -1, 0.0, 0.0, 0.0)]           # b1 no calls, defined outside the index
    for i, r in enumerate(rows):
        best[i] = r
    id_function = {b"a1": b"Alpha", b"a2": b"Alpha", b"a3": b"gamma", b"a4": b"gamma ?? beta", b"a6": b"beta",
                   b"b1": b"rare thing"}
    records = [[(b"a%d" % i, b"ACDEFGHIKL") for i in range(1, 7)], [(b"b1", b"ACDEFGHIKL")]]
    lab = recall.labels(id_function, records, FUNCTIONS)
    assert lab.tolist() == [0, 0, 2, -1, -2, 1, -1]
    changed = [1, 2, 3, 5, 6]  # by index: a4's label is OTHER, so it counts as changed
    out = str(tmp_path / "r")
    recall.write_recall(out, ["/some/where/g.fa", "h.fa"], records, id_function, FUNCTIONS, best, changed)
    for sub in ("Calls", "New"):
        assert sorted(os.listdir(os.path.join(out, sub))) == ["g.fa", "h.fa"]
        for leaf in ("g.fa", "h.fa"):
            want = open(os.path.join(GOLDEN, "recall", sub, leaf), "rb").read()
            assert open(os.path.join(out, sub, leaf), "rb").read() == want, (sub, leaf)
    # the report files
    fn = np.array([(2, 1, 1), (1, 0, 1), (1, 0, 0)], kgx.RECALL_FUNCTION_DTYPE)
    pairs = np.array([(0, 1, 1)], kgx.RECALL_PAIR_DTYPE)
    recall.write_report(out, FUNCTIONS, fn, pairs)
    assert open(os.path.join(out, "functions.tsv"), "rb").read() == b"0\tAlpha\t2\t1\t1\n1\tbeta\t1\t0\t1\n2\tgamma\t1\t0\t0\n"
    assert open(os.path.join(out, "confusions.tsv"), "rb").read() == b"0\t1\t1\n"


def test_floats_print_as_the_library_prints_them(kgx):
    buf = ctypes.create_string_buffer(64)
    for x in (0.0, 12.0, 0.5, 1e6, 999999.0, 1234567.0, 59.454422, 1e-5, 0.0001, 3.4e38, 100000.0, 1e5 + 0.5, -2.5):
        n = kgx.lib().kgx_format_g6(ctypes.c_float(x), buf, 64)
        assert recall.format_float(x) == buf.raw[:n], x
    assert recall.format_float(1e6) == b"1e+06" and recall.format_float(12) == b"12"


def test_validation_line_from_cells():
    cell = [[10, 2, 1, 3],   # kept: match, mismatch, ambiguous, none
            [0, 4, 1, 2],    # other
            [0, 1, 0, 5]]    # none: the last is "" == ""
    assert recall.validation_line("seq/g1.fa", 31, cell, 2) == "seq/g1.fa: count=31 correct=15 incorrect=14 missing=2"
    assert recall.validation_line("x", 0, np.zeros((3, 4)), 0) == "x: count=0 correct=0 incorrect=0 missing=0"


def test_fasta_records_without_an_id_are_kept_for_the_count(tmp_path):
    p = tmp_path / "v.fa"
    p.write_bytes(b">id1 desc\nACD\nEFG\n>\nKLM\n>id2\nNPQ\n")
    assert recall.read_fasta_all(str(p)) == [(b"id1", b"ACDEFG"), (b"", b"KLM"), (b"id2", b"NPQ")]


def test_function_index_round_trip(tmp_path):
    from close_kmers_amd import signatures
    signatures.write_indexes(str(tmp_path), FUNCTIONS)
    assert recall.read_function_index(str(tmp_path)) == FUNCTIONS


def test_symbols_are_declared_bound_and_exported(kgx):
    names = ["kgx_recall_run", "kgx_recall_stats_get", "kgx_recall_best", "kgx_recall_functions",
             "kgx_recall_changed", "kgx_recall_confusions", "kgx_recall_destroy"]
    header = open(os.path.join(kbuild.INCLUDE, "kgx.h")).read()
    for n in names:
        assert n in kgx.SIGNATURES and n in kgx.header_symbols() and hasattr(kgx.lib(), n), n
    assert re.search(r"#define KGX_LABEL_OTHER \(-1\)", header) and re.search(r"#define KGX_LABEL_NONE +\(-2\)", header)
    assert (kgx.LABEL_OTHER, kgx.LABEL_NONE) == (-1, -2)
    # kgx_recall_stats: 15 u64, n_pieces, 4 floats, padded to 8
    assert ctypes.sizeof(kgx.RecallStats) == 144 and kgx.RecallStats.n_pieces.offset == 120
    assert kgx.RECALL_FUNCTION_DTYPE.itemsize == 12 and kgx.RECALL_PAIR_DTYPE.itemsize == 16


def test_null_arguments_are_einval_without_a_device(kgx):
    out = ctypes.c_void_p()
    off = np.zeros(1, np.uint64)
    assert kgx.lib().kgx_recall_run(None, None, None, off.ctypes.data, None, 0, 1, 0, ctypes.byref(out)) == kgx.KGX_EINVAL
    assert kgx.lib().kgx_recall_run(None, None, None, None, None, 0, 1, 0, None) == kgx.KGX_EINVAL
    assert kgx.lib().kgx_recall_stats_get(None, None) == kgx.KGX_EINVAL
    assert kgx.lib().kgx_recall_destroy(None) == kgx.KGX_OK
