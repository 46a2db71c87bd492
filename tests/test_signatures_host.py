"""Signature selection without a device: the CPU restatement against the
hand-checked fixture, the front end's function selection and files, the table
size rule, and the error a missing device gives (never a CPU fallback)."""
import json
import os

import numpy as np
import pytest

import sig_restate
from close_kmers_amd import signatures, synth
from helpers import GOLDEN

FIXTURE = os.path.join(GOLDEN, "signatures", "hand_checked.json")


def test_restatement_matches_hand_checked_fixture():
    fx = json.load(open(FIXTURE))
    seqs = [s.encode() for s in fx["sequences"]]
    recs, stats = sig_restate.select(seqs, fx["seq_function"], fx["n_functions"])
    assert stats == fx["stats"]
    assert [int(r["raw_key"]).to_bytes(8, "big").decode() for r in recs] == [r["kmer"] for r in fx["records"]]
    for got, want in zip(recs, fx["records"]):
        for f in ("function_index", "n_tuples", "n_best", "median_offset"):
            assert int(got[f]) == want[f], (want["kmer"], f)
        assert (int(got["code"]) <= synth.MAX_ENCODED) == want["storable"]
        assert int(np.float32(got["function_wt"]).view(np.uint32)) == want["function_wt_bits"], want["kmer"]
    # the cases the fixture exists for
    by = {r["kmer"]: r for r in fx["records"]}
    assert (by["ACDEFGHI"]["n_best"], by["ACDEFGHI"]["n_tuples"]) == (4, 5)            # exactly 80%: kept
    assert {(d["n_best"], d["n_tuples"]) for d in fx["dropped"]} >= {(3, 4), (7, 9)}  # 75%, 77.8%: dropped
    assert by["QQRRSSTT"]["offsets"] == [8, 8, 17, 35] and by["QQRRSSTT"]["median_offset"] == 17  # upper middle
    assert by["GGHHIIKK"]["offsets"] == [17, 35] and by["GGHHIIKK"]["median_offset"] == 35
    assert not by["acdefghi"]["storable"]


def test_keep_test_is_the_float_form():
    assert sig_restate.keep(4, 5) and not sig_restate.keep(3, 4) and not sig_restate.keep(7, 9)
    assert sig_restate.keep(8, 10) and sig_restate.keep(4000, 5000) and not sig_restate.keep(3999, 5000)
    # float(count) rounds above 2^24: 16777217 -> 16777216, whose 0.8 is 13421772.8 -> float 13421773
    assert sig_restate.keep(13421773, 16777217) and not sig_restate.keep(13421772, 16777217)


def test_entries_truncate_the_median_to_uint16():
    recs = np.zeros(2, sig_restate.RECORD_DTYPE)
    recs["median_offset"] = [70000, 65535]
    assert sig_restate.entries(recs)[3].tolist() == [70000 - 65536, 65535]


# ---- front end -----------------------------------------------------------------

def _genomes(n, ids_of):
    return [[i.encode() for i in ids_of(g)] for g in range(n)]


def test_min_reps_boundary_and_keep_list():
    idf = {b"a%d" % g: b"alpha" for g in range(5)}
    idf.update({b"b%d" % g: b"beta" for g in range(4)})
    idf.update({b"c0": b"gamma", b"e0": b""})
    genomes = _genomes(5, lambda g: [f"a{g}", f"b{g}", f"c{g}", f"e{g}", "unknown"])
    assert signatures.kept_functions(idf, genomes) == [b"alpha"]                  # 5 of 5 kept, 4 of 5 not
    assert signatures.kept_functions(idf, genomes, min_reps=4) == [b"alpha", b"beta"]
    assert signatures.kept_functions(idf, genomes, keep=["gamma"]) == [b"alpha", b"gamma"]
    assert signatures.kept_functions(idf, genomes, keep=["absent"]) == [b"alpha"]  # never seen: not created
    # the same id twice in one genome is one genome
    assert signatures.kept_functions({b"x": b"f"}, [[b"x", b"x"]] * 1, min_reps=2) == []


def test_sorted_numbering_is_bytewise():
    idf = {b"1": b"beta", b"2": b"Zeta", b"3": b"alpha", b"4": b"\xc3\xa9psilon", b"5": b"Alpha 2"}
    got = signatures.kept_functions(idf, [[b"1", b"2", b"3", b"4", b"5"]], min_reps=1)
    assert got == [b"Alpha 2", b"Zeta", b"alpha", b"beta", b"\xc3\xa9psilon"]


def test_definitions_override_order_and_columns(tmp_path):
    a, b = tmp_path / "a.tsv", tmp_path / "b.tsv"
    a.write_bytes(b"p1\tfirst\textra\np2\tkept as is\nno tab here\np3\tgone\n")
    b.write_bytes(b"p1\tsecond\np3\t\n\np4\tlast line without newline")
    assert signatures.read_definitions([str(a), str(b)]) == {b"p1": b"second", b"p2": b"kept as is", b"p3": b"",
                                                               b"p4": b"last line without newline"}
    assert signatures.read_definitions([str(b), str(a)])[b"p1"] == b"first"


def test_fasta_and_labels(tmp_path):
    fa = tmp_path / "g.fa"
    fa.write_bytes(b">p1 some text\nACDE\r\nFG HI\n>p2\n\n>\nKLMN\n>p3\tx\nacd*\n")
    recs = signatures.read_fasta(str(fa))
    assert recs == [(b"p1", b"ACDEFGHI"), (b"p2", b""), (b"p3", b"acd*")]
    res, off, fn = signatures.label({b"p1": b"f", b"p3": b"g"}, [recs], [b"f"])
    assert bytes(res) == b"ACDEFGHIacd*" and off.tolist() == [0, 8, 8, 12] and fn.tolist() == [0, -1, -1]


def test_function_index_bytes(tmp_path):
    assert signatures.function_index_bytes([b"Alpha", b"beta (EC 1.1.1.1)"]) == b"0\tAlpha\n1\tbeta (EC 1.1.1.1)\n"
    assert signatures.function_index_bytes([]) == b""
    signatures.write_indexes(str(tmp_path / "d"), [b"f0", b"f1"])
    assert (tmp_path / "d" / "function.index").read_bytes() == b"0\tf0\n1\tf1\n"
    assert (tmp_path / "d" / "otu.index").read_bytes() == b""


def test_prime_rule_around_list_entries():
    """The size is the first listed prime p > 3 * KS.  No listed size is a
    multiple of 3, so 3 * KS never equals one; the rule is pinned at the
    nearest values on both sides and through the list's unsorted tail."""
    primes = synth.BUILDER_PRIMES
    assert all(p % 3 for p in primes)
    assert signatures.table_size(0) == 3769
    assert signatures.table_size(1256) == 3769      # 3 KS = 3768, one below
    assert signatures.table_size(1257) == 6337      # 3 KS = 3771, the first value above
    assert signatures.table_size(357913941) == 1 << 30          # 3 KS = 2^30 - 1
    assert signatures.table_size(357913942) == 1400303159       # 3 KS = 2^30 + 2
    assert signatures.table_size(715827883) == 3559786523       # 3 KS = 2^31 + 1: 1190492993 is skipped
    with pytest.raises(ValueError):
        signatures.table_size(6461346257)


def test_select_without_device_is_edevice(kgx):
    """No device, no answer: the selection never runs on the CPU."""
    res = np.frombuffer(b"ACDEFGHIKLMN", np.uint8)
    with pytest.raises(kgx.KgxError) as e:
        kgx.Signatures(res, [0, 12], [0], 1, device=kgx.device_count())
    assert e.value.code == kgx.KGX_EDEVICE
    if kgx.device_count() == 0:
        with pytest.raises(kgx.KgxError) as e:
            kgx.Signatures(res, [0, 12], [0], 1)
        assert e.value.code == kgx.KGX_EDEVICE
    assert kgx.SIG_RECORD_DTYPE.itemsize == 40
