"""Signature selection on the device (csrc/kgx_sig.hip) against the CPU
restatement tests/sig_restate.py.

The edge corpus (sig_corpora.edge_corpus) holds, over a 4-letter alphabet so
that sets collide: lengths 0, 7, 8, 9 .. 60; X, * and lower-case stretches,
with a lower-case k-mer that is kept; unlabelled (-1) copies of labelled
sequences; a k-mer repeated inside one sequence; one 70,000-residue sequence
(medians above 65535: the uint16 truncation); sets of 16 | 17 and 4096 | 4097
tuples (the thread | wave | workgroup thresholds); a k-mer in 100 sequences
(wave path); one in 5,000 at exactly 80% (workgroup path, kept) and its twin
at 3999 of 5000 (dropped).

Weights: every record is compared and must be within 1 f32 ulp -- the two
double logs are each within ~1 double ulp of libm's, their sum is rounded to
f32, so the results differ only when the sum lies within ~2^-50 of an f32
rounding boundary, and then by one step.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import sig_corpora
import sig_restate
from close_kmers_amd import build as kbuild
from close_kmers_amd import synth
from helpers import GOLDEN, pack, write_fasta

pytestmark = pytest.mark.gpu

INT_FIELDS = ("raw_key", "code", "function_index", "n_tuples", "n_best", "median_offset")
WANT = 1 | 2 | 8  # hits, calls, best


def _pack(seqs):
    return pack([(str(i), s) for i, s in enumerate(seqs)])


def _compare(got, gstats, want, wstats, what):
    """Integer fields and statistics equal, weights within 1 ulp; returns the
    number of weights that are not bit-equal."""
    assert gstats == wstats, what
    assert len(got) == len(want), what
    for f in INT_FIELDS:
        bad = np.nonzero(got[f] != want[f])[0]
        assert not len(bad), (what, f, bad[:5], got[bad[:5]], want[bad[:5]])
    d = sig_restate.ulp_distance(got["function_wt"], want["function_wt"])
    differ = int((d != 0).sum())
    print(f"{what}: {len(got)} records, {differ} weights not bit-equal, max distance {int(d.max()) if len(d) else 0} ulp")
    assert not len(d) or d.max() <= 1, (what, np.nonzero(d > 1)[0][:5])
    return differ


@pytest.fixture(scope="module")
def edge(gpu):
    seqs, fn, nf = sig_corpora.edge_corpus()
    want, wstats = sig_restate.select(seqs, fn, nf)
    res, off = _pack(seqs)
    with gpu.Signatures(res, off, fn, nf) as sig:
        yield sig, want, wstats


def test_edge_records_and_stats(edge):
    sig, want, wstats = edge
    got = sig.records()
    assert (np.diff(got["raw_key"].astype(np.uint64)) > 0).all()  # ascending, unique
    _compare(got, sig.stats(), want, wstats, "edge corpus")
    # the corpus does hold what its description says
    key = lambda k: int.from_bytes(k, "big")  # noqa: E731
    by = {int(r["raw_key"]): r for r in got}
    assert (by[key(b"TVWYTVWY")]["n_best"], by[key(b"TVWYTVWY")]["n_tuples"]) == (4000, 5000)
    assert key(b"YWVTYWVT") not in by
    assert by[key(b"SSSSTTTT")]["n_tuples"] == 100 and by[key(b"KLKLKLKL")]["n_tuples"] == 3
    assert by[key(b"wywywywy")]["code"] > synth.MAX_ENCODED
    assert got["median_offset"].max() == 70000
    assert wstats["n_kept"] > wstats["n_storable"] > 0 and wstats["n_sets"] > wstats["n_kept"]


def test_edge_image_holds_the_storable_records(edge, gpu):
    sig, _, wstats = edge
    got = sig.records()
    keys, fI, oI, avg, wt = sig_restate.entries(got)  # the device's own records as entries
    assert int(avg.max()) < 65536 and 70000 - 65536 in avg.tolist()
    img, stored = sig.image()
    with img:
        assert img.num_sigs == wstats["num_sigs_rule"] and stored == wstats["n_storable"] == len(keys)
        t = img.download()
        t = t[t["which_kmer"] <= synth.MAX_ENCODED]
        t = t[np.argsort(t["which_kmer"])]
        assert np.array_equal(t["which_kmer"], keys)  # records are in raw-key order = code order for upper case
        assert np.array_equal(t["function_index"], fI) and np.array_equal(t["otu_index"], oI)
        assert np.array_equal(t["avg_from_end"], avg)
        assert np.array_equal(t["function_wt"].view(np.uint32), wt.view(np.uint32))
        # each stored k-mer is found by a probe of itself (9 residues: one window)
        kmers = [int(k).to_bytes(8, "big") + b"A" for k in got["raw_key"][got["code"] <= synth.MAX_ENCODED]]
        res, off = _pack(kmers)
        with gpu.Context(img) as ctx:
            r = ctx.process_batch(res, off, want=gpu.WANT_HITS)
        assert np.array_equal(np.diff(r.hit_offsets.astype(np.int64)), np.ones(len(kmers), np.int64))
        assert np.array_equal(r.hits["which_kmer"], keys) and np.array_equal(r.hits["function_index"], fI)
        assert np.array_equal(r.hits["avg_from_end"], avg) and (r.hits["pos"] == 0).all()
        assert np.array_equal(r.hits["function_wt"].view(np.uint32), wt.view(np.uint32))
    with pytest.raises(gpu.KgxError) as e:  # half full, as kgx_image_build
        sig.image(num_sigs=2 * wstats["n_storable"])
    assert e.value.code == -7


def test_hand_checked_fixture_on_device(gpu):
    fx = json.load(open(os.path.join(GOLDEN, "signatures", "hand_checked.json")))
    seqs = [s.encode() for s in fx["sequences"]]
    res, off = _pack(seqs)
    with gpu.Signatures(res, off, fx["seq_function"], fx["n_functions"]) as sig:
        got, stats, ms = sig.records(), sig.stats(), sig.stage_ms()
    assert tuple(ms) == gpu.SIG_STAGES and all(v >= 0 for v in ms.values()) and ms["order"] > 0
    assert stats == fx["stats"]
    assert [int(k).to_bytes(8, "big").decode() for k in got["raw_key"]] == [r["kmer"] for r in fx["records"]]
    for f in ("function_index", "n_tuples", "n_best", "median_offset"):
        assert got[f].tolist() == [r[f] for r in fx["records"]], f
    want_wt = np.array([r["function_wt_bits"] for r in fx["records"]], np.uint32).view(np.float32)
    assert sig_restate.ulp_distance(got["function_wt"], want_wt).max() <= 1


def test_offsets_need_not_start_at_zero(gpu):
    seqs, fn, nf = sig_corpora.family_corpus()
    res, off = _pack(seqs)
    with gpu.Signatures(res, off, fn, nf) as a, \
            gpu.Signatures(np.concatenate([np.full(13, ord("A"), np.uint8), res]), off + np.uint64(13), fn, nf) as b:
        ra, rb = a.records(), b.records()
        assert a.stats() == b.stats() and len(ra) == len(rb)
        for f in ra.dtype.names:  # field by field: the struct's padding is nobody's to compare
            assert ra[f].tobytes() == rb[f].tobytes(), f


def test_family_image_calls_like_the_oracle(gpu, oracle_lib, tmp_path):
    seqs, fn, nf = sig_corpora.family_corpus()
    want, wstats = sig_restate.select(seqs, fn, nf)
    res, off = _pack(seqs)
    d = str(tmp_path / "data")
    with gpu.Signatures(res, off, fn, nf) as sig:
        differ = _compare(sig.records(), sig.stats(), want, wstats, "family corpus")
        img, stored = sig.image()
        with img:
            assert stored == wstats["n_storable"]
            own = img.download()
            os.makedirs(d)
            img.save(d)
    # the restated image, unless some weight differs in its last bit: then the device's own table
    table = sig_restate.table(want) if differ == 0 else own
    ref = oracle_lib.process_batch(table, res, off, want=WANT)
    assert (ref.best["kind"] == 1).all() and np.array_equal(ref.best["function_index"], np.array(fn))  # the fixture
    with gpu.Image.open(d) as img, gpu.Context(img) as ctx:
        assert img.num_sigs == wstats["num_sigs_rule"]
        got = ctx.process_batch(res, off, want=WANT)
    assert oracle_lib.diff_batch(got, ref, WANT) == {"hits": [], "calls": [], "best": []}
    assert len(got.hits) > 1000 and len(got.calls) >= len(seqs)


def test_error_returns(gpu):
    res, off = _pack([b"ACDEFGHIKL", b"ACDEFGHIKL"])
    with pytest.raises(gpu.KgxError) as e:
        gpu.Signatures(res, off, [0, 2], 2)
    assert e.value.code == -6 and "n_functions" in gpu.last_error()
    with gpu.Signatures(res, off, [0, -1], 2) as sig:  # -1 is no function, not an error
        assert sig.stats()["n_tuples"] == 3
    # empty corpora: no sequence; sequences but no window; windows but no tuple
    for seqs, fn in (([], []), ([b"ACDEFGH", b""], [0, 0]), ([b"ACDEXGHIKL"], [0]), ([b"ACDEFGHIKL"], [-1])):
        res, off = _pack(seqs)
        with gpu.Signatures(res, off, fn, 1) as sig:
            st = sig.stats()
            assert len(sig.records()) == 0 and st["n_kept"] == 0 and st["n_tuples"] == 0
            assert st["num_sigs_rule"] == synth.BUILDER_PRIMES[0]
            img, stored = sig.image()
            with img:
                assert img.num_sigs == synth.BUILDER_PRIMES[0] and stored == 0


def test_cli_builds_a_directory_the_query_driver_reads(gpu, oracle_lib, tmp_path):
    """TSV + FASTA -> data directory -> kgx_query text == the oracle's over the same directory."""
    from close_kmers_amd import signatures
    seqs, fn, nf = sig_corpora.family_corpus()
    names = ["zeta", "Alpha", "beta", "gamma", "delta", "rare"]  # sorted: Alpha beta delta gamma rare zeta
    defs = tmp_path / "defs.tsv"
    fastas = []
    with open(defs, "w") as f:
        for g in range(6):  # genome g holds member g of every family; "rare" only in genomes 0-2
            recs = []
            for fam in range(6):
                if names[fam] == "rare" and g > 2:
                    continue
                rid = f"fig|{g}.1.peg.{fam}"
                f.write(f"{rid}\t{names[fam]}\textra column\n")
                recs.append((rid, seqs[fam * 6 + g].decode()))
            fastas.append(str(tmp_path / f"g{g}.fa"))
            write_fasta(fastas[-1], recs)
    out = str(tmp_path / "data")
    cmd = [sys.executable, "-m", "close_kmers_amd.signatures", "--definitions", str(defs), "--fasta", *fastas,
           "--min-reps", "4", "--keep-function", "rare", "--out", out]
    r = subprocess.run(cmd, capture_output=True, timeout=300, cwd=kbuild.ROOT)
    assert r.returncode == 0, r.stderr.decode()
    stats = json.loads(r.stdout)
    assert stats["n_functions"] == 6 and stats["n_stored"] == stats["n_storable"] > 1000
    assert open(os.path.join(out, "function.index"), "rb").read() == \
        signatures.function_index_bytes([n.encode() for n in sorted(names)])
    assert open(os.path.join(out, "otu.index"), "rb").read() == b""
    q = subprocess.run([kbuild.QUERY, out, fastas[0], "query"], capture_output=True, timeout=300)
    assert q.returncode == 0, q.stderr.decode()
    assert q.stdout == oracle_lib.query_text(out, fastas[0], "query") and b"Alpha" in q.stdout
