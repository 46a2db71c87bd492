"""Signature selection in key-range passes (kgx_sig_select_passes,
csrc/kgx_sig.hip and the planner csrc/kgx_sig_plan.h): under
any budget of tuples per pass the records -- weights included, as bits -- the
statistics and the image are those of the single pass, and the passes are the
greedy packing of the device's own counts.

Budgets of the edge corpus (tests/sig_corpora.py; T tuples, W windows, M =
5,000 the largest set, D the largest count of a first-two-letters bin):
W (nothing is counted), T (planned, one pass), D (every bin fits: cuts at
depth 0 only), (D + M) // 2 and M (bins above the budget are refined).  A
pass is never split below a set, so M - 1 is KGX_ERANGE.

The lower-case k-mer: ranks put upper case before lower, so under every budget
wywywywy lies in no earlier pass than any upper-case key; at budget M it lies
in a later one, because the last upper-case set, YWVTYWVT of exactly M tuples,
fills its pass.
"""
import collections
import math
import os
import subprocess

import numpy as np
import pytest

import sig_corpora
import sig_restate
from close_kmers_amd import build as kbuild
from close_kmers_amd import synth
from helpers import pack, write_fasta
from test_gpu_signatures import INT_FIELDS, _compare

pytestmark = pytest.mark.gpu

KGX_EINVAL, KGX_ERANGE = -1, -6


def _pack(seqs):
    return pack([(str(i), s) for i, s in enumerate(seqs)])


def _key(kmer: bytes) -> int:
    return int.from_bytes(kmer, "big")


def _set_sizes(seqs, fn) -> collections.Counter:
    """k-mer -> its tuples, by sig_restate's letters."""
    sizes = collections.Counter()
    for s, f in zip(seqs, fn):
        if f < 0:
            continue
        for p in range(len(s) - 7):
            if all(c in sig_restate.LETTERS for c in s[p:p + 8]):
                sizes[bytes(s[p:p + 8])] += 1
    return sizes


def _bits_equal(a, b, what):
    assert len(a) == len(b), what
    for f in a.dtype.names:  # field by field: the struct's padding is nobody's to compare
        assert a[f].tobytes() == b[f].tobytes(), (what, f)


def _check_passes(passes, stats, budget):
    """What every list of passes satisfies; returns it."""
    T = stats["n_tuples"]
    for i, p in enumerate(passes):
        assert p["lo_key"] < p["hi_key"], (budget, i, p)
        assert i == 0 or passes[i - 1]["hi_key"] <= p["lo_key"], (budget, i)
        assert 0 < p["n_tuples"] <= budget, (budget, i, p)
        assert 0 < p["n_sets"] <= p["n_tuples"] and p["n_kept"] <= p["n_sets"], (budget, i, p)
    for k in ("n_tuples", "n_sets", "n_kept"):
        assert sum(p[k] for p in passes) == stats[k], (budget, k)
    assert math.ceil(T / budget) <= len(passes) <= 2 * T / budget + 1, (budget, len(passes))
    return passes


def _pass_of(passes, key: int) -> int:
    hit = [i for i, p in enumerate(passes) if p["lo_key"] <= key < p["hi_key"]]
    assert len(hit) == 1, (key, hit)
    return hit[0]


@pytest.fixture(scope="module")
def edge(gpu):
    seqs, fn, nf = sig_corpora.edge_corpus()
    want, wstats = sig_restate.select(seqs, fn, nf)
    sizes = _set_sizes(seqs, fn)
    res, off = _pack(seqs)
    with gpu.Signatures(res, off, fn, nf) as sig:
        single = sig.records(), sig.stats(), sig.passes()
    return {"res": res, "off": off, "fn": fn, "nf": nf, "want": want, "wstats": wstats, "sizes": sizes,
            "single": single}


def _budgets(edge):
    sizes, st = edge["sizes"], edge["wstats"]
    M = max(sizes.values())
    depth0 = collections.Counter()
    for kmer, n in sizes.items():
        depth0[kmer[:2]] += n
    D = max(depth0.values())
    return M, D, st["n_tuples"], st["n_windows"]


def test_edge_corpus_is_what_the_budgets_assume(edge):
    M, D, T, W = _budgets(edge)
    assert M == 5000 and edge["want"]["n_tuples"].max() == 5000
    assert sum(edge["sizes"].values()) == T
    assert M < (D + M) // 2 < D < T < W  # five different budgets, two of them below a depth-0 bin
    recs, stats, passes = edge["single"]
    assert passes == [{"lo_key": 0, "hi_key": 2 ** 64 - 1, "n_tuples": T, "n_sets": stats["n_sets"],
                       "n_kept": stats["n_kept"]}]


@pytest.mark.parametrize("which", ["windows", "tuples", "depth0", "refined", "largest_set"])
def test_edge_budget_sweep(edge, gpu, which):
    M, D, T, W = _budgets(edge)
    B = {"windows": W, "tuples": T, "depth0": D, "refined": (D + M) // 2, "largest_set": M}[which]
    with gpu.Signatures(edge["res"], edge["off"], edge["fn"], edge["nf"], max_pass_tuples=B) as sig:
        got, stats, passes, ms = sig.records(), sig.stats(), sig.passes(), sig.stage_ms()
    srecs, sstats, _ = edge["single"]
    _bits_equal(got, srecs, which)  # weights included
    assert stats == sstats
    _compare(got, stats, edge["want"], edge["wstats"], f"edge corpus, {B} tuples per pass")
    assert tuple(ms) == gpu.SIG_STAGES and all(v >= 0 for v in ms.values()) and ms["order"] > 0
    _check_passes(passes, stats, B)
    print(f"{which}: budget {B}, {len(passes)} passes for {T} tuples")
    if which in ("windows", "tuples"):
        assert len(passes) == 1
        if which == "windows":  # within the budget: nothing is counted, every key is the pass's
            assert (passes[0]["lo_key"], passes[0]["hi_key"]) == (0, 2 ** 64 - 1)
        else:  # planned: from the first bin that holds a tuple to the end of the last
            first, last = min(edge["sizes"])[:2], max(edge["sizes"])[:2]
            assert passes[0]["lo_key"] == _key(first + bytes(6))
            assert passes[0]["hi_key"] == _key(last + bytes(6)) + (1 << 48)
        return
    assert len(passes) > 1
    deep = [p for p in passes if p["lo_key"] & ((1 << 48) - 1) or p["hi_key"] & ((1 << 48) - 1)]
    assert bool(deep) == (which != "depth0"), (which, deep[:3])
    # every record lies in exactly one pass, in key order; upper case before lower
    at = [_pass_of(passes, int(k)) for k in got["raw_key"]]
    assert at == sorted(at)
    counts = collections.Counter(at)
    assert [counts[i] for i in range(len(passes))] == [p["n_kept"] for p in passes]
    upper = [i for i, r in zip(at, got) if r["code"] <= synth.MAX_ENCODED]
    lower = _pass_of(passes, _key(b"wywywywy"))
    assert _key(b"wywywywy") in got["raw_key"].tolist() and lower >= max(upper)
    if which == "largest_set":
        assert lower > max(upper)
        twin = passes[_pass_of(passes, _key(b"YWVTYWVT"))]  # dropped, and a pass of its own
        assert (twin["n_tuples"], twin["n_sets"], twin["n_kept"]) == (M, 1, 0)


def test_error_returns(edge, gpu):
    M, _, _, _ = _budgets(edge)
    with pytest.raises(gpu.KgxError) as e:
        gpu.Signatures(edge["res"], edge["off"], edge["fn"], edge["nf"], max_pass_tuples=M - 1)
    # the first set of M tuples in key order
    assert e.value.code == KGX_ERANGE and "TVWYTVWY" in gpu.last_error() and str(M) in gpu.last_error()
    for B in (2 ** 31, 2 ** 40, 2 ** 64 - 1):
        with pytest.raises(gpu.KgxError) as e:
            gpu.Signatures(edge["res"], edge["off"], edge["fn"], edge["nf"], max_pass_tuples=B)
        assert e.value.code == KGX_EINVAL and "max_pass_tuples" in gpu.last_error()
    with gpu.Signatures(edge["res"], edge["off"], edge["fn"], edge["nf"], max_pass_tuples=2 ** 31 - 1) as sig:
        assert sig.stats() == edge["single"][1] and len(sig.passes()) == 1


def _family_files(tmp_path):
    """The family corpus as six genomes with a definitions file (as the CLI test lays it out)."""
    seqs, _, _ = sig_corpora.family_corpus()
    names = ["zeta", "Alpha", "beta", "gamma", "delta", "rare"]
    defs = str(tmp_path / "defs.tsv")
    fastas = []
    with open(defs, "w") as f:
        for g in range(6):
            recs = []
            for fam in range(6):
                if names[fam] == "rare" and g > 2:
                    continue
                rid = f"fig|{g}.1.peg.{fam}"
                f.write(f"{rid}\t{names[fam]}\n")
                recs.append((rid, seqs[fam * 6 + g].decode()))
            fastas.append(str(tmp_path / f"g{g}.fa"))
            write_fasta(fastas[-1], recs)
    return defs, fastas


def test_family_image_and_data_directory(gpu, tmp_path):
    from close_kmers_amd import signatures
    seqs, fn, nf = sig_corpora.family_corpus()
    res, off = _pack(seqs)
    with gpu.Signatures(res, off, fn, nf) as one:
        T = one.stats()["n_tuples"]
        B = T // 4
        with gpu.Signatures(res, off, fn, nf, max_pass_tuples=B) as many:
            passes = _check_passes(many.passes(), many.stats(), B)
            assert len(passes) >= 4 and many.stats() == one.stats()
            _bits_equal(many.records(), one.records(), "family corpus")
            (ia, sa), (ib, sb) = one.image(), many.image()
            with ia, ib:
                assert sa == sb == one.stats()["n_storable"] and ia.num_sigs == ib.num_sigs
                ta, tb = ia.download(), ib.download()
                ta, tb = ta[np.argsort(ta["which_kmer"], kind="stable")], tb[np.argsort(tb["which_kmer"], kind="stable")]
                assert ta.tobytes() == tb.tobytes()
                assert int((ta["which_kmer"] <= synth.MAX_ENCODED).sum()) == sa
    # the front end: the same directory, read by the query driver to the same text
    defs, fastas = _family_files(tmp_path)
    texts, stats = [], []
    for name, budget in (("single", 0), ("passes", 1000)):
        out = str(tmp_path / name)
        stats.append(signatures.build_data_dir([defs], fastas, out, min_reps=4, keep=["rare"],
                                               max_pass_tuples=budget))
        q = subprocess.run([kbuild.QUERY, out, fastas[0], "query"], capture_output=True, timeout=300)
        assert q.returncode == 0, q.stderr.decode()
        texts.append(q.stdout)
        assert os.path.getsize(os.path.join(out, "kmer.table.mem_map")) > 0
    assert stats[0]["n_passes"] == 1 and stats[1]["n_passes"] >= 4 and stats[1]["n_tuples"] > 3000
    assert {k: v for k, v in stats[0].items() if k != "n_passes"} == \
        {k: v for k, v in stats[1].items() if k != "n_passes"}
    assert texts[0] == texts[1] and b"Alpha" in texts[0]


def test_unchanged_behaviour_under_a_budget(gpu):
    # empty corpora: no sequence; sequences but no window; windows but no tuple; nothing labelled
    for seqs, fn in (([], []), ([b"ACDEFGH", b""], [0, 0]), ([b"ACDEXGHIKL"], [0]), ([b"ACDEFGHIKL"], [-1])):
        res, off = _pack(seqs)
        with gpu.Signatures(res, off, fn, 1) as a, gpu.Signatures(res, off, fn, 1, max_pass_tuples=1) as b:
            assert a.passes() == b.passes() == [] and a.stats() == b.stats()
            assert len(b.records()) == 0 and b.stats()["num_sigs_rule"] == synth.BUILDER_PRIMES[0]
            assert tuple(b.stage_ms()) == gpu.SIG_STAGES and all(v >= 0 for v in b.stage_ms().values())
            img, stored = b.image()
            with img:
                assert img.num_sigs == synth.BUILDER_PRIMES[0] and stored == 0
    # offsets that do not start at zero, in passes
    seqs, fn, nf = sig_corpora.family_corpus()
    res, off = _pack(seqs)
    shifted = np.concatenate([np.full(13, ord("A"), np.uint8), res])
    with gpu.Signatures(res, off, fn, nf) as a, \
            gpu.Signatures(shifted, off + np.uint64(13), fn, nf, max_pass_tuples=500) as b:
        assert a.stats() == b.stats() and len(b.passes()) >= 8
        _bits_equal(a.records(), b.records(), "shifted offsets")
        for f in INT_FIELDS:
            assert np.array_equal(a.records()[f], b.records()[f])
