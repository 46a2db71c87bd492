"""The designed fq corpus (tests/fq_restate.py) without a GPU: the Python
restatement equals the oracle on every read, every mutant (a slip the
fragment kernels could have) differs from the oracle on some read, and the
corpus holds the edges it promises.  tests/test_gpu_fq_edges.py then runs the
same reads through the device paths."""
import numpy as np
import pytest

import fq_restate as fr


@pytest.fixture(scope="module")
def corpus():
    return fr.corpus()


@pytest.fixture(scope="module")
def oracle_fragments(corpus, oracle_lib):
    return {name: [oracle_lib.fq_fragments(r) for r in reads] for name, reads in corpus.items()}


def test_corpus_size(corpus):
    assert set(corpus) == {"lengths", "sweep140", "sweep197", "sweep262", "pairs", "every_byte", "neighbours"}
    assert [len(r) for r in corpus["lengths"]] == list(fr.LENGTHS)
    for L in fr.SWEEP_LENGTHS:
        assert len(corpus[f"sweep{L}"]) == 6 * (L - 2) and {len(r) for r in corpus[f"sweep{L}"]} == {L}
    assert len(corpus["every_byte"]) == 256 * 7 * 3
    n = sum(len(v) for v in corpus.values())
    assert 11000 < n < 13000 and sum(len(r) for v in corpus.values() for r in v) < 3 << 20
    assert fr.corpus() is corpus  # built once, shared


def test_restatement_equals_oracle_on_every_read(corpus, oracle_fragments):
    n = 0
    for name, reads in corpus.items():
        for i, dna in enumerate(reads):
            want = oracle_fragments[name][i]
            assert fr.fragments(dna) == want, (name, i, dna)
            n += len(want)
    assert n > 60000


@pytest.mark.parametrize("mutant", sorted(fr.MUTANTS))
def test_every_mutant_differs_from_the_oracle(corpus, oracle_fragments, mutant):
    f = fr.MUTANTS[mutant]
    caught = {}
    for name, reads in corpus.items():
        for i in range(len(reads)):
            if f(reads, i) != oracle_fragments[name][i]:
                caught[name] = i
                break
    assert caught, mutant
    # the classes built for a slip are among those that catch it
    designed = {"keep > 11": "pairs", "keep > 9": "pairs", "no TGA": "sweep197", "N a base": "every_byte",
                "U not a base": "every_byte", "frame -k from offset k": "lengths",
                "complement without reversal": "sweep140", "stop dropped at a 64-base edge": "sweep262",
                "stop across a read boundary": "neighbours"}
    assert designed[mutant] in caught, (mutant, caught)


def test_anchor_translation_is_the_moved_helper():
    """_translate_anchor (moved here from test_gpu_fq.py): forward and reverse
    anchors of a read give the restatement's fragments."""
    dna = b"GGCTAAgcuGCCGGNGCGCCGGCGCGGCCGCGGCGCCGCGCGGCGCCGGCGTTAGC"
    s = fr.frame_proteins(dna)
    assert fr._translate_anchor(dna, 0 << 1, len(dna) // 3) == s[0][1]
    assert fr._translate_anchor(dna, (len(dna) - 2) << 1 | 1, (len(dna) - 1) // 3) == s[4][1]


def _runs(corpus, names):
    for name in names:
        for dna in corpus[name]:
            for frame, (nc, runs) in fr.frame_runs(dna).items():
                for start, n in runs:
                    yield frame, nc, start, n


def test_corpus_has_runs_of_10_and_11_at_every_edge(corpus):
    """Per frame: a kept run of exactly 11 and a dropped run of exactly 10
    that ends at the frame's end, whose last codon is codon 63, and that
    starts at codon 0."""
    seen = set()
    for frame, nc, start, n in _runs(corpus, ("sweep197", "sweep262", "pairs")):
        if n in (10, 11):
            if start + n == nc:
                seen.add((frame, n, "frame end"))
            if start + n - 1 == 63:
                seen.add((frame, n, "codon 63"))
            if start == 0:
                seen.add((frame, n, "codon 0"))
    want = {(f, n, e) for f in fr.FRAMES for n in (10, 11) for e in ("frame end", "codon 63", "codon 0")}
    assert want <= seen, sorted(want - seen)


def test_corpus_has_each_spelling_at_each_step_and_block_edge(corpus):
    """Per spelling: a stop whose last base has index 62, 63, 0, 1, 2 (mod 64)
    and 7, 0, 1 (mod 8), in blocks 0..4; its written forms include lower case
    and U."""
    seen64, seen8, blocks, forms = set(), set(), set(), set()
    for L in fr.SWEEP_LENGTHS:
        for dna in corpus[f"sweep{L}"]:
            for stop, q in fr.designed_stops(dna):
                seen64.add((stop, q % 64))
                seen8.add((stop, q % 8))
                blocks.add((stop, q // 64))
                forms.add((stop, bytes(dna[q - 2:q + 1])))
    for stop in fr.SPELLINGS:
        assert {(stop, m) for m in (62, 63, 0, 1, 2)} <= seen64, stop
        assert {(stop, m) for m in (7, 0, 1)} <= seen8, stop
        assert {(stop, b) for b in range(5)} <= blocks, stop
        for form in (stop, stop.lower(), stop.replace("T", "U"), stop.lower().replace("t", "u")):
            assert (stop, form.encode()) in forms, (stop, form)


def test_corpus_has_reads_around_short_read_with_all_frames(corpus, oracle_fragments):
    """Reads of 192..197 bases (a frame of exactly 64 codons, the wave path's
    last length 194 and the serial path's first) with a fragment in each frame."""
    for L in range(192, 198):
        i = fr.LENGTHS.index(L)
        assert len(corpus["lengths"][i]) == L
        assert {f for f, _ in oracle_fragments["lengths"][i]} == set(fr.FRAMES), L
    # and with a stop in them: the 197-base sweep
    assert any(len({f for f, _ in w}) == 6 and len(w) == 7 for w in oracle_fragments["sweep197"])


def test_every_byte_class_covers_all_values_and_only_bases_stop(corpus, oracle_fragments):
    reads = corpus["every_byte"]
    assert {b for r in reads for b in r[58:63]} == set(range(256))
    stops = 0
    for k, (dna, want) in enumerate(zip(reads, oracle_fragments["every_byte"])):
        b, pat, o = k // 21, fr.BYTE_PATTERNS[k % 21 // 3], 58 + k % 3
        at = o + pat.index("?")
        assert dna[at] == b
        # the stops the byte completes: those that go when it is no base
        mine = set(fr.designed_stops(dna)) - set(fr.designed_stops(dna[:at] + b"N" + dna[at + 1:]))
        if bytes([b]) in b"ACGTUacgtu":
            stops += len(mine)
        else:  # one 'X' codon per frame, and no run broken by it
            assert not mine and sorted(f for f, s in want if "X" in s) == sorted(fr.FRAMES), (k, b)
            assert sum(s.count("X") for _, s in want) == 6
            assert want == fr.fragments(dna[:at] + b"N" + dna[at + 1:])  # any such byte is as good as N
    # TA[AG] T[AGTU]A [TU]AA [TUC]TA C[TU]A TC[A]: 14 bytes, in both cases, at three offsets
    assert stops >= 14 * 2 * 3


def test_neighbours_spell_stops_only_across_read_boundaries(corpus, oracle_fragments):
    """The class' reads spell stops across their boundaries (with empty and
    1-2 base reads between): none may show in a read's own fragments."""
    reads = corpus["neighbours"]
    text = b"".join(reads)
    ends = set(np.cumsum([len(r) for r in reads]).tolist())  # index of each later read's first base
    across = [(s, q) for s, q in fr.designed_stops(text) if q in ends or q - 1 in ends]
    assert {s for s, _ in across} == set(fr.SPELLINGS)
    assert len(across) > 60
    assert any(len(r) == 0 for r in reads) and any(len(r) == 1 for r in reads) and any(len(r) == 2 for r in reads)
    assert sum(len(w) for w in oracle_fragments["neighbours"]) > 300
