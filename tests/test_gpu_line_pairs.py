"""The pairs layout of the line index (KGX_LINE_PAIRS, csrc/kgx_line_home.h): a
7-mer S owns the aligned 128-byte block of lines 2k and 2k + 1; keys that end
in S are homed on line 2k, keys that begin with S on line 2k + 1, so every
stored key has two records and a line collects one role's keys only.  The
aligned line probe starts the even window of a pair on line 2k and the odd one
on line 2k + 1.  Like twins, pairs change where a chain starts, never what it
finds: every path that reads the index returns the oracle's hits and calls over
the reference table bit for bit, at either parity of a window.

The `World` is that of test_gpu_line_twins.py (crowded 7-mers, both parities of
every batch).  The small indexes hold keys that all begin with one 7-mer: on 7
lines that 7-mer and all its keys' last seven residues are chosen in the last
block, so lines 4 to 6 fill, the homeless last line holds records and chains
wrap through it to line 0.  On 3 lines (3 keys at the twins' load cut) nothing
can overflow; there the homeless line stays empty and every chain ends on its
block.  Unset, pairs are on only past KGX_LINE_PAIRS_MIN_LINES lines: the last
test builds 70,000 keys at load 1 for that."""
import numpy as np
import pytest

from helpers import ALPHA, DesignedImage, encode, pack, random_protein
from test_gpu_line_marks import PRM
from test_gpu_line_twins import CUT, World, two_home_keys
from test_gpu_parity import assert_same
from test_gpu_probe_defer import _compare, _contexts, _set
from test_line_home_native import CORE, mix32

pytestmark = pytest.mark.gpu

LOADS = (1, 36, CUT)
MIN_LINES = 1 << 22  # KGX_LINE_PAIRS_MIN_LINES (include/kgx.h)


def block_of(m, n_lines):
    """the block of 7-mer m: today's 35-bit value modulo the n_lines >> 1 blocks"""
    return (mix32(m ^ 0x85EBCA6B) << 3 | (mix32(m) & 7)) % (n_lines >> 1)


def pair_homes(key, n_lines):
    """a key's two homes: its first seven residues' in role 1, its last seven's in role 0"""
    return 2 * block_of(key // 20, n_lines) + 1, 2 * block_of(key % CORE, n_lines)


@pytest.fixture(scope="module")
def world(oracle_lib):
    return World(oracle_lib)


def _index(monkeypatch, img, keys, load, pairs="1", twins="1", marks="1", mode="1"):
    """the index rebuilt under the four variables (read at each call; None:
    unset), and its statistics against the rule"""
    for name, v in (("KGX_LINE_PAIRS", pairs), ("KGX_LINE_TWINS", twins), ("KGX_LINE_MARKS", marks),
                    ("KGX_LINE_HOME", mode)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    img.set_line_index(load)
    n_lines = img.line_count
    assert n_lines > 0 and n_lines % 2 == 1 and img.line_home == int(mode or 1)
    st = img.line_stats()
    assert st["stored"] == len(keys) and st["reserved"] == 0
    twins_on = twins != "0" and marks != "0" and mode != "0" and load <= CUT
    on = twins_on and n_lines >= 3 and (pairs == "1" or (pairs is None and n_lines > MIN_LINES))
    assert img.line_pairs == int(on)
    if on:
        assert img.line_twins == len(keys)  # every key has two records
        assert all(a != b and max(a, b) < n_lines - 1 for a, b in (pair_homes(k, n_lines) for k in keys[:2000]))
    elif twins_on:
        assert img.line_twins == two_home_keys(keys, n_lines)
    else:
        assert img.line_twins == 0
    if marks != "0":
        assert st["missing"] == 0 and st["unjustified"] == 0, st
    return st


def _world_batches(gpu, ctxs, w, tag):
    for r, res, off, want in w.batches:
        _compare(gpu, ctxs, res, off, want, (tag, len(r)))


@pytest.mark.parametrize("load", LOADS)
def test_batches_every_variant_tile_and_form_at_both_parities(gpu, world, monkeypatch, load):
    w = world
    with gpu.Image.from_table(w.table) as img:
        ctxs = _contexts(gpu, monkeypatch, img)  # KGX_PROBE_DEFER 1 and 0
        try:
            st = _index(monkeypatch, img, w.keys, load)
            if load == 36:
                assert st["past_home"] >= 16 + 16  # the crowded homes: 20 records of a role on 4-record lines
            for variant in (-1, 0, 2, 3):
                for probe_j in (1, 2, 3, 4):
                    _set(ctxs, "probe_variant", variant)
                    _set(ctxs, "probe_j", probe_j)
                    _world_batches(gpu, ctxs, w, (variant, probe_j))
            _set(ctxs, "probe_variant", 2)  # a capped grid: waves stride over the tiles
            _set(ctxs, "probe_j", 2)
            _set(ctxs, "probe_persist", 1)
            _world_batches(gpu, ctxs, w, "persist")
            _set(ctxs, "probe_persist", 0)
            _set(ctxs, "probe_variant", -1)
            _set(ctxs, "line_index", 0)  # the reference slots while the image keeps its index
            _world_batches(gpu, ctxs, w, "slots")
            _set(ctxs, "line_index", 1)
            img.set_filter(16)  # with a filter the probes go to the per-bucket kernel over the index
            for variant, probe_j in ((-1, 2), (0, 1), (2, 3), (3, 4)):
                _set(ctxs, "probe_variant", variant)
                _set(ctxs, "probe_j", probe_j)
                _world_batches(gpu, ctxs, w, ("filter", variant, probe_j))
        finally:
            for ctx in ctxs:
                ctx.close()


def _svc_equal(img, seq, want, i, prm, tag):
    """one call of the call service against sequence i of the oracle's batch"""
    hits, calls = img.svc_call(seq.encode(), prm)
    lo, hi = int(want.hit_offsets[i]), int(want.hit_offsets[i + 1])
    for f in ("which_kmer", "pos", "function_index", "otu_index", "avg_from_end"):
        assert np.array_equal(hits[f], want.hits[f][lo:hi]), (tag, f)
    assert np.array_equal(hits["function_wt"].view(np.uint32), want.hits["function_wt"][lo:hi].view(np.uint32)), tag
    lo, hi = int(want.call_offsets[i]), int(want.call_offsets[i + 1])
    for f in ("start", "end", "count", "function_index"):
        assert np.array_equal(calls[f], want.calls[f][lo:hi]), (tag, f)
    assert np.array_equal(calls["weighted_hits"].view(np.uint32),
                          want.calls["weighted_hits"][lo:hi].view(np.uint32)), tag


class Small:
    """n keys that begin with one 7-mer S, for an index of `n_lines` lines at
    the twins' load cut.  On 7 lines S and the seven 7-mers S[1:] + r all lie
    in the last block: line 4 takes 7 records and line 5 another 7, 14 records
    that fill lines 4, 5, 6 and wrap to line 0."""

    def __init__(self, oracle_lib, n_lines):
        rng = np.random.default_rng(n_lines)
        n = {3: 3, 7: 7, 1: 1}[n_lines]
        last = (n_lines >> 1) - 1
        while True:
            s = int(rng.integers(0, CORE))
            ends = [int(r) for r in rng.permutation(20)[:n]]
            keys = [s * 20 + r for r in ends]
            if n_lines == 1 or all(block_of(k // 20, n_lines) == last and block_of(k % CORE, n_lines) == last
                                   for k in keys):
                break
        self.n_lines, self.keys = n_lines, keys
        s7 = "".join(ALPHA[s // 20 ** (6 - i) % 20] for i in range(7))
        d = DesignedImage()
        for i, r in enumerate(ends):
            d.add(s7 + ALPHA[r], 1 + i % 5, oI=i % 3, avg=i, wt=0.5 + i / 4)
        assert [encode(s7 + ALPHA[r]) for r in ends] == keys and d.order == keys
        self.table = d.table()
        recs = [s7 + a + "A" for a in ALPHA]  # all 20 keys S + a, stored or absent, one window each
        recs += [a + s7 + b + "A" for a, b in zip(ALPHA, ALPHA[5:] + ALPHA[:5])]  # behind another window
        recs.append("".join(s7 + a for a in ALPHA) + "A")
        recs += [random_protein(rng, int(rng.integers(8, 150))) for _ in range(10)]
        recs += ["", s7 + "X", "L" * 30]
        self.recs = [(f"s{i}", r) for i, r in enumerate(recs)]
        self.batches = []
        for r in (self.recs, [("one", "ACDEFGHIK")] + self.recs):  # either parity
            res, off = pack(r)
            want = oracle_lib.process_batch(self.table, res, off, params=PRM)
            assert set(int(k) for k in want.hits["which_kmer"]) == set(keys)
            self.batches.append((r, res, off, want))


@pytest.mark.parametrize("n_lines", (3, 7, 1))
def test_small_indexes_and_the_homeless_last_line(gpu, oracle_lib, monkeypatch, n_lines):
    w = Small(oracle_lib, n_lines)
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img:
        ctxs = _contexts(gpu, monkeypatch, img)
        try:
            st = _index(monkeypatch, img, w.keys, CUT)
            assert img.line_count == n_lines and img.line_pairs == int(n_lines >= 3)
            if n_lines == 7:
                # lines 4, 5 and 6 full and two records on line 0: the chains wrap through the
                # homeless line.  Three keys lie past line 4; of the seven homed on line 5 it
                # holds at most four (either copy counts) and at least two, as the build's races fell
                assert st["full_lines"] == 3 and 3 + 3 <= st["past_home"] <= 3 + 5, st
            if n_lines == 3:
                assert st["full_lines"] == 0 and st["past_home"] == 0
            for probe_j in (1, 2, 3, 4):
                _set(ctxs, "probe_j", probe_j)
                _world_batches(gpu, ctxs, w, probe_j)
            _set(ctxs, "probe_variant", 0)  # the per-bucket kernel from the minimizer home
            _world_batches(gpu, ctxs, w, "bucket")
            _set(ctxs, "probe_variant", -1)
            recs, _, _, want = w.batches[0]
            for i in list(range(0, 41, 3)) + [40]:  # the call service over the same index
                _svc_equal(img, recs[i][1], want, i, prm, (n_lines, i))
        finally:
            for ctx in ctxs:
                ctx.close()


@pytest.mark.parametrize("probe", ["thread", "quad"])
def test_call_service_and_small_fused_batch(gpu, world, oracle_lib, monkeypatch, probe):
    """These start at the minimizer home, under pairs the home of the
    lower-hashing 7-mer in its role."""
    w = world
    monkeypatch.setenv("KGX_SVC_PROBE", probe)
    prm = gpu.Params(*PRM)
    recs, _, _, want = w.batches[0]
    pick = list(range(0, 84, 5)) + [20, 41, 62, 83, 84, 85, 100, 101, 140, 141, 144, 149, 150, 152, 160]
    pick += list(range(len(recs) - 5, len(recs)))
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        for load in (36, CUT):
            _index(monkeypatch, img, w.keys, load)
            for i in pick:
                _svc_equal(img, recs[i][1], want, i, prm, (load, recs[i][0]))
            if probe == "thread":
                ctx.set_option("small_fused", 1)
                for sel in (pick[:9], pick[9:22], pick[22:]):
                    r, o = pack([recs[i] for i in sel])
                    assert_same(ctx.process_batch(r, o, prm),
                                oracle_lib.process_batch(w.table, r, o, params=PRM), len(sel))
                ctx.set_option("small_fused", 0)


def test_fq_dna_probe_forward_and_reverse(gpu, world, oracle_lib, monkeypatch):
    from tests_golden_codons import back_translate, revcomp
    w = world
    rng = np.random.default_rng(29)
    reads = []
    for i in range(80):
        src = w.src[i % 28]
        at = int(rng.integers(0, len(src) - 60))
        dna = back_translate(src[at:at + int(rng.integers(12, 60))], rng)
        reads.append((dna if i % 2 else revcomp(dna)).encode())
    for j, x in enumerate(w.cores):  # the crowded chains from DNA, both strands
        dna = back_translate("".join(a + x for a in ALPHA[:8]) + w.src[j][:12], rng)
        reads += [dna.encode(), revcomp(dna).encode()]
    res, off = pack([("r", x) for x in reads])
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        h = ctx.fragments_to_host(ctx.fq_fragments(res, off))
        want = oracle_lib.process_batch(w.table, h["residues"], h["offsets"], params=PRM, want=3)
        assert len(want.calls) > 20
        ctx.set_option("fq_residues", 0)  # fragments left as DNA: the DNA line probe
        _index(monkeypatch, img, w.keys, 36)
        for fq_j in (1, 2, 3, 4):
            ctx.set_option("fq_probe_j", fq_j)
            got = ctx.run_fragments(ctx.fq_fragments(res, off), prm, want=3)
            assert np.array_equal(got.hit_offsets, want.hit_offsets)
            for f in ("which_kmer", "pos", "function_index", "otu_index"):
                assert np.array_equal(got.hits[f], want.hits[f]), (fq_j, f)
            assert np.array_equal(got.call_offsets, want.call_offsets)
            for f in ("start", "end", "count", "function_index"):
                assert np.array_equal(got.calls[f], want.calls[f]), (fq_j, f)
            assert np.array_equal(got.calls["weighted_hits"].view(np.uint32),
                                  want.calls["weighted_hits"].view(np.uint32)), fq_j


def test_switches(gpu, world, monkeypatch):
    w = world
    prm = gpu.Params(*PRM)

    def equal(ctx, tag):
        for r, res, off, want in w.batches:
            try:
                assert_same(ctx.process_batch(res, off, prm), want, len(r))
            except AssertionError as e:
                raise AssertionError(f"{tag}: {e}") from e

    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        st = _index(monkeypatch, img, w.keys, 36, pairs="1")
        lines = img.line_count
        assert img.line_pairs == 1 and img.line_twins == w.n_keys
        for bad in ("2", "yes", "01"):
            monkeypatch.setenv("KGX_LINE_PAIRS", bad)
            with pytest.raises(gpu.KgxError):
                img.set_line_index(36)
            # the old index is kept, pairs and all
            assert img.line_count == lines and img.line_pairs == 1 and img.line_stats() == st
        equal(ctx, "kept")
        # 0, and unset on an index this small: the twins on one line of before
        st0 = _index(monkeypatch, img, w.keys, 36, pairs="0")
        assert img.line_count == lines and img.line_pairs == 0
        assert img.line_twins == two_home_keys(w.keys, lines) < w.n_keys
        equal(ctx, "off")
        stu = _index(monkeypatch, img, w.keys, 36, pairs=None)
        assert img.line_pairs == 0 and img.line_twins == two_home_keys(w.keys, lines)
        assert stu["full_lines"] == st0["full_lines"]  # (which copy lies past its home varies with the build's races)
        equal(ctx, "unset")
        # no pairs without twins, without marks, or under the mod home
        _index(monkeypatch, img, w.keys, 36, pairs="1", twins="0")
        assert img.line_pairs == 0 and img.line_twins == 0
        equal(ctx, "no twins")
        _index(monkeypatch, img, w.keys, 36, pairs="1", marks="0")
        assert img.line_pairs == 0
        equal(ctx, "no marks")
        _index(monkeypatch, img, w.keys, 36, pairs="1", mode="0")
        assert img.line_pairs == 0
        equal(ctx, "mod home")
        _index(monkeypatch, img, w.keys, CUT + 1, pairs="1")  # past the twins' load cut
        assert img.line_pairs == 0
        _index(monkeypatch, img, w.keys, 36, pairs="1")
        assert img.line_pairs == 1
        equal(ctx, "on again")
        img.set_line_index(0)
        assert img.line_pairs == 0 and img.line_twins == 0


def test_unset_is_on_past_the_size_cut(gpu, oracle_lib, monkeypatch):
    """70,000 keys at load 1: about 4.5 M lines, more than KGX_LINE_PAIRS_MIN_LINES"""
    from close_kmers_amd import synth
    spec = synth.ImageSpec(70000)
    keys, fI, oI, avg, wt = spec.unique_entries()
    table = oracle_lib.build_table(spec.num_sigs, keys, fI, oI, avg, wt)
    res, off = synth.make_queries(spec, 300, x_permille=5)
    want = oracle_lib.process_batch(table, res, off, params=PRM)
    assert len(want.hits) > 1000
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        _index(monkeypatch, img, [int(k) for k in keys], 1, pairs=None)
        assert img.line_count > MIN_LINES and img.line_pairs == 1 and img.line_twins == len(keys)
        assert_same(ctx.process_batch(res, off, gpu.Params(*PRM)), want, 300)
        _index(monkeypatch, img, [int(k) for k in keys], 1, pairs="0")
        assert img.line_pairs == 0
        assert_same(ctx.process_batch(res, off, gpu.Params(*PRM)), want, 300)
