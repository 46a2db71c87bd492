"""Twin records of the line index (KGX_LINE_TWINS, csrc/kgx_line_home.h): under
the minimizer home with marks, at loads up to KGX_LINE_TWINS_MAX_LOAD, every
key whose two 7-mers are homed on different lines is stored under both, and
the aligned line probe starts an even window of the batch at the home of its
last seven residues and an odd one at the home of its first seven.  Twins
change which line a chain starts on, never what it finds: every path that
reads the index returns the oracle's hits and calls over the reference table
bit for bit, whichever parity a window falls on.

The image crowds 7-mers on purpose: four 7-mers X with 5, 9, 20 and all 40 of
the keys a+X and X+a stored, so with twins the home of X carries up to 40
records, stored keys deep in its chain and absent siblings that must miss.
Every batch is run twice, as it is and behind a sequence of one window, which
moves every window to the other parity."""
import numpy as np
import pytest

from helpers import ALPHA, DesignedImage, encode, pack, random_protein
from test_gpu_line_marks import N_FUNCS, PRM, STORED, _crowded_cores, _mutate, _raw_hits
from test_gpu_parity import _dev_alloc, assert_same
from test_line_home_native import CORE, mix32

pytestmark = pytest.mark.gpu

CUT = 64  # KGX_LINE_TWINS_MAX_LOAD (include/kgx.h): twins at loads up to it
LOADS = (1, 36, CUT, CUT + 1, 255)


def seven_mer_home(m, n_lines):
    return (mix32(m ^ 0x85EBCA6B) << 3 | (mix32(m) & 7)) % n_lines


def two_home_keys(keys, n_lines):
    """keys whose two 7-mers are homed on different lines: the twin records"""
    return sum(seven_mer_home(k // 20, n_lines) != seven_mer_home(k % CORE, n_lines) for k in keys)


class World:
    def __init__(self, oracle_lib):
        rng = np.random.default_rng(1212)
        d = DesignedImage()
        self.src = [random_protein(rng, int(rng.integers(90, 140))) for _ in range(28)]
        for t, s in enumerate(self.src):
            d.add_windows(s, range(len(s) - 7), fI=t % N_FUNCS, oI=t % 9, rng=rng)
        self.cores = _crowded_cores(len(STORED))
        self.crowd_stored, self.crowd_absent = [], []
        for x, n in zip(self.cores, STORED):
            around = [a + x for a in ALPHA] + [x + a for a in ALPHA]
            pick = set(int(i) for i in rng.permutation(40)[:n])
            for i, k in enumerate(around):
                if i in pick:
                    d.add(k, 1 + i % 5, oI=i % 7, avg=i, wt=0.25 + i / 8)
                    self.crowd_stored.append(k)
                else:
                    self.crowd_absent.append(k)
        d.add("L" * 8, 5, wt=2.0)  # homopolymers: one 7-mer, one home, no twin
        d.add("W" * 8, 2, wt=0.5)
        self.table = d.table()
        self.keys = [int(k) for k in d.order]
        self.n_keys = len(self.keys)
        assert 2000 < self.n_keys < 5000

        recs = []
        # every one of the 40 keys around X, stored or not, as two windows (a
        # sequence of n residues has n - 8 windows): a+X first, X+r second
        for x in self.cores:
            for i, a in enumerate(ALPHA):
                recs.append(a + x + ALPHA[(i + 3) % 20] + "A")
            recs.append("".join(a + x for a in ALPHA) + "A")  # and in one long sequence
        n_crowd = len(recs)
        for s in self.src:  # the sources whole and mutated
            recs += [s, _mutate(rng, s, 9)]
        # window counts around the instruction groups, the slices and the tiles
        for n in (8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129):
            recs.append((self.src[n % 28] + self.src[(n + 1) % 28])[:n + 8])
        # pairs split by a sequence boundary: runs of sequences with one and with three windows
        recs += [self.src[3][:9], self.src[3][1:10], self.src[3][2:13], self.src[4][:11], self.src[4][3:12]]
        recs += [self.src[5][:8], "", random_protein(rng, 8)]  # no window at all
        for i in range(16):  # uniform sequences: absent keys
            recs.append(random_protein(rng, int(rng.integers(8, 200))))
        for i in range(6):  # an X every few residues: a pair with one dead window
            b = list(self.src[i])
            for p in range(int(rng.integers(0, 9)), len(b), 11):
                b[p] = "X"
            recs.append("".join(b))
        recs += ["L" * 40, "A" * 40, "L" * 9, "W" * 137, "LLLLLLLWWWWWWWWA"]  # homopolymers, stored and not
        self.recs = [(f"q{i}", s) for i, s in enumerate(recs)]
        # the same behind one window: every window at the other parity
        self.shifted = [("one", self.src[9][:9])] + self.recs
        self.batches = []
        for r in (self.recs, self.shifted):
            res, off = pack(r)
            self.batches.append((r, res, off, oracle_lib.process_batch(self.table, res, off, params=PRM)))
        windows = [sum(max(0, len(s) - 8) for _, s in r) for r in (self.recs, self.shifted)]
        assert windows[1] == windows[0] + 1  # one of the two batches has an odd number of windows
        # stored keys deep in the chains are found, absent siblings miss, at either parity
        for r, _, _, want in self.batches:
            skip = len(r) - len(self.recs)
            lo, hi = int(want.hit_offsets[skip]), int(want.hit_offsets[skip + n_crowd])
            found = set(int(k) for k in want.hits["which_kmer"][lo:hi])
            assert all(encode(k) in found for k in self.crowd_stored)
            assert not any(encode(k) in found for k in self.crowd_absent)
        assert len(self.crowd_stored) == sum(STORED) and len(self.crowd_absent) == 160 - sum(STORED)


@pytest.fixture(scope="module")
def world(oracle_lib):
    return World(oracle_lib)


def _index(monkeypatch, img, w, load, twins="1", marks="1", mode="1"):
    """the index rebuilt under the three variables (read at each call; None:
    unset), and its statistics against the rule"""
    for name, v in (("KGX_LINE_TWINS", twins), ("KGX_LINE_MARKS", marks), ("KGX_LINE_HOME", mode)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, v)
    img.set_line_index(load)
    assert img.line_count > 0 and img.line_home == int(mode or 1)
    st = img.line_stats()
    assert st["stored"] == w.n_keys and st["reserved"] == 0
    on = twins != "0" and marks != "0" and mode != "0" and load <= CUT
    if on:
        assert img.line_twins == two_home_keys(w.keys, img.line_count) > 0
    else:
        assert img.line_twins == 0
    if marks != "0":
        assert st["missing"] == 0 and st["unjustified"] == 0, st
    return st


def _batches_equal(gpu, ctx, w, tag):
    prm = gpu.Params(*PRM)
    for r, res, off, want in w.batches:
        try:
            assert_same(ctx.process_batch(res, off, prm), want, len(r))
        except AssertionError as e:
            raise AssertionError(f"{tag}, batch of {len(r)}: {e}") from e


@pytest.mark.parametrize("load", LOADS)
def test_batches_every_variant_and_tile_at_both_parities(gpu, world, monkeypatch, load):
    w = world
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        st = _index(monkeypatch, img, w, load)
        if load == 36:
            assert st["past_home"] >= 36 + 16  # the crowded homes: 40 and 20 records on 4-record lines
        for variant in (-1, 0, 2, 3):
            for probe_j in (1, 2, 3, 4):
                ctx.set_option("probe_variant", variant)
                ctx.set_option("probe_j", probe_j)
                _batches_equal(gpu, ctx, w, (variant, probe_j))
        ctx.set_option("probe_variant", 2)  # a capped grid: waves stride over the tiles
        ctx.set_option("probe_j", 2)
        ctx.set_option("probe_persist", 1)
        _batches_equal(gpu, ctx, w, "persist")
        ctx.set_option("probe_persist", 0)
        ctx.set_option("probe_variant", -1)
        ctx.set_option("line_index", 0)  # the reference slots while the image keeps its index
        _batches_equal(gpu, ctx, w, "slots")
        ctx.set_option("line_index", 1)
        img.set_filter(16)  # with a filter the probes go to the per-bucket kernel over the index
        for variant, probe_j in ((-1, 2), (0, 1), (2, 3), (3, 4)):
            ctx.set_option("probe_variant", variant)
            ctx.set_option("probe_j", probe_j)
            _batches_equal(gpu, ctx, w, ("filter", variant, probe_j))


def test_switches(gpu, world, monkeypatch):
    w = world
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        st = _index(monkeypatch, img, w, 36, twins="1")
        lines, twins = img.line_count, img.line_twins
        for bad in ("2", "yes", "01"):
            monkeypatch.setenv("KGX_LINE_TWINS", bad)
            with pytest.raises(gpu.KgxError):
                img.set_line_index(36)
            # the old index is kept, twins and all
            assert img.line_count == lines and img.line_twins == twins and img.line_stats() == st
        _batches_equal(gpu, ctx, w, "kept")
        _index(monkeypatch, img, w, 36, twins=None)  # unset: twins
        _batches_equal(gpu, ctx, w, "unset")
        st0 = _index(monkeypatch, img, w, 36, twins="0")
        assert img.line_count == lines and st0["past_home"] < st["past_home"]
        _batches_equal(gpu, ctx, w, "off")
        _index(monkeypatch, img, w, 36, twins="1", marks="0")  # twins need marks
        _batches_equal(gpu, ctx, w, "no marks")
        _index(monkeypatch, img, w, 36, twins="1", mode="0")  # and the minimizer home
        _batches_equal(gpu, ctx, w, "mod home")
        monkeypatch.setenv("KGX_LINE_HOME", "2")  # still refused
        with pytest.raises(gpu.KgxError):
            img.set_line_index(36)
        _index(monkeypatch, img, w, 36, twins="1")
        assert img.line_home == 1 and img.line_twins == twins
        img.set_line_index(0)
        assert img.line_twins == 0


@pytest.mark.parametrize("load", (36, CUT))
def test_hit_records_leave_the_probe_without_mark_bits(gpu, world, monkeypatch, load):
    """The same context over the twin index and over the reference slots: hit
    records and mask words are byte for byte the same (the two copies of a key
    differ in their mark bits only), and bit 31 is clear."""
    w = world
    L = gpu.lib()
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        st = _index(monkeypatch, img, w, load)
        assert st["mark_bits"] > 0  # there is something to clear
        for r, res, off, want in w.batches:
            n, n_res = len(r), len(res)
            d_res = _dev_alloc(gpu, max(16, n_res))
            d_off = _dev_alloc(gpu, (n + 1) * 8)
            try:
                gpu.check(L.kgx_memcpy_h2d(d_res, res.ctypes.data, n_res), "h2d")
                gpu.check(L.kgx_memcpy_h2d(d_off, off.ctypes.data, off.nbytes), "h2d")
                for variant, probe_j in ((-1, 2), (0, 2), (3, 2), (2, 4)):
                    ctx.set_option("probe_variant", variant)
                    ctx.set_option("probe_j", probe_j)
                    ctx.set_option("line_index", 0)
                    hot0, mask0, used0 = _raw_hits(gpu, ctx, d_res, d_off, n, n_res)
                    assert used0.sum() == int(want.hit_offsets[-1])
                    ctx.set_option("line_index", 1)
                    hot1, mask1, used1 = _raw_hits(gpu, ctx, d_res, d_off, n, n_res)
                    assert mask1.tobytes() == mask0.tobytes()
                    assert np.array_equal(used1, used0)
                    assert hot1[used1].tobytes() == hot0[used0].tobytes(), (variant, probe_j)
                    assert not (hot1[used1][:, 3] >> 31).any()
            finally:
                L.kgx_device_free(d_res)
                L.kgx_device_free(d_off)


@pytest.mark.parametrize("probe", ["thread", "quad"])
def test_call_service_and_small_fused_batch(gpu, world, oracle_lib, monkeypatch, probe):
    """These start at the minimizer home: over a twin index they find the
    record that home's walk placed, or the twin before it on the chain."""
    w = world
    monkeypatch.setenv("KGX_SVC_PROBE", probe)
    prm = gpu.Params(*PRM)
    recs, _, _, want = w.batches[0]
    # the crowded keys one by one and in one sequence, sources, mutants, edges, misses, homopolymers
    pick = list(range(0, 84, 5)) + [20, 41, 62, 83, 84, 85, 100, 101, 140, 141, 144, 149, 150, 152, 160]
    pick += list(range(len(recs) - 5, len(recs)))
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        for load in (36, CUT):
            _index(monkeypatch, img, w, load)
            for i in pick:
                name, s = recs[i]
                hits, calls = img.svc_call(s.encode(), prm)
                lo, hi = int(want.hit_offsets[i]), int(want.hit_offsets[i + 1])
                for f in ("which_kmer", "pos", "function_index", "otu_index", "avg_from_end"):
                    assert np.array_equal(hits[f], want.hits[f][lo:hi]), (load, name, f)
                assert np.array_equal(hits["function_wt"].view(np.uint32),
                                      want.hits["function_wt"][lo:hi].view(np.uint32)), (load, name)
                lo, hi = int(want.call_offsets[i]), int(want.call_offsets[i + 1])
                for f in ("start", "end", "count", "function_index"):
                    assert np.array_equal(calls[f], want.calls[f][lo:hi]), (load, name, f)
                assert np.array_equal(calls["weighted_hits"].view(np.uint32),
                                      want.calls["weighted_hits"][lo:hi].view(np.uint32)), (load, name)
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
    rng = np.random.default_rng(23)
    reads = []
    for i in range(120):
        src = w.src[i % 28]
        at = int(rng.integers(0, len(src) - 60))
        p = src[at:at + int(rng.integers(12, 60))]
        if i % 5 == 0:
            p = _mutate(rng, p, 13)
        dna = back_translate(p, rng)
        reads.append((dna if i % 2 else revcomp(dna)).encode())
    for j, x in enumerate(w.cores):  # the crowded chains from DNA, both strands
        p = "".join(a + x for a in ALPHA[:8]) + w.src[j][:12]
        dna = back_translate(p, rng)
        reads += [dna.encode(), revcomp(dna).encode()]
    reads.append(back_translate("L" * 30, rng).encode())
    res, off = pack([("r", x) for x in reads])
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        h = ctx.fragments_to_host(ctx.fq_fragments(res, off))
        want = oracle_lib.process_batch(w.table, h["residues"], h["offsets"], params=PRM, want=3)
        assert len(want.calls) > 30
        ctx.set_option("fq_residues", 0)  # fragments left as DNA: the DNA line probe
        for load in (36, CUT):
            _index(monkeypatch, img, w, load)
            for fq_j in (1, 2, 3, 4):
                ctx.set_option("fq_probe_j", fq_j)
                got = ctx.run_fragments(ctx.fq_fragments(res, off), prm, want=3)
                assert np.array_equal(got.hit_offsets, want.hit_offsets)
                for f in ("which_kmer", "pos", "function_index", "otu_index"):
                    assert np.array_equal(got.hits[f], want.hits[f]), (load, fq_j, f)
                assert np.array_equal(got.call_offsets, want.call_offsets)
                for f in ("start", "end", "count", "function_index"):
                    assert np.array_equal(got.calls[f], want.calls[f]), (load, fq_j, f)
                assert np.array_equal(got.calls["weighted_hits"].view(np.uint32),
                                      want.calls["weighted_hits"].view(np.uint32)), (load, fq_j)
