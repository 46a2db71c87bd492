"""The home line of the line index (KGX_LINE_HOME, csrc/kgx_line_home.h): 0 =
key mod n_lines, 1 = the minimizer home, under which neighbouring windows of a
sequence share a line one time in three.  The home is the index's own choice:
under either, every path that probes it -- batches under every probe variant
and tile size, a capped grid, the presence filter, the small fused batch, the
call service's two probe loops, the fq DNA probe -- must return the oracle's
hits, calls and best calls over the reference table, bit for bit.

The images are built where the minimizer home differs most from the mod home:
keys that are consecutive windows of proteins (shared 7-mers are the rule),
proteins stored at every other window (present and absent keys as neighbours),
one 7-mer extended by all 20 residues on either side (40 keys, one minimizer:
a chain of ten lines from one home), a stored homopolymer (both 7-mers equal),
at the benchmark's load and at a load where every line is full."""
import numpy as np
import pytest

from helpers import ALPHA, DesignedImage, encode, pack, random_protein
from test_gpu_parity import _best_as_reference, _same_decision, assert_same
from test_line_home_native import minimizer

pytestmark = pytest.mark.gpu

LOADS = (36, 255)  # keys per 64 lines: the benchmark's, and every line full
MODES = (0, 1)
PRM = (2, 200, 0, 0)
# the 7-mer of the star keys: its hash is below that of every 7-mer beside it
# in them, so it is the minimizer of all 40 (World checks)
CORE7 = "SSCTAWA"
N_FUNCS = 6


def _mutate(rng, s, every):
    """one substitution every `every` residues"""
    b = list(s)
    for i in range(int(rng.integers(0, every)), len(b), every):
        b[i] = ALPHA[(ALPHA.index(b[i]) + 1 + int(rng.integers(0, 19))) % 20]
    return "".join(b)


class World:
    def __init__(self, oracle_lib):
        rng = np.random.default_rng(2024)
        d = DesignedImage()
        self.full = [random_protein(rng, int(rng.integers(200, 330))) for _ in range(90)]
        for t, s in enumerate(self.full):  # every window: consecutive keys
            d.add_windows(s, range(len(s) - 7), fI=t % N_FUNCS, oI=t % 11, rng=rng)
        self.alt = [random_protein(rng, 150) for _ in range(20)]
        for t, s in enumerate(self.alt):  # every other window: hits beside misses
            d.add_windows(s, range(0, len(s) - 7, 2), fI=(t + 1) % N_FUNCS, rng=rng)
        for a in ALPHA:  # the star: 40 keys over one 7-mer
            d.add(a + CORE7, 3, wt=1.25)
            d.add(CORE7 + a, 4, wt=0.75)
            assert minimizer(encode(a + CORE7)) == minimizer(encode(CORE7 + a)) == encode(CORE7)
        d.add("L" * 8, 5, wt=2.0)
        self.table = d.table()
        self.n_keys = len(d.order)

        recs = []
        # window counts around the 16-window instruction groups, the 64-window
        # slices and the 128-window tiles, first in the batch and again later
        edges = [n + 8 for n in (15, 16, 17, 63, 64, 65, 127, 128, 129)]
        for n in edges:
            recs.append(self.full[len(recs) % 90][:n])
        for n in (8, 9, 10, 11):  # one to three windows, and none
            recs += [self.full[3][5:5 + n], self.alt[2][4:4 + n], random_protein(rng, n)]
        recs += [self.full[7], "", self.full[8]]  # an empty sequence between two others
        for i in range(40):  # the sources, whole and with substitutions
            s = self.full[i]
            recs += [s, _mutate(rng, s, 9), _mutate(rng, s, 23)]
        for s in self.alt:  # present and absent keys as neighbours
            recs += [s, _mutate(rng, s, 17)]
        for i in range(30):  # uniform sequences: misses, the occasional chance hit
            recs.append(random_protein(rng, int(rng.integers(8, 300))))
        for i in range(20):  # an X every few residues: dead windows right before live ones
            b = list(self.full[40 + i])
            for p in range(int(rng.integers(0, 9)), len(b), int(rng.integers(9, 14))):
                b[p] = "X"
            recs.append("".join(b))
        recs += ["L" * 40, "A" * 40, "L" * 9, "W" * 137]  # homopolymers, stored and not
        for a in ALPHA:  # the star's chain from both sides, present and absent ends
            recs.append(a + CORE7 + ALPHA[(ALPHA.index(a) + 7) % 20] + self.full[0][:20])
        recs += [CORE7 + "AC", "Y" + CORE7[:6] + "AAA"]
        for n in edges:
            recs.append(_mutate(rng, self.full[50 + len(recs) % 40][:n], 11))
        self.recs = [(f"q{i}", s) for i, s in enumerate(recs)]
        self.res, self.off = pack(self.recs)
        self.want = oracle_lib.process_batch(self.table, self.res, self.off, params=PRM)
        assert int(self.want.hit_offsets[-1]) > 20000
        self.names = [f"function {i}" for i in range(N_FUNCS + 2)]
        self.want_best = []
        for s in range(len(self.recs)):
            c = self.want.calls[int(self.want.call_offsets[s]):int(self.want.call_offsets[s + 1])]
            self.want_best.append(oracle_lib.find_best_call(c, self.names))


@pytest.fixture(scope="module")
def world(oracle_lib):
    return World(oracle_lib)


def _index(monkeypatch, img, mode, load):
    """the index rebuilt under KGX_LINE_HOME = mode (read at each call)"""
    monkeypatch.setenv("KGX_LINE_HOME", str(mode))
    img.set_line_index(load)
    assert img.line_count > 0 and img.line_home == mode


@pytest.mark.parametrize("load", LOADS)
def test_batches_every_variant_and_tile_under_both_homes(gpu, world, monkeypatch, load):
    w = world
    n = len(w.recs)
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        for mode in MODES + (0,):  # and back: the mode belongs to the index, not the process
            _index(monkeypatch, img, mode, load)
            for variant in (-1, 0, 2, 3):
                for probe_j in (1, 2, 3, 4):
                    ctx.set_option("probe_variant", variant)
                    ctx.set_option("probe_j", probe_j)
                    assert_same(ctx.process_batch(w.res, w.off, prm), w.want, n)
            # a capped grid: the line probe's waves stride over the tiles
            ctx.set_option("probe_variant", 2)
            ctx.set_option("probe_j", 2)
            ctx.set_option("probe_persist", 1)
            assert_same(ctx.process_batch(w.res, w.off, prm), w.want, n)
            ctx.set_option("probe_persist", 0)
            ctx.set_option("probe_variant", -1)
            # best calls on the device
            got = ctx.process_batch(w.res, w.off, prm, want=gpu.WANT_CALLS | gpu.WANT_BEST)
            assert np.array_equal(got.call_offsets, w.want.call_offsets)
            for s in range(n):
                assert _same_decision(_best_as_reference(got.best[s], w.names), w.want_best[s]), (mode, s)
            # the reference slots while the image keeps its index
            ctx.set_option("line_index", 0)
            assert_same(ctx.process_batch(w.res, w.off, prm), w.want, n)
            ctx.set_option("line_index", 1)


@pytest.mark.parametrize("mode", MODES)
def test_presence_filter_on_top(gpu, world, monkeypatch, mode):
    """With a filter the probes go to the per-bucket kernel over the index."""
    w = world
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        img.set_filter(16)
        for load in LOADS:
            _index(monkeypatch, img, mode, load)
            for variant, probe_j in ((-1, 2), (0, 1), (2, 3), (3, 4)):
                ctx.set_option("probe_variant", variant)
                ctx.set_option("probe_j", probe_j)
                assert_same(ctx.process_batch(w.res, w.off, prm), w.want, len(w.recs))


@pytest.mark.parametrize("probe", ["thread", "quad"])
@pytest.mark.parametrize("mode", MODES)
def test_call_service_and_small_fused_batch(gpu, world, oracle_lib, monkeypatch, mode, probe):
    w = world
    monkeypatch.setenv("KGX_SVC_PROBE", probe)
    prm = gpu.Params(*PRM)
    # the edge lengths, a source, substitutions, alternating hits, X, homopolymers, the star
    pick = list(range(0, 21, 3)) + [21, 23, 24, 25, 26, 144, 145, 190, 214, 215, 234, 235, 236, 237, 238, 245,
                                    258, 259, 260, 265, 268]
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        for load in LOADS:
            _index(monkeypatch, img, mode, load)
            for i in pick:
                name, s = w.recs[i]
                hits, calls = img.svc_call(s.encode(), prm)
                lo, hi = int(w.want.hit_offsets[i]), int(w.want.hit_offsets[i + 1])
                for f in ("which_kmer", "pos", "function_index", "otu_index", "avg_from_end"):
                    assert np.array_equal(hits[f], w.want.hits[f][lo:hi]), (load, name, f)
                assert np.array_equal(hits["function_wt"].view(np.uint32),
                                      w.want.hits["function_wt"][lo:hi].view(np.uint32)), (load, name)
                lo, hi = int(w.want.call_offsets[i]), int(w.want.call_offsets[i + 1])
                for f in ("start", "end", "count", "function_index"):
                    assert np.array_equal(calls[f], w.want.calls[f][lo:hi]), (load, name, f)
                assert np.array_equal(calls["weighted_hits"].view(np.uint32),
                                      w.want.calls["weighted_hits"][lo:hi].view(np.uint32)), (load, name)
            if probe == "thread":
                ctx.set_option("small_fused", 1)
                for sel in (pick[:8], pick[8:20], [21, 22, 23]):  # the last: an empty sequence between two
                    r, o = pack([w.recs[i] for i in sel])
                    assert_same(ctx.process_batch(r, o, prm), oracle_lib.process_batch(w.table, r, o, params=PRM),
                                len(sel))
                ctx.set_option("small_fused", 0)


@pytest.mark.parametrize("mode", MODES)
def test_fq_dna_probe_forward_and_reverse(gpu, world, oracle_lib, monkeypatch, mode):
    from tests_golden_codons import back_translate, revcomp
    w = world
    rng = np.random.default_rng(17)
    reads = []
    for i in range(240):
        src = (w.full if i % 3 else w.alt)[i % 20]
        at = int(rng.integers(0, len(src) - 60))
        p = src[at:at + int(rng.integers(12, 60))]
        if i % 5 == 0:
            p = _mutate(rng, p, 13)
        dna = back_translate(p, rng)
        reads.append((dna if i % 2 else revcomp(dna)).encode())
    reads.append(back_translate("L" * 30, rng).encode())
    reads.append(revcomp(back_translate("S" + CORE7 + "T" + w.full[1][:12], rng)).encode())
    res, off = pack([("r", x) for x in reads])
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        h = ctx.fragments_to_host(ctx.fq_fragments(res, off))
        want = oracle_lib.process_batch(w.table, h["residues"], h["offsets"], params=PRM, want=3)
        assert len(want.calls) > 50
        ctx.set_option("fq_residues", 0)  # fragments left as DNA: the DNA line probe
        for load in LOADS:
            _index(monkeypatch, img, mode, load)
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


def test_an_unknown_home_mode_is_refused_and_the_index_kept(gpu, world, monkeypatch):
    w = world
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        _index(monkeypatch, img, 0, 36)
        lines = img.line_count
        monkeypatch.setenv("KGX_LINE_HOME", "2")
        with pytest.raises(gpu.KgxError):
            img.set_line_index(36)
        assert img.line_count == lines and img.line_home == 0
        assert_same(ctx.process_batch(w.res, w.off, gpu.Params(*PRM)), w.want, len(w.recs))
        monkeypatch.delenv("KGX_LINE_HOME")
        img.set_line_index(36)
        assert img.line_home == 1  # unset: the default home, the minimizer
