"""The line probe's deferred form (KGX_PROBE_DEFER, csrc/kgx_probe.hip): over
an index with marks every 64-window slice runs its first round, and the
tile's chains that left their first line are listed in LDS in window order and
walked together afterwards, 16 to a load instruction.  The switch is read when
a context is created: 1 or unset the deferred form, 0 the rounds per slice.
It changes when a chain's later lines are read, never what the chain finds:
both forms return the oracle's hits and calls over the reference table, and
their hit records at the used slots and their mask words are byte for byte
the same, for tiles of 64 to 256 windows, both homes, with and without twin
records.

What can go wrong only here: more open chains in a tile than one pass of 16
or one slice of 64 holds, a list that ends exactly on a pass boundary, chains
of many rounds that wrap the table, and a wave that walks several tiles and
must start each with an empty list.

A sequence of n residues has n - 8 windows, so the one-window sequences here
are 9 residues long.  A capped grid (probe_persist 1) holds 4 tiles per
workgroup on each of the device's 256 compute units; only a batch with more
tiles than those 1,024 makes a wave walk a second tile, so the persist batches
hold 1,280 tiles of 64 windows and run at that tile size (and once at 128,
where the grid covers them)."""
import numpy as np
import pytest

from helpers import ALPHA, pack, random_protein
from test_gpu_line_marks import PRM, _raw_hits
from test_gpu_line_probe_aligned import Tiny, _decode8
from test_gpu_line_twins import World, _index
from test_gpu_parity import _dev_alloc, assert_same

pytestmark = pytest.mark.gpu

FORMS = ("1", "0")
MODES = ("0", "1")
TWINS = ("0", "1")
K_SWEEP = (0, 1) + tuple(range(10, 25)) + tuple(range(58, 73)) + (128,)


def _contexts(gpu, monkeypatch, img):
    """one context per form: the variable is read when the context is made"""
    out = []
    for form in FORMS:
        monkeypatch.setenv("KGX_PROBE_DEFER", form)
        out.append(gpu.Context(img))
    monkeypatch.delenv("KGX_PROBE_DEFER")
    return out


class _Device:
    """a batch's residues and offsets on the device"""

    def __init__(self, gpu, res, off):
        self.gpu, self.L = gpu, gpu.lib()
        self.n, self.n_res = len(off) - 1, len(res)
        self.d_res = _dev_alloc(gpu, max(16, self.n_res))
        self.d_off = _dev_alloc(gpu, (self.n + 1) * 8)
        gpu.check(self.L.kgx_memcpy_h2d(self.d_res, res.ctypes.data, self.n_res), "h2d")
        gpu.check(self.L.kgx_memcpy_h2d(self.d_off, off.ctypes.data, off.nbytes), "h2d")

    def free(self):
        self.L.kgx_device_free(self.d_res)
        self.L.kgx_device_free(self.d_off)


def _compare(gpu, ctxs, res, off, want, tag):
    """both forms against the oracle, and against each other byte for byte"""
    prm = gpu.Params(*PRM)
    n = len(off) - 1
    dev = _Device(gpu, res, off)
    try:
        raw = []
        for form, ctx in zip(FORMS, ctxs):
            try:
                assert_same(ctx.process_batch(res, off, prm), want, n)
            except AssertionError as e:
                raise AssertionError(f"{tag}, KGX_PROBE_DEFER={form}: {e}") from e
            raw.append(_raw_hits(gpu, ctx, dev.d_res, dev.d_off, n, dev.n_res))
        (hot1, mask1, used1), (hot0, mask0, used0) = raw
        assert mask1.tobytes() == mask0.tobytes(), tag
        assert np.array_equal(used1, used0), tag
        assert used1.sum() == int(want.hit_offsets[-1]), tag
        assert hot1[used1].tobytes() == hot0[used0].tobytes(), tag
    finally:
        dev.free()


def _set(ctxs, name, value):
    for ctx in ctxs:
        ctx.set_option(name, value)


# tiles that a capped grid holds at once on an MI355X: 4 per workgroup, one
# workgroup on each of its 256 compute units
PERSIST_TILES = 4 * 256


@pytest.fixture(scope="module")
def world(oracle_lib):
    return World(oracle_lib)


@pytest.mark.parametrize("n_keys,n_lines", [(27, 7), (35, 9)])
def test_tiny_full_indexes_many_stragglers_and_rounds(gpu, oracle_lib, monkeypatch, n_keys, n_lines):
    """Load 255: nearly every window leaves its first line and chains wrap the
    table; the sequence of all twins in a row puts more than 64 open chains
    into one tile.  (Twin records are built up to load 64 only: here the
    variable changes nothing, and both values must say so.)"""
    w = Tiny(oracle_lib, n_keys, n_lines)
    assert max(len(s) for _, s in w.recs) - 8 > 600  # hundreds of absent keys in a row
    with gpu.Image.from_table(w.table) as img:
        ctxs = _contexts(gpu, monkeypatch, img)
        try:
            for mode in MODES:
                for twins in TWINS:
                    st = _index(monkeypatch, img, w, 255, twins=twins, mode=mode)
                    assert img.line_count == n_lines and st["full_lines"] >= n_lines - 2
                    for probe_j in (1, 2, 3, 4):
                        _set(ctxs, "probe_j", probe_j)
                        _compare(gpu, ctxs, w.res, w.off, w.want, (mode, twins, probe_j))
        finally:
            for ctx in ctxs:
                ctx.close()


def _crowd_pool(w):
    """the 40 keys around the 7-mer that has all 40 stored (one home, ten
    lines of records under twins), then those around the other three"""
    pool = []
    for x in reversed(w.cores):
        pool += [a + x for a in ALPHA] + [x + a for a in ALPHA]
    return pool


@pytest.fixture(scope="module")
def boundary_batches(world, oracle_lib):
    """k one-window sequences of crowded keys in front of absent random ones,
    128 sequences (256 for k = 128).  The first 40 keys and the next 40 are
    the same 40 around one 7-mer, so up to k = 80 at least 9 in 10 are open
    after round 0 under the minimizer home."""
    rng = np.random.default_rng(14)
    pool = _crowd_pool(world)
    pool = pool[:40] + pool[:40] + pool[40:]
    out = []
    for k in K_SWEEP:
        n = 256 if k == 128 else 128
        recs = [key + "A" for key in pool[:k]]
        while len(recs) < n:
            recs.append(random_protein(rng, 9))
        res, off = pack([(f"b{i}", r) for i, r in enumerate(recs)])
        want = oracle_lib.process_batch(world.table, res, off, params=PRM)
        out.append((k, res, off, want, recs))
    return out


@pytest.mark.parametrize("twins", TWINS)
@pytest.mark.parametrize("mode", MODES)
def test_pass_boundaries(gpu, world, boundary_batches, monkeypatch, mode, twins):
    """The number of open chains of a tile swept across 16 / 17 and 64 / 65,
    wherever the build placed the keys."""
    w = world
    with gpu.Image.from_table(w.table) as img:
        ctxs = _contexts(gpu, monkeypatch, img)
        try:
            st = _index(monkeypatch, img, w, 36, twins=twins, mode=mode)
            if mode == "1":
                assert st["past_home"] >= 36 + 16  # 40 and 20 records on 4-record lines
            for probe_j in (1, 2, 3, 4):
                _set(ctxs, "probe_j", probe_j)
                for k, res, off, want, _ in boundary_batches:
                    _compare(gpu, ctxs, res, off, want, (mode, twins, probe_j, k))
        finally:
            for ctx in ctxs:
                ctx.close()


def _repeat_to(recs, windows):
    """recs repeated until they hold more than `windows` windows"""
    per = sum(max(0, len(s) - 8) for s in recs)
    return recs * (windows // per + 1)


def test_persist_resets_the_list_between_tiles_world(gpu, world, boundary_batches, oracle_lib, monkeypatch):
    """A capped grid and more tiles than it holds: every wave walks a second
    tile, crowded tiles and quiet ones mixed."""
    w = world
    tiles = PERSIST_TILES
    one = [s for _, s in w.recs]
    for k in (17, 65, 128):
        one += next(b[4] for b in boundary_batches if b[0] == k)
    recs = _repeat_to(one, 64 * (tiles + tiles // 4))
    res, off = pack([(f"p{i}", s) for i, s in enumerate(recs)])
    want = oracle_lib.process_batch(w.table, res, off, params=PRM)
    with gpu.Image.from_table(w.table) as img:
        ctxs = _contexts(gpu, monkeypatch, img)
        try:
            _index(monkeypatch, img, w, 36)
            _set(ctxs, "probe_persist", 1)
            for probe_j in (1, 2):
                _set(ctxs, "probe_j", probe_j)
                _compare(gpu, ctxs, res, off, want, ("persist", probe_j))
        finally:
            for ctx in ctxs:
                ctx.close()


def test_persist_resets_the_list_between_tiles_tiny(gpu, oracle_lib, monkeypatch):
    w = Tiny(oracle_lib, 27, 7)
    tiles = PERSIST_TILES
    recs = _repeat_to([s for _, s in w.recs], 64 * (tiles + tiles // 4))
    res, off = pack([(f"p{i}", s) for i, s in enumerate(recs)])
    want = oracle_lib.process_batch(w.table, res, off, params=PRM)
    with gpu.Image.from_table(w.table) as img:
        ctxs = _contexts(gpu, monkeypatch, img)
        try:
            _index(monkeypatch, img, w, 255, mode="1")
            _set(ctxs, "probe_persist", 1)
            _set(ctxs, "probe_j", 1)
            _compare(gpu, ctxs, res, off, want, "persist tiny")
        finally:
            for ctx in ctxs:
                ctx.close()


@pytest.mark.parametrize("n_keys,n_lines", [(11, 3), (27, 7)])
def test_dna_probe_both_strands_both_forms(gpu, oracle_lib, monkeypatch, n_keys, n_lines):
    from tests_golden_codons import back_translate, revcomp
    w = Tiny(oracle_lib, n_keys, n_lines)
    rng = np.random.default_rng(n_keys)
    prots = [w.s, w.s[2:]]
    t8 = [_decode8(t) for _, t in w.twins]
    prots += [t + w.s[:5] for t in t8[:40]] + ["".join(t8[i:i + 4]) for i in range(0, 40, 4)]
    prots.append("".join(t8[:30]))  # more than 64 open chains in a row
    reads = []
    for p in prots:
        dna = back_translate(p, rng)
        reads += [dna.encode(), revcomp(dna).encode()]
    res, off = pack([("r", x) for x in reads])
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img:
        ctxs = _contexts(gpu, monkeypatch, img)
        try:
            h = ctxs[0].fragments_to_host(ctxs[0].fq_fragments(res, off))
            want = oracle_lib.process_batch(w.table, h["residues"], h["offsets"], params=PRM, want=3)
            assert len(want.hits) >= 2 * (n_keys - 1)
            _set(ctxs, "fq_residues", 0)  # fragments left as DNA: the DNA line probe
            for mode in MODES:
                _index(monkeypatch, img, w, 255, mode=mode)
                assert img.line_count == n_lines
                for fq_j in (1, 2):
                    _set(ctxs, "fq_probe_j", fq_j)
                    got = [ctx.run_fragments(ctx.fq_fragments(res, off), prm, want=3) for ctx in ctxs]
                    for form, g in zip(FORMS, got):
                        tag = (mode, fq_j, form)
                        assert np.array_equal(g.hit_offsets, want.hit_offsets), tag
                        for f in ("which_kmer", "pos", "function_index", "otu_index"):
                            assert np.array_equal(g.hits[f], want.hits[f]), tag + (f,)
                        assert np.array_equal(g.call_offsets, want.call_offsets), tag
                        for f in ("start", "end", "count", "function_index"):
                            assert np.array_equal(g.calls[f], want.calls[f]), tag + (f,)
                        assert np.array_equal(g.calls["weighted_hits"].view(np.uint32),
                                              want.calls["weighted_hits"].view(np.uint32)), tag
                    assert got[0].hits.tobytes() == got[1].hits.tobytes()
                    assert got[0].calls.tobytes() == got[1].calls.tobytes()
        finally:
            for ctx in ctxs:
                ctx.close()


def test_a_bad_value_is_refused_at_context_creation(gpu, world, monkeypatch):
    w = world
    with gpu.Image.from_table(w.table) as img:
        for bad in ("2", "yes", "01", "-1"):
            monkeypatch.setenv("KGX_PROBE_DEFER", bad)
            with pytest.raises(gpu.KgxError):
                gpu.Context(img)
        for good in ("0", "1", ""):
            monkeypatch.setenv("KGX_PROBE_DEFER", good)
            with gpu.Context(img) as ctx:
                r, res, off, want = w.batches[0]
                assert_same(ctx.process_batch(res, off, gpu.Params(*PRM)), want, len(r))
        monkeypatch.delenv("KGX_PROBE_DEFER")
        with gpu.Context(img) as ctx:
            r, res, off, want = w.batches[0]
            assert_same(ctx.process_batch(res, off, gpu.Params(*PRM)), want, len(r))
