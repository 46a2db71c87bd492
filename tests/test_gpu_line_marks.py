"""Overflow marks of the line index (KGX_LINE_MARKS, csrc/kgx_line_home.h):
16 spare bits per index line say which hash classes of keys were pushed past
that full line, and the line probe ends a chain at the first full line whose
mark for its key is clear.  Marks change how far a chain walks, never what it
finds: with marks built (1) and not (0), under both homes, every path that
reads the index -- batches under every probe variant and tile size, the small
fused batch, the call service's two probe loops, the fq DNA probe -- returns
the oracle's hits and calls over the reference table bit for bit, and a hit
record leaves the probe with the mark bits cleared.

The images crowd homes on purpose: four 7-mers X whose hash is so low that X
is the minimizer of every key X.r and r.X, with 5, 9, 20 and all 40 of those
keys stored, so one home line carries a chain of up to ten lines, stored keys
deep in it and absent siblings that must miss; at the benchmark's load, at a
load where nearly every line is full and marked, and at a load where none is;
and indexes of 1, 3 and 7 lines, where chains wrap the table."""
import ctypes

import numpy as np
import pytest

from helpers import ALPHA, DesignedImage, encode, pack, random_protein
from test_gpu_parity import _dev_alloc, assert_same
from test_line_home_native import CORE, minimizer, mix32

pytestmark = pytest.mark.gpu

LOADS = (36, 255, 1)  # keys per 64 lines: the benchmark's, nearly every line full, nearly none
MODES = (0, 1)
MARKS = (1, 0)
PRM = (2, 200, 0, 0)
N_FUNCS = 6
STORED = (5, 9, 20, 40)  # of the 40 keys around each crowded 7-mer


def _decode7(x):
    s = ""
    for _ in range(7):
        s = ALPHA[x % 20] + s
        x //= 20
    return s


def _crowded_cores(n):
    """7-mers that are the minimizer of all 40 keys around them: their hash is
    below that of every 7-mer they overlap with"""
    rng = np.random.default_rng(5)
    out = []
    while len(out) < n:
        x = int(rng.integers(0, CORE))
        if mix32(x) > 2 ** 32 // 4000:
            continue
        keys = [r * CORE + x for r in range(20)] + [x * 20 + r for r in range(20)]
        if all(minimizer(k) == x for k in keys) and len(set(keys)) == 40:
            out.append(_decode7(x))
    return out


def _mutate(rng, s, every):
    b = list(s)
    for i in range(int(rng.integers(0, every)), len(b), every):
        b[i] = ALPHA[(ALPHA.index(b[i]) + 1 + int(rng.integers(0, 19))) % 20]
    return "".join(b)


class World:
    def __init__(self, oracle_lib):
        rng = np.random.default_rng(77)
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
        self.table = d.table()
        self.n_keys = len(d.order)
        assert 2000 < self.n_keys < 5000

        recs = []
        # every one of the 40 keys around X, stored or not, as two windows (a
        # sequence of n residues has n - 8 windows: one residue follows them)
        for x in self.cores:
            for i, a in enumerate(ALPHA):
                recs.append(a + x + ALPHA[(i + 3) % 20] + "A")
            recs.append("".join(a + x for a in ALPHA) + "A")  # and in one long sequence
        for i, s in enumerate(self.src):  # the sources whole, cut at slice and tile edges, and mutated
            recs += [s, _mutate(rng, s, 9)]
        for n in (15, 16, 17, 63, 64, 65, 127, 128, 129):
            recs.append((self.src[n % 28] + self.src[(n + 1) % 28])[:n + 8])
        recs += [self.src[3][:8], "", self.src[4][:9], random_protein(rng, 8)]
        for i in range(24):  # uniform sequences: absent keys
            recs.append(random_protein(rng, int(rng.integers(8, 200))))
        for i in range(6):  # an X every few residues
            b = list(self.src[i])
            for p in range(int(rng.integers(0, 9)), len(b), 11):
                b[p] = "X"
            recs.append("".join(b))
        self.recs = [(f"q{i}", s) for i, s in enumerate(recs)]
        self.res, self.off = pack(self.recs)
        self.want = oracle_lib.process_batch(self.table, self.res, self.off, params=PRM)
        # stored keys deep in the chains are found, absent siblings miss
        found = set(int(k) for k in self.want.hits["which_kmer"])
        assert all(encode(k) in found for k in self.crowd_stored)
        assert not any(encode(k) in found for k in self.crowd_absent)
        assert len(self.crowd_stored) == sum(STORED) and len(self.crowd_absent) == 160 - sum(STORED)


@pytest.fixture(scope="module")
def world(oracle_lib):
    return World(oracle_lib)


def _index(monkeypatch, img, marks, mode, load):
    """the index rebuilt under KGX_LINE_MARKS and KGX_LINE_HOME (read at each call)"""
    monkeypatch.setenv("KGX_LINE_MARKS", str(marks))
    monkeypatch.setenv("KGX_LINE_HOME", str(mode))
    img.set_line_index(load)
    assert img.line_count > 0 and img.line_home == mode
    st = img.line_stats()
    _check_stats(st, marks)
    return st


def _check_stats(st, marks):
    assert st["past_home"] <= st["stored"] and st["reserved"] == 0
    if marks:
        assert st["missing"] == 0 and st["unjustified"] == 0, st
        assert (st["marked_lines"] > 0) == (st["past_home"] > 0), st
        assert st["marked_lines"] <= st["full_lines"] and st["marked_lines"] <= st["mark_bits"], st
    else:
        assert st["mark_bits"] == 0 and st["marked_lines"] == 0 and st["unjustified"] == 0, st
        assert (st["missing"] > 0) == (st["past_home"] > 0), st


@pytest.mark.parametrize("load", LOADS)
@pytest.mark.parametrize("mode", MODES)
def test_batches_every_variant_and_tile_with_and_without_marks(gpu, world, monkeypatch, mode, load):
    w = world
    n = len(w.recs)
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        for marks in MARKS + (1,):  # and back: the marks belong to the index, not the process
            st = _index(monkeypatch, img, marks, mode, load)
            assert st["stored"] == w.n_keys
            if mode == 1 and load != 1:
                assert st["past_home"] >= 36 + 16  # the crowded homes: 40 and 20 keys on 4-record lines
            if load == 255:
                assert st["full_lines"] > 0.9 * img.line_count
                if marks:
                    assert st["marked_lines"] > 0.5 * img.line_count
            for variant in (-1, 0, 2, 3):
                for probe_j in (1, 2, 3, 4):
                    ctx.set_option("probe_variant", variant)
                    ctx.set_option("probe_j", probe_j)
                    assert_same(ctx.process_batch(w.res, w.off, prm), w.want, n)
            ctx.set_option("probe_variant", 2)  # a capped grid: waves stride over the tiles
            ctx.set_option("probe_j", 2)
            ctx.set_option("probe_persist", 1)
            assert_same(ctx.process_batch(w.res, w.off, prm), w.want, n)
            ctx.set_option("probe_persist", 0)
            ctx.set_option("probe_variant", -1)


@pytest.mark.parametrize("n_lines,n_keys", [(1, 3), (3, 11), (7, 27)])
def test_chains_that_wrap_a_tiny_index(gpu, oracle_lib, monkeypatch, n_lines, n_keys):
    """n_keys keys in 4 * n_lines buckets at load 255: at most one bucket is
    empty, so nearly every chain runs to the table's end and round again."""
    rng = np.random.default_rng(n_lines)
    d = DesignedImage()
    s = random_protein(rng, n_keys + 7)
    d.add_windows(s, range(n_keys), fI=2, oI=1, rng=rng)
    assert len(d.order) == n_keys
    table = d.table()
    recs = [("s", s + "A"), ("m", _mutate(rng, s, 5) + "C"), ("r", random_protein(rng, 150)), ("t", s[3:])]
    res, off = pack(recs)
    want = oracle_lib.process_batch(table, res, off, params=PRM)
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        for marks in MARKS:
            for mode in MODES:
                st = _index(monkeypatch, img, marks, mode, 255)
                assert img.line_count == n_lines and st["stored"] == n_keys
                assert len(want.hits) >= n_keys  # every stored key is asked for
                for variant, probe_j in ((-1, 2), (2, 1), (0, 2), (3, 1)):
                    ctx.set_option("probe_variant", variant)
                    ctx.set_option("probe_j", probe_j)
                    assert_same(ctx.process_batch(res, off, prm), want, len(recs))
                for name, q in recs:  # the call service's loop over the same index
                    hits, _ = img.svc_call(q.encode(), prm)
                    i = [r[0] for r in recs].index(name)
                    lo, hi = int(want.hit_offsets[i]), int(want.hit_offsets[i + 1])
                    assert np.array_equal(hits["which_kmer"], want.hits["which_kmer"][lo:hi]), (marks, mode, name)


def _raw_hits(gpu, ctx, d_res, d_off, n, n_res):
    """the probe's hit records and mask words as the device holds them, and
    the slots of the hot plane that hold a record"""
    L = gpu.lib()
    out = gpu.DeviceResult()
    p = gpu.Params(*PRM)
    gpu.check(L.kgx_run_device(ctx.handle, ctypes.byref(p), d_res, d_off, n, n_res, 3, ctypes.byref(out)),
              "run_device")
    ctx.synchronize()
    assert out.hit_format == gpu.HIT_PACKED16
    wb = np.empty(n + 1, np.uint64)
    gpu.check(L.kgx_memcpy_d2h(wb.ctypes.data, out.window_base, wb.nbytes), "d2h")
    W = int(wb[-1])
    hot = np.empty((W, 4), np.uint32)
    mask = np.empty((W + 63) // 64, np.uint64)
    gpu.check(L.kgx_memcpy_d2h(hot.ctypes.data, out.hits_hot, hot.nbytes), "d2h")
    gpu.check(L.kgx_memcpy_d2h(mask.ctypes.data, out.hit_mask, mask.nbytes), "d2h")
    T = out.tile_windows
    used = np.zeros(W, bool)
    pc = np.array([bin(int(x)).count("1") for x in mask])
    for t in range((W + T - 1) // T):  # a tile's hits are compacted from its first slot
        used[t * T:t * T + int(pc[t * (T // 64):(t + 1) * (T // 64)].sum())] = True
    return hot, mask, used


@pytest.mark.parametrize("load", (36, 255))
@pytest.mark.parametrize("mode", MODES)
def test_hit_records_leave_the_probe_without_mark_bits(gpu, world, monkeypatch, mode, load):
    """The same context over the index and over the reference slots: the hit
    records (with the scorer's flags in bits 28-30 of their last dword) and
    the mask words are byte for byte the same, and bit 31 is clear."""
    w = world
    L = gpu.lib()
    n, n_res = len(w.recs), len(w.res)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        d_res = _dev_alloc(gpu, max(16, n_res))
        d_off = _dev_alloc(gpu, (n + 1) * 8)
        try:
            gpu.check(L.kgx_memcpy_h2d(d_res, w.res.ctypes.data, n_res), "h2d")
            gpu.check(L.kgx_memcpy_h2d(d_off, w.off.ctypes.data, w.off.nbytes), "h2d")
            ctx.set_option("line_index", 0)
            hot0, mask0, used0 = _raw_hits(gpu, ctx, d_res, d_off, n, n_res)
            assert used0.sum() == int(w.want.hit_offsets[-1])
            for marks in MARKS:
                st = _index(monkeypatch, img, marks, mode, load)
                for variant, probe_j in ((-1, 2), (0, 2), (3, 2), (2, 4)):
                    ctx.set_option("probe_variant", variant)
                    ctx.set_option("probe_j", probe_j)
                    ctx.set_option("line_index", 0)
                    hot0, mask0, used0 = _raw_hits(gpu, ctx, d_res, d_off, n, n_res)
                    ctx.set_option("line_index", 1)
                    hot1, mask1, used1 = _raw_hits(gpu, ctx, d_res, d_off, n, n_res)
                    assert mask1.tobytes() == mask0.tobytes()
                    assert np.array_equal(used1, used0)
                    assert hot1[used1].tobytes() == hot0[used0].tobytes(), (marks, variant, probe_j)
                    assert not (hot1[used1][:, 3] >> 31).any()
                if marks and (mode == 1 or load == 255):
                    assert st["mark_bits"] > 0  # there was something to clear
        finally:
            L.kgx_device_free(d_res)
            L.kgx_device_free(d_off)


@pytest.mark.parametrize("probe", ["thread", "quad"])
@pytest.mark.parametrize("mode", MODES)
def test_call_service_and_small_fused_batch(gpu, world, oracle_lib, monkeypatch, mode, probe):
    w = world
    monkeypatch.setenv("KGX_SVC_PROBE", probe)
    prm = gpu.Params(*PRM)
    # the crowded keys one by one and in one sequence, sources, mutants, edges, misses
    pick = list(range(0, 84, 5)) + [20, 41, 62, 83, 84, 85, 100, 101, 140, 141, 144, 149, 150, 152, 160, 170, 178]
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        for marks in MARKS:
            for load in (36, 255):
                _index(monkeypatch, img, marks, mode, load)
                for i in pick:
                    name, s = w.recs[i]
                    hits, calls = img.svc_call(s.encode(), prm)
                    lo, hi = int(w.want.hit_offsets[i]), int(w.want.hit_offsets[i + 1])
                    for f in ("which_kmer", "pos", "function_index", "otu_index", "avg_from_end"):
                        assert np.array_equal(hits[f], w.want.hits[f][lo:hi]), (marks, load, name, f)
                    assert np.array_equal(hits["function_wt"].view(np.uint32),
                                          w.want.hits["function_wt"][lo:hi].view(np.uint32)), (marks, load, name)
                    lo, hi = int(w.want.call_offsets[i]), int(w.want.call_offsets[i + 1])
                    for f in ("start", "end", "count", "function_index"):
                        assert np.array_equal(calls[f], w.want.calls[f][lo:hi]), (marks, load, name, f)
                    assert np.array_equal(calls["weighted_hits"].view(np.uint32),
                                          w.want.calls["weighted_hits"][lo:hi].view(np.uint32)), (marks, load, name)
                if probe == "thread":
                    ctx.set_option("small_fused", 1)
                    for sel in (pick[:9], pick[9:22], [149, 150, 151]):  # the last: an empty sequence inside
                        r, o = pack([w.recs[i] for i in sel])
                        assert_same(ctx.process_batch(r, o, prm),
                                    oracle_lib.process_batch(w.table, r, o, params=PRM), len(sel))
                    ctx.set_option("small_fused", 0)


@pytest.mark.parametrize("mode", MODES)
def test_fq_dna_probe_forward_and_reverse(gpu, world, oracle_lib, monkeypatch, mode):
    from tests_golden_codons import back_translate, revcomp
    w = world
    rng = np.random.default_rng(19)
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
    res, off = pack([("r", x) for x in reads])
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        h = ctx.fragments_to_host(ctx.fq_fragments(res, off))
        want = oracle_lib.process_batch(w.table, h["residues"], h["offsets"], params=PRM, want=3)
        assert len(want.calls) > 30
        ctx.set_option("fq_residues", 0)  # fragments left as DNA: the DNA line probe
        for marks in MARKS:
            for load in (36, 255):
                _index(monkeypatch, img, marks, mode, load)
                for fq_j in (1, 2, 3, 4):
                    ctx.set_option("fq_probe_j", fq_j)
                    got = ctx.run_fragments(ctx.fq_fragments(res, off), prm, want=3)
                    assert np.array_equal(got.hit_offsets, want.hit_offsets)
                    for f in ("which_kmer", "pos", "function_index", "otu_index"):
                        assert np.array_equal(got.hits[f], want.hits[f]), (marks, load, fq_j, f)
                    assert np.array_equal(got.call_offsets, want.call_offsets)
                    for f in ("start", "end", "count", "function_index"):
                        assert np.array_equal(got.calls[f], want.calls[f]), (marks, load, fq_j, f)
                    assert np.array_equal(got.calls["weighted_hits"].view(np.uint32),
                                          want.calls["weighted_hits"].view(np.uint32)), (marks, load, fq_j)


@pytest.mark.parametrize("mode", MODES)
def test_stats_need_an_index_and_a_bad_marks_value_is_refused(gpu, world, monkeypatch, mode):
    w = world
    # the mod home spreads the crowded keys, so it needs the full table to push keys on
    load = 36 if mode == 1 else 255
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        with pytest.raises(gpu.KgxError):
            img.line_stats()  # no index
        st = _index(monkeypatch, img, 1, mode, load)
        assert st["marked_lines"] > 0 and st["mark_bits"] >= st["marked_lines"]
        lines = img.line_count
        for bad in ("2", "yes", "01"):
            monkeypatch.setenv("KGX_LINE_MARKS", bad)
            with pytest.raises(gpu.KgxError):
                img.set_line_index(load)
            # the old index is kept, marks and all (which bits are set depends
            # on the build's insertion order, so the same bits mean the same index)
            assert img.line_count == lines and img.line_home == mode and img.line_stats() == st
        assert_same(ctx.process_batch(w.res, w.off, gpu.Params(*PRM)), w.want, len(w.recs))
        monkeypatch.delenv("KGX_LINE_MARKS")
        img.set_line_index(load)
        _check_stats(img.line_stats(), 1)  # unset: the default, marks
        assert img.line_stats()["marked_lines"] > 0
        monkeypatch.setenv("KGX_LINE_MARKS", "0")
        img.set_line_index(load)
        _check_stats(img.line_stats(), 0)
        assert_same(ctx.process_batch(w.res, w.off, gpu.Params(*PRM)), w.want, len(w.recs))
        img.set_line_index(0)
        with pytest.raises(gpu.KgxError):
            img.line_stats()
