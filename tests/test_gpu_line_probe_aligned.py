"""The line probe's aligned slice body (probe_slice_aligned, csrc/kgx_probe.hip),
which every index with marks runs: 32-bit line numbers, the key handed to the
quad as its low word and a word that packs key bits 32-34 with the open-chain
bit and the key's mark, and the home taken from the two 7-mers the encode
holds.  Small designed images where only that code can go wrong, compared
with the oracle bit for bit, and with the same context probing the reference
slots (option line_index 0), record bytes and mask words.

Twins: keys equal in their low 32 bits and different in bits 32-34, one
stored and the other asked for, on indexes so small that they meet in one
line (on one line all of them do; on 3, 7 and 9 lines those that share their
home, and Tiny counts them).  A compare that dropped the high bits would
report the twin as a hit.

What the builder cannot make, and so is not here.  An index of 2 lines: line
counts are odd and prime to 5, so the 7 keys that ask for 2 lines get 3.  An
index with every line full and marked for an absent key, whose chain would
end only by the round bound (n_lines + 2 rounds): the load is at most 255
keys per 64 lines, so at least one bucket stays empty, and in a full table
the line that took the last key was never passed, so it carries no mark.  On
every index the builder makes, a chain ends by a match, an empty bucket or a
clear mark; the bound is a guard.  The fullest indexes there are, one empty
bucket in the whole table, are here: absent keys walk them through the wrap
from the last line to line 0 until they meet that bucket or a clear mark."""
import ctypes

import numpy as np
import pytest

from helpers import ALPHA, DesignedImage, pack, random_protein
from test_gpu_line_marks import PRM, World, _index, _mutate, _raw_hits
from test_gpu_parity import _dev_alloc, assert_same
from test_line_home_native import line_home

pytestmark = pytest.mark.gpu

MODES = (0, 1)
MARKS = (1, 0)
EDGES = (63, 64, 65, 127, 128, 129)
# keys stored, lines the builder gives them at load 255 (one bucket of the table left empty)
TINY = [(3, 1), (7, 3), (11, 3), (27, 7), (35, 9)]


def _decode8(k):
    s = ""
    for _ in range(8):
        s = ALPHA[k % 20] + s
        k //= 20
    return s


class Tiny:
    """n_keys windows of one protein stored; asked for: the protein, every
    twin of a stored key alone and in one sequence, mutants, random
    sequences, sequences of 0 and 1 window, windows killed by X"""

    def __init__(self, oracle_lib, n_keys, n_lines):
        rng = np.random.default_rng(100 + n_keys)
        d = DesignedImage()
        self.s = random_protein(rng, n_keys + 7)
        d.add_windows(self.s, range(n_keys), fI=2, oI=1, rng=rng)
        assert len(d.order) == n_keys
        self.n_keys, self.n_lines = n_keys, n_lines
        self.table = d.table()
        stored = set(d.order)
        self.twins = []  # (stored key, its twin)
        for k in d.order:
            for m in range(-5, 6):
                t = k + m * 2 ** 32
                if m and 0 <= t < 20 ** 8 and t not in stored:
                    self.twins.append((k, t))
        assert len(self.twins) >= 3 * n_keys
        # twins that start their chain in the stored key's home line
        self.meet = {mode: sum(line_home(k, n_lines, mode) == line_home(t, n_lines, mode) for k, t in self.twins)
                     for mode in MODES}
        # (2^32 mod 7 = 2^32 mod 9 = 4: under the mod home on 7 or 9 lines a twin never starts
        # in its partner's line, and reaches it only by walking the full lines between)
        assert self.meet[1] >= 3 and (self.meet[0] >= 3 or n_lines > 3), self.meet
        t8 = [_decode8(t) for _, t in self.twins]
        recs = [self.s + "A", self.s[3:], _mutate(rng, self.s, 5) + "C"]
        recs += [t + "A" for t in t8]
        recs.append("".join(t8) + "A")
        recs += ["", self.s[:8], self.s[:9], "X" * 8, "X" * 9, "X" * 80]
        recs += [random_protein(rng, int(rng.integers(9, 160))) for _ in range(12)]
        for p0 in (0, 4, 7):  # an X every 11 residues: three windows in eleven live
            b = list(self.s + "".join(t8[:6]) + "A")
            for p in range(p0, len(b), 11):
                b[p] = "X"
            recs.append("".join(b))
        self.recs = [(f"q{i}", r) for i, r in enumerate(recs)]
        self.res, self.off = pack(self.recs)
        self.want = oracle_lib.process_batch(self.table, self.res, self.off, params=PRM)
        found = set(int(k) for k in self.want.hits["which_kmer"])
        assert found == stored  # every stored key is found, and no twin


@pytest.mark.parametrize("n_keys,n_lines", TINY)
def test_twins_and_wrapping_chains_on_tiny_indexes(gpu, oracle_lib, monkeypatch, n_keys, n_lines):
    w = Tiny(oracle_lib, n_keys, n_lines)
    L = gpu.lib()
    n, n_res = len(w.recs), len(w.res)
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        d_res = _dev_alloc(gpu, max(16, n_res))
        d_off = _dev_alloc(gpu, (n + 1) * 8)
        try:
            gpu.check(L.kgx_memcpy_h2d(d_res, w.res.ctypes.data, n_res), "h2d")
            gpu.check(L.kgx_memcpy_h2d(d_off, w.off.ctypes.data, w.off.nbytes), "h2d")
            for marks in MARKS:
                for mode in MODES:
                    st = _index(monkeypatch, img, marks, mode, 255)
                    assert img.line_count == n_lines and st["stored"] == n_keys
                    if n_keys == 4 * n_lines - 1:  # one empty bucket in the table
                        assert st["full_lines"] == n_lines - 1
                    for probe_j in (1, 2, 3, 4):
                        ctx.set_option("probe_j", probe_j)
                        ctx.set_option("line_index", 1)
                        assert_same(ctx.process_batch(w.res, w.off, prm), w.want, n)
                        hot1, mask1, used1 = _raw_hits(gpu, ctx, d_res, d_off, n, n_res)
                        ctx.set_option("line_index", 0)
                        hot0, mask0, used0 = _raw_hits(gpu, ctx, d_res, d_off, n, n_res)
                        assert mask1.tobytes() == mask0.tobytes(), (marks, mode, probe_j)
                        assert np.array_equal(used1, used0)
                        assert hot1[used1].tobytes() == hot0[used0].tobytes(), (marks, mode, probe_j)
                        assert used1.sum() == int(w.want.hit_offsets[-1])
                    ctx.set_option("line_index", 1)
        finally:
            L.kgx_device_free(d_res)
            L.kgx_device_free(d_off)


@pytest.fixture(scope="module")
def world(oracle_lib):
    return World(oracle_lib)


@pytest.fixture(scope="module")
def edge_batches(world, oracle_lib):
    """batches whose first sequence has exactly 63 .. 129 windows, so that the
    second one's windows begin at that lane of a slice or tile; then a
    sequence of one window, one of none, one killed by X, and stored keys"""
    out = []
    for n in EDGES:
        first = (world.src[n % 28] + world.src[(n + 5) % 28])[:n + 8]
        assert len(first) == n + 8
        recs = [first, world.src[1][:9], world.src[2][:8], "", "X" * 30, world.src[(n + 2) % 28],
                world.cores[0] + "AC", world.src[3][:40] + "X" + world.src[3][41:]]
        res, off = pack([(f"e{i}", r) for i, r in enumerate(recs)])
        out.append((n, res, off, len(recs), oracle_lib.process_batch(world.table, res, off, params=PRM)))
    return out


@pytest.mark.parametrize("load", (36, 255))
@pytest.mark.parametrize("mode", MODES)
def test_slice_and_tile_edges_every_tile_size(gpu, world, edge_batches, monkeypatch, mode, load):
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(world.table) as img, gpu.Context(img) as ctx:
        _index(monkeypatch, img, 1, mode, load)
        for probe_j in (1, 2, 3, 4):
            ctx.set_option("probe_j", probe_j)
            for n, res, off, n_seq, want in edge_batches:
                ctx.set_option("line_index", 1)
                got = ctx.process_batch(res, off, prm)
                assert_same(got, want, n_seq)
                ctx.set_option("line_index", 0)
                assert_same(ctx.process_batch(res, off, prm), want, n_seq)
            ctx.set_option("line_index", 1)
            assert_same(ctx.process_batch(world.res, world.off, prm), world.want, len(world.recs))


@pytest.mark.parametrize("n_keys,n_lines", [(11, 3), (27, 7)])
def test_dna_probe_twins_both_strands(gpu, oracle_lib, monkeypatch, n_keys, n_lines):
    from tests_golden_codons import back_translate, revcomp
    w = Tiny(oracle_lib, n_keys, n_lines)
    rng = np.random.default_rng(n_keys)
    prots = [w.s, w.s[2:], _mutate(rng, w.s, 7)]
    t8 = [_decode8(t) for _, t in w.twins]
    prots += [t + w.s[:5] for t in t8[:40]] + ["".join(t8[i:i + 4]) for i in range(0, 40, 4)]
    reads = []
    for i, p in enumerate(prots):
        dna = back_translate(p, rng)
        reads += [dna.encode(), revcomp(dna).encode()]
    res, off = pack([("r", x) for x in reads])
    prm = gpu.Params(*PRM)
    with gpu.Image.from_table(w.table) as img, gpu.Context(img) as ctx:
        h = ctx.fragments_to_host(ctx.fq_fragments(res, off))
        want = oracle_lib.process_batch(w.table, h["residues"], h["offsets"], params=PRM, want=3)
        # the protein on both strands: all its windows but the last, which no residue follows
        assert len(want.hits) >= 2 * (n_keys - 1)
        ctx.set_option("fq_residues", 0)  # fragments left as DNA: the DNA line probe
        for marks in MARKS:
            for mode in MODES:
                _index(monkeypatch, img, marks, mode, 255)
                assert img.line_count == n_lines
                for fq_j in (1, 2):
                    ctx.set_option("fq_probe_j", fq_j)
                    for line_index in (1, 0):
                        ctx.set_option("line_index", line_index)
                        got = ctx.run_fragments(ctx.fq_fragments(res, off), prm, want=3)
                        assert np.array_equal(got.hit_offsets, want.hit_offsets)
                        for f in ("which_kmer", "pos", "function_index", "otu_index"):
                            assert np.array_equal(got.hits[f], want.hits[f]), (marks, mode, fq_j, line_index, f)
                        assert np.array_equal(got.call_offsets, want.call_offsets)
                        for f in ("start", "end", "count", "function_index"):
                            assert np.array_equal(got.calls[f], want.calls[f]), (marks, mode, fq_j, f)
                        assert np.array_equal(got.calls["weighted_hits"].view(np.uint32),
                                              want.calls["weighted_hits"].view(np.uint32))
                ctx.set_option("line_index", 1)
