"""The lean lane scorer (option score_lean, csrc/kgx_score.hip): calls without
OTU output under order_constraint 0 run score_lean_kernel, which reads two
dwords of each hit record and, at score_lean 2, first packs the lanes whose
sequences pass the min_hits early-out into whole waves of their workgroup.
Neither may change a result: at score_lean 0, 1 and 2 and want 3 and 11 every
sequence's hit count, call count, calls, best call and hits are the oracle's
bit for bit, and on the device score_lean 2 leaves what score_lean 0 leaves.

What can go wrong only here: a packed lane that scores another lane's
sequence (wave and workgroup edges, every pattern of staying lanes), a
workgroup in which nobody or everybody stays, 32-bit slot arithmetic, the
8-byte record read at a 4-byte boundary, and the batch remainders of the
double-buffered record loads.

A sequence of n residues has n - 8 windows (none below 9), so the batches hold
9-residue sequences for one window and 72-residue ones for exactly one mask
word.  The image holds about 1e5 keys: a synthetic table plus source proteins
whose every 8-mer is stored, functions laid out in blocks, alternations and
pairs so that pair switches and carried pairs occur.  Host batches take the
small path; small_wave 0 sends it to the hybrid scorer, whose lane kernel is
the one under test (kgx_run_device and bench.py reach it the same way)."""
import ctypes

import numpy as np
import pytest

from close_kmers_amd import synth
from helpers import ALPHA, encode, pack, random_protein

LEANS = (0, 1, 2)
WANTS = (3, 11)
STAY_LENGTHS = (15, 71, 72, 73, 135, 300, 700)
ALL_LENGTHS = (8, 9) + STAY_LENGTHS
RUN_HITS = (1, 3, 4, 5, 7, 8, 9, 15, 16, 17)  # 3, 4, 5: the edges of the lean form's 4-record batches
PATTERNS = ("all", "none", "alternating", "last", "wave2", "all")
SIZES = (1, 63, 64, 65, 255, 256, 257, 513)


def _stays(pattern, lane):
    return {"all": True, "none": False, "alternating": lane % 2 == 0, "last": lane == 255,
            "wave2": 128 <= lane < 192}[pattern]


class World:
    """the table, the source proteins and the batches, with the oracle's results"""

    def __init__(self, oracle):
        self.oracle = oracle
        rng = np.random.default_rng(1717)
        spec = synth.ImageSpec(100000)
        keys, fI, oI, avg, wt = spec.unique_entries()
        have = set(keys.tolist())
        self.sources = [random_protein(rng, 800) for _ in range(8)]
        dk, df, do, da, dw = [], [], [], [], []
        for src in self.sources:
            p = 0
            while p + 8 <= len(src):
                blk = int(rng.integers(2, 40))
                style = int(rng.integers(0, 3))  # one function, alternating, pairs
                base = int(rng.integers(0, 6))
                for q in range(p, min(p + blk, len(src) - 7)):
                    f = base + (0 if style == 0 else (q - p) & 1 if style == 1 else (q - p) // 2 & 1)
                    k = encode(src[q:q + 8])
                    if k in have:
                        continue
                    have.add(k)
                    dk.append(k)
                    df.append(f)
                    do.append(int(rng.integers(-1, 9)))
                    da.append(int(rng.integers(0, 400)))
                    dw.append([0.0, 1.0, float(np.float32(rng.random() * 3))][int(rng.integers(0, 3))])
                p += blk
        keys = np.concatenate([keys, np.array(dk, np.uint64)])
        self.n_keys = len(keys)
        self.table = oracle.build_table(synth.builder_num_sigs(self.n_keys), keys,
                                        np.concatenate([fI, np.array(df, np.int32)]),
                                        np.concatenate([oI, np.array(do, np.int32)]),
                                        np.concatenate([avg, np.array(da, np.uint16)]),
                                        np.concatenate([wt, np.array(dw, np.float32)]))
        self.rng = rng
        self._refs = {}
        self.batches = {"patterns": self._patterns(), "lengths": self._lengths(), "runs": self._runs(),
                        "gaps": self._gaps(), "short": self._short()}
        base = self._sizes_base()
        for n in SIZES:
            self.batches[f"size{n}"] = pack(base[:n])

    # ---- sequences ----
    def planted(self, length):
        src = self.sources[int(self.rng.integers(0, len(self.sources)))]
        a = int(self.rng.integers(0, len(src) - length + 1))
        return src[a:a + length]

    def substituted(self, seq, positions):
        """seq with the residues at `positions` changed: each kills the (up to) 8 windows over it"""
        s = list(seq)
        for p in positions:
            s[p] = ALPHA[(ALPHA.index(s[p]) + 7) % 20]
        return "".join(s)

    def leaver(self, i):
        """below min_hits 5: no windows, no hits, or 1..4 hits"""
        kind = i % 6
        if kind == 0:
            return random_protein(self.rng, int(self.rng.integers(9, 60)))
        if kind == 1:
            return self.planted(8 + 1 + i % 4)
        if kind == 2:
            return random_protein(self.rng, i % 8)  # shorter than 8 residues, the empty one included
        if kind == 3:
            return random_protein(self.rng, 300)
        if kind == 4:
            return self.planted(8)  # 8 residues: a stored 8-mer, but no window
        return ""

    def hitless(self, i):
        return random_protein(self.rng, (0, 5, 9, 40, 73, 300)[i % 6])

    # ---- batches ----
    def _patterns(self):
        recs = []
        for pattern in PATTERNS:
            for lane in range(256):
                if _stays(pattern, lane):
                    s = self.planted(STAY_LENGTHS[(lane + len(recs)) % len(STAY_LENGTHS)])
                else:
                    s = self.hitless(lane) if pattern == "none" else self.leaver(lane)
                recs.append(("", s))
        recs.append(("", self.planted(300)))  # a last workgroup of one lane
        return pack(recs)

    def _lengths(self):
        recs = []
        for order in ((72, 73, 71, 700, 9, 8, 135, 15, 300), ALL_LENGTHS, ALL_LENGTHS[::-1]):
            for k, length in enumerate(order):
                recs.append(("", self.planted(length)))
                recs.append(("", random_protein(self.rng, (k * 3) % 8)))  # no windows
        return pack(recs)

    def _runs(self):
        """72-residue sequences (64 windows: with only such sequences before it,
        each is exactly one mask word) whose hits are one run of c windows, at
        the word's start, inside it and at its end: planted copies with every
        residue outside the run's own changed"""
        recs = []
        for c in RUN_HITS:
            for a in (0, 11, 64 - c):
                keep = range(a, a + c + 7)
                recs.append(("", self.substituted(self.planted(72), [p for p in range(72) if p not in keep])))
        self.run_counts = [c for c in RUN_HITS for _ in range(3)]
        return pack(recs)

    def _gaps(self):
        """planted sequences cut by substitutions (8 windows lost at each: a gap
        flush at max_gap 3), and whole sources: blocks of one function next to
        another (the pair switch with its carried pair), alternations and pairs"""
        recs = []
        for i in range(40):
            s = self.planted(300)
            pos = sorted(set(int(x) for x in self.rng.integers(0, 300, int(self.rng.integers(1, 9)))))
            recs.append(("", self.substituted(s, pos)))
        for src in self.sources:
            recs.append(("", src))
            recs.append(("", src[100:400]))
        return pack(recs)

    def _short(self):
        """fq-like fragments, under 64 residues a sequence on average: launch_score
        then takes the 2-record batches (score_lean_kernel<*, 2, *>).  Planted
        fragments of 1 to 40 windows, so that runs of 1..5 hits and of many
        2-record batches occur, beside hitless and windowless ones; three
        workgroups, the middle one with every other lane staying at min_hits 5"""
        recs = []
        for i in range(700):
            k = i % 8
            if 256 <= i < 512:
                s = self.planted(8 + 5 + i % 36) if i % 2 == 0 else random_protein(self.rng, 9 + i % 20)
            elif k < 5:
                s = self.planted(8 + 1 + (i // 8 * 5 + k) % 40)
            elif k == 5:
                s = random_protein(self.rng, 9 + i % 30)
            elif k == 6:
                s = random_protein(self.rng, i % 9)
            else:
                s = self.substituted(self.planted(40), [12 + i % 10])  # two short runs around a gap
            recs.append(("", s))
        return pack(recs)

    def _sizes_base(self):
        recs = [("", self.planted(300))]
        for i in range(1, max(SIZES)):
            stay = self.rng.random() < 0.5
            recs.append(("", self.planted(STAY_LENGTHS[i % len(STAY_LENGTHS)]) if stay else self.leaver(i)))
        return recs

    def ref(self, name, params, want=11):
        key = (name, tuple(params), want)
        if key not in self._refs:
            res, off = self.batches[name]
            self._refs[key] = self.oracle.process_batch(self.table, res, off, params=params, want=want)
        return self._refs[key]


@pytest.fixture(scope="module")
def world(oracle_lib):
    return World(oracle_lib)


# ---------------------------------------------------------------------------
# the inputs are what they are meant to be (the oracle alone, no GPU)

def test_inputs_have_the_intended_shapes(world):
    w = world
    # patterns: which lanes of each workgroup reach min_hits 5, and min_hits 1 in the "none" one
    ref = w.ref("patterns", (5, 200, 0, 0))
    hits = np.diff(ref.hit_offsets.astype(np.int64))
    assert len(hits) == 256 * len(PATTERNS) + 1
    for g, pattern in enumerate(PATTERNS):
        stay = hits[256 * g:256 * (g + 1)] >= 5
        assert stay.tolist() == [_stays(pattern, lane) for lane in range(256)], pattern
        if pattern == "none":
            assert hits[256 * g:256 * (g + 1)].sum() == 0
    assert hits[-1] >= 5
    calls = np.diff(ref.call_offsets.astype(np.int64))
    assert (calls > 0).sum() > 500 and calls.max() > 1
    assert set(np.unique(ref.best["kind"])) >= {0, 1}
    # lengths: the window counts, all hit
    res, off = w.batches["lengths"]
    lens = np.diff(off.astype(np.int64))
    hits = np.diff(w.ref("lengths", (1, 200, 0, 0)).hit_offsets.astype(np.int64))
    assert (hits[0::2] == np.maximum(lens[0::2] - 8, 0)).all() and (hits[1::2] == 0).all()
    assert set(hits.tolist()) >= {0, 1, 7, 63, 64, 65, 127, 292, 692}
    assert (lens[1::2] < 8).all()
    # a 64-window sequence that starts on a mask word boundary, and one that ends on one
    wb = np.concatenate([[0], np.cumsum(np.maximum(lens - 8, 0))])
    assert any(wb[i] % 64 == 0 and wb[i + 1] - wb[i] == 64 for i in range(len(lens)))
    # runs: 64 windows each, so one mask word each, holding one run of c hits
    res, off = w.batches["runs"]
    assert (np.diff(off.astype(np.int64)) == 72).all()
    r1 = w.ref("runs", (1, 200, 0, 0))
    assert np.diff(r1.hit_offsets.astype(np.int64)).tolist() == w.run_counts
    for s, c in enumerate(w.run_counts):
        pos = r1.hits["pos"][int(r1.hit_offsets[s]):int(r1.hit_offsets[s + 1])]
        assert (np.diff(pos.astype(np.int64)) == 1).all() and len(pos) == c
    # gaps: a small max_gap cuts runs that the default keeps whole
    wide = np.diff(w.ref("gaps", (1, 200, 0, 0)).call_offsets.astype(np.int64))
    tight = np.diff(w.ref("gaps", (1, 3, 0, 0)).call_offsets.astype(np.int64))
    assert tight.sum() > wide.sum() > len(wide)
    # short: the 2-record batches' condition, and sequences on both sides of min_hits 5
    res, off = w.batches["short"]
    assert len(res) < 64 * (len(off) - 1)
    for name in ("patterns", "lengths", "runs", "gaps"):
        assert len(w.batches[name][0]) >= 64 * (len(w.batches[name][1]) - 1), name
    hits = np.diff(w.ref("short", (5, 200, 0, 0)).hit_offsets.astype(np.int64))
    assert set(hits.tolist()) >= set(range(0, 33))
    assert ((hits[256:512] >= 5) == (np.arange(256) % 2 == 0)).all()
    assert (np.diff(w.ref("short", (5, 200, 0, 0)).call_offsets.astype(np.int64)) > 0).sum() > 100
    # sizes
    for n in SIZES:
        assert len(w.batches[f"size{n}"][1]) == n + 1


# ---------------------------------------------------------------------------
# the device

@pytest.fixture(scope="module", params=[36, 0], ids=["line_index", "reference_slots"])
def device(request, gpu, world):
    img = gpu.Image.from_table(world.table)
    if request.param:
        img.set_line_index(request.param)
        assert img.line_count > 0
    ctx = gpu.Context(img)
    ctx.set_option("small_wave", 0)  # small host batches: the hybrid scorer, lanes for these lengths
    yield ctx
    ctx.close()
    img.close()


def _run(gpu, w, ctx, name, params, want, lean, expect_lean=None):
    res, off = w.batches[name]
    ctx.set_option("score_lean", lean)
    before = ctx.stat("lean_scores")
    got = ctx.process_batch(res, off, gpu.Params(*params), want=want)
    took = ctx.stat("lean_scores") - before
    assert took == (int(lean > 0) if expect_lean is None else expect_lean), (name, params, want, lean)
    ref = w.ref(name, params, want | 11 if not want & 4 else 15)
    assert np.array_equal(got.hit_offsets, ref.hit_offsets), (name, params, want, lean)
    bad = w.oracle.diff_batch(got, ref, want)
    assert bad == {k: [] for k in bad}, (name, params, want, lean, {k: v[:8] for k, v in bad.items()})
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("min_hits", [1, 5, 0])
def test_patterns_of_staying_lanes(gpu, world, device, min_hits):
    for want in WANTS:
        for lean in LEANS:
            _run(gpu, world, device, "patterns", (min_hits, 200, 0, 0), want, lean)


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES)
def test_wave_and_workgroup_edges(gpu, world, device, n):
    for want in WANTS:
        for lean in LEANS:
            _run(gpu, world, device, f"size{n}", (5, 200, 0, 0), want, lean)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["lengths", "runs", "gaps"])
def test_lengths_batch_remainders_and_gap_flushes(gpu, world, device, name):
    for params in ((1, 200, 0, 0), (5, 200, 0, 0), (0, 200, 0, 0), (1, 3, 0, 0), (5, 3, 0, 0), (2, 0, 0, 0),
                   (3, 10, 0, 2)):
        for want in WANTS:
            for lean in LEANS:
                _run(gpu, world, device, name, params, want, lean)


@pytest.mark.gpu
def test_short_sequences_take_the_two_record_batches(gpu, world, device):
    for params in ((5, 200, 0, 0), (1, 200, 0, 0), (0, 200, 0, 0), (3, 2, 0, 0)):
        for want in WANTS:
            for lean in LEANS:
                _run(gpu, world, device, "short", params, want, lean)


@pytest.mark.gpu
def test_option_values_and_error_text(gpu, device):
    """score_lean is declared after the 43 options that tests/native/options_check.cpp
    records, so its accepted values and its error text are held here"""
    set_option = gpu.lib().kgx_ctx_set_option
    for v in (0, 1, 2):
        assert set_option(device.handle, b"score_lean", v) == 0, gpu.last_error()
    for v in (-1, 3):
        assert set_option(device.handle, b"score_lean", v) == gpu.KGX_EINVAL
        assert gpu.last_error() == "score_lean must be 0, 1 or 2"
    device.set_option("score_lean", 1)


@pytest.mark.gpu
def test_order_constraint_and_otu_take_the_general_kernel(gpu, world, device):
    for lean in LEANS:
        _run(gpu, world, device, "gaps", (5, 200, 1, 0), 3, lean, expect_lean=0)
        _run(gpu, world, device, "gaps", (5, 200, 1, 0), 11, lean, expect_lean=0)
        _run(gpu, world, device, "patterns", (5, 200, 0, 0), 7, lean, expect_lean=0)
        _run(gpu, world, device, "patterns", (5, 200, 0, 0), 15, lean, expect_lean=0)


@pytest.mark.gpu
@pytest.mark.parametrize("name,params", [("patterns", (5, 200, 0, 0)), ("patterns", (0, 200, 0, 0)),
                                         ("gaps", (1, 3, 0, 0)), ("size257", (5, 200, 0, 0))])
def test_packed_lean_leaves_what_the_general_kernel_leaves_on_the_device(gpu, world, device, name, params):
    """kgx_run_device at score_lean 0 and 2: the counts, every sequence's calls
    in its own stretch of the calls array, and the best calls, read back from
    the device as the kernels left them."""
    L = gpu.lib()
    ctx = device
    res, off = world.batches[name]
    n, n_res = len(off) - 1, len(res)
    d_res, d_off = ctypes.c_void_p(), ctypes.c_void_p()
    gpu.check(L.kgx_device_alloc(0, max(16, n_res), ctypes.byref(d_res)), "alloc")
    gpu.check(L.kgx_device_alloc(0, (n + 1) * 8, ctypes.byref(d_off)), "alloc")
    try:
        gpu.check(L.kgx_memcpy_h2d(d_res, res.ctypes.data, n_res), "h2d")
        gpu.check(L.kgx_memcpy_h2d(d_off, off.ctypes.data, off.nbytes), "h2d")
        left = []
        for lean in (0, 2):
            ctx.set_option("score_lean", lean)
            out = gpu.DeviceResult()
            p = gpu.Params(*params)
            gpu.check(L.kgx_run_device(ctx.handle, ctypes.byref(p), d_res, d_off, n, n_res, 11, ctypes.byref(out)),
                      "run_device")
            ctx.synchronize()
            wb = np.empty(n + 1, np.uint64)
            hc, cc = np.empty(n, np.uint32), np.empty(n, np.uint32)
            best = np.empty(n, gpu.BEST_DTYPE)
            calls = np.empty(int(np.maximum(np.diff(off.astype(np.int64)) - 8, 0).sum()), gpu.CALL_DTYPE)
            for a, ptr in ((wb, out.window_base), (hc, out.hit_count), (cc, out.call_count), (best, out.best),
                           (calls, out.calls)):
                if a.nbytes:
                    gpu.check(L.kgx_memcpy_d2h(a.ctypes.data, ptr, a.nbytes), "d2h")
            assert int(wb[-1]) == len(calls)
            mine = np.concatenate([calls[int(wb[s]):int(wb[s]) + int(cc[s])] for s in range(n)] or [calls[:0]])
            left.append((hc, cc, mine.tobytes(), best.tobytes()))
        assert np.array_equal(left[0][0], left[1][0]) and np.array_equal(left[0][1], left[1][1])
        assert left[0][2] == left[1][2] and left[0][3] == left[1][3]
        ref = world.ref(name, params)
        assert np.array_equal(left[1][0], np.diff(ref.hit_offsets).astype(np.uint32))
        assert np.array_equal(left[1][1], np.diff(ref.call_offsets).astype(np.uint32))
    finally:
        L.kgx_device_free(d_res)
        L.kgx_device_free(d_off)
        ctx.set_option("score_lean", 1)


@pytest.mark.gpu
def test_environment_switch_sets_the_default(gpu, world, device, monkeypatch):
    img = device.image
    res, off = world.batches["size65"]
    for value, lean in (("0", 0), ("1", 1), ("2", 1), ("", 1)):
        monkeypatch.setenv("KGX_SCORE_LEAN", value)
        with gpu.Context(img) as ctx:
            ctx.set_option("small_wave", 0)
            ctx.process_batch(res, off, gpu.Params(5, 200, 0, 0), want=11)
            assert ctx.stat("lean_scores") == lean, value
    monkeypatch.setenv("KGX_SCORE_LEAN", "3")
    with pytest.raises(Exception):
        gpu.Context(img)
    assert "KGX_SCORE_LEAN" in gpu.last_error()
    monkeypatch.delenv("KGX_SCORE_LEAN")
