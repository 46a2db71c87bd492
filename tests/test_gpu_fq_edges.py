"""The designed fq corpus (tests/fq_restate.py; tests/test_fq_restate.py shows
what it holds and which slips it tells apart) through every kernel that
translates reads, every read compared with the oracle:

  A  fq_residues 1, fq_count 0   fq_count_kernel + fq_emit_kernel (wave per read; serial past 194 bases)
  B  fq_residues 1, fq_count 1   fq_count_lane_kernel<false> + fq_emit_kernel
  C  fq_residues 0, fq_fused 0   fq_count_lane_kernel<true> + fq_desc_lane_kernel
  D  fq_residues 0, fq_fused 1   fq_anchor_fused_kernel
  E  anchors -> lookup           encode_tile_dna (the DNA probe)

at every start alignment, across the staged / global switch of a wave's span,
and with designed fragments at both ends of the bases for the probe."""
import ctypes

import numpy as np
import pytest

import fq_restate as fr
from close_kmers_amd import abi
from helpers import DesignedImage, pack, random_protein, synthetic_table
from tests_golden_codons import back_translate, revcomp

pytestmark = pytest.mark.gpu

PATHS = {"A": (1, 0, 1), "B": (1, 1, 1), "C": (0, 1, 0), "D": (0, 1, 1)}  # fq_residues, fq_count, fq_fused
COUNT_SPAN = 12288  # kgx_fq.hip: the bytes of a wave's 64 reads that stage_span takes
CLASSES = ("lengths", "sweep140", "sweep197", "sweep262", "pairs", "every_byte", "neighbours")


class DeviceReads:
    """Reads on the device, their first base `shift` bytes past an aligned
    allocation.  The bytes before and after them are T and A, so a kernel that
    looked past a read's ends there would find stops."""

    def __init__(self, reads, shift=0):
        self.L = L = abi.lib()
        res, self.off = pack([("r", r) for r in reads])
        self.bases, self.n = res.tobytes(), len(reads)
        host = np.frombuffer(b"T" * shift + self.bases + b"A" * 64, np.uint8)
        self.d_b, self.d_o = ctypes.c_void_p(), ctypes.c_void_p()
        abi.check(L.kgx_device_alloc(0, host.nbytes, ctypes.byref(self.d_b)), "alloc")
        abi.check(L.kgx_device_alloc(0, self.off.nbytes, ctypes.byref(self.d_o)), "alloc")
        assert self.d_b.value % 16 == 0
        abi.check(L.kgx_memcpy_h2d(self.d_b, host.ctypes.data, host.nbytes), "h2d")
        abi.check(L.kgx_memcpy_h2d(self.d_o, self.off.ctypes.data, self.off.nbytes), "h2d")
        self.ptr = self.d_b.value + shift  # never below the allocation

    def tile_spans(self):
        """stage_span's measure of each tile of 64 reads (paths B, C, D): its
        bytes from the 16-aligned address at or below its first base; a tile
        is staged in LDS up to COUNT_SPAN and read from memory past it."""
        off = self.off.astype(np.int64)
        first, end = off[:-1:64], off[np.minimum(np.arange(64, self.n + 64, 64), self.n)]
        return (self.ptr + first) % 16 + end - first

    def free(self):
        self.L.kgx_device_free(self.d_b)
        self.L.kgx_device_free(self.d_o)

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.free()


def fragments_on(ctx, dev, path):
    for k, v in zip(("fq_residues", "fq_count", "fq_fused"), PATHS[path]):
        ctx.set_option(k, v)
    f = abi.Fragments()
    abi.check(dev.L.kgx_fq_fragments_device(ctx.handle, dev.ptr, dev.d_o, dev.n, ctypes.byref(f)), "fragments")
    return f, ctx.fragments_to_host(f)


def check_paths(ctx, dev, want, paths="ABCD", anchors=None):
    """Every path's fragment batch against `want` (fq_restate.expected of the
    oracle's fragments): A and B whole; C and D their offsets and counts, and
    each anchor translated to the fragment's residues.  Returns the anchors."""
    o = want["offsets"].astype(np.int64)
    text = want["residues"].tobytes().decode()
    for p in paths:
        f, h = fragments_on(ctx, dev, p)
        assert f.n_reads == dev.n and f.n_fragments == len(o) - 1 and f.n_residues == o[-1], p
        if PATHS[p][0]:
            for k in ("residues", "offsets", "read", "frame", "frame_counts"):
                assert np.array_equal(h[k], want[k]), (p, k)
            continue
        assert h["residues"] is None and h["read"] is None and f.n_bases == len(dev.bases)
        for k in ("offsets", "frame_counts"):
            assert np.array_equal(h[k], want[k]), (p, k)
        if anchors is None:
            anchors = h["anchors"]
            for i in range(len(anchors)):
                assert fr._translate_anchor(dev.bases, int(anchors[i]), int(o[i + 1] - o[i])) == text[o[i]:o[i + 1]], \
                    (p, i)
        else:  # the anchors already translated, bit for bit
            assert np.array_equal(h["anchors"], anchors), p
    return anchors


@pytest.fixture(scope="module")
def corpus():
    return fr.corpus()


@pytest.fixture(scope="module")
def want(corpus, oracle_lib):
    return {name: fr.expected(reads, oracle_lib.fq_fragments) for name, reads in corpus.items()}


@pytest.fixture(scope="module")
def ctx(gpu):
    spec, table = synthetic_table(20000)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as c:
        yield c


@pytest.fixture(scope="module")
def uploaded(gpu, corpus):
    """Each class on the device, once for the module."""
    devs = {name: DeviceReads(corpus[name]) for name in CLASSES}
    yield devs
    for d in devs.values():
        d.free()


def test_corpus_classes(corpus):
    assert set(corpus) == set(CLASSES)


@pytest.mark.parametrize("name", CLASSES)
def test_every_read_on_every_path(ctx, uploaded, want, name):
    """No sampling: the whole fragment batch of a class, on paths A to D.
    lengths: A's wave path up to 194 bases and its serial path past them, a
    frame of exactly 64 codons; the sweeps and pairs: stops8 / frame_runs /
    kept_runs with a stop's last base on every 8-base step and 64-base block
    edge and runs of 10, 11, 12 codons; every_byte: nibbles4 and base_class on
    all 256 values; neighbours: reads that spell stops only when read together."""
    check_paths(ctx, uploaded[name], want[name])
    assert len(want[name]["offsets"]) - 1 >= {"lengths": 1000, "neighbours": 300}.get(name, 3000)
    # 64 reads of 197 bases or more span more than COUNT_SPAN: on B, C and D
    # those classes run lane_read_runs_global here, and lane_read_runs_ns in
    # test_long_reads_staged; the others are staged
    spans = uploaded[name].tile_spans()
    if name in LONG_CLASSES:
        assert (spans[:-1] > COUNT_SPAN).all()
    else:
        assert (spans <= COUNT_SPAN).all()


LONG_CLASSES = ("sweep197", "sweep262", "pairs")


@pytest.mark.parametrize("name", LONG_CLASSES)
def test_long_reads_staged(ctx, corpus, oracle_lib, name):
    """The classes of 197- to 262-base reads with an empty read after every
    second read: a tile of 64 then spans at most 43 x 262 bytes and is staged,
    so stops8 and the carries of lane_read_runs_ns (px, prev) meet each
    spelling's last base on every 8-base step and every edge of blocks 0..4."""
    reads = [r for i in range(0, len(corpus[name]), 2) for r in (*corpus[name][i:i + 2], b"")]
    with DeviceReads(reads) as dev:
        assert (dev.tile_spans() <= COUNT_SPAN).all()
        check_paths(ctx, dev, fr.expected(reads, oracle_lib.fq_fragments))


@pytest.mark.parametrize("name", ["lengths", "neighbours", "sweep140", "sweep197"])
def test_start_alignment(ctx, corpus, want, name):
    """The first read at 0..3 (mod 4) and 0, 1, 15 (mod 16): read_mis and
    load_read_dword (A), stage_span's 16-aligned start (B, C, D).  The reads
    after it take every alignment anyway; this moves all of them together.
    (sweep140 is staged, sweep197 read from memory: test_every_read_on_every_path.)"""
    anchors = None
    for shift in (0, 1, 2, 3, 15):
        with DeviceReads(corpus[name], shift) as dev:
            assert dev.ptr % 16 == shift
            anchors = check_paths(ctx, dev, want[name], anchors=anchors)


@pytest.mark.parametrize("span", [COUNT_SPAN - 1, COUNT_SPAN, COUNT_SPAN + 1])
@pytest.mark.parametrize("mis", [0, 1, 15])
def test_span_edge_between_staged_and_global(ctx, corpus, oracle_lib, mis, span):
    """Three tiles of 64 reads; the middle one's 16-aligned span is COUNT_SPAN
    - 1 or COUNT_SPAN bytes (staged in LDS) or COUNT_SPAN + 1 (read from
    memory, lane_read_runs_global), with its first base at 0, 1 or 15 (mod 16);
    the tiles around it are staged.  The reads are cut from the 197-base sweep,
    so they hold stops."""
    src = corpus["sweep197"]

    def take(i, n):
        return src[(i * 37) % len(src)][:n]
    tile0 = [take(i, 192) for i in range(63)] + [take(63, 176)]
    mid = [take(64 + i, 192) for i in range(63)] + [take(127, span - mis - 63 * 192)]
    tile2 = [take(128 + i, 150) for i in range(64)]
    reads = tile0 + mid + tile2
    with DeviceReads(reads, shift=mis) as dev:
        off = dev.off.astype(np.int64)

        assert (dev.ptr + off[64]) % 16 == mis
        assert dev.tile_spans().tolist()[1] == span and max(dev.tile_spans().tolist()[::2]) <= COUNT_SPAN
        check_paths(ctx, dev, fr.expected(reads, oracle_lib.fq_fragments))


# ---- path E: the DNA probe over designed fragments at the ends of the bases ----

N_PROTEINS, PROTEIN = 20, 40


@pytest.fixture(scope="module")
def designed(gpu, oracle_lib):
    rng = np.random.default_rng(19)
    prots = [random_protein(rng, PROTEIN) for _ in range(N_PROTEINS)]
    image = DesignedImage()
    for i, p in enumerate(prots):
        image.add_windows(p, range(PROTEIN - 7), fI=1 + i, wt=1.0)
    return prots, image.table()


def _probe_reads(rng, prots, j, first_reverse):
    """Reads back-translated from the designed proteins.  The first read's
    fragment (reverse strand if first_reverse, else forward) reaches base j of
    the bases; the last read's fragment (the other strand) ends j bases before
    their end.  Between them: fragments of exactly 11 residues, one N at each
    of the eight places of a window, lower case and u, reads without hits."""
    def dna(p):
        return back_translate(p, rng)

    def strand(d, reverse):
        return revcomp(d) if reverse else d
    gc = "GCCGGCGGCC"
    reads = [gc[:j] + strand(dna(prots[0]), first_reverse)]
    eleven = dna(prots[2][3:14]) + "TAA" + dna(prots[3][10:21]) + "TAG" + dna(prots[4][:25])
    reads += [eleven, revcomp(eleven), "", gc * 9]
    for i in range(8):  # an X codon 10 + i: at place 7 - k of window 3 + i + k
        d = list(dna(prots[5 + i]))
        d[3 * (10 + i) + i % 3] = "Nn"[i % 2]
        reads.append(strand("".join(d), i % 2 == 1))
    for i in (13, 14):
        reads.append(strand(dna(prots[i]), i % 2 == 1).lower().replace("t", "u"))
    reads += [dna(prots[15] + prots[16]), revcomp(dna(prots[17])) + dna(prots[18])]
    reads.append(strand(dna(prots[1]), not first_reverse) + gc[:j])
    return [r.encode() for r in reads]


@pytest.mark.parametrize("first_reverse", [True, False])
@pytest.mark.parametrize("j", [0, 1, 2])
def test_dna_probe_at_the_ends_of_the_bases(gpu, oracle_lib, designed, j, first_reverse):
    """encode_tile_dna takes a window's 24 bytes as two 16-byte loads, or byte
    by byte where those would leave the bases (the first 4 - alignment and the
    last ~32 bytes).  With the bases at pointer alignment 0..3, fq_probe_j 1
    and 4: hits and calls equal the oracle's over the translated fragments and
    the residue probe's, and hits exist in a fragment of each strand at the
    first and the last 32 bytes (both strands at both ends over the two
    values of first_reverse).  A fragment of n residues has n - 8 windows
    (kguts.cc:792), so its last codon is in none: the windows nearest the ends
    start at base j (forward) or j + 3 (reverse) and end j + 3 (forward) or j
    (reverse) bases before the end."""
    prots, table = designed
    reads = _probe_reads(np.random.default_rng(100 + 2 * j + first_reverse), prots, j, first_reverse)
    exp = fr.expected(reads, oracle_lib.fq_fragments)
    assert 11 in np.diff(exp["offsets"].astype(np.int64)) and b"X" in exp["residues"].tobytes()
    wanted = oracle_lib.process_batch(table, exp["residues"], exp["offsets"], want=3)
    prm = gpu.Params(5, 200, 0, 0)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as c:
        for shift in range(4):
            with DeviceReads(reads, shift) as dev:
                anchors = check_paths(c, dev, exp, paths="ACD")
                f, _ = fragments_on(c, dev, "B")
                results = [c.run_fragments(f, prm, want=3)]
                for probe_j in (1, 4):
                    c.set_option("fq_probe_j", probe_j)
                    f, _ = fragments_on(c, dev, "D")
                    assert not f.residues
                    results.append(c.run_fragments(f, prm, want=3))
                for r in results:
                    assert np.array_equal(r.hit_offsets, wanted.hit_offsets)
                    for k in ("which_kmer", "pos", "function_index", "otu_index", "avg_from_end"):
                        assert np.array_equal(r.hits[k], wanted.hits[k]), k
                    assert np.array_equal(r.call_offsets, wanted.call_offsets)
                    for k in ("start", "end", "count", "function_index"):
                        assert np.array_equal(r.calls[k], wanted.calls[k]), k
                    assert np.array_equal(r.calls["weighted_hits"].view(np.uint32),
                                          wanted.calls["weighted_hits"].view(np.uint32))
                # the first byte of every hit window, by strand
                ho = wanted.hit_offsets.astype(np.int64)
                seq = np.repeat(np.arange(len(ho) - 1), np.diff(ho))
                a, rev = (anchors[seq] >> 1).astype(np.int64), (anchors[seq] & 1).astype(bool)
                p = wanted.hits["pos"].astype(np.int64)
                lo = np.where(rev, a - 3 * p - 23, a + 3 * p)
                n = len(dev.bases)
                assert lo.min() >= 0 and (lo + 24).max() <= n
                if first_reverse:
                    assert (lo[rev] == j + 3).any() and (lo[~rev] + 24 == n - j - 3).any()
                else:
                    assert (lo[~rev] == j).any() and (lo[rev] + 24 == n - j).any()
    assert len(wanted.calls) >= 15 and len(wanted.hits) > 300
