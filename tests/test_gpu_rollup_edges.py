"""The /lookup rollups (kgx_kmap_rollup, kgx_pool_lookup: rollup_tiles_kernel,
rollup_events_kernel, rollup_group_kernel, rollup_emit_kernel and the two
scans, csrc/kgx_tables.hip) at the boundaries of their kernels, against
LookupRequest::on_hit (lookup_request.cc:446-482).

The yardstick is rollup_yardstick.expected: the oracle's hits
(oracle.process_batch, want 1) through oracle.lookup_rollup.  Every case
compares the offsets and, for every sequence, id, hit_count, hit_total and
the bits of weighted_total, in both rollup modes.

Most tables are designed (helpers.DesignedImage): every window of a designed
sequence but its last is a k-mer of the image, so a sequence of size + 8
residues has exactly `size` hits (a sequence's last window is never looked
up), and the ids of its hits are chosen one by one.
"""
import numpy as np
import pytest

import rollup_yardstick as ys
from close_kmers_amd import synth
from helpers import ALPHA, DesignedImage, pack, random_protein, synthetic_table
from test_gpu_tables import _family_proteins

pytestmark = pytest.mark.gpu

# The kernels' constants, restated (csrc/kgx_tables.hip)
ROLL_FILL = 192             # kRollFill: ids per LDS table pass
ROLL_SLOTS = 256            # kRollH: slots of the LDS table
ROLL_HASH_MUL = 0x9E3779B1  # roll_hash: (id * mul) >> 24, the id's home slot
ROLL_CLASS_MUL = 0x85EBCA6B  # roll_class: ((id * mul) >> 13) & (P - 1)
ROLL_CLASS_SHIFT = 13
ROLL_MAX_P = 16             # kRollMaxP: the most id classes
SCAN_ONE_MAX = 8192         # kScanOneMax: values one workgroup scans; past it hipcub
ROLL_TILES = 2              # kRollTiles: tiles per wave of passes 1 and 2
NO_ID = 0xFFFFFFFF          # reserved (upload_ids)

ROLL_HASH_INV = pow(ROLL_HASH_MUL, -1, 1 << 32)
ROLL_CLASS_INV = pow(ROLL_CLASS_MUL, -1, 1 << 32)
assert ROLL_CLASS_INV == 0xA5CB9243

MODES = (False, True)  # peg (kmer_to_id_, append), family (kmer_to_family_id_, set)


def roll_hash(ids):
    return ((np.asarray(ids, np.uint64) * ROLL_HASH_MUL) & 0xFFFFFFFF) >> 24


def roll_class(ids, P):
    return (((np.asarray(ids, np.uint64) * ROLL_CLASS_MUL) & 0xFFFFFFFF) >> ROLL_CLASS_SHIFT) & (P - 1)


def ids_with_home(slot, count, start=0):
    """`count` ids whose roll_hash is `slot`"""
    x = (np.uint64(slot) << np.uint64(24)) + np.arange(start, start + count, dtype=np.uint64)
    ids = (x * ROLL_HASH_INV) & 0xFFFFFFFF
    assert (roll_hash(ids) == slot).all() and len(np.unique(ids)) == count and NO_ID not in ids
    return ids.astype(np.uint32)


def collision_ids(r0, count):
    """ids whose product with roll_class's multiplier is r0 .. r0 + count - 1
    (< 2^13): class 0 at every P, so no doubling of P separates them"""
    assert r0 >= 1 and r0 + count <= 1 << ROLL_CLASS_SHIFT
    ids = (np.arange(r0, r0 + count, dtype=np.uint64) * ROLL_CLASS_INV) & 0xFFFFFFFF
    for P in (2, 16, 1 << 18, 1 << 31):
        assert not roll_class(ids, P).any()
    return ids.astype(np.uint32)


_CODE = np.full(256, 255, np.uint8)
for _i, _ch in enumerate(ALPHA):
    _CODE[ord(_ch)] = _i


def window_keys(seq: str, n: int) -> np.ndarray:
    """the encoded 8-mers at positions 0 .. n - 1"""
    c = _CODE[np.frombuffer(seq.encode(), np.uint8)].astype(np.uint64)
    k = np.zeros(n, np.uint64)
    for j in range(8):
        k = k * np.uint64(20) + c[j:j + n]
    return k


class Designed:
    """Sequences whose looked-up windows all hit, each window a k-mer of its own."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.image = DesignedImage()
        self.keys = set()

    def all_hit(self, size):
        """(sequence of size + 8 residues, its `size` window k-mers in order)"""
        while True:
            s = random_protein(self.rng, size + 8)
            keys = window_keys(s, size + 1)  # the last window too: it must stay absent
            if len(set(keys.tolist())) == size + 1 and self.keys.isdisjoint(keys.tolist()):
                break
        self.keys.update(keys.tolist())
        self.image.add_windows(s, range(size), fI=1 + len(self.image.order) % 50, wt=1.0)
        return s, keys[:size]

    def distinct_ids(self, n, exclude=()):
        """n distinct random ids over the 32 bits, none reserved or excluded"""
        ids = np.unique(self.rng.integers(0, NO_ID, 2 * n + 16, dtype=np.uint64).astype(np.uint32))
        ids = np.setdiff1d(ids, np.asarray(exclude, np.uint32))
        assert len(ids) >= n
        return self.rng.permutation(ids)[:n]

    def table(self):
        return self.image.table()


def _expect(oracle_lib, table, res, off, kms, ids):
    """{family: (offsets, rows)} of the yardstick, and the oracle's hits per sequence"""
    r = oracle_lib.process_batch(table, res, off, want=1)
    want = {}
    for family in MODES:
        orc = ys.oracle_kmap(oracle_lib, kms, ids, family)
        want[family] = oracle_lib.lookup_rollup(orc, r.hit_offsets, r.hits["which_kmer"], family)
    return want, np.diff(r.hit_offsets.astype(np.int64))


def _rollups(gpu, ctx, res, off, kms, ids, want, wants=(0,), what=""):
    """the device's rollups of (res, off) in both modes, after a pass of each of `wants`"""
    for family in MODES:
        with gpu.Kmap(0, gpu.KMAP_SET if family else gpu.KMAP_APPEND) as dev:
            dev.add(kms, ids)
            for w in wants:
                ctx.process_batch(res, off, want=w)
                roff, rows = dev.rollup(ctx, gpu.ROLLUP_FAMILY if family else gpu.ROLLUP_PEG)
                ys.assert_rows(roff, rows, *want[family], what=(what, "family" if family else "peg", "want", w))


def _rows_per_seq(want, family=True):
    return np.diff(want[family][0].astype(np.int64))


# --- distinct-id counts ---------------------------------------------------

SIZES = (1, 63, 64, 65, 191, 192, 193, 256, 257, 384, 385, 1000)


@pytest.mark.parametrize("twice", [False, True])
def test_distinct_id_counts(gpu, oracle_lib, twice):
    """Sequences with exactly SIZES distinct ids, one id per hit (a chunk of 64
    events more or less, the table's fill more or less, two and three table
    passes, six), shuffled in one batch; with `twice`, every id is touched
    again after the last new one, so the sums continue across chunks and, in
    the class path, across passes."""
    d = Designed(101)
    sizes = [int(x) for x in d.rng.permutation(SIZES)]
    all_ids = d.distinct_ids(sum(sizes))
    seqs, kms, ids, at = [], [], [], 0
    for size in sizes:
        s, keys = d.all_hit(size)
        seqs.append(s + s if twice else s)
        kms.append(keys)
        ids.append(all_ids[at:at + size])
        at += size
    kms, ids = np.concatenate(kms), np.concatenate(ids)
    table = d.table()
    res, off = pack([(str(i), s) for i, s in enumerate(seqs)])
    want, hits = _expect(oracle_lib, table, res, off, kms, ids)
    assert hits.tolist() == [(2 if twice else 1) * s for s in sizes]
    for family in MODES:
        assert _rows_per_seq(want, family).tolist() == sizes  # the counts are what the names say
        assert (want[family][1]["hit_count"] == (2 if twice else 1)).all()
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        _rollups(gpu, ctx, res, off, kms, ids, want, what="distinct ids")


# --- the LDS table's probing ------------------------------------------------

def test_table_probing(gpu, oracle_lib):
    """192 ids whose home is slot 255 (the chain wraps to slot 0 and fills
    0..190), 193 of them (one more than a pass holds, all in one chain), and
    192 ids with every slot from 64 to 255 a home; each set once and twice."""
    d = Designed(202)
    sets = [ids_with_home(255, ROLL_FILL), ids_with_home(255, ROLL_FILL + 1, start=5000),
            np.concatenate([ids_with_home(slot, 1, start=7 * slot) for slot in range(64, ROLL_SLOTS)])]
    assert sorted(roll_hash(sets[2]).tolist()) == list(range(64, ROLL_SLOTS))
    seqs, kms, ids = [], [], []
    for twice in (False, True):
        for want_ids in sets:
            s, keys = d.all_hit(len(want_ids))
            seqs.append(s + s if twice else s)
            kms.append(keys)
            ids.append(d.rng.permutation(want_ids))
    kms, ids = np.concatenate(kms), np.concatenate(ids)
    table = d.table()
    res, off = pack([(str(i), s) for i, s in enumerate(seqs)])
    want, hits = _expect(oracle_lib, table, res, off, kms, ids)
    assert _rows_per_seq(want).tolist() == [192, 193, 192] * 2
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        _rollups(gpu, ctx, res, off, kms, ids, want, what="table probing")


# --- id classes ---------------------------------------------------------------

def _skew_world(oracle_lib):
    """600 ids of class 0 at P = 4, one per hit, in one sequence (then twice),
    between ordinary sequences: P doubles four times (1 -> 16), the flags
    reset between; the largest class is above the table's fill at 8 and
    within it at 16."""
    d = Designed(303)
    draw = np.unique(d.rng.integers(0, NO_ID, 6000, dtype=np.uint64))
    draw = d.rng.permutation(draw[roll_class(draw, 4) == 0])[:600].astype(np.uint32)
    assert len(draw) == 600
    assert np.bincount(roll_class(draw, 8)).max() > ROLL_FILL
    assert np.bincount(roll_class(draw, ROLL_MAX_P)).max() <= ROLL_FILL
    sizes = [40, 600, 70, 600, 30]
    id_sets = [d.distinct_ids(40, draw), draw, d.distinct_ids(70, draw), d.rng.permutation(draw),
               d.distinct_ids(30, draw)]
    seqs, kms, ids = [], [], []
    for i, (size, want_ids) in enumerate(zip(sizes, id_sets)):
        s, keys = d.all_hit(size)
        seqs.append(s + s if i == 3 else s)
        kms.append(keys)
        ids.append(want_ids)
    kms, ids = np.concatenate(kms), np.concatenate(ids)
    table = d.table()
    res, off = pack([(str(i), s) for i, s in enumerate(seqs)])
    want, hits = _expect(oracle_lib, table, res, off, kms, ids)
    assert _rows_per_seq(want).tolist() == sizes
    return table, res, off, kms, ids, want


@pytest.fixture(scope="module")
def skew_world(oracle_lib):
    return _skew_world(oracle_lib)


def test_class_skew(gpu, skew_world):
    table, res, off, kms, ids, want = skew_world
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        _rollups(gpu, ctx, res, off, kms, ids, want, what="class skew")


def test_class_collision(gpu, oracle_lib):
    """Ids that share every bit roll_class reads -- (r * 0xA5CB9243) mod 2^32,
    r < 8192: class 0 at every P -- so no number of classes separates them:
    400 in one sequence between two ordinary ones, and 250 interleaved with
    250 random ids in another.  The class loop gives up doubling at
    ROLL_MAX_P and takes the ids ROLL_FILL at a time in first-touch order:
    ceil(400 / 192) = ceil(500 / 192) = 3 such passes.

    Before that bound the kernel doubled P to 2^31, failed in the first pass
    each time, wrapped P to 0 and returned no rows for these two sequences."""
    d = Designed(404)
    col = collision_ids(1, 400)
    col2 = collision_ids(1001, 250)
    rnd = d.distinct_ids(250, np.concatenate([col, col2]))
    mixed = np.empty(500, np.uint32)
    mixed[0::2], mixed[1::2] = col2, rnd
    id_sets = [d.distinct_ids(50), col, d.distinct_ids(70), mixed, d.distinct_ids(30)]
    seqs, kms, ids = [], [], []
    for i, want_ids in enumerate(id_sets):
        s, keys = d.all_hit(len(want_ids))
        seqs.append(s + s if i in (1, 3) else s)  # the collision ids touched twice
        kms.append(keys)
        ids.append(want_ids)
    kms, ids = np.concatenate(kms), np.concatenate(ids)
    table = d.table()
    res, off = pack([(str(i), s) for i, s in enumerate(seqs)])
    want, hits = _expect(oracle_lib, table, res, off, kms, ids)
    assert _rows_per_seq(want).tolist() == [50, 400, 70, 500, 30]
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        _rollups(gpu, ctx, res, off, kms, ids, want, what="class collision")


# --- tile sizes and layouts ---------------------------------------------------

def _mapping(rng, kmers, pool, most=9, share=0.85):
    """(k-mer, id) pairs: `share` of the k-mers mapped, each to 1..most ids of the pool"""
    km = kmers[rng.random(len(kmers)) < share]
    n = rng.integers(1, most + 1, len(km))
    return np.repeat(km, n), pool[rng.integers(0, len(pool), int(n.sum()))]


def _hits_of(oracle_lib, table, seq):
    res, off = pack([("s", seq)])
    r = oracle_lib.process_batch(table, res, off, want=1)
    return r.hits["which_kmer"], r.hits["pos"]


def _tile_world(oracle_lib):
    """About 400 sequences over a synthetic image: family members, empty,
    7-residue and hit-free sequences, two of about 1,200 aa (the class path),
    and a sequence of 40 hits, none of them mapped, between two mapped ones;
    k-mers map to 1-9 ids of a small pool (ties, repeated ids in peg lists)."""
    spec, table = synthetic_table(60000)
    rng = np.random.default_rng(505)
    fam = _family_proteins(spec, rng, 40, 10)
    long_seqs = [b"".join(fam[10 * f] for f in range(a, a + 5)) for a in (2, 7)]  # five families each
    units = [[s] for s in fam[2:]] + [[s] for s in long_seqs]
    units += [[b""], [b""], [b"ACDEFGH"], [bytes(synth.ALPHA[rng.integers(0, 20, 300)])],
              [bytes(synth.ALPHA[rng.integers(0, 20, 9)])]]
    # source protein 45 is in no family above: a prefix of it with exactly 40 hits
    src = bytes(synth.ALPHA[synth.source_residue_codes(np.arange(45, 46))].reshape(-1))
    k45, pos = _hits_of(oracle_lib, table, src)
    assert len(pos) > 40
    lone = src[:int(pos[39]) + 9]
    lone_k, _ = _hits_of(oracle_lib, table, lone)
    assert len(lone_k) == 40
    units.append([fam[0], lone, fam[1]])
    seqs = [s for i in rng.permutation(len(units)) for s in units[i]]
    at = next(i for i, s in enumerate(seqs) if s is lone)
    res, off = pack([("s", s) for s in seqs])
    r = oracle_lib.process_batch(table, res, off, want=1)
    uk = np.setdiff1d(np.unique(r.hits["which_kmer"]), k45)
    pool = np.array([3, 7, 11, 12, 40, 41, 1000, 77777, (1 << 31) + 5, 0, NO_ID - 1] + list(range(100, 120)),
                    np.uint32)
    kms, ids = _mapping(rng, uk, pool)
    # the long sequences' k-mers to ids of their own, so they take the class path
    long_k = np.unique(np.concatenate([_hits_of(oracle_lib, table, s)[0] for s in long_seqs]))
    kms = np.concatenate([kms, long_k])
    ids = np.concatenate([ids, (500000 + np.arange(len(long_k))).astype(np.uint32)])
    want, hits = _expect(oracle_lib, table, res, off, kms, ids)
    rows = _rows_per_seq(want)
    assert hits[at] == 40 and rows[at] == 0 and rows[at - 1] > 0 and rows[at + 1] > 0
    assert rows.max() > 2 * ROLL_FILL and 380 <= len(seqs) <= 420
    return table, res, off, kms, ids, want


@pytest.fixture(scope="module")
def tile_world(oracle_lib):
    return _tile_world(oracle_lib)


@pytest.mark.parametrize("layout", ["packed_lines", "packed", "aos"])
def test_tile_sizes_and_layouts(gpu, tile_world, layout):
    """The corpus at every tile size (probe_j 1, 2, 3, 5, 8: T = 64 .. 512, not
    a power of two at 3 and 5), on PACKED16 with the line index on and off
    and on AOS24 (which has no line index: it holds PACKED16 records), after
    want 0, 1 and 3."""
    table, res, off, kms, ids, want = tile_world
    with gpu.Image.from_table(table) as img:
        if layout == "aos":
            img.set_layout(gpu.Image.AOS24)
        if layout == "packed_lines":
            img.set_line_index(36)
            assert img.line_count > 0
        assert img.layout == (gpu.Image.AOS24 if layout == "aos" else gpu.Image.PACKED16)
        with gpu.Context(img) as ctx:
            for j in (1, 2, 3, 5, 8):
                ctx.set_option("probe_j", j)
                _rollups(gpu, ctx, res, off, kms, ids, want, wants=(0, 1, 3), what=(layout, "probe_j", j))


# --- event ranges ---------------------------------------------------------------

@pytest.mark.parametrize("gaps", [False, True])
def test_event_ranges(gpu, oracle_lib, gaps):
    """All-hit sequences at probe_j = 1 (64 windows per tile, 128 per wave).
    By window: A [0, 64) ends at the last window of tile 0, which is hit 64 of
    wave 0's list (its run ends at lane 63); B [64, 512) starts at hit 65,
    covers 7 tiles and 4 waves and ends at a tile's last window; C is one
    window; D [513, 576) and F [641, 768) end at a tile's and a wave's last
    window.  Lists have 1 or 9 ids.  With `gaps`, a fifth of the inner
    sequences' k-mers are unmapped (lanes without events inside and at the
    ends of runs); the first and the last sequence stay mapped."""
    d = Designed(606 + gaps)
    sizes = [64, 448, 1, 63, 65, 127, 129, 64, 200]
    ends = np.cumsum(sizes)
    assert ends[0] == 64 and ends[1] == 8 * 64 and ends[3] % 64 == 0 and ends[5] % (64 * ROLL_TILES) == 0
    pool = d.distinct_ids(40)
    seqs, kms, ids = [], [], []
    for i, size in enumerate(sizes):
        s, keys = d.all_hit(size)
        seqs.append(s)
        for q, k in enumerate(keys):
            if gaps and 0 < i < len(sizes) - 1 and d.rng.random() < 0.2:
                continue
            n = 9 if (q + i) % 3 == 0 else 1
            kms.append(np.full(n, k, np.uint64))
            ids.append(d.rng.permutation(pool)[:n])
    kms, ids = np.concatenate(kms), np.concatenate(ids)
    table = d.table()
    res, off = pack([(str(i), s) for i, s in enumerate(seqs)])
    want, hits = _expect(oracle_lib, table, res, off, kms, ids)
    assert hits.tolist() == sizes  # every window but the last of each sequence hits
    rows = _rows_per_seq(want)
    assert rows[0] > 0 and rows[-1] > 0
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        ctx.set_option("probe_j", 1)
        _rollups(gpu, ctx, res, off, kms, ids, want, what=("event ranges", gaps))


# --- scan paths -------------------------------------------------------------------

def _waves(n_residues, probe_j):
    """nw of rollup_tiles: max_tiles = n_residues / T + 1 (plan), kRollTiles tiles per wave"""
    max_tiles = n_residues // (64 * probe_j) + 1
    return (max_tiles + ROLL_TILES - 1) // ROLL_TILES


def _filled(rng, members, n_seq, n_residues, places):
    """n_seq sequences of n_residues in all: the members in len(places) groups
    at those fractions of the batch, random protein between them"""
    n_fill = n_seq - len(members)
    room = n_residues - sum(len(m) for m in members)
    assert n_fill > 0 and room >= 9 * n_fill
    lens = 9 + rng.multinomial(room - 9 * n_fill, np.full(n_fill, 1.0 / n_fill))
    assert lens.min() >= 9 and int(lens.sum()) == room
    fill = [bytes(synth.ALPHA[rng.integers(0, 20, int(n))]) for n in lens]
    groups = np.array_split(np.arange(len(members)), len(places))
    seqs, used = [], 0
    for frac, g in zip(places, groups):
        upto = int(round(frac * n_fill))
        seqs += fill[used:upto]
        used = upto
        seqs += [members[i] for i in g]
    seqs += fill[used:]
    assert len(seqs) == n_seq and sum(len(s) for s in seqs) == n_residues
    return seqs


SCAN_CASES = {
    # name: (sequences, residues or None, probe_j, row scan (n + 1), event scan (nw + 1))
    "n+1=8192": (8191, None, 2, "one workgroup", "one workgroup"),
    "n+1=8193": (8192, None, 2, "hipcub", "one workgroup"),
    "nw+1=8192": (2000, 1048320 + 60, 1, "one workgroup", "one workgroup"),
    "nw+1=8193": (2000, 1048448 + 60, 1, "one workgroup", "hipcub"),
    "both past": (8200, 1048448 + 100, 1, "hipcub", "hipcub"),
}
_scan_cache = {}


def _scan_case(oracle_lib, name):
    """The case's batch and its yardstick, computed once for both small_batch settings."""
    if name in _scan_cache:
        return _scan_cache[name]
    n_seq, n_res, probe_j, row_scan, event_scan = SCAN_CASES[name]
    if "world" not in _scan_cache:
        _scan_cache["world"] = synthetic_table(60000)
    spec, table = _scan_cache["world"]
    rng = np.random.default_rng(707 + n_seq)
    members = _family_proteins(spec, rng, 40, 5)  # 200 family members
    if n_res is None:
        # pieces of 20-40 aa, seven in ten cut out of a family member; the members' pieces in front,
        # in the middle and at the very end too
        seqs = []
        for i in range(n_seq):
            n = int(rng.integers(20, 41))
            if rng.random() < 0.7 or i < 50 or i >= n_seq - 50:
                m = members[int(rng.integers(0, len(members)))]
                a = int(rng.integers(0, len(m) - n))
                seqs.append(m[a:a + n])
            else:
                seqs.append(bytes(synth.ALPHA[rng.integers(0, 20, n)]))
    else:
        # the windows end near 0.985 of the waves (8 residues per sequence are no window): members in
        # front, in the middle, around the last waves that have windows, and at the very end
        seqs = _filled(rng, members, n_seq, n_res, (0.0, 0.5, 0.97, 1.0))
    res, off = pack([("s", s) for s in seqs])
    assert len(off) - 1 == n_seq
    nw = _waves(len(res), probe_j)
    assert (n_seq + 1 <= SCAN_ONE_MAX) == (row_scan == "one workgroup"), (n_seq, row_scan)
    assert (nw + 1 <= SCAN_ONE_MAX) == (event_scan == "one workgroup"), (nw, event_scan)
    if name.startswith("n+1"):
        assert n_seq + 1 == int(name[4:])
    if name.startswith("nw+1"):
        assert nw + 1 == int(name[5:])
    r = oracle_lib.process_batch(table, res, off, want=1)
    uk = np.unique(r.hits["which_kmer"])
    pool = np.concatenate([np.arange(1, 300), [(1 << 31) + 9]]).astype(np.uint32)
    kms, ids = _mapping(rng, uk, pool, most=4)
    want, hits = _expect(oracle_lib, table, res, off, kms, ids)
    rows = _rows_per_seq(want)
    assert rows[0] > 0 and rows[-1] > 0 and (rows > 0).sum() > 150 and (rows == 0).any()
    _scan_cache[name] = (table, res, off, kms, ids, want, probe_j)
    return _scan_cache[name]


@pytest.mark.parametrize("small_batch", ["default", 0])
@pytest.mark.parametrize("name", list(SCAN_CASES))
def test_scan_paths(gpu, oracle_lib, name, small_batch):
    """The rows' scan takes one workgroup (scan_one_kernel) up to n + 1 = 8,192
    values and hipcub past it; the event scan of rollup_tiles makes the same
    choice on nw + 1, independently: the four combinations, the two
    thresholds at their last and first value.  _scan_case asserts from the
    restated arithmetic which branch each case takes."""
    table, res, off, kms, ids, want, probe_j = _scan_case(oracle_lib, name)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        ctx.set_option("probe_j", probe_j)
        if small_batch != "default":
            ctx.set_option("small_batch", small_batch)
        _rollups(gpu, ctx, res, off, kms, ids, want, what=(name, "small_batch", small_batch))


# --- presizing ----------------------------------------------------------------------

def test_presized_exactly_and_one_short(gpu, oracle_lib):
    """A context's rollup is enqueued sized for hint + hint / 8 + 4096 events,
    hint being its previous rollup's count (rollup_enqueue): a batch with
    exactly that many events fits; one with one event more writes nothing and
    runs again at its true size (rollup_finish).  One designed sequence, one
    event per hit, adjusts the count."""
    d = Designed(808)
    base = [d.all_hit(n) for n in (300, 77, 150)]
    base_ids = [d.distinct_ids(n) for n in (300, 77, 150)]
    hint = 527
    cap = hint + hint // 8 + 4096
    extra, extra_keys = d.all_hit(cap - hint + 1)
    extra_ids = d.rng.integers(0, 5000, len(extra_keys)).astype(np.uint32)  # ~4,000 distinct: the class path
    kms = np.concatenate([k for _, k in base] + [extra_keys])
    ids = np.concatenate(base_ids + [extra_ids])
    table = d.table()
    base_seqs = [s for s, _ in base]

    def batch(n_extra):
        """the base sequences with the first n_extra hits of the designed one in the middle"""
        seqs = base_seqs[:2] + ([extra[:n_extra + 8]] if n_extra else []) + base_seqs[2:]
        res, off = pack([(str(i), s) for i, s in enumerate(seqs)])
        want, hits = _expect(oracle_lib, table, res, off, kms, ids)
        assert int(hits.sum()) == hint + n_extra  # one event per hit
        return res, off, want

    runs = [batch(0), batch(cap - hint), batch(0), batch(cap - hint + 1), batch(0)]
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        for family in MODES:
            with gpu.Kmap(0, gpu.KMAP_SET if family else gpu.KMAP_APPEND) as dev:
                dev.add(kms, ids)
                for i, (res, off, want) in enumerate(runs):
                    ctx.process_batch(res, off, want=0)
                    roff, rows = dev.rollup(ctx, gpu.ROLLUP_FAMILY if family else gpu.ROLLUP_PEG)
                    ys.assert_rows(roff, rows, *want[family], what=("presizing", family, i))


# --- through the pool -------------------------------------------------------------------

@pytest.mark.parametrize("n_ctx", [1, 3])
@pytest.mark.parametrize("corpus", ["tiles", "skew"])
def test_pool_lookup_matches_yardstick(gpu, tile_world, skew_world, corpus, n_ctx):
    """kgx_pool_lookup (shards on n_ctx contexts, rows stitched in sequence
    order) over the tile-size corpus and the class-skew corpus, against the
    yardstick for every sequence."""
    table, res, off, kms, ids, want = tile_world if corpus == "tiles" else skew_world
    with gpu.Image.from_table(table) as img, gpu.Pool([img], n_ctx) as pool:
        for family in MODES:
            with gpu.Kmap(0, gpu.KMAP_SET if family else gpu.KMAP_APPEND) as dev:
                dev.add(kms, ids)
                for _ in range(2):  # the second call's rollups are sized by the first's counts
                    got, roff, rows = pool.lookup([dev], res, off, want=gpu.WANT_BEST,
                                                  mode=gpu.ROLLUP_FAMILY if family else gpu.ROLLUP_PEG)
                    ys.assert_rows(roff, rows, *want[family], what=(corpus, n_ctx, family))
