"""Grouping by k-mer set on the device (csrc/kgx_uniq.hip, abi.Unique,
close_kmers_amd/unique_prots.py) against the yardstick: the oracle's hits
(oracle.process_batch, want 1) through tests/uniq_restate.py.  Every case
compares groups(), group_of(), sets() and the stats' counts exactly.

The oracle takes a sequence as its bytes; the host-buffer path cuts one at
its first NUL, so the yardstick is given the bytes before it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import sig_corpora
import sig_restate
import uniq_restate
from close_kmers_amd import image_files
from helpers import ALPHA, DesignedImage, encode, pack, random_protein, write_fasta

pytestmark = pytest.mark.gpu

# csrc/kgx_uniq.hip: a list of at most kUniqThreadList keys is digested by one
# thread, a longer one by a wave; the head test and the gather of the groups'
# lists take kUniqWaveStep keys per step
THREAD_LIST, WAVE_STEP = 32, 64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def decode(key: int) -> str:
    s = ""
    for _ in range(8):
        s = ALPHA[key % 20] + s
        key //= 20
    return s


def of_keys(keys) -> bytes:
    """A sequence whose set is exactly `keys`: the 8-mers, an X after each
    (every window over an X is skipped; the last window of a sequence is
    never looked up, so each 8-mer needs a residue behind it)."""
    return "".join(decode(int(k)) + "X" for k in keys).encode()


def _pack(seqs):
    return pack([(str(i), s) for i, s in enumerate(seqs)])


def yardstick(oracle_lib, table, seqs):
    """groups, key tuples and the hit count of the sequences, each cut at its first NUL"""
    res, off = _pack([s.split(b"\0")[0] for s in seqs])
    r = oracle_lib.process_batch(table, res, off, want=1)
    groups, keys = uniq_restate.groups(r.hit_offsets, r.hits["which_kmer"])
    return groups, keys, int(r.hit_offsets[-1])


def check(u, want, n_seq, what=""):
    groups, keys, n_hits = want
    goff, members = u.groups()
    assert goff[0] == 0 and len(goff) == len(groups) + 1, what
    got = [members[int(goff[g]):int(goff[g + 1])].tolist() for g in range(len(goff) - 1)]
    assert got == groups, what
    assert np.array_equal(u.group_of(), uniq_restate.group_of(groups, n_seq)), what
    soff, k = u.sets()
    assert soff[0] == 0 and len(soff) == len(keys) + 1, what
    assert [tuple(int(x) for x in k[int(soff[g]):int(soff[g + 1])]) for g in range(len(soff) - 1)] == keys, what
    st = u.stats()
    assert st["n_seq"] == n_seq and st["n_hits"] == n_hits, (what, st)
    assert st["n_set_keys"] == sum(len(kk) * len(g) for kk, g in zip(keys, groups)), (what, st)
    assert st["n_groups"] == len(groups), (what, st)
    assert st["n_empty"] == (len(groups[0]) if groups and keys[0] == () else 0), (what, st)
    assert st["largest_group"] == max((len(g) for g in groups), default=0), (what, st)
    return st


@pytest.fixture(scope="module")
def world(gpu, oracle_lib):
    seqs, fn, nf = sig_corpora.family_corpus()
    recs, _ = sig_restate.select(seqs, fn, nf)
    table = sig_restate.table(recs)
    # member 3's ascending key list, for the lists that are prefixes of it
    res, off = _pack([seqs[3]])
    full = sorted(set(int(x) for x in oracle_lib.process_batch(table, res, off, want=1).hits["which_kmer"]))
    assert len(full) > 8
    rng = np.random.default_rng(17)
    q = list(seqs)                                             # 0-35: the members
    q += [seqs[0], seqs[7], seqs[20]]                          # 36-38: exact copies
    q += [seqs[5] + seqs[5], seqs[9][60:] + seqs[9][:60]]      # 39 doubled, 40 halves swapped
    for m in (3, 14, 25):                                      # 41-49: truncations (subsets)
        q += [seqs[m][:30], seqs[m][:60], seqs[m][:90]]
    q += [of_keys(full[:1]), of_keys(full[:2]), of_keys(full[:5]), of_keys(full)]  # 50-53: prefixes of member 3's list
    q += [of_keys(full[:2][::-1] + full[:2])]                  # 54: the two-key prefix, other order and multiplicities
    q += [random_protein(rng, 120).encode(), random_protein(rng, 40).encode()]     # 55, 56
    q += [b"", b"ACDEFGH", seqs[4].lower(), b"MMMMMMMMMMMM", b""]                  # 57-61: empty sets
    x = bytearray(seqs[4])                                     # 62: lower case and X inside a member
    x[20:32] = bytes(x[20:32]).lower()
    x[70] = ord("X")
    x[90] = ord("*")
    q.append(bytes(x))
    q += [seqs[6][:60] + b"\0" + seqs[6][61:], b"\0" + seqs[8][1:]]               # 63, 64: a NUL
    q += [seqs[i] for i in (30, 31, 32, 33)]                   # 65-68: more copies, far from their originals
    q += [seqs[0], seqs[7][:60], seqs[20]]                     # 69-71
    for m in (1, 12, 23, 34):                                  # 72-87: every window start shifted
        q += [seqs[m][1:], seqs[m][2:], seqs[m][:119], b"A" + seqs[m]]
    q += [seqs[6][:60], seqs[0]]                               # 88, 89
    res, off = _pack(q)
    want = yardstick(oracle_lib, table, q)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        yield {"ctx": ctx, "img": img, "seqs": seqs, "q": q, "res": res, "off": off, "want": want, "table": table,
               "oracle": oracle_lib, "full": full}


def normal_batch_ok(w, gpu):
    """the context still answers a batch as the oracle does"""
    res, off = _pack(w["seqs"])
    got = w["ctx"].process_batch(res, off, gpu.Params(5, 200, 0, 0), want=1 | 2 | 8)
    want = w["oracle"].process_batch(w["table"], res, off, params=(5, 200, 0, 0), want=1 | 2 | 8)
    assert w["oracle"].diff_batch(got, want, 1 | 2 | 8) == {"hits": [], "calls": [], "best": []}


def test_the_yardstick_holds_what_the_corpus_promises(world):
    groups, keys, n_hits = world["want"]
    assert len(world["q"]) == 90 and n_hits > 1000
    # a group of three or more whose members are not neighbours
    far = [g for g in groups if len(g) >= 3 and all(b - a > 1 for a, b in zip(g, g[1:]))]
    assert far and any(g[0] == 0 and g[-1] == 89 for g in far)
    assert keys[0] == () and len(groups[0]) >= 4 and {57, 58, 59, 60, 61}.issubset(groups[0])
    # a list that is a proper prefix of another, next to it in the order
    assert any(len(a) < len(b) and b[:len(a)] == a for a, b in zip(keys[1:], keys[2:]))
    full = tuple(world["full"])
    for n in (1, 2, 5):
        assert full[:n] in keys
    assert groups[keys.index(full[:2])] == [51, 54] and 3 in groups[keys.index(full)] and 53 in groups[keys.index(full)]
    # the order is not the order by size
    assert sorted(keys, key=lambda k: (len(k), k)) != keys
    # the NUL cuts: 63 is its first 60 residues
    assert groups[uniq_restate.group_of(groups, 90)[63]] == [63, 88] and 64 in groups[0]


def test_checked_corpus(world, gpu):
    with gpu.Unique(world["ctx"], world["res"], world["off"]) as u:
        st = check(u, world["want"], 90)
        ms = u.stage_ms()
    assert st["n_pieces"] == 1 and st["digest_bits"] == 64
    assert tuple(ms) == gpu.UNIQ_STAGES and all(v >= 0 for v in ms.values()) and ms["pass"] > 0 and ms["group"] > 0
    normal_batch_ok(world, gpu)


def test_digest_bits_change_no_result(world, gpu):
    compares = {}
    for bits in (0, 1, 7, 64):
        with gpu.Unique(world["ctx"], world["res"], world["off"], digest_bits=bits) as u:
            st = check(u, world["want"], 90, f"digest_bits {bits}")
        assert st["digest_bits"] == bits
        compares[bits] = st["list_compares"]
    assert compares[0] > 0 and compares[64] <= compares[0], compares
    with pytest.raises(gpu.KgxError) as e:
        gpu.Unique(world["ctx"], world["res"], world["off"], digest_bits=65)
    assert e.value.code == gpu.KGX_EINVAL


@pytest.mark.parametrize("piece", [1, 100, 0])
def test_piece_invariance(world, gpu, piece):
    with gpu.Unique(world["ctx"], world["res"], world["off"], piece_residues=piece) as u:
        st = check(u, world["want"], 90, f"piece {piece}")
    assert st["n_pieces"] == uniq_restate.pieces_by_rule(world["off"], piece)
    assert st["n_pieces"] == {1: 90, 0: 1}.get(piece, st["n_pieces"]) and (piece != 100 or 30 < st["n_pieces"] < 90)


def test_layouts_and_line_index(world, gpu):
    img, ctx = world["img"], world["ctx"]
    try:
        assert img.layout == gpu.Image.PACKED16
        for load in (36, 0):
            img.set_line_index(load)
            assert (img.line_count > 0) == (load > 0)
            with gpu.Unique(ctx, world["res"], world["off"], piece_residues=500) as u:
                check(u, world["want"], 90, f"PACKED16, line index {load}")
        img.set_layout(gpu.Image.AOS24)
        with gpu.Unique(ctx, world["res"], world["off"], piece_residues=500) as u:
            check(u, world["want"], 90, "AOS24")
    finally:
        img.set_layout(gpu.Image.PACKED16)
        img.set_line_index(0)
    normal_batch_ok(world, gpu)


def test_keys_are_compared_in_all_35_bits(gpu, oracle_lib):
    c, k = encode("AAAACDEF"), encode("CDEFGHIK")
    k_hi, k_mid = k + 2 ** 32, k + 2 ** 32 - 7
    assert c < k < k_mid < k_hi < 20 ** 8 and k < 20 ** 8 - 2 ** 32
    assert k & 0xFFFFFFFF == k_hi & 0xFFFFFFFF and k_mid & 0xFFFFFFFF < k & 0xFFFFFFFF
    d = DesignedImage()
    for f, key in enumerate((c, k, k_hi, k_mid)):
        d.add(decode(key), f)
    table = d.table()
    seqs = [of_keys([c, k_hi]), of_keys([c, k]), of_keys([c, k_mid]), of_keys([k_hi, c])]
    want = yardstick(oracle_lib, table, seqs)
    assert want[1] == [(c, k), (c, k_mid), (c, k_hi)] and want[0] == [[1], [2], [0, 3]]
    res, off = _pack(seqs)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        for bits in (64, 0):
            with gpu.Unique(ctx, res, off, digest_bits=bits) as u:
                check(u, want, 4, f"digest_bits {bits}")
        img.set_layout(gpu.Image.AOS24)
        with gpu.Unique(ctx, res, off) as u:
            check(u, want, 4, "AOS24")


def test_list_lengths_around_every_threshold(gpu, oracle_lib):
    rng = np.random.default_rng(23)
    p = random_protein(rng, 5000)
    d = DesignedImage()
    d.add_windows(p, range(len(p) - 8), 1)
    table = d.table()
    sizes = [1, 2, THREAD_LIST - 1, THREAD_LIST, THREAD_LIST + 1, WAVE_STEP - 1, WAVE_STEP, WAVE_STEP + 1,
             2 * WAVE_STEP, 2 * WAVE_STEP + 1, len(p) - 8]
    # a sequence's last window is never looked up: size + 8 residues give `size` windows
    seqs = [p[:s + 8].encode() for s in sizes]
    seqs = seqs + seqs[::-1]
    want = yardstick(oracle_lib, table, seqs)
    assert sorted(len(k) for k in want[1]) == sizes and all(len(g) == 2 for g in want[0])
    res, off = _pack(seqs)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        for bits in (64, 0):
            with gpu.Unique(ctx, res, off, digest_bits=bits) as u:
                check(u, want, len(seqs), f"digest_bits {bits}")


def test_a_group_larger_than_a_workgroup(world, gpu):
    full = world["full"]
    table_keys = np.sort(world["table"]["which_kmer"][world["table"]["which_kmer"] < 20 ** 8])
    assert len(table_keys) > 301
    seqs = []
    for i in range(300):
        seqs += [world["seqs"][2], of_keys([table_keys[i], table_keys[i + 1]])]
    want = yardstick(world["oracle"], world["table"], seqs)
    assert len(want[0]) == 301 and max(len(g) for g in want[0]) == 300 and len(full) > 0
    res, off = _pack(seqs)
    for bits, piece in ((64, 0), (3, 4000)):
        with gpu.Unique(world["ctx"], res, off, piece_residues=piece, digest_bits=bits) as u:
            st = check(u, want, 600, f"digest_bits {bits}, piece {piece}")
        assert st["largest_group"] == 300


def test_edges(world, gpu):
    ctx = world["ctx"]
    with gpu.Unique(ctx, np.zeros(0, np.uint8), np.zeros(1, np.uint64)) as u:
        st = check(u, ([], [], 0), 0, "no sequence")
        assert st["n_pieces"] == 0
    normal_batch_ok(world, gpu)
    one = [world["seqs"][11]]
    res, off = _pack(one)
    with gpu.Unique(ctx, res, off) as u:
        check(u, yardstick(world["oracle"], world["table"], one), 1, "one sequence")
    empty = [b""] * 70
    res, off = _pack(empty)
    for piece in (0, 1):
        with gpu.Unique(ctx, res, off, piece_residues=piece) as u:
            st = check(u, ([list(range(70))], [()], 0), 70, "all empty")
            # no residue ever takes a piece above its bound: one piece
            assert st["n_empty"] == 70 and st["n_pieces"] == uniq_restate.pieces_by_rule(off, piece) == 1
    # offsets that do not start at 0
    shifted = np.concatenate([np.full(13, ord("A"), np.uint8), world["res"]])
    with gpu.Unique(ctx, shifted, world["off"] + np.uint64(13), piece_residues=700) as u:
        check(u, world["want"], 90, "offsets from 13")
    bad = world["off"].copy()
    bad[5] = bad[7]
    with pytest.raises(gpu.KgxError) as e:
        gpu.Unique(ctx, world["res"], bad)
    assert e.value.code == gpu.KGX_EINVAL
    normal_batch_ok(world, gpu)


def test_command_line(world, gpu, tmp_path):
    from close_kmers_amd import unique_prots
    q = world["q"]
    data = image_files.write_data_dir(str(tmp_path / "data"), world["table"], [f"function {i}" for i in range(6)])
    # two FASTA files read as one input; no record holds a NUL or is empty in a FASTA file
    keep = [i for i, s in enumerate(q) if s and b"\0" not in s]
    ids = [("" if n == 4 else f"prot{n}|x") for n in range(len(keep))]
    seqs = [q[i] for i in keep]
    half = len(keep) // 2
    fa = [str(tmp_path / "a.fa"), str(tmp_path / "b.fa")]
    write_fasta(fa[0], [(f"{i} some description" if i else "", s.decode()) for i, s in zip(ids[:half], seqs[:half])])
    write_fasta(fa[1], [(i, s.decode()) for i, s in zip(ids[half:], seqs[half:])])
    groups, _, _ = yardstick(world["oracle"], world["table"], seqs)
    goff = np.cumsum([0] + [len(g) for g in groups])
    want = unique_prots.format_groups([i.encode() for i in ids], goff, [i for g in groups for i in g])
    assert want == uniq_restate.text([i.encode() for i in ids], groups) and want.count(b"\n") == len(groups)
    r = subprocess.run([sys.executable, "-m", "close_kmers_amd.unique_prots", data, *fa], cwd=ROOT,
                       capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr.decode(errors="replace")
    assert r.stdout == want
    out = str(tmp_path / "groups.txt")
    assert unique_prots.main([data, *fa, "--output", out, "--piece-residues", "300"]) == 0
    assert open(out, "rb").read() == want
