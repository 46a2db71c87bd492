"""Recall on the device (csrc/kgx_recall.hip, abi.Recall, close_kmers_amd/recall.py)
against a CPU yardstick: sig_restate.select -> sig_restate.table ->
oracle.process_batch(params (5, 200, 0, 0), hits | calls | best).best, then the
cells, per-function counts, changed list and confusions in numpy, from the
definitions of include/kgx.h.

best is compared as bits: with Context.process_batch on the same image in all
six fields; with the oracle in kind, score, weighted_score, score_offset where
kind != 0, fi0 where kind is 1 or 2 and fi1 where kind is 2.  In kind 3 the
oracle's decision carries -1 / -1 where kgx_best_call carries the top two
functions (kgx.h), so there the two arrays differ by their definitions.
"""
import ctypes
import os

import numpy as np
import pytest

import sig_corpora
import sig_restate
from close_kmers_amd import image_files
from helpers import pack, random_protein, write_fasta

pytestmark = pytest.mark.gpu

WANT = 1 | 2 | 8
PARAMS = (5, 200, 0, 0)
OTHER, NONE = -1, -2


def _pack(seqs):
    return pack([(str(i), s) for i, s in enumerate(seqs)])


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tallies(kind, fi0, lab, n_functions):
    """cells, per-function (labelled, correct, called), changed, confusions."""
    kind, fi0, lab = np.asarray(kind), np.asarray(fi0), np.asarray(lab)
    cc = np.where(kind == 1, np.where(fi0 == lab, 0, 1), np.where(kind == 2, 2, 3))
    lc = np.where(lab >= 0, 0, np.where(lab == OTHER, 1, 2))
    cell = np.zeros((3, 4), np.uint64)
    np.add.at(cell, (lc, cc), 1)
    fn = np.stack([np.bincount(lab[lab >= 0], minlength=n_functions),
                   np.bincount(lab[cc == 0], minlength=n_functions),
                   np.bincount(fi0[kind == 1], minlength=n_functions)], axis=1)
    changed = np.nonzero(((cc == 3) & (lab != NONE)) | (cc == 1) | (cc == 2))[0]
    mis = (lc == 0) & (cc == 1)
    if not mis.any():
        return cell, fn, changed, []
    pairs, counts = np.unique(np.stack([lab[mis], fi0[mis]], axis=1), axis=0, return_counts=True)
    return cell, fn, changed, [(int(a), int(b), int(c)) for (a, b), c in zip(pairs, counts)]


def check_tallies(r, kind, fi0, lab, n_functions, what=""):
    cell, fn, changed, pairs = tallies(kind, fi0, lab, n_functions)
    st = r.stats()
    assert st["n_seq"] == len(lab), what
    assert np.array_equal(st["cell"], cell), (what, st["cell"], cell)
    got = r.functions()
    assert len(got) == n_functions
    for j, f in enumerate(("labelled", "correct", "called")):
        assert np.array_equal(got[f], fn[:, j]), (what, f)
    assert np.array_equal(r.changed(), changed), what
    assert st["n_changed"] == len(changed) and st["n_confusions"] == len(pairs)
    c = r.confusions()
    assert [(int(x["label"]), int(x["called"]), int(x["count"])) for x in c] == pairs, what
    return cell


def pieces_by_rule(off, piece):
    """A piece is closed before the sequence that would take it above `piece` residues."""
    n, s0, count = len(off) - 1, 0, 0
    while s0 < n:
        s1 = s0 + 1
        while s1 < n and int(off[s1 + 1]) - int(off[s0]) <= piece:
            s1 += 1
        count += 1
        s0 = s1
    return count


@pytest.fixture(scope="module")
def world(gpu, oracle_lib):
    seqs, fn, nf = sig_corpora.family_corpus()
    recs, _ = sig_restate.select(seqs, fn, nf)
    table = sig_restate.table(recs)
    q, lab = list(seqs), list(fn)
    for a in range(6):
        b = (a + 1) % 6
        for cut in (50, 55, 60, 65, 70):
            q.append(seqs[6 * a][:cut] + seqs[6 * b + 1][cut:])
            lab.append(a)
    q.append(seqs[0][:40] + seqs[6][40:80] + seqs[12][80:])
    lab.append(0)
    q.append(random_protein(np.random.default_rng(5), 120).encode())
    lab.append(2)
    q += [b"", b"ACDEFGH", seqs[3][:20]]
    lab += [1, 3, 0]
    res, off = _pack(q)
    ref = oracle_lib.process_batch(table, res, off, params=PARAMS, want=WANT).best
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        yield {"ctx": ctx, "seqs": seqs, "fn": fn, "nf": nf, "q": q, "res": res, "off": off,
               "lab": np.array(lab, np.int32), "ref": ref, "table": table, "oracle": oracle_lib}


def normal_batch_ok(w, gpu):
    """the context still answers a batch as the oracle does"""
    got = w["ctx"].process_batch(w["res"], w["off"], gpu.Params(*PARAMS), want=WANT)
    want = w["oracle"].process_batch(w["table"], w["res"], w["off"], params=PARAMS, want=WANT)
    assert w["oracle"].diff_batch(got, want, WANT) == {"hits": [], "calls": [], "best": []}


def test_the_yardstick_holds_what_the_corpus_promises(world):
    ref, lab = world["ref"], world["lab"]
    kind = ref["kind"]
    assert np.bincount(kind, minlength=4).tolist() == [3, 59, 8, 1]
    assert (kind[:36] == 1).all() and np.array_equal(ref["fi0"][:36], lab[:36])
    for a in range(6):
        k = kind[36 + 5 * a:41 + 5 * a].tolist()
        m = (ref["fi0"][36 + 5 * a:41 + 5 * a] == a).tolist()
        assert k[0] == 1 and not m[0] and k[2] == 2 and k[4] == 1 and m[4], a  # cut 50 mismatch, 60 ambiguous, 70 match
        if a in (3, 4):  # a second ambiguous row: cut 55 of family 3, cut 65 of family 4
            assert k.count(2) == 2 and k[1 if a == 3 else 3] == 2, a
        else:            # cut 55 mismatch, cut 65 match
            assert k[1] == k[3] == 1 and not m[1] and m[3], a
    assert kind[66] == 3 and kind[67:70].tolist() == [0, 0, 0]
    assert kind[70] == 1 and ref["fi0"][70] == 0


def test_checked_corpus(world, gpu):
    ctx, res, off, lab, ref, nf = (world[k] for k in ("ctx", "res", "off", "lab", "ref", "nf"))
    with gpu.Recall(ctx, res, off, lab, nf, gpu.Params(*PARAMS)) as r:
        best = r.best()
        cell = check_tallies(r, ref["kind"], ref["fi0"], lab, nf, "all kept")
        ms = r.stage_ms()
    assert tuple(ms) == gpu.RECALL_STAGES and all(v >= 0 for v in ms.values()) and ms["pass"] > 0
    assert (cell[0] > 0).all() and not cell[1:].any()
    # best against the oracle, as bits
    k = best["kind"]
    assert np.array_equal(k, ref["kind"])
    for f in ("score", "weighted_score"):
        assert np.array_equal(_bits(best[f]), _bits(ref[f])), f
    assert np.array_equal(_bits(best["score_offset"])[k != 0], _bits(ref["score_offset"])[k != 0])
    assert np.array_equal(best["fi0"][(k == 1) | (k == 2)], ref["fi0"][(k == 1) | (k == 2)])
    assert np.array_equal(best["fi1"][k == 2], ref["fi1"][k == 2])
    # and against the lookup path on the same image, every field
    got = ctx.process_batch(res, off, gpu.Params(*PARAMS), want=WANT).best
    for f in best.dtype.names:
        assert np.array_equal(_bits(best[f]), _bits(got[f])), f
    # other and none labels: every reachable cell is hit
    lab2 = lab.copy()
    lab2[[1, 36, 38, 67]] = OTHER    # match -> other/mismatch; mismatch; ambiguous; none
    lab2[[2, 41, 43, 68]] = NONE
    with gpu.Recall(ctx, res, off, lab2, nf, gpu.Params(*PARAMS)) as r:
        cell = check_tallies(r, ref["kind"], ref["fi0"], lab2, nf, "other and none")
        best2 = r.best()
    assert (cell[0] > 0).all() and (cell[1:, 1:] > 0).all() and not cell[1:, 0].any()
    assert best2.tobytes() == best.tobytes()


@pytest.mark.parametrize("piece", [300, 50])
def test_piece_invariance(world, gpu, piece):
    ctx, res, off, lab, nf = (world[k] for k in ("ctx", "res", "off", "lab", "nf"))
    lab = lab.copy()
    lab[[1, 36, 38, 67]] = OTHER
    lab[[2, 41, 43, 68]] = NONE
    with gpu.Recall(ctx, res, off, lab, nf, gpu.Params(*PARAMS)) as a, \
            gpu.Recall(ctx, res, off, lab, nf, gpu.Params(*PARAMS), piece_residues=piece) as b:
        sa, sb = a.stats(), b.stats()
        assert sa["n_pieces"] == 1 and sb["n_pieces"] == pieces_by_rule(off, piece) > 30
        assert np.array_equal(sa["cell"], sb["cell"])
        assert (sa["n_changed"], sa["n_confusions"]) == (sb["n_changed"], sb["n_confusions"])
        for f in ("best", "functions", "changed", "confusions"):
            assert getattr(a, f)().tobytes() == getattr(b, f)().tobytes(), f


def cycled(world, n):
    seqs = [world["seqs"][i % 36] for i in range(n)]
    ref = world["ref"][:36][np.arange(n) % 36]
    return _pack(seqs) + (ref,)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_wave_aggregation_shapes(world, gpu, n):
    res, off, ref = cycled(world, n)
    for what, lab in (("one label", np.full(n, 2, np.int32)),
                      ("64 consecutive labels distinct", (17 + np.arange(n) % 64).astype(np.int32)),
                      ("labels as called", ref["fi0"].astype(np.int32))):
        with gpu.Recall(world["ctx"], res, off, lab, 100, gpu.Params(*PARAMS)) as r:
            check_tallies(r, ref["kind"], ref["fi0"], lab, 100, f"{what}, n_seq {n}")


def test_five_thousand_sequences_with_one_label(world, gpu):
    res, off, ref = cycled(world, 5000)
    lab = np.full(5000, 4, np.int32)
    with gpu.Recall(world["ctx"], res, off, lab, 100, gpu.Params(*PARAMS)) as r:
        check_tallies(r, ref["kind"], ref["fi0"], lab, 100)
        fn = r.functions()
    assert fn["labelled"][4] == 5000 and fn["labelled"].sum() == 5000 and 0 < fn["correct"][4] == fn["called"][4]


def test_offsets_starting_at_13(world, gpu):
    ctx, res, off, lab, nf = (world[k] for k in ("ctx", "res", "off", "lab", "nf"))
    with gpu.Recall(ctx, res, off, lab, nf, gpu.Params(*PARAMS)) as a, \
            gpu.Recall(ctx, np.concatenate([np.full(13, ord("A"), np.uint8), res]), off + np.uint64(13), lab, nf,
                       gpu.Params(*PARAMS)) as b:
        assert np.array_equal(a.stats()["cell"], b.stats()["cell"])
        for f in ("best", "functions", "changed", "confusions"):
            assert getattr(a, f)().tobytes() == getattr(b, f)().tobytes(), f


def test_a_nul_cuts_a_sequence_as_in_the_lookup(world, gpu):
    ctx, lab, nf = world["ctx"], world["lab"], world["nf"]
    q = list(world["q"])
    q[4] = q[4][:70] + b"\0" + q[4][71:]   # a member: its call is made from 70 residues
    q[40] = b"\0" + q[40][1:]
    res, off = _pack(q)
    got = ctx.process_batch(res, off, gpu.Params(*PARAMS), want=WANT).best
    assert got["kind"][40] == 0 and got[4].tobytes() != world["ref"][4].tobytes()
    for piece in (0, 300):
        with gpu.Recall(ctx, res, off, lab, nf, gpu.Params(*PARAMS), piece_residues=piece) as r:
            assert r.best().tobytes() == got.tobytes()
            check_tallies(r, got["kind"], got["fi0"], lab, nf, f"NUL, piece {piece}")


def test_error_cases(world, gpu):
    ctx, res, off, lab, nf = (world[k] for k in ("ctx", "res", "off", "lab", "nf"))
    with gpu.Recall(ctx, np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.int32), nf) as r:
        st = r.stats()
        assert st["n_seq"] == 0 and st["n_pieces"] == 0 and not st["cell"].any()
        assert len(r.best()) == len(r.changed()) == len(r.confusions()) == 0
        assert len(r.functions()) == nf and not r.functions()["labelled"].any()
    normal_batch_ok(world, gpu)
    for bad, code in ((-3, gpu.KGX_EINVAL), (nf, gpu.KGX_EINVAL)):
        lab2 = lab.copy()
        lab2[5] = bad
        with pytest.raises(gpu.KgxError) as e:
            gpu.Recall(ctx, res, off, lab2, nf)
        assert e.value.code == code
        normal_batch_ok(world, gpu)
    with pytest.raises(gpu.KgxError) as e:  # the image calls functions 3, 4 and 5
        gpu.Recall(ctx, res, off, np.minimum(lab, 2), 3)
    assert e.value.code == gpu.KGX_ERANGE
    normal_batch_ok(world, gpu)


# ---- end to end: files in, files out -------------------------------------------

NAMES = ["zeta", "Alpha", "beta", "gamma", "delta", "rare"]  # family -> function; the index is the sorted order


def g6(x) -> bytes:
    """the float as the C library formats it (kgx_format_g6), not as recall.py does"""
    from close_kmers_amd import abi
    buf = ctypes.create_string_buffer(64)
    n = abi.lib().kgx_format_g6(ctypes.c_float(float(x)), buf, 64)
    return buf.raw[:n]


def expected_files(ids, old, best, functions):
    """Calls and New bytes of one FASTA file from the yardstick's best calls."""
    calls, new = b"", b""
    for rid, was, b in zip(ids, old, best):
        if b["kind"] == 1:
            func = functions[b["fi0"]]
        elif b["kind"] == 2:
            func = b" ?? ".join(sorted([functions[b["fi0"]], functions[b["fi1"]]], reverse=True))
        else:
            func = b""
        calls += rid + b"\t" + func + b"\t" + g6(b["score"]) + b"\t" + g6(b["weighted_score"]) + b"\n"
        if func != was:
            new += rid + b"\t" + was + b"\t" + func + b"\n"
    return calls, new


def write_corpus(tmp_path, seqs):
    """genome g holds member g of every family; defs_swapped.tsv: two ids of genome 0 trade functions"""
    defs, swapped, fastas, ids = tmp_path / "defs.tsv", tmp_path / "defs_swapped.tsv", [], []
    with open(defs, "w") as f, open(swapped, "w") as fs:
        for g in range(6):
            recs = []
            for fam in range(6):
                rid = f"fig|{g}.1.peg.{fam}"
                f.write(f"{rid}\t{NAMES[fam]}\textra column\n")
                fs.write(f"{rid}\t{NAMES[1 - fam] if g == 0 and fam in (0, 1) else NAMES[fam]}\n")
                recs.append((rid, seqs[fam * 6 + g].decode()))
            fastas.append(str(tmp_path / f"g{g}.fa"))
            write_fasta(fastas[-1], recs)
            ids.append([r[0].encode() for r in recs])
    return str(defs), str(swapped), fastas, ids


def check_recall_dir(rec, fastas, ids, id_function, functions, best, fn):
    """Calls/, New/ and the two reports of a recall directory against the yardstick; returns New's bytes."""
    _, per_fn, _, pairs = tallies(best["kind"], best["fi0"], fn, len(functions))
    new_total = b""
    for g, p in enumerate(fastas):
        leaf = os.path.basename(p)
        old = [id_function[r] for r in ids[g]]
        calls, new = expected_files(ids[g], old, best[6 * g:6 * g + 6], functions)
        assert open(os.path.join(rec, "Calls", leaf), "rb").read() == calls, leaf
        assert open(os.path.join(rec, "New", leaf), "rb").read() == new, leaf
        new_total += new
    rows = [ln.split(b"\t") for ln in open(os.path.join(rec, "functions.tsv"), "rb").read().splitlines()]
    assert [r[1] for r in rows] == functions
    assert [[int(x) for x in r[2:]] for r in rows] == per_fn.tolist()
    rows = [tuple(int(x) for x in ln.split()) for ln in open(os.path.join(rec, "confusions.tsv")).read().splitlines()]
    assert rows == pairs
    return new_total


def test_end_to_end(gpu, oracle_lib, tmp_path, capsys):
    from close_kmers_amd import recall, signatures
    seqs, _, _ = sig_corpora.family_corpus()
    defs, swapped, fastas, ids = write_corpus(tmp_path, seqs)
    # a validation folder of the same files; one record without an id, which the annotations name
    val = tmp_path / "val"
    os.makedirs(val / "seq")
    os.makedirs(val / "anno")
    for p in fastas:
        with open(val / "seq" / os.path.basename(p), "wb") as f:
            f.write(open(p, "rb").read() + (b">\nACDEFGHIKLMNPQ\n" if p == fastas[2] else b""))
    with open(val / "anno" / "anno.tsv", "wb") as f:
        f.write(open(defs, "rb").read() + b"\tsomething\n")
    out, rec = str(tmp_path / "data"), str(tmp_path / "recall")
    stats = signatures.build_data_dir([defs], fastas, out, recall_output=rec, validation_folder=str(val))
    printed = capsys.readouterr().out.splitlines()

    # the yardstick over the same records, in file order
    id_function = signatures.read_definitions([defs])
    records = [signatures.read_fasta(p) for p in fastas]
    functions = sorted(n.encode() for n in NAMES)
    res, off, fn = signatures.label(id_function, records, functions)
    flat = [s for recs in records for _, s in recs]
    want, _ = sig_restate.select(flat, fn.tolist(), 6)
    table = sig_restate.table(want)
    own = image_files.read_image(out)
    if own.tobytes() != table.tobytes():  # a weight off in its last bit (test_gpu_signatures.py): the device's table
        table = own
    best = oracle_lib.process_batch(table, res, off, params=PARAMS, want=WANT).best
    cell, _, changed, _ = tallies(best["kind"], best["fi0"], fn, 6)
    assert np.array_equal(np.array(stats["recall"]["cell"], np.uint64), cell)
    assert stats["recall"]["n_changed"] == len(changed) == 0
    assert check_recall_dir(rec, fastas, ids, id_function, functions, best, fn) == b""  # every protein recalls its own
    # validation: per file, the same six records against the same strings
    lines = []
    for g, p in enumerate(fastas):
        c, _, _, _ = tallies(best["kind"][6 * g:6 * g + 6], best["fi0"][6 * g:6 * g + 6], fn[6 * g:6 * g + 6], 6)
        correct = int(c[0, 0] + c[2, 3])
        extra = 1 if g == 2 else 0
        lines.append(f"{val / 'seq' / os.path.basename(p)}: count={6 + extra} correct={correct} "
                     f"incorrect={6 - correct} missing={extra}")
    assert stats["validation"] == lines and [ln for ln in printed if ": count=" in ln] == lines
    assert all("correct=6 incorrect=0" in ln for ln in lines)

    # two definitions swapped, recalled against the directory just written: the two rows are New
    rec2 = str(tmp_path / "recall_swapped")
    assert recall.main(["--data", out, "--definitions", swapped, "--fasta", *fastas, "--recall-output", rec2]) == 0
    id2 = signatures.read_definitions([swapped])
    fn2 = recall.labels(id2, records, functions)
    assert (fn2 != fn).sum() == 2
    new = check_recall_dir(rec2, fastas, ids, id2, functions, best, fn2)
    assert new == b"fig|0.1.peg.0\tAlpha\tzeta\nfig|0.1.peg.1\tzeta\tAlpha\n"
    assert open(os.path.join(rec2, "New", "g1.fa"), "rb").read() == b""
