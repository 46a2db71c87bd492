"""The kernels against the reference's own recorded answers
(golden/reference/, written by golden/make_reference_runs.py from the
reference's KmerGuts, KmerImage and FastqParser): hits, calls, OTU tallies and
best calls of every scoring route, the call service, the FASTQ parser,
validate_fastq's error and the image builder.  Bit for bit, no tolerances; the
CPU oracle takes no part in what is expected here.

Scorer routes by length (csrc/kgx_internal.h): the hybrid scores sequences of
up to LONG_SEQ = 2,048 windows in lanes and those of (2,048, RUN_CAP = 39,998]
windows with the wave scorer; score_variant 1 gives every sequence up to
RUN_CAP windows to the wave scorer and longer ones to the long scorer.  A
sequence of n residues has n - 8 windows, so the recorded sequences of 2,056 /
2,057 and 40,006 / 40,007 residues lie on either side of both, and the
saturation case (golden/cap, 40,172 residues) is past the second.
"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest

import ref_corpora
from helpers import GOLDEN

sys.path.insert(0, GOLDEN)
import make_reference_runs as recorder  # noqa: E402
import oracle  # noqa: E402  (record layouts and diff_batch only; nothing here runs the oracle)

pytestmark = pytest.mark.gpu

REF = os.path.join(GOLDEN, "reference")
FUNCTIONS = ref_corpora.FUNCTIONS
STRICT_FINISHED = 3


class Recorded:
    """One recorded corpus: inputs and, per parameter set, the reference's rows."""

    def __init__(self, stem):
        z = np.load(os.path.join(REF, stem + ".npz"))
        self.z = z
        self.names = json.load(open(os.path.join(REF, stem + ".json")))
        self.res, self.off = z["residues"], z["offsets"]
        self.params = [tuple(int(x) for x in p) for p in z["params"]]
        self.n = len(self.off) - 1
        self.seqs = [bytes(self.res[int(self.off[s]):int(self.off[s + 1])]) for s in range(self.n)]

    def want(self, i):
        z = self.z
        return oracle.BatchResult(z["hit_offsets"], z["hits"], z[f"call_offsets_{i}"], z[f"calls_{i}"],
                                  z[f"otu_offsets_{i}"], z[f"otus_{i}"].reshape(-1, 2), 0, 0, 0.0)

    def best(self, i):
        return self.z[f"best_{i}"], self.names["best_function"][i]


def _name(fi):
    return FUNCTIONS[fi] if 0 <= fi < len(FUNCTIONS) else "INVALID_OFFSET"


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _f32bits(x) -> int:
    return int(np.float32(x).view(np.uint32))


def bad_best(got, rows, texts):
    """Sequences whose kgx_best_call differs from the recorded find_best_call
    outputs (function_index, function, score, weighted_score, score_offset)."""
    bad = []
    for s, (g, r, fn) in enumerate(zip(got, rows, texts)):
        kind = 0 if not r["offset_set"] else 2 if " ?? " in fn else 1 if fn else 3
        ok = int(g["kind"]) == kind
        ok &= _bits(g["score"]) == _bits(r["score"]) and _bits(g["weighted_score"]) == _bits(r["weighted_score"])
        if kind:
            ok &= _bits(g["score_offset"]) == _bits(r["score_offset"])
        if kind == 1:
            ok &= int(g["fi0"]) == int(r["function_index"]) and _name(int(g["fi0"])) == fn
        elif kind == 2:
            f1, f2 = _name(int(g["fi0"])), _name(int(g["fi1"]))
            if f2 > f1:
                f1, f2 = f2, f1
            ok &= f1 + " ?? " + f2 == fn and int(r["function_index"]) == -1
        else:
            ok &= int(r["function_index"]) == -1
        if not ok:
            bad.append(s)
    return bad


@pytest.fixture(scope="module")
def designed():
    d = Recorded("designed")
    image = np.load(os.path.join(REF, "image.npz"))["image"]
    d.table = np.frombuffer(image.tobytes()[24:], oracle.SIG_DTYPE)  # the file the reference wrote
    assert len(d.table) == int(d.z["num_sigs"][0])
    return d


@pytest.fixture(scope="module")
def random_run():
    d = Recorded("random")
    d.entries, d.num_sigs = recorder.load_random_table(os.path.join(REF, "random_table.npz"))
    return d


@pytest.fixture(scope="module")
def routing():
    r = json.load(open(os.path.join(REF, "routing.json")))
    seqs = ref_corpora.routing_seqs()
    assert [(n, len(s), hashlib.sha256(s).hexdigest()) for n, s in seqs] == \
        [(q["name"], q["length"], q["sha256"]) for q in r["sequences"]]
    assert [len(s) - 8 for _, s in seqs] == [2048, 2049, 39998, 39999]
    r["res"] = np.frombuffer(b"".join(s for _, s in seqs), np.uint8)
    r["off"] = np.cumsum([0] + [len(s) for _, s in seqs]).astype(np.uint64)
    return r


INDEX_MODES = ("slots", "twins", "pairs")


@pytest.fixture(scope="module", params=INDEX_MODES)
def devices(request, gpu, designed, random_run):
    """{corpus: (image, context)} over the reference slots, over the line index
    with twins, and over the line index in the pairs layout."""
    mode = request.param
    mp = pytest.MonkeyPatch()
    for k, v in (("KGX_LINE_TWINS", "1"), ("KGX_LINE_MARKS", "1"), ("KGX_LINE_HOME", "1"),
                 ("KGX_LINE_PAIRS", "1" if mode == "pairs" else "0")):
        mp.setenv(k, v)
    img_d = gpu.Image.from_table(designed.table)
    img_r, stored = gpu.Image.build(*random_run.entries, random_run.num_sigs)
    assert stored == len(random_run.entries[0])
    out = {}
    try:
        for name, img in (("designed", img_d), ("random", img_r)):
            assert img.layout == gpu.Image.PACKED16
            if mode != "slots":
                img.set_line_index(36)
                assert img.line_count > 0 and img.line_pairs == int(mode == "pairs")
                st = img.line_stats()
                assert st["missing"] == 0 and st["unjustified"] == 0, st
            out[name] = (img, gpu.Context(img))
        if mode == "twins":
            assert img_r.line_twins > 0
        yield out
    finally:
        mp.undo()
        for img, ctx in out.values():
            ctx.close()
        img_d.close()
        img_r.close()


# option sets: every route that scores.  "want" 3 = hits | calls (what the lean
# scorer takes, with order_constraint 0); 15 adds OTU tallies and best calls.
ROUTES = {
    "default": ({}, 15),
    "hybrid": ({"small_wave": 0, "score_variant": 0}, 15),
    "wave": ({"small_wave": 0, "score_variant": 1}, 15),
    "lane": ({"small_wave": 0, "score_variant": 2}, 15),
    "lean0": ({"small_wave": 0, "score_lean": 0}, 3),
    "lean1": ({"small_wave": 0, "score_lean": 1}, 3),
    "lean2": ({"small_wave": 0, "score_lean": 2}, 3),
    "small_wave": ({"small_wave": 1}, 15),
    "small_fused": ({"small_fused": 1}, 3),  # one launch per batch: hits | calls, order_constraint 0
    "plan_fused0": ({"small_wave": 0, "plan_fused": 0}, 15),
    "plan_fused1": ({"small_wave": 0, "plan_fused": 1}, 15),
    "plan_fused2": ({"small_wave": 0, "plan_fused": 2}, 15),
}
DEFAULTS = {"small_wave": 1, "score_variant": 0, "score_lean": 1, "small_fused": 0, "plan_fused": 0}


def _apply(ctx, options):
    for k, v in {**DEFAULTS, **options}.items():
        ctx.set_option(k, v)


def _digests(got, s):
    h = got.hits[int(got.hit_offsets[s]):int(got.hit_offsets[s + 1])]
    c = got.calls[int(got.call_offsets[s]):int(got.call_offsets[s + 1])]
    o = got.otus[int(got.otu_offsets[s]):int(got.otu_offsets[s + 1])]
    return {"n_hits": len(h), "hits_sha256": recorder.hits_digest(h), "n_calls": len(c),
            "calls_sha256": recorder.rows_digest(c, recorder.CALL_FIELDS),
            "otus": [[int(a), int(b)] for a, b in zip(o["otu_index"], o["count"])]}


def _best_of_json(b):
    """(rows, texts) as Recorded.best gives them, from a JSON best entry
    [function_index, function, score, weighted bits, offset or null]."""
    row = np.zeros(1, recorder.BEST_REC)
    row["function_index"], row["score"] = b[0], b[2]
    row["weighted_score"] = np.array([b[3]], np.uint32).view(np.float32)
    row["score_offset"], row["offset_set"] = (0.0 if b[4] is None else b[4]), b[4] is not None
    return row, [b[1]]


@pytest.mark.parametrize("route", list(ROUTES))
def test_process_batch_routes(gpu, devices, designed, random_run, routing, route):
    options, mask = ROUTES[route]
    lean = route.startswith("lean")
    narrow = lean or route == "small_fused"  # routes that take order_constraint 0 only
    for name, rec in (("designed", designed), ("random", random_run)):
        img, ctx = devices[name]
        _apply(ctx, options)
        ran = 0
        for i, p in enumerate(rec.params):
            if narrow and p[2]:
                continue
            before = ctx.stat("lean_scores"), ctx.stat("fused_batches")
            got = ctx.process_batch(rec.res, rec.off, gpu.Params(*p), want=mask)
            bad = oracle.diff_batch(got, rec.want(i), mask & 7)
            if mask & 8:
                bad["best"] = bad_best(got.best, *rec.best(i))
            assert bad == {k: [] for k in bad}, (name, route, p, {k: v[:8] for k, v in bad.items()})
            if lean:
                assert ctx.stat("lean_scores") - before[0] == int(route != "lean0"), (name, route, p)
            if route == "small_fused":
                assert ctx.stat("fused_batches") - before[1] == 1, (name, p)
            ran += 1
        assert ran >= (5 if narrow else 8)
    # the sequences on either side of the scorer boundaries, over the designed table
    img, ctx = devices["designed"]
    for run in routing["runs"]:
        p = tuple(run["params"])
        if narrow and p[2]:
            continue
        got = ctx.process_batch(routing["res"], routing["off"], gpu.Params(*p), want=mask)
        for s, want in enumerate(run["sequences"]):
            g = _digests(got, s)
            if not mask & 4:
                g["otus"] = want["otus"]
            assert g == {k: want[k] for k in g}, (route, p, routing["sequences"][s]["name"])
            if mask & 8:
                assert not bad_best(got.best[s:s + 1], *_best_of_json(want["best"])), (route, p, s)
    _apply(ctx, {})


@pytest.mark.parametrize("variant", [0, 1, 2])
def test_saturated_run(gpu, variant):
    """golden/cap: more hits in one run than the buffer counts (kguts.cc:850-851)."""
    cap = json.load(open(os.path.join(REF, "cap.json")))
    d = os.path.join(GOLDEN, "cap")
    lines = open(os.path.join(d, "input.fasta")).read().split("\n")
    seq = "".join(lines[1:]).encode()
    assert len(seq) - 8 > 39998
    res, off = np.frombuffer(seq, np.uint8), np.array([0, len(seq)], np.uint64)
    with gpu.Image.open(os.path.join(d, "data")) as img, gpu.Context(img) as ctx:
        ctx.set_option("small_wave", 0)
        ctx.set_option("score_variant", variant)
        for run in cap["runs"]:
            got = ctx.process_batch(res, off, gpu.Params(*run["params"]), want=15)
            assert len(got.hits) == run["n_hits"] > 39998
            assert recorder.hits_digest(got.hits) == run["hits_sha256"]
            calls = [[int(c["start"]), int(c["end"]), int(c["count"]), int(c["function_index"]),
                      _f32bits(c["weighted_hits"])] for c in got.calls]
            assert calls == run["calls"], run["params"]
            assert [[int(a), int(b)] for a, b in zip(got.otus["otu_index"], got.otus["count"])] == run["otus"]
            b = run["best"][0]
            kind = 0 if b[4] is None else 2 if " ?? " in b[1] else 1 if b[1] else 3
            g = got.best[0]
            assert (int(g["kind"]), float(g["score"]), _f32bits(g["weighted_score"])) == (kind, b[2], b[3])
            if kind == 1:
                assert int(g["fi0"]) == b[0] and float(g["score_offset"]) == b[4]


def _one(hits, calls, otus):
    u = np.uint64
    return oracle.BatchResult(np.array([0, len(hits)], u), hits, np.array([0, len(calls)], u), calls,
                              np.array([0, len(otus)], u), otus, 0, 0, 0.0)


@pytest.mark.parametrize("probe", ["thread", "quad"])
def test_call_service_on_the_designed_corpus(gpu, designed, monkeypatch, probe):
    monkeypatch.setenv("KGX_SVC_PROBE", probe)
    with gpu.Image.from_table(designed.table) as img:
        assert img.layout == gpu.Image.PACKED16
        for indexed in (False, True):
            if indexed:
                img.set_line_index(36)
            served = 0
            for i, p in enumerate(designed.params):
                if p[2]:
                    continue  # the service leaves order_constraint to the batch paths
                want = designed.want(i)
                for s, seq in enumerate(designed.seqs):
                    hits, calls, otus = img.svc_call(seq, gpu.Params(*p), otus=True)
                    got = _one(hits, calls, otus)
                    one = _one(*(a[int(o[s]):int(o[s + 1])] for a, o in ((want.hits, want.hit_offsets),
                                                                         (want.calls, want.call_offsets),
                                                                         (want.otus, want.otu_offsets))))
                    one.hits = one.hits.copy()
                    one.hits["seq"] = 0
                    bad = oracle.diff_batch(got, one, 7)
                    assert bad == {k: [] for k in bad}, (probe, indexed, p, designed.names["sequences"][s], bad)
                    served += 1
            assert served == 6 * designed.n


def test_best_calls_from_recorded_calls(gpu, devices, designed, random_run):
    """kgx_find_best_calls over the reference's own calls."""
    kinds = set()
    for name, rec in (("designed", designed), ("random", random_run)):
        _, ctx = devices[name]
        for i in range(len(rec.params)):
            w = rec.want(i)
            got = ctx.find_best_calls(w.calls, w.call_offsets)
            assert not bad_best(got, *rec.best(i)), (name, rec.params[i])
            kinds |= set(int(k) for k in got["kind"])
    assert kinds == {0, 1, 2, 3}


def test_image_builder_writes_the_reference_file(gpu, designed):
    z = designed.z
    img, stored = gpu.Image.build(z["table_keys"], z["table_fI"], z["table_oI"], z["table_avg"], z["table_wt"],
                                  int(z["num_sigs"][0]))
    with img:
        assert stored == len(z["table_keys"])
        got = img.download()
    assert got.tobytes() == designed.table.tobytes()
    hdr = np.array([len(got), 24, 1], np.int64).tobytes()
    assert hdr + got.tobytes() == np.load(os.path.join(REF, "image.npz"))["image"].tobytes()


# ---------------------------------------------------------------------------
_CASES = []


def _fastq_cases():
    if _CASES:
        return _CASES
    out = _CASES
    for c in json.load(open(os.path.join(REF, "fastq.json"))):
        if "placed" in c:
            text = ref_corpora.placed_fastq(*c["placed"])
            assert hashlib.sha256(text).hexdigest() == c["text_sha256"]
        else:
            text = c["text"].encode("latin-1")
        out.append((text, c))
    return out


def _records(ctx, r):
    h = ctx.fq_reads_to_host(r)
    ro, io = h["read_offsets"].astype(np.int64), h["id_offsets"].astype(np.int64)
    b, i = h["bases"].tobytes(), h["ids"].tobytes()
    return [(i[io[k]:io[k + 1]], b[ro[k]:ro[k + 1]]) for k in range(r.n_reads)]


def _same_records(got, outcome):
    if "records" in outcome:
        return [[a.decode("latin-1"), b.decode("latin-1")] for a, b in got] == outcome["records"]
    return (len(got), recorder.records_digest(got)) == (outcome["n_records"], outcome["records_sha256"])


@pytest.fixture(scope="module")
def fq_ctx(gpu):
    from close_kmers_amd.fastq_to_protein import placeholder_image
    with placeholder_image(gpu, 0) as img, gpu.Context(img) as ctx:
        yield ctx


def test_fq_parse_lenient_against_fastq_parser(fq_ctx):
    """Flags 0: on past errors, records ended by their quality line; the first
    error is reported once a record past it is consumed."""
    errors = 0
    for text, c in _fastq_cases():
        if not text:
            continue
        want = c["lenient"]
        r = fq_ctx.fq_parse(text, 0)
        assert _same_records(_records(fq_ctx, r), want), text[-80:]
        if want["error"] is None:
            assert r.error == 0, text[-80:]
        else:
            if want["error"][1] <= r.newlines:
                assert r.error, text[-80:]
            if r.error:
                assert [r.error_text(), 1 + r.error_newlines] == want["error"][:2], text[-80:]
                errors += 1
    # every placed piece but "truncated" has its error in front of well-formed records
    assert errors >= sum(p != "truncated" for p, _ in ref_corpora.placed_fastq_cases())


def test_fq_parse_strict_against_fastq_parser(fq_ctx):
    """STRICT | FINISHED: the parse ends at the first error and hands over the
    record in progress; without an error parse_complete's record counts only
    if it has an id (the tools drop records without one)."""
    errors = 0
    for text, c in _fastq_cases():
        want = dict(c["strict"])
        r = fq_ctx.fq_parse(text, STRICT_FINISHED)
        got = _records(fq_ctx, r)
        if want["error"] is None:
            assert r.error == 0, text[-80:]
            if "records" in want:
                if not want["records"][-1][0]:
                    want["records"] = want["records"][:-1]
                assert _same_records(got, want), text[-80:]
            elif want["last"] is not None and not want["last"][0]:
                assert (len(got), recorder.records_digest(got)) == (want["n_records"] - 1, want["head_sha256"])
            else:
                assert _same_records(got, want), text[-80:]
        else:
            assert _same_records(got, want), text[-80:]
            assert [r.error_text(), 1 + r.error_newlines, got[-1][0].decode("latin-1")] == want["error"], text[-80:]
            errors += 1
    assert errors > 100


def test_validate_fastq_error_line_against_fastq_parser(fq_ctx):
    from close_kmers_amd import validate_fastq
    checked = 0
    for text, c in _fastq_cases():
        want = c["strict"]
        if not text or "records" not in want:
            continue
        lengths, error = validate_fastq.validate(fq_ctx, [text])
        assert (None if error is None else list(error)) == want["error"], text[-80:]
        assert [int(x) for x in lengths] == [len(s) for rid, s in want["records"] if rid], text[-80:]
        checked += 1
    for piece, at in ref_corpora.placed_fastq_cases()[::3]:
        text = ref_corpora.placed_fastq(piece, at)
        want = next(c for t, c in _fastq_cases() if c.get("placed") == [piece, at])["strict"]
        _, error = validate_fastq.validate(fq_ctx, [text[:4096], text[4096:]] if len(text) > 4096 else [text])
        assert (None if error is None else list(error)) == want["error"], (piece, at)
    assert checked > 100
