"""Record the reference's own answers under tests/golden/reference/.

    python tests/golden/make_reference_runs.py

Needs oracle/_ref/libref.so (make -C oracle ref): the reference's KmerGuts,
KmerImage and FastqParser, compiled from its sources.  The device tests have no
reference tree beside them, so they compare the kernels with these files.

  designed.npz      the designed table's entries in insertion order, the
                    sequences, the parameter sets, and per parameter set the
                    reference's hits, calls, OTU tallies and best calls
  designed.json     sequence names, function names, best-call function text
  random_table.npz  the random corpus's table entries (narrow integer types)
  random.npz/.json  the first RANDOM_SLICE random sequences, as designed.*
  image.npz         the kmer.table.mem_map that the reference's insert_kmer /
                    save_kmer_hash_table write for the designed entries
  routing.json      sequences of 2,056 / 2,057 / 40,006 / 40,007 residues
                    (ref_corpora.routing_seqs: the lengths at which the device
                    changes scorer) over the designed table, as digests
  cap.json          the saturation case as a recipe (golden/cap's inputs), the
                    reference's call records, hit count and a digest of its hits
  fastq.json        FASTQ texts and FastqParser's records and first error:
                    "strict" (stop at the first error, then parse_complete),
                    "lenient" (go on past errors, no parse_complete) and
                    "handler" (go on, then parse_complete); longer texts that
                    put a malformed byte on a lane or tile edge as a recipe
                    (ref_corpora.placed_fastq) with a digest of the records

Data only.  build_all(engine) returns {file name: bytes}; the same function
runs over the CPU oracle and the restatements (engine="oracle"), and a test
requires both engines to give the committed bytes.
"""
from __future__ import annotations

import hashlib
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import oracle  # noqa: E402
import f2p_restate  # noqa: E402
import ref_corpora  # noqa: E402
from close_kmers_amd import image_files  # noqa: E402
from helpers import pack  # noqa: E402

OUT = os.path.join(HERE, "reference")
BEST_REC = np.dtype([("function_index", "<i4"), ("score", "<f4"), ("weighted_score", "<f4"),
                     ("score_offset", "<f4"), ("offset_set", "<i4")])
TABLE_REC = np.dtype([("key", "<u4"), ("fI", "i1"), ("oI", "i1"), ("avg", "u1"), ("wt", "<f4")])


def npz_bytes(arrays: dict) -> bytes:
    """An .npz whose bytes depend on the arrays alone (stored, fixed dates)."""
    buf = io.BytesIO()
    with zipfile.ZipFile(buf, "w", zipfile.ZIP_STORED) as z:
        for name in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[name]), version=(1, 0))
            zi = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.external_attr = 0o644 << 16
            z.writestr(zi, b.getvalue())
    return buf.getvalue()


def json_bytes(obj) -> bytes:
    return (json.dumps(obj, indent=0, sort_keys=True, ensure_ascii=True) + "\n").encode()


def hits_digest(hits: np.ndarray) -> str:
    h = hashlib.sha256()
    for f in ("which_kmer", "otu_index", "avg_from_end", "function_index", "function_wt", "pos"):
        h.update(np.ascontiguousarray(hits[f]).tobytes())
    return h.hexdigest()


def records_digest(records) -> str:
    h = hashlib.sha256()
    for rid, seq in records:
        h.update(b"R\t" + rid + b"\t" + seq + b"\n")
    return h.hexdigest()


# ---------------------------------------------------------------------------
class OracleEngine:
    """The CPU oracle and the Python restatements."""
    name = "oracle"

    def open(self, table, functions, data_dir=None):
        self.table, self.functions = table, functions

    def close(self):
        pass

    def run(self, seqs, params):
        res, off = pack(seqs)
        r = oracle.process_batch(self.table, res, off, params=params, want=7)
        best = []
        for s in range(len(seqs)):
            best.append(oracle.find_best_call(r.calls[int(r.call_offsets[s]):int(r.call_offsets[s + 1])],
                                              self.functions))
        return r.hit_offsets, r.hits, r.call_offsets, r.calls, r.otu_offsets, r.otus, best

    def build_image(self, num_sigs, entries) -> bytes:
        with tempfile.TemporaryDirectory() as d:
            path = image_files.write_image(d, oracle.build_table(num_sigs, *entries))
            return open(path, "rb").read()

    def fastq(self, text: bytes):
        handler = oracle.fq_frames(text)
        lenient = f2p_restate.parse(text, stop_at_error=False)
        return {"strict": f2p_restate.parse(text, stop_at_error=True), "lenient": lenient,
                "handler": (handler, lenient[1])}


class ReferenceEngine:
    """The reference's own code (oracle/_ref/libref.so)."""
    name = "reference"

    def open(self, table, functions, data_dir=None):
        self.tmp = None
        if data_dir is None:
            self.tmp = tempfile.TemporaryDirectory()
            data_dir = image_files.write_data_dir(self.tmp.name, table, functions, ["otu0"])
        self.kg = oracle.RefKmerGuts(data_dir)

    def close(self):
        self.kg.close()
        if self.tmp:
            self.tmp.cleanup()

    def run(self, seqs, params):
        ho, co, oo = [0], [0], [0]
        hits, calls, otus, best = [], [], [], []
        for s, (_, seq) in enumerate(seqs):
            h, c, o = self.kg.process_aa(seq, params)
            h["seq"] = s
            hits.append(h), calls.append(c), otus.append(o)
            ho.append(ho[-1] + len(h)), co.append(co[-1] + len(c)), oo.append(oo[-1] + len(o))
            best.append(self.kg.find_best_call(c))
        u = np.uint64
        return (np.array(ho, u), np.concatenate(hits) if hits else np.zeros(0, oracle.HIT_DTYPE),
                np.array(co, u), np.concatenate(calls) if calls else np.zeros(0, oracle.CALL_DTYPE),
                np.array(oo, u), np.concatenate(otus) if otus else np.zeros((0, 2), np.int32), best)

    def build_image(self, num_sigs, entries) -> bytes:
        with tempfile.TemporaryDirectory() as d:
            path = os.path.join(d, "image")
            oracle.ref_build_image(num_sigs, *entries, path)
            return open(path, "rb").read()

    def fastq(self, text: bytes):
        return {"strict": oracle.ref_fastq_parse(text, True, True),
                "lenient": oracle.ref_fastq_parse(text, False, False),
                "handler": oracle.ref_fastq_parse(text, False, True)}


def engine_of(name: str):
    return ReferenceEngine() if name == "reference" else OracleEngine()


# ---------------------------------------------------------------------------
def best_rows(best) -> np.ndarray:
    out = np.zeros(len(best), BEST_REC)
    for i, (fi, _, score, wscore, off) in enumerate(best):
        out[i] = (fi, score, wscore, 0.0 if off is None else off, off is not None)
    return out


def corpus_files(eng, stem, entries, num_sigs, seqs, param_sets, table_in_npz=True):
    """Run every parameter set; the hits must not depend on it."""
    table = oracle.build_table(num_sigs, *entries)
    eng.open(table, ref_corpora.FUNCTIONS)
    res, off = pack(seqs)
    arrays = {"num_sigs": np.array([num_sigs], np.uint64), "residues": res, "offsets": off,
              "params": np.array(param_sets, np.int32)}
    if table_in_npz:
        for n, a in zip(("keys", "fI", "oI", "avg", "wt"), entries):
            arrays["table_" + n] = a
    names = {"sequences": [n for n, _ in seqs], "functions": ref_corpora.FUNCTIONS, "best_function": []}
    first = None
    for i, p in enumerate(param_sets):
        ho, hits, co, calls, oo, otus, best = eng.run(seqs, p)
        hits = hits.copy()
        hits["reserved"] = 0
        if first is None:
            first = (ho, hits)
            arrays["hit_offsets"], arrays["hits"] = ho, hits
        else:
            assert np.array_equal(first[0], ho) and first[1].tobytes() == hits.tobytes()
        arrays[f"call_offsets_{i}"], arrays[f"calls_{i}"] = co, calls
        arrays[f"otu_offsets_{i}"], arrays[f"otus_{i}"] = oo, otus.astype(np.int32).reshape(-1, 2)
        arrays[f"best_{i}"] = best_rows(best)
        names["best_function"].append([b[1] for b in best])
    eng.close()
    return {stem + ".npz": npz_bytes(arrays), stem + ".json": json_bytes(names)}


def random_table_file():
    (keys, fI, oI, avg, wt), num_sigs = ref_corpora.random_table()
    t = np.zeros(len(keys), TABLE_REC)
    t["key"], t["fI"], t["oI"], t["avg"], t["wt"] = keys, fI, oI, avg, wt
    assert np.array_equal(t["key"].astype(np.uint64), keys) and np.array_equal(t["avg"].astype(np.uint16), avg)
    return npz_bytes({"entries": t, "num_sigs": np.array([num_sigs], np.uint64)})


def load_random_table(path):
    z = np.load(path)
    t = z["entries"]
    return (t["key"].astype(np.uint64), t["fI"].astype(np.int32), t["oI"].astype(np.int32),
            t["avg"].astype(np.uint16), t["wt"].astype(np.float32)), int(z["num_sigs"][0])


def cap_file(eng):
    d = os.path.join(HERE, "cap")
    table = image_files.read_image(os.path.join(d, "data"))
    functions = [ln.split("\t", 1)[1].rstrip("\n") for ln in open(os.path.join(d, "data", "function.index"))]
    recs = oracle.fasta_parse(open(os.path.join(d, "input.fasta"), "rb").read()).splitlines()
    seqs = [(r.split("\t")[0], r.split("\t")[1].encode()) for r in recs]
    eng.open(table, functions, data_dir=os.path.join(d, "data"))
    out = {"inputs": "tests/golden/cap: data/ and input.fasta", "runs": []}
    for p in [(5, 200, 0, 0), (2, 200, 1, 0)]:
        ho, hits, co, calls, oo, otus, best = eng.run(seqs, p)
        out["runs"].append({
            "params": list(p), "n_hits": int(ho[-1]), "hits_sha256": hits_digest(hits),
            "calls": [[int(c["start"]), int(c["end"]), int(c["count"]), int(c["function_index"]),
                       int(np.float32(c["weighted_hits"]).view(np.uint32))] for c in calls],
            "otus": [[int(a), int(b)] for a, b in otus],
            "best": [[b[0], b[1], float(b[2]), int(np.float32(b[3]).view(np.uint32)),
                      None if b[4] is None else float(b[4])] for b in best]})
    eng.close()
    return json_bytes(out)


def rows_digest(a: np.ndarray, fields) -> str:
    h = hashlib.sha256()
    for f in fields:
        h.update(np.ascontiguousarray(a[f]).tobytes())
    return h.hexdigest()


CALL_FIELDS = ("start", "end", "count", "function_index", "weighted_hits")


def routing_file(eng):
    """Sequences at the scorer boundaries, as digests: they are ref_corpora.routing_seqs()."""
    entries, num_sigs, _ = ref_corpora.designed()
    seqs = ref_corpora.routing_seqs()
    eng.open(oracle.build_table(num_sigs, *entries), ref_corpora.FUNCTIONS)
    out = {"sequences": [{"name": n, "length": len(s), "sha256": hashlib.sha256(s).hexdigest()} for n, s in seqs],
           "runs": []}
    for p in ref_corpora.ROUTING_PARAMS:
        ho, hits, co, calls, oo, otus, best = eng.run(seqs, p)
        per_seq = []
        for s in range(len(seqs)):
            h = hits[int(ho[s]):int(ho[s + 1])]
            c = calls[int(co[s]):int(co[s + 1])]
            b = best[s]
            per_seq.append({"n_hits": len(h), "hits_sha256": hits_digest(h), "n_calls": len(c),
                            "calls_sha256": rows_digest(c, CALL_FIELDS),
                            "otus": [[int(a), int(n)] for a, n in otus[int(oo[s]):int(oo[s + 1])]],
                            "best": [b[0], b[1], float(b[2]), int(np.float32(b[3]).view(np.uint32)),
                                     None if b[4] is None else float(b[4])]})
        out["runs"].append({"params": list(p), "sequences": per_seq})
    eng.close()
    return json_bytes(out)


def _outcome(res, digest_only):
    records, error = res
    o = {"error": None if error is None else [error[0], error[1], error[2].decode("latin-1")]}
    if digest_only:
        o["n_records"], o["records_sha256"] = len(records), records_digest(records)
        o["head_sha256"] = records_digest(records[:-1])  # without the last record
        o["last"] = [x.decode("latin-1") for x in records[-1]] if records else None
    else:
        o["records"] = [[r.decode("latin-1"), s.decode("latin-1")] for r, s in records]
    return o


def fastq_file(eng):
    cases = []
    for text in ref_corpora.fastq_texts():
        res = eng.fastq(text)
        cases.append({"text": text.decode("latin-1"), **{k: _outcome(v, False) for k, v in res.items()}})
    for piece, at in ref_corpora.placed_fastq_cases():
        text = ref_corpora.placed_fastq(piece, at)
        res = eng.fastq(text)
        cases.append({"placed": [piece, at], "text_sha256": hashlib.sha256(text).hexdigest(),
                      **{k: _outcome(v, True) for k, v in res.items()}})
    return json_bytes(cases)


def build_all(engine: str) -> dict:
    eng = engine_of(engine)
    files = {}
    entries, num_sigs, seqs = ref_corpora.designed()
    files.update(corpus_files(eng, "designed", entries, num_sigs, seqs, ref_corpora.DESIGNED_PARAMS))
    files["image.npz"] = npz_bytes({"image": np.frombuffer(eng.build_image(num_sigs, entries), np.uint8)})
    rentries, rnum = ref_corpora.random_table()
    files["random_table.npz"] = random_table_file()
    files.update(corpus_files(eng, "random", rentries, rnum, ref_corpora.random_seqs()[:ref_corpora.RANDOM_SLICE],
                              ref_corpora.RANDOM_PARAMS, table_in_npz=False))
    files["cap.json"] = cap_file(eng)
    files["routing.json"] = routing_file(eng)
    files["fastq.json"] = fastq_file(eng)
    return files


def main() -> None:
    if oracle.ref_lib() is None:
        sys.exit("oracle/_ref/libref.so is missing: make -C oracle ref (needs the reference's sources)")
    os.makedirs(OUT, exist_ok=True)
    total = 0
    for name, data in sorted(build_all("reference").items()):
        open(os.path.join(OUT, name), "wb").write(data)
        total += len(data)
        print(f"{name}: {len(data)} bytes")
    print(f"total {total} bytes")


if __name__ == "__main__":
    main()
