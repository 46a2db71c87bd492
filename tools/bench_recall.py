"""Recall benchmark: labelled proteins back through the image built from them.

    python tools/bench_recall.py [--n-prot 100000] [--fam-size 10] [--reps 3] [--piece-residues N]
        [--out profiles/recall_bench.json]

Corpus: tools/bench_signatures.py's (families of fam_size proteins of 300 aa,
10% substitutions, labelled with their family).  The image is selected and
built from it on the device, then two ways to the same tallies are timed from
host buffers, wall clock, --reps runs each after one warm-up:

  recall      one kgx_recall_run (abi.Recall): comparison and tallies on the
              device; its four stage times are those of the best run;
  host tally  what the library offered before: Context.process_batch with
              want = CALLS | BEST over the same pieces, the best calls
              concatenated and the cells, per-function counts, changed list and
              confusion pairs made in numpy.

The results of the two must be equal.  Prints one JSON line and writes it to
--out.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

PIECE_DEFAULT = 1 << 25  # kgx_recall_run's piece_residues 0


def pieces(off: np.ndarray, piece: int) -> list[tuple[int, int]]:
    """kgx_recall_run's pieces: closed before the sequence that would take one above `piece` residues."""
    out, n, s0 = [], len(off) - 1, 0
    while s0 < n:
        s1 = int(np.searchsorted(off, off[s0] + np.uint64(piece), side="right")) - 1
        s1 = min(n, max(s1, s0 + 1))
        out.append((s0, s1))
        s0 = s1
    return out


def host_tally(ctx, abi, res, off, lab, n_fn, cuts, params):
    best = []
    for s0, s1 in cuts:
        r = ctx.process_batch(res[int(off[s0]):int(off[s1])], off[s0:s1 + 1] - off[s0], params,
                              want=abi.WANT_CALLS | abi.WANT_BEST, copy=False)
        best.append(r.best.copy())
    best = np.concatenate(best)
    kind, fi0 = best["kind"], best["fi0"]
    cc = np.where(kind == 1, np.where(fi0 == lab, 0, 1), np.where(kind == 2, 2, 3))
    lc = np.where(lab >= 0, 0, np.where(lab == -1, 1, 2))
    cell = np.bincount(lc * 4 + cc, minlength=12).reshape(3, 4)
    fn = np.stack([np.bincount(lab[lab >= 0], minlength=n_fn), np.bincount(lab[cc == 0], minlength=n_fn),
                   np.bincount(fi0[kind == 1], minlength=n_fn)], axis=1)
    changed = np.nonzero(((cc == 3) & (lab != -2)) | (cc == 1) | (cc == 2))[0]
    mis = (lc == 0) & (cc == 1)
    keys, counts = np.unique(lab[mis].astype(np.int64) << 32 | fi0[mis].astype(np.int64), return_counts=True)
    return best, cell, fn, changed, keys, counts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-prot", type=int, default=100000)
    ap.add_argument("--fam-size", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--piece-residues", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "recall_bench.json"))
    args = ap.parse_args()

    from bench_signatures import labelled_corpus
    from close_kmers_amd import abi
    res, off, lab, n_fn = labelled_corpus(args.n_prot, args.fam_size)
    params = abi.parse_params({"min_hits": 5, "max_gap": 200})
    cuts = pieces(off, args.piece_residues or PIECE_DEFAULT)
    with abi.Signatures(res, off, lab, n_fn) as sig:
        img, stored = sig.image()
    with img, abi.Context(img) as ctx:
        t_recall, t_host, stages, keep = [], [], None, None
        for rep in range(args.reps + 1):  # the first run of each warms the runtime and the buffers up
            t0 = time.perf_counter()
            r = abi.Recall(ctx, res, off, lab, n_fn, params, args.piece_residues)
            dt = time.perf_counter() - t0
            if rep:
                if not t_recall or dt < min(t_recall):
                    stages = r.stage_ms()
                t_recall.append(dt)
            if rep == args.reps:
                keep = (r.best(), r.stats(), r.functions(), r.changed(), r.confusions())
            r.close()
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            h = host_tally(ctx, abi, res, off, lab, n_fn, cuts, params)
            dt = time.perf_counter() - t0
            if rep:
                t_host.append(dt)
    best, st, fn, changed, conf = keep
    hb, hcell, hfn, hchanged, hkeys, hcounts = h
    equal = (best.tobytes() == hb.tobytes() and np.array_equal(st["cell"], hcell) and
             np.array_equal(np.stack([fn["labelled"], fn["correct"], fn["called"]], axis=1), hfn) and
             np.array_equal(changed, hchanged) and
             np.array_equal(conf["label"].astype(np.int64) << 32 | conf["called"].astype(np.int64), hkeys) and
             np.array_equal(conf["count"], hcounts))
    out = {"metric": "recall_proteins_per_s", "value": len(lab) / min(t_recall), "unit": "proteins/s",
           "n_prot": len(lab), "n_functions": n_fn, "residues": int(res.size), "n_stored": stored,
           "n_pieces": st["n_pieces"], "recall_ms": [round(t * 1e3, 3) for t in sorted(t_recall)],
           "stage_ms": {k: round(v, 3) for k, v in stages.items()},
           "host_tally_ms": [round(t * 1e3, 3) for t in sorted(t_host)],
           "host_tally_spread_ms": round((max(t_host) - min(t_host)) * 1e3, 3),
           "gain_ms": round((min(t_host) - min(t_recall)) * 1e3, 3),
           "host_tally_proteins_per_s": len(lab) / min(t_host),
           "cell": st["cell"].tolist(), "n_changed": st["n_changed"], "n_confusions": st["n_confusions"],
           "results_equal": bool(equal)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
