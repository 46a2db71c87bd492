"""unique_prots benchmark: proteins grouped by their signature k-mer sets.

    python tools/bench_unique.py [--n-prot 200000] [--n-keys 2000000] [--reps 3] [--piece-residues N]
        [--digest-bits 64] [--out profiles/unique_bench.json]

Corpus: synth.make_queries' proteins of 300 aa against the synthetic image of
--n-keys keys (every other protein planted from one of the image's source
proteins with 10% substitutions, the others random); 80% of the corpus are
such proteins, 10% exact copies of some of them and 10% copies with 1% of the
residues substituted, all shuffled with a fixed seed.  Two ways to the same
groups are timed from host buffers, wall clock, --reps runs each after one
warm-up:

  unique      one kgx_uniq_run (abi.Unique): sets, grouping and order on the
              device; its five stage times are those of the best run;
  host path   what the library offered before: Context.process_batch with
              want = HITS over the same pieces (32 B per hit to the host), the
              sets by numpy.unique over sequence << 35 | key, the groups in a
              dict keyed by each list's big-endian bytes, whose order is the
              lists' lexicographic order.

The groups of the two must be equal.  Prints one JSON line and writes it to
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

PIECE_DEFAULT = 1 << 25  # kgx_uniq_run's piece_residues 0


def corpus(spec, n_prot: int, seed: int = 0x5EED0061):
    from close_kmers_amd import synth
    rng = np.random.default_rng(seed)
    n_base = max(1, n_prot * 8 // 10)
    n_exact = (n_prot - n_base) // 2
    n_near = n_prot - n_base - n_exact
    res, off = synth.make_queries(spec, n_base)
    base = np.asarray(res, np.uint8).reshape(n_base, -1)
    exact = base[rng.integers(0, n_base, n_exact)]
    near = base[rng.integers(0, n_base, n_near)].copy()
    m = rng.random(near.shape) < 0.01
    near[m] = synth.ALPHA[rng.integers(0, 20, int(m.sum()))]
    rows = np.concatenate([base, exact, near])[rng.permutation(n_prot)]
    return rows.reshape(-1).copy(), np.arange(0, rows.size + 1, rows.shape[1], dtype=np.uint64)


def host_groups(ctx, abi, res, off, cuts):
    """(group_offsets, members) by the host path."""
    n = len(off) - 1
    pairs = []
    for s0, s1 in cuts:
        r = ctx.process_batch(res[int(off[s0]):int(off[s1])], off[s0:s1 + 1] - off[s0], None, want=abi.WANT_HITS,
                              copy=False)
        seq = np.repeat(np.arange(s0, s1, dtype=np.uint64), np.diff(r.hit_offsets).astype(np.int64))
        pairs.append(np.unique(seq << np.uint64(35) | r.hits["which_kmer"].astype(np.uint64)))
    uq = np.concatenate(pairs) if pairs else np.zeros(0, np.uint64)
    keys = (uq & np.uint64((1 << 35) - 1)).astype(">u8")
    start = np.zeros(n + 1, np.int64)
    start[1:] = np.cumsum(np.bincount((uq >> np.uint64(35)).astype(np.int64), minlength=n))
    raw = keys.tobytes()
    groups: dict[bytes, list[int]] = {}
    for i in range(n):
        groups.setdefault(raw[8 * start[i]:8 * start[i + 1]], []).append(i)
    order = sorted(groups)
    goff = np.zeros(len(order) + 1, np.uint64)
    goff[1:] = np.cumsum([len(groups[k]) for k in order])
    members = np.fromiter((i for k in order for i in groups[k]), np.uint32, n)
    return goff, members


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-prot", type=int, default=200000)
    ap.add_argument("--n-keys", type=int, default=2000000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--piece-residues", type=int, default=0)
    ap.add_argument("--digest-bits", type=int, default=64)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "unique_bench.json"))
    args = ap.parse_args()

    from bench_recall import pieces
    from close_kmers_amd import abi, synth
    spec = synth.ImageSpec(args.n_keys)
    res, off = corpus(spec, args.n_prot)
    cuts = pieces(off, args.piece_residues or PIECE_DEFAULT)
    img, stored = abi.Image.synthetic(args.n_keys, spec.num_sigs)
    with img, abi.Context(img) as ctx:
        t_uniq, t_host, stages, keep = [], [], None, None
        for rep in range(args.reps + 1):  # the first run of each warms the runtime and the buffers up
            t0 = time.perf_counter()
            u = abi.Unique(ctx, res, off, args.piece_residues, args.digest_bits)
            dt = time.perf_counter() - t0
            if rep:
                if not t_uniq or dt < min(t_uniq):
                    stages = u.stage_ms()
                t_uniq.append(dt)
            if rep == args.reps:
                keep = (u.groups(), u.stats())
            u.close()
        for rep in range(args.reps + 1):
            t0 = time.perf_counter()
            h = host_groups(ctx, abi, res, off, cuts)
            dt = time.perf_counter() - t0
            if rep:
                t_host.append(dt)
    (goff, members), st = keep
    equal = np.array_equal(goff, h[0]) and np.array_equal(members, h[1])
    n = len(off) - 1
    out = {"metric": "unique_proteins_per_s", "value": n / min(t_uniq), "unit": "proteins/s",
           "n_prot": n, "residues": int(res.size), "n_stored": stored, "digest_bits": args.digest_bits,
           "unique_ms": [round(t * 1e3, 3) for t in sorted(t_uniq)],
           "stage_ms": {k: round(v, 3) for k, v in stages.items()},
           "host_path_ms": [round(t * 1e3, 3) for t in sorted(t_host)],
           "host_path_spread_ms": round((max(t_host) - min(t_host)) * 1e3, 3),
           "gain_ms": round((min(t_host) - min(t_uniq)) * 1e3, 3),
           "host_path_proteins_per_s": n / min(t_host),
           "stats": st, "results_equal": bool(equal)}
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(line + "\n")
    return 0 if equal else 1


if __name__ == "__main__":
    sys.exit(main())
