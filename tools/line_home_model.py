#!/usr/bin/env python3
"""Occupancy model of the line index under its two homes (CPU only, numpy).

The line index (kgx_image_set_line_index) stores every key in 64-B lines of 4
buckets by linear probing from the start of the key's home line; a probe costs
one random line request per line its chain touches.  This model builds the
index at the benchmark's ratios and counts those lines under

    mod        home = key mod n_lines
    minimizer  home = hash of whichever of the key's two 7-mers hashes lower
               (csrc/kgx_line_home.h), so neighbouring windows of a sequence
               share their home line one time in three

for stored keys, for absent keys, and for a query batch shaped like the
benchmark's (half the sequences planted copies of source proteins with 10%
substitutions, half uniform), where two neighbouring windows homed on one line
ask for it once when one wave instruction serves both (15 pairs in 16).

The benchmark's image has 20^7 = 1.28e9 7-mers, 1.0e9 keys (a quarter of them
consecutive windows of source proteins, as synth.py plants them) and 1.78e9
lines: 0.78 keys and 1.39 lines per 7-mer.  The model keeps those two ratios
over a smaller alphabet (default 10 letters: 1e7 7-mers) so that the table
fits in memory; sharing and lumpiness depend on the ratios, not on the size.

    python tools/line_home_model.py [--alphabet 10] [--seed 1] [--json]
"""
import argparse
import json

import numpy as np

M32 = np.uint64(0xFFFFFFFF)


def mix32(x):
    """kgx_line_home.h mix32 over uint64 arrays holding 32-bit values"""
    x = (x + np.uint64(0x9E3779B9)) & M32
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7FEB352D)) & M32
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846CA68B)) & M32
    x ^= x >> np.uint64(16)
    return x


def homes(keys, n_lines, mode, alpha):
    """line_home with the alphabet's 7-mers: A = key / alpha, B = key mod alpha^7"""
    keys = keys.astype(np.uint64)
    if mode == "mod":
        return (keys % np.uint64(n_lines)).astype(np.int64)
    a, b = keys // np.uint64(alpha), keys % np.uint64(alpha ** 7)
    ha, hb = mix32(a), mix32(b)
    m = np.where(ha <= hb, a, b)
    hm = np.minimum(ha, hb)
    x = (mix32(m ^ np.uint64(0x85EBCA6B)) << np.uint64(3)) | (hm & np.uint64(7))
    return (x % np.uint64(n_lines)).astype(np.int64)


def windows(codes, alpha):
    """8-mer keys of every window of each row of codes"""
    n = codes.shape[1] - 7
    k = np.zeros((codes.shape[0], n), np.uint64)
    for j in range(8):
        k = k * np.uint64(alpha) + codes[:, j:j + n].astype(np.uint64)
    return k


def build(home, n_lines):
    """Linear-probe insertion, 4 buckets a line, from the start of the home
    line; returns each key's bucket and the occupancy.  Keys are placed in
    rounds: of the keys that want one bucket the first keeps it (as one of the
    racing CAS inserts does), the others move on."""
    nb = 4 * n_lines
    occ = np.zeros(nb, bool)
    at = np.full(len(home), -1, np.int64)
    todo = np.arange(len(home))
    x = home * 4
    while len(todo):
        free = ~occ[x]
        cand, cx = todo[free], x[free]
        ux, first = np.unique(cx, return_index=True)
        occ[ux] = True
        at[cand[first]] = ux
        placed = np.zeros(len(todo), bool)
        placed[np.nonzero(free)[0][first]] = True
        todo, x = todo[~placed], (x[~placed] + 1) % nb
    return at, occ


def full_run(occ, n_lines):
    """for every line, the number of consecutive full lines starting there (wrapping)"""
    full = occ.reshape(n_lines, 4).all(axis=1)
    f2 = np.concatenate([full, full])  # one wrap
    idx = np.arange(2 * n_lines)
    # the next line at or after i that is not full, by a reverse running minimum
    nxt = np.minimum.accumulate(np.where(~f2, idx, 2 * n_lines)[::-1])[::-1]
    return np.minimum(nxt - idx, n_lines)[:n_lines]


def model(alpha, seed):
    rng = np.random.default_rng(seed)
    n7 = alpha ** 7
    n_keys = int(0.78125 * n7)    # 1.0e9 / 1.28e9
    n_lines = int(1.3889 * n7) | 1  # 1.778e9 / 1.28e9 (36 keys per 64 lines), odd
    n_src = (n_keys // 4) // 292
    src = rng.integers(0, alpha, (n_src, 300), dtype=np.int8)
    planted = windows(src, alpha).ravel()
    rand = rng.integers(0, alpha ** 8, n_keys, dtype=np.uint64)
    keys = np.concatenate([planted, rand])
    _, first = np.unique(keys, return_index=True)
    keys = keys[np.sort(first)][:n_keys]  # distinct, the planted ones first
    # queries: half planted with 10% substitutions, half uniform
    n_q = 4000
    q_src = src[rng.integers(0, n_src, n_q // 2)]
    sub = rng.random(q_src.shape) < 0.1
    q_pl = np.where(sub, rng.integers(0, alpha, q_src.shape, dtype=np.int8), q_src)
    q_un = rng.integers(0, alpha, (n_q // 2, 300), dtype=np.int8)
    qk = windows(np.concatenate([q_pl, q_un]), alpha)  # rows: sequences
    absent = rng.integers(0, alpha ** 8, 2_000_000, dtype=np.uint64)
    skeys = np.sort(keys)
    absent = absent[skeys[np.minimum(np.searchsorted(skeys, absent), len(skeys) - 1)] != absent]

    out = {"alphabet": alpha, "seven_mers": n7, "keys": len(keys), "lines": n_lines,
           "keys_per_7mer": len(keys) / n7, "lines_per_7mer": n_lines / n7, "homes": {}}
    for mode in ("mod", "minimizer"):
        h = homes(keys, n_lines, mode, alpha)
        at, occ = build(h, n_lines)
        lines_present = (at // 4 - h) % n_lines + 1
        run = full_run(occ, n_lines)
        lines_absent = run[homes(absent, n_lines, mode, alpha)] + 1
        # the query batch: lines per window, and what neighbours share
        qh = homes(qk.ravel(), n_lines, mode, alpha).reshape(qk.shape)
        pos = np.searchsorted(skeys, qk.ravel())
        present = (skeys[np.minimum(pos, len(skeys) - 1)] == qk.ravel()).reshape(qk.shape)
        order = np.argsort(keys)
        q_lines = np.where(present,
                           lines_present[order[np.minimum(pos, len(skeys) - 1)]].reshape(qk.shape),
                           run[qh] + 1)
        same = qh[:, 1:] == qh[:, :-1]
        # no more than two in a row share: a pair counts when the window before it did not pair
        pair = same.copy()
        for j in range(1, pair.shape[1]):
            pair[:, j] &= ~pair[:, j - 1]
        saved = np.where(pair, np.minimum(q_lines[:, 1:], q_lines[:, :-1]), 0)
        requests = (q_lines.sum() - 15.0 / 16.0 * saved.sum()) / q_lines.size
        out["homes"][mode] = {
            "lines_per_present_key": float(lines_present.mean()),
            "present_keys_past_first_line": float((lines_present > 1).mean()),
            "longest_chain_lines": int(lines_present.max()),
            "full_lines": float((run > 0).mean()),
            "lines_per_absent_key": float(lines_absent.mean()),
            "query_lines_per_window": float(q_lines.mean()),
            "query_windows_past_first_line": float((q_lines > 1).mean()),
            "neighbours_sharing_home": float(same.mean()),
            "neighbours_sharing_home_planted": float(same[:n_q // 2].mean()),
            "neighbours_sharing_home_uniform": float(same[n_q // 2:].mean()),
            "query_requests_per_window": float(requests),
        }
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alphabet", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    r = model(a.alphabet, a.seed)
    if a.json:
        print(json.dumps(r))
        return
    print(f"alphabet {r['alphabet']}: {r['seven_mers']:,} 7-mers, {r['keys']:,} keys ({r['keys_per_7mer']:.2f} per 7-mer), "
          f"{r['lines']:,} lines ({r['lines_per_7mer']:.2f} per 7-mer)")
    for mode, m in r["homes"].items():
        print(f"{mode}:")
        for k, v in m.items():
            print(f"  {k:36s} {v:.4f}" if isinstance(v, float) else f"  {k:36s} {v}")


if __name__ == "__main__":
    main()
