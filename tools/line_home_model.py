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
    twins      the minimizer index with every key stored a second time from
               the home of its other 7-mer (twin records, KGX_LINE_TWINS); a
               window with an even index in the batch is looked up from the
               home of its last seven residues and the odd window after it
               from the home of its first seven, the same 7-mer, so the two
               always share their line and one instruction serves both
    pairs      twins with a 7-mer's two roles homed on the halves of a 128-byte
               block (KGX_LINE_PAIRS): keys that end in the 7-mer on line 2k,
               keys that begin with it on line 2k + 1 of the n_lines >> 1
               blocks.  The even window starts at line 2k and the odd one after
               it at 2k + 1, one aligned 128-byte request for the two; a line
               collects one role's keys only.  Its rows count a block asked for
               by a pair once (after the first lines the two chains are on
               different blocks) and report the 64-byte lines fetched as well

for stored keys, for absent keys, and for a query batch shaped like the
benchmark's (half the sequences planted copies of source proteins with 10%
substitutions, half uniform), where two neighbouring windows homed on one line
ask for it once when one wave instruction serves both (15 pairs in 16).

Under each home it then adds overflow marks (csrc/kgx_line_home.h line_mark):
a full line remembers, in 1 or in 16 bits, which keys were pushed on past it,
and an absent key's chain ends at the first full line whose bit for it is
clear instead of at the first line with an empty bucket.  Printed for no
marks, 1 bit and 16 bits: lines per window, windows past their first line,
lines per absent key, and requests per window under two models of merging
(within one wave instruction, as above; within a 128-window tile, where every
line a tile's windows touch is asked for once), and the fraction of lines that
are full and were ever passed, the only ones a mark can sit on.

For the twins and pairs rows it also counts the line probe's rounds (round_stats): the
share of 64-window slices whose longest chain has 2, 3, 4 or more lines, the
chains a 128-window tile has open after every window's first line (mean, and
how often more than the 16 that one load instruction serves), and the rounds
and dependent round trips per tile when each slice walks its own chains
against one first round per slice and the tile's open chains walked together
afterwards (KGX_PROBE_DEFER).

The benchmark's image has 20^7 = 1.28e9 7-mers, 1.0e9 keys (a quarter of them
consecutive windows of source proteins, as synth.py plants them) and 1.78e9
lines: 0.78 keys and 1.39 lines per 7-mer.  The model keeps those two ratios
over a smaller alphabet (default 10 letters: 1e7 7-mers) so that the table
fits in memory; sharing and lumpiness depend on the ratios, not on the size.

    python tools/line_home_model.py [--alphabet 10] [--seed 1] [--load 36] [--json]
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


def seven_mer_homes(keys, n_lines, alpha):
    """the homes of a key's two 7-mers (seven_mer_home) and whether the first
    one is the minimizer"""
    keys = keys.astype(np.uint64)
    a, b = keys // np.uint64(alpha), keys % np.uint64(alpha ** 7)
    ha, hb = mix32(a), mix32(b)
    xa = (mix32(a ^ np.uint64(0x85EBCA6B)) << np.uint64(3)) | (ha & np.uint64(7))
    xb = (mix32(b ^ np.uint64(0x85EBCA6B)) << np.uint64(3)) | (hb & np.uint64(7))
    return (xa % np.uint64(n_lines)).astype(np.int64), (xb % np.uint64(n_lines)).astype(np.int64), ha <= hb


def line_mark(keys):
    """kgx_line_home.h line_mark over uint64 arrays"""
    keys = keys.astype(np.uint64)
    x = (((keys & M32) ^ np.uint64(0x27D4EB2F)) + (keys >> np.uint64(32)) * np.uint64(0xC2B2AE35)) & M32
    return (mix32(x) >> np.uint64(28)).astype(np.int64)


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


def set_marks(keys, home, at, n_lines, bits):
    """the marks of a built index: every key placed past its home line sets
    bit line_mark(key) (bit 0 when bits == 1) on each line from its home to
    the one before its own"""
    return set_marks_walk(keys, home, (at // 4 - home) % n_lines, n_lines, bits)


def set_marks_walk(keys, home, walk, n_lines, bits):
    """the same for keys that pass `walk` lines from `home`"""
    marks = np.zeros(n_lines, np.uint32)
    g = line_mark(keys) if bits == 16 else np.zeros(len(keys), np.int64)
    todo = np.nonzero(walk > 0)[0]
    d = 0
    while len(todo):
        np.bitwise_or.at(marks, (home[todo] + d) % n_lines, (np.uint32(1) << g[todo].astype(np.uint32)))
        d += 1
        todo = todo[walk[todo] > d]
    return marks


def marked_chain(keys, home, full, marks, n_lines, bits):
    """lines an absent key's chain touches: on from a full line only while the
    line's mark for the key is set"""
    g = line_mark(keys) if bits == 16 else np.zeros(len(keys), np.int64)
    lines = np.ones(len(keys), np.int64)
    todo = np.arange(len(keys))
    line = home.copy()
    while len(todo):
        go = full[line[todo]] & ((marks[line[todo]] >> g[todo].astype(np.uint32)) & np.uint32(1)).astype(bool)
        todo = todo[go]
        line[todo] = (line[todo] + 1) % n_lines
        lines[todo] += 1
    return lines


def tile_requests(qh, q_lines, n_lines, tile=128):
    """requests per window when every line the windows of one 128-window tile
    touch is asked for once (the batch's windows in sequence order)"""
    h, n = qh.ravel(), q_lines.ravel()
    t = np.arange(len(h)) // tile
    rep = np.repeat(np.arange(len(h)), n)
    step = np.arange(len(rep)) - np.repeat(np.cumsum(n) - n, n)
    touched = t[rep] * np.int64(n_lines) + (h[rep] + step) % n_lines
    return len(np.unique(touched)) / len(h)


def round_stats(ql, slice_w=64, tile=128, quads=16):
    """The line probe's rounds over the batch's windows in order (ql: lines per
    window).  A 64-window slice that walks its own chains runs as many rounds
    as its longest chain has lines.  The deferred form (KGX_PROBE_DEFER) runs
    one round per slice and then the tile's open chains, in window order, 16
    to a load instruction: a pass of 16 runs as many one-instruction rounds
    as its longest chain has lines past the first."""
    n = ql.ravel()
    n = n[:len(n) // tile * tile]
    per_slice = n.reshape(-1, slice_w).max(axis=1)
    t = n.reshape(-1, tile)
    opened = (t > 1).sum(axis=1)
    deferred = np.zeros(len(t), np.int64)  # one-instruction rounds after the slices' first rounds
    passes = np.zeros(len(t), np.int64)
    for i, row in enumerate(t):
        rest = row[row > 1] - 1
        for p in range(0, len(rest), quads):
            deferred[i] += rest[p:p + quads].max()
            passes[i] += 1
    slices = tile // slice_w
    return {
        "slices_with_2_rounds_or_more": float((per_slice >= 2).mean()),
        "slices_with_3_rounds_or_more": float((per_slice >= 3).mean()),
        "slices_with_4_rounds_or_more": float((per_slice >= 4).mean()),
        "slice_rounds_per_tile": float(per_slice.reshape(-1, slices).sum(axis=1).mean()),
        "open_chains_per_tile_after_round_0": float(opened.mean()),
        "tiles_with_more_than_16_open_chains": float((opened > quads).mean()),
        "deferred_passes_per_tile": float(passes.mean()),
        "deferred_rounds_per_tile": float(deferred.mean()),
        "dependent_round_trips_per_tile": {"per_slice": float(per_slice.reshape(-1, slices).sum(axis=1).mean()),
                                           "deferred": float(slices + deferred.mean())},
    }


def role_homes(keys, n_lines, alpha, pairs):
    """the homes of a key's first and of its last seven residues and whether
    the first is the minimizer; pairs: lines 2k + 1 and 2k of the 7-mers' blocks"""
    if not pairs:
        return seven_mer_homes(keys, n_lines, alpha)
    a, b, amin = seven_mer_homes(keys, n_lines >> 1, alpha)
    return 2 * a + 1, 2 * b, amin


def twins_model(keys, skeys, order, absent, qk, n_q, n_lines, alpha, pairs=False):
    """the minimizer index with twin records, probed by the even/odd choice;
    the columns of the other two homes.  pairs: the same over the halves of
    128-byte blocks"""
    n = len(keys)
    hA, hB, amin = role_homes(keys, n_lines, alpha, pairs)
    two = hA != hB
    h1, h2 = np.where(amin, hA, hB), np.where(amin, hB, hA)
    at, occ = build(np.concatenate([h1, h2[two]]), n_lines)  # every record goes to its walk's first empty bucket
    line1 = at[:n] // 4
    line2 = line1.copy()
    line2[two] = at[n:] // 4
    # lines passed from a home before the first line that holds the key
    dA = np.minimum((line1 - hA) % n_lines, (line2 - hA) % n_lines)
    dB = np.minimum((line1 - hB) % n_lines, (line2 - hB) % n_lines)
    per_home = np.concatenate([np.where(amin, dA, dB), np.where(amin, dB, dA)[two]]) + 1
    run = full_run(occ, n_lines)
    full = run > 0
    # queries: window g of the batch (sequences laid end to end) starts at
    # the home of its first 7-mer when g is odd, of its last when g is even
    odd = (np.arange(qk.size).reshape(qk.shape) & 1).astype(bool)
    qA, qB, _ = role_homes(qk.ravel(), n_lines, alpha, pairs)
    qh = np.where(odd, qA.reshape(qk.shape), qB.reshape(qk.shape))
    pos = np.minimum(np.searchsorted(skeys, qk.ravel()), len(skeys) - 1)
    present = (skeys[pos] == qk.ravel()).reshape(qk.shape)
    idx = order[pos].reshape(qk.shape)
    ql_present = np.where(odd, dA[idx], dB[idx]) + 1
    aA, aB, _ = role_homes(absent, n_lines, alpha, pairs)
    ah = np.where(np.arange(len(absent)) & 1, aA, aB)
    # neighbours that ask for one line (pairs: for the two halves of one block)
    same = (qh[:, 1:] >> 1 == qh[:, :-1] >> 1) if pairs else (qh[:, 1:] == qh[:, :-1])
    pair = same & ~odd[:, :-1]  # the even window and the one after it: neighbouring quads of one instruction
    keys2, home2, walk2 = np.concatenate([keys, keys]), np.concatenate([hA, hB]), np.concatenate([dA, dB])
    variants = {}
    for bits in (0, 1, 16):
        if bits:
            mk = set_marks_walk(keys2, home2, walk2, n_lines, bits)
            la = marked_chain(absent, ah, full, mk, n_lines, bits)
            ql = np.where(present, ql_present,
                          marked_chain(qk.ravel(), qh.ravel(), full, mk, n_lines, bits).reshape(qk.shape))
        else:
            mk, la, ql = np.zeros(n_lines, np.uint32), run[ah] + 1, np.where(present, ql_present, run[qh] + 1)
        # twins: the two chains of a pair walk the same lines; pairs: they share the first
        # request, the block, and are on different blocks from then on
        sv = np.where(pair, 1 if pairs else np.minimum(ql[:, 1:], ql[:, :-1]), 0)
        variants[str(bits)] = {
            "query_lines_per_window": float(ql.mean()),  # the 64-B lines fetched
            "query_windows_past_first_line": float((ql > 1).mean()),
            "lines_per_absent_key": float(la.mean()),
            "query_lines_per_absent_window": float(ql[~present].mean()),
            "query_lines_per_present_window": float(ql[present].mean()),
            "query_requests_per_window": float((ql.sum() - sv.sum()) / ql.size),
            "pairs_needing_more_than_one_request": float((np.maximum(ql[:, 1:], ql[:, :-1])[pair] > 1).mean()),
            "query_requests_per_window_tile_merge": float(tile_requests(qh, ql, n_lines)),
            "lines_marked": float((mk != 0).mean()),
            "mark_bits_per_marked_line": float(np.array([bin(int(v)).count("1") for v in mk[mk != 0][:100000]]).mean())
            if (mk != 0).any() else 0.0,
            "rounds": round_stats(ql),
        }
        if pairs:
            # the even window's second line is the half its neighbour has just fetched:
            # a request still, but one the caches answer
            reuse = (pair & (ql[:, :-1] > 1)).sum()
            variants[str(bits)]["query_requests_per_window_neighbour_half_from_cache"] = float(
                (ql.sum() - sv.sum() - reuse) / ql.size)
    q0 = variants["0"]
    return {
        "query_windows_absent": float((~present).mean()),
        "marks": variants,
        "twin_records_per_key": float(two.mean()),
        "buckets_filled": float(occ.mean()),
        "lines_per_present_key": float(per_home.mean()),
        "present_keys_past_first_line": float((per_home > 1).mean()),
        "longest_chain_lines": int(per_home.max()),
        "full_lines": float(full.mean()),
        "lines_per_absent_key": float((run[ah] + 1).mean()),
        "query_lines_per_window": q0["query_lines_per_window"],
        "query_windows_past_first_line": q0["query_windows_past_first_line"],
        "neighbours_sharing_home": float(same.mean()),
        "neighbours_sharing_home_planted": float(same[:n_q // 2].mean()),
        "neighbours_sharing_home_uniform": float(same[n_q // 2:].mean()),
        "query_requests_per_window": q0["query_requests_per_window"],
    }


def model(alpha, seed, load=36):
    rng = np.random.default_rng(seed)
    n7 = alpha ** 7
    n_keys = int(0.78125 * n7)    # 1.0e9 / 1.28e9
    n_lines = int(n_keys * 64 / load) | 1  # 36 keys per 64 lines: 1.778e9 / 1.28e9 = 1.39 per 7-mer; odd
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
    out["homes"]["twins"] = None  # printed last
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
        # overflow marks: none, 1 bit and 16 bits per line
        full = run > 0
        order_pos = order[np.minimum(pos, len(skeys) - 1)]
        variants = {}
        for bits in (0, 1, 16):
            if bits:
                mk = set_marks(keys, h, at, n_lines, bits)
                la = marked_chain(absent, homes(absent, n_lines, mode, alpha), full, mk, n_lines, bits)
                ql = np.where(present, lines_present[order_pos].reshape(qk.shape),
                              marked_chain(qk.ravel(), qh.ravel(), full, mk, n_lines, bits).reshape(qk.shape))
            else:
                mk, la, ql = np.zeros(n_lines, np.uint32), lines_absent, q_lines
            sv = np.where(pair, np.minimum(ql[:, 1:], ql[:, :-1]), 0)
            variants[str(bits)] = {
                "query_lines_per_window": float(ql.mean()),
                "query_windows_past_first_line": float((ql > 1).mean()),
                "lines_per_absent_key": float(la.mean()),
                "query_lines_per_absent_window": float(ql[~present].mean()),
                "query_lines_per_present_window": float(ql[present].mean()),
                "query_requests_per_window": float((ql.sum() - 15.0 / 16.0 * sv.sum()) / ql.size),
                "query_requests_per_window_tile_merge": float(tile_requests(qh, ql, n_lines)),
                "lines_marked": float((mk != 0).mean()),
                "mark_bits_per_marked_line": float(np.array([bin(int(v)).count("1") for v in mk[mk != 0][:100000]]).mean())
                if (mk != 0).any() else 0.0,
            }
        out["homes"][mode] = {
            "query_windows_absent": float((~present).mean()),
            "marks": variants,
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
    del out["homes"]["twins"]
    out["homes"]["twins"] = twins_model(keys, skeys, np.argsort(keys), absent, qk, n_q, n_lines, alpha)
    out["homes"]["pairs"] = twins_model(keys, skeys, np.argsort(keys), absent, qk, n_q, n_lines, alpha, pairs=True)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--alphabet", type=int, default=10)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--load", type=int, default=36, help="keys per 64 lines (kgx_image_set_line_index)")
    ap.add_argument("--json", action="store_true")
    a = ap.parse_args()
    r = model(a.alphabet, a.seed, a.load)
    if a.json:
        print(json.dumps(r))
        return
    print(f"alphabet {r['alphabet']}: {r['seven_mers']:,} 7-mers, {r['keys']:,} keys ({r['keys_per_7mer']:.2f} per 7-mer), "
          f"{r['lines']:,} lines ({r['lines_per_7mer']:.2f} per 7-mer)")
    for mode, m in r["homes"].items():
        print(f"{mode}:")
        for k, v in m.items():
            if k != "marks":
                print(f"  {k:36s} {v:.4f}" if isinstance(v, float) else f"  {k:36s} {v}")
        print(f"  overflow marks ({m['marks']['16']['lines_marked']:.2%} of lines are full and were passed, "
              f"{m['full_lines']:.2%} are full):")
        print("    bits  lines/window  past first line  absent-key lines  requests/window (instruction / tile merge)")
        for bits, v in m["marks"].items():
            print(f"    {bits:>4s}  {v['query_lines_per_window']:12.4f}  {v['query_windows_past_first_line']:15.2%}  "
                  f"{v['lines_per_absent_key']:16.4f}  {v['query_requests_per_window']:.4f} / "
                  f"{v['query_requests_per_window_tile_merge']:.4f}")
        if "rounds" in m["marks"]["16"]:
            print("  the line probe's rounds, 16 mark bits (a 128-window tile of two 64-window slices):")
            for k, v in m["marks"]["16"]["rounds"].items():
                print(f"    {k:38s} {v:.4f}" if isinstance(v, float) else f"    {k:38s} {v}")


if __name__ == "__main__":
    main()
