"""Signature k-mer selection restated on the CPU, the
yardstick of the signature tests: plain dicts, numpy.float32 where the
reference's locals are float and math.log for its double log.

    tuples   every window of 8 bytes out of the 40 letters, in a sequence whose
             function is >= 0: key = the raw bytes, (function, n = len - p, seq)
    set      the tuples of one key; kept iff
             not (float(best_count) < float(double(float(count)) * 0.8))
    record   best function, count, best_count, sorted(n)[count // 2], weight
    weight   float(log((NSiFj + 1.0) / (NSi - NSiFj + 1.0))
                   + log(double((NSF - NFj + KS) / (NFj + KS))))
             with NSF, KS, NSi, NFj, NSiFj float: the first quotient is taken
             in double, the second in float
"""
from __future__ import annotations

import math

import numpy as np

from close_kmers_amd import synth

LETTERS = frozenset(b"ACDEFGHIKLMNPQRSTVWYacdefghiklmnpqrstvwy")
UPPER = b"ACDEFGHIKLMNPQRSTVWY"
F = np.float32

RECORD_DTYPE = np.dtype([("raw_key", "<u8"), ("code", "<u8"), ("function_index", "<i4"), ("n_tuples", "<u4"),
                         ("n_best", "<u4"), ("median_offset", "<i4"), ("function_wt", "<f4")])


def keep(best_count: int, count: int) -> bool:
    thresh = F(float(F(count)) * 0.8)
    return not (F(best_count) < thresh)


def _log(x: float) -> float:
    """C's log over the whole line (math.log raises where C returns)."""
    if x != x or x < 0:
        return math.nan
    if x == 0:
        return -math.inf
    return math.log(x)


def weight(NSF: int, KS: int, NSi: int, NFj: int, NSiFj: int) -> np.float32:
    NSF, KS, NSi, NFj, NSiFj = F(NSF), F(KS), F(NSi), F(NFj), F(NSiFj)
    first = (float(NSiFj) + 1.0) / (float(NSi - NSiFj) + 1.0)
    second = (NSF - NFj + KS) / (NFj + KS)  # float32 throughout
    assert isinstance(second, np.float32)
    return F(_log(first) + _log(float(second)))


def code_of(kmer: bytes) -> int:
    """The base-20 code, or 20^8 + 1 when a byte is not an upper-case residue."""
    v = 0
    for c in kmer:
        i = UPPER.find(bytes([c]))
        if i < 0:
            return synth.EMPTY_KEY
        v = v * 20 + i
    return v


def select(seqs: list[bytes], seq_function, n_functions: int):
    """(records as RECORD_DTYPE in ascending raw key order, stats dict)."""
    NF = [0] * n_functions
    sets: dict[bytes, list] = {}
    n_windows = n_tuples = 0
    for ordinal, (seq, f) in enumerate(zip(seqs, seq_function)):
        f = int(f)
        if f < 0:
            continue
        NF[f] += 1
        for p in range(len(seq) - 7):
            n_windows += 1
            kmer = bytes(seq[p:p + 8])
            if all(c in LETTERS for c in kmer):
                n_tuples += 1
                sets.setdefault(kmer, []).append((f, len(seq) - p, ordinal))
    kept = []
    with_signature = set()
    for kmer in sorted(sets):
        tuples = sets[kmer]
        counts: dict[int, int] = {}
        for f, _, _ in tuples:
            counts[f] = counts.get(f, 0) + 1
        best = max(counts, key=lambda f: counts[f])
        if not keep(counts[best], len(tuples)):
            continue
        median = sorted(n for _, n, _ in tuples)[len(tuples) // 2]
        with_signature.update(o for _, _, o in tuples)
        kept.append((kmer, best, len(tuples), counts[best], median))
    NSF, KS = len(with_signature), len(kept)
    recs = np.zeros(KS, RECORD_DTYPE)
    for r, (kmer, best, count, best_count, median) in zip(recs, kept):
        r["raw_key"] = int.from_bytes(kmer, "big")
        r["code"] = code_of(kmer)
        r["function_index"] = best
        r["n_tuples"] = count
        r["n_best"] = best_count
        r["median_offset"] = median
        r["function_wt"] = weight(NSF, KS, count, NF[best], best_count)
    stats = {"n_windows": n_windows, "n_tuples": n_tuples, "n_sets": len(sets), "n_kept": KS,
             "n_storable": int((recs["code"] <= synth.MAX_ENCODED).sum()), "n_seqs_with_signature": NSF,
             "num_sigs_rule": synth.builder_num_sigs(KS)}
    return recs, stats


def entries(recs: np.ndarray):
    """What the builder inserts: the storable records as keys, fI, oI, avg, wt."""
    r = recs[recs["code"] <= synth.MAX_ENCODED]
    return (r["code"].astype(np.uint64), r["function_index"].astype(np.int32), np.full(len(r), -1, np.int32),
            (r["median_offset"].astype(np.int64) & 0xFFFF).astype(np.uint16), r["function_wt"].astype(np.float32))


def table(recs: np.ndarray, num_sigs: int | None = None) -> np.ndarray:
    """The image the reference's write_hashtable makes of the records."""
    import oracle
    n = num_sigs or synth.builder_num_sigs(len(recs))
    return oracle.build_table(n, *entries(recs))


def ulp_distance(a, b) -> np.ndarray:
    """Distance in f32 steps between two float32 arrays (NaN == NaN: 0)."""
    def ordered(x):
        i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    d = np.abs(ordered(a) - ordered(b))
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    return np.where(both_nan, 0, np.where(one_nan, 1 << 40, d))
