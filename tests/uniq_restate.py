"""unique_prots.cc restated on the CPU, the yardstick of the
unique tests.

Which hits form a protein's set
    its set is the set of distinct which_kmer values of its hits; a hit is
    every window lookup_hash_entry finds in gather_hits' window walk
    (kguts.cc:798-815).  hit_cb runs before the gap rule, the order constraint,
    the 40,000-hit cap and min_hits, so no scoring parameter touches the set.
    Lower case, X, * and the like are invalid and a window over them is
    skipped; a sequence is cut at its first NUL; sequences shorter than 8
    residues, empty ones and ones without a hit have the empty set.  All of
    that is the oracle's hit list (oracle.process_batch, want 1).

Groups and their order
    proteins with identical sets form one group, members in input order;
    groups stand as std::map orders std::set<u64> keys: lexicographic
    comparison of the ascending key lists, a proper prefix before the longer
    list, the empty set first.  Python's tuple order is that order.

Text (unique_prots.cc:101-108)
    per group every id followed by a tab, the last one too, then a newline.
"""
from __future__ import annotations

import numpy as np


def groups(hit_offsets, which_kmer):
    """(groups, keys): groups[g] the ascending sequence indices of group g,
    keys[g] its ascending key tuple, in the order above."""
    off = np.asarray(hit_offsets, np.int64)
    k = np.asarray(which_kmer, np.uint64)
    by_set: dict[tuple, list[int]] = {}
    for i in range(len(off) - 1):
        key = tuple(sorted(set(int(x) for x in k[off[i]:off[i + 1]])))
        by_set.setdefault(key, []).append(i)
    order = sorted(by_set)
    return [by_set[key] for key in order], order


def group_of(groups_, n_seq: int) -> np.ndarray:
    out = np.full(n_seq, -1, np.int64)
    for g, members in enumerate(groups_):
        out[members] = g
    return out


def text(ids, groups_) -> bytes:
    return b"".join(b"".join(ids[i] + b"\t" for i in members) + b"\n" for members in groups_)


def pieces_by_rule(off, piece: int, max_seqs: int = 1 << 29) -> int:
    """A piece is closed before the sequence that would take it above `piece`
    residues (0: 2^25), and at max_seqs sequences."""
    piece = piece or 1 << 25
    n, s0, count = len(off) - 1, 0, 0
    while s0 < n:
        s1 = s0 + 1
        while s1 < n and s1 - s0 < max_seqs and int(off[s1 + 1]) - int(off[s0]) <= piece:
            s1 += 1
        count += 1
        s0 = s1
    return count
