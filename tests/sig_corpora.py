"""Labelled corpora of the signature tests: (sequences, seq_function, n_functions)."""
from __future__ import annotations

import numpy as np

from helpers import ALPHA

# the segment kernel's path thresholds (csrc/kgx_sig.hip: kSmallSet, kWaveSet)
SMALL_SET, WAVE_SET = 16, 4096


def family_corpus(seed: int = 3, n_functions: int = 6, members: int = 6, length: int = 120, rate: float = 0.1):
    """n_functions families of `members` proteins, each a copy of its family's
    random ancestor with substitutions at `rate`.  The seed was chosen on the
    CPU (restatement + oracle): every member's best call is its own function."""
    rng = np.random.default_rng(seed)
    seqs, fn = [], []
    for f in range(n_functions):
        anc = rng.integers(0, 20, length)
        for _ in range(members):
            m = anc.copy()
            hit = rng.random(length) < rate
            m[hit] = rng.integers(0, 20, int(hit.sum()))
            seqs.append("".join(ALPHA[i] for i in m).encode())
            fn.append(f)
    return seqs, fn, n_functions


def _copies(kmer: bytes, counts) -> tuple[list[bytes], list[int]]:
    """counts[f] sequences that are exactly `kmer`, labelled f."""
    seqs, fn = [], []
    for f, c in enumerate(counts):
        seqs += [kmer] * c
        fn += [f] * c
    return seqs, fn


def edge_corpus(seed: int = 11):
    """Every rule and every kernel path of the selection in one small corpus
    (tests/test_gpu_signatures.py lists what is in it)."""
    rng = np.random.default_rng(seed)
    n_functions = 3
    sub = b"ACDE"
    seqs: list[bytes] = []
    fn: list[int] = []

    def add(s: bytes, f: int) -> None:
        seqs.append(s)
        fn.append(f)

    # ~80 slices of 6 ancestors over 4 letters, lightly mutated: sets collide, functions mix
    ancestors = [bytes(sub[i] for i in rng.integers(0, 4, 60)) for _ in range(6)]
    lengths = [0, 7, 8, 9, 10, 15, 16, 17, 59, 60] + list(rng.integers(0, 61, 70))
    for i, ln in enumerate(lengths):
        a = ancestors[int(rng.integers(0, 6))]
        start = int(rng.integers(0, 60 - ln + 1))
        s = bytearray(a[start:start + ln])
        for p in np.nonzero(rng.random(ln) < 0.04)[0]:
            s[p] = sub[int(rng.integers(0, 4))]
        kind = i % 8
        if kind == 5 and ln:
            s[int(rng.integers(0, ln))] = ord("X")
        if kind == 6 and ln:
            s[int(rng.integers(0, ln))] = ord("*")
        if kind == 7 and ln >= 12:
            p = int(rng.integers(0, ln - 11))
            s[p:p + 12] = bytes(s[p:p + 12]).lower()
        # a function mostly tied to the ancestor, sometimes another, sometimes none
        f = int(rng.choice([ancestors.index(a) % 3, int(rng.integers(0, 3)), -1], p=[0.7, 0.15, 0.15]))
        add(bytes(s), f)
    # unlabelled copies of labelled sequences: they add nothing anywhere
    for i in (20, 30, 40):
        add(seqs[i], -1)
    # a lower-case k-mer that is kept (one set of one tuple) and one mixed-case
    add(b"wywywywy", 1)
    add(b"WYWYwywyW", 2)
    # a k-mer three times inside one sequence, and once in another
    add(b"KLKLKLKLKLKL", 0)
    add(b"LKLKLKLK", 0)
    # one long sequence: unique k-mers at its start have n ~ 70000 (> uint16), the rest is 4 letters
    long_tail = bytes(b"FGHI"[i] for i in rng.integers(0, 4, 70000 - 16))
    add(b"NNNNPPPPQQQQRRRR" + long_tail, 2)
    # set sizes on both sides of each path threshold, all of one function but where said
    for kmer, counts in ((b"MMMMNNNN", (SMALL_SET,)), (b"MMMMPPPP", (SMALL_SET + 1,)),
                         (b"MMMMQQQQ", (0, WAVE_SET)), (b"MMMMRRRR", (0, WAVE_SET + 1)),
                         (b"SSSSTTTT", (90, 10)),          # 100 sequences: wave path, kept
                         (b"TVWYTVWY", (4000, 1000)),      # 5000: workgroup path, exactly 80%: kept
                         (b"YWVTYWVT", (3999, 1001))):     # its twin just under: dropped
        s, f = _copies(kmer, counts)
        seqs += s
        fn += f
    # interleave, so neighbouring sequences differ in function and the big sets are scattered
    order = rng.permutation(len(seqs))
    return [seqs[i] for i in order], [fn[i] for i in order], n_functions
