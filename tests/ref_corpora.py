"""Corpora for the reference pin (test_reference_pin.py), its recordings
(golden/make_reference_runs.py) and the GPU tests over them.

designed()   one small table and sequences built to take every branch of the
             reference's gather_hits / process_set_of_hits (kguts.cc:734-877).
random_*()   short sequences over a 4-letter alphabet against a dense table
             with three functions, so that runs switch often.
trace()      a plain model of the run rules that replays the hits the
             reference reported, names the branch each one takes and returns
             the calls it implies.  A test first checks those calls against the
             reference's, and only then reads the branch tally.
fastq_texts()  well-formed and malformed FASTQ.

Everything here is a function of fixed seeds: the recordings depend on it.
"""
from __future__ import annotations

from collections import Counter

import numpy as np

from helpers import ALPHA, DesignedImage, encode, random_protein

CAP = 40000  # MAX_HITS_PER_SEQ (kmer_params.h:20)
M32 = 0xFFFFFFFF

# (min_hits, max_gap, order_constraint, min_weighted_hits); min_hits >= 2 always
DESIGNED_PARAMS = [
    (2, 5, 0, 0),
    (3, 10, 0, 0),
    (2, 0, 0, 0),
    (2, -3, 0, 0),
    (2, 30, 1, 0),
    (2, 30, 0, 3),
    (5, 200, 0, 0),
    (3, 30, 1, 2),
]
RANDOM_PARAMS = [
    (2, 5, 0, 0),
    (3, 200, 0, 0),
    (2, 8, 1, 0),
    (3, 40, 1, 1),
    (2, 12, 0, 2),
    (5, 200, 0, 0),
    (2, -2, 0, 0),
    (3, 4, 0, 3),
]
FUNCTIONS = ["alpha synthase", "beta kinase", "Gamma reductase (EC 1.1.1.1)", "delta", "epsilon transporter",
             "zeta", "eta / theta", "iota"]
DESIGNED_BUCKETS = 2003


class _Designer:
    def __init__(self):
        self.rng = np.random.default_rng(20240521)
        self.img = DesignedImage()
        self.seqs: list[tuple[str, bytes]] = []

    def protein(self, n: int) -> str:
        return random_protein(self.rng, n)

    def store(self, seq: str, pos: int, fI: int, oI: int = 0, avg: int | None = None, wt: float = 1.0):
        k = encode(seq[pos:pos + 8])
        assert k not in self.img.entries, "designed windows must be distinct"
        self.img.add(seq[pos:pos + 8], fI, oI, max(0, len(seq) - pos) if avg is None else avg, wt)

    def add(self, name: str, seq) -> None:
        self.seqs.append((name, seq.encode("latin-1") if isinstance(seq, str) else seq))

    def kmer_with_home(self, home: int) -> str:
        while True:
            k = self.protein(8)
            if encode(k) % DESIGNED_BUCKETS == home and encode(k) not in self.img.entries:
                return k


def designed():
    """(entries, num_sigs, [(name, bytes)]): entries = (keys, fI, oI, avg, wt)
    in insertion order."""
    d = _Designer()
    N = DESIGNED_BUCKETS

    # -- probe chains: inserted first, so the slots are as designed ----------
    b = 1000
    k1, k2, k3 = (d.kmer_with_home(b) for _ in range(3))
    for i, k in enumerate((k1, k2, k3)):
        d.img.add(k, 1, i, 30, 1.0)
    k4 = d.kmer_with_home(b)                     # absent: passes three stored keys
    w1, w2 = d.kmer_with_home(N - 1), d.kmer_with_home(N - 1)
    d.img.add(w1, 1, 0, 20, 1.0)
    d.img.add(w2, 1, 1, 19, 1.0)                 # lands in bucket 0
    w3 = d.kmer_with_home(N - 1)                 # absent: wraps past both
    d.add("chain", d.protein(9) + k1 + k2 + k3 + k4 + d.protein(9))
    d.add("wrap", d.protein(5) + w1 + w2 + w3 + w2 + d.protein(9))

    # -- window walk: a protein with every window stored --------------------
    P = d.protein(60)
    for p in range(len(P) - 7):
        d.store(P, p, 1, p % 3, wt=1.0)
    for n in (0, 1, 7, 8, 9, 16, 60):
        d.add(f"len{n}", P[:n])
    for j in range(8):                           # an ambiguous residue at window position j
        d.add(f"ambig_at{j}", P[:j] + "X" + P[j:30])
    d.add("ambig_enters", P[:20] + "X" + P[20:45])
    d.add("ambig_runs", P[:12] + "XX" + P[12:15] + "x" + P[15:17] + "*" + P[17:40])
    d.add("ambig_bytes", P[:10].encode() + b"\x80" + P[10:25].encode() + b"\xff\x01" + P[25:50].encode())
    d.add("ambig_tail", P[:30] + "X")
    d.add("ambig_all", "XXXXXXXXXXXX")

    # -- gap rule -------------------------------------------------------------
    def planted(name, length, hits):
        """hits: (pos, fI, oI, avg or None, wt); the windows must not overlap
        into one another's keys, which distinct random residues ensure."""
        s = d.protein(length)
        for pos, fI, oI, avg, wt in hits:
            d.store(s, pos, fI, oI, avg, wt)
        d.add(name, s)

    planted("gap_flush", 120, [(p, 2, 0, None, 1.0) for p in (10, 12, 14, 40, 42)])
    planted("gap_reset", 120, [(p, 2, 0, None, 1.0) for p in (10, 40, 41, 90)])
    planted("gap_edge", 120, [(p, 2, 0, None, 1.0) for p in (10, 15, 21, 31, 42)])  # gaps 5, 6, 10, 11
    planted("starts_at0", 80, [(p, 2, 1, None, 1.0) for p in (0, 1, 2, 3, 4, 9)])   # negative max_gap wraps

    # -- run switches -----------------------------------------------------------
    def run(name, fis, start=10, step=1, wts=None, ois=None, length=120):
        planted(name, length, [(start + i * step, f, 0 if ois is None else ois[i], None,
                                1.0 if wts is None else wts[i]) for i, f in enumerate(fis)])

    run("switch_carry", [1, 1, 1, 2, 2, 2])
    run("switch_after_carry", [1, 1, 2, 2, 3, 3])
    run("switch_chain", [1, 1, 2, 2, 3, 3, 4, 4, 4, 1, 1])
    run("interleaved", [1, 2, 1, 2, 1, 2, 2, 1, 1])
    run("single_foreign", [1, 1, 1, 2, 1, 1, 1, 3, 1])
    run("switch_short", [1, 1, 1, 1, 2, 2], step=3)
    run("invalid_function", [100000, 100000, 100000, -1, -1, -1])
    # weights on either side of the integer thresholds 3 and 2
    run("w2_9", [5, 5, 5], wts=[0.95, 0.95, 1.0])
    run("w3_1", [5, 5, 5], wts=[1.05, 1.05, 1.0])
    run("w3_0", [5, 5, 5, 5], wts=[0.75, 0.75, 0.75, 0.75])
    run("w1_9", [5, 5, 5], wts=[0.95, 0.95, 0.0])
    run("w2_1", [5, 5, 5], wts=[1.05, 1.05, 0.0])
    run("w_mixed", [5, 6, 5, 6, 5, 6, 6], wts=[1.3, 9.0, 1.3, 9.0, 0.3, 0.25, 0.25])

    # -- order constraint: d = (pos - prev.pos) - (prev.avg - avg), unsigned ------
    def order(name, hits):
        planted(name, 140, [(pos, fI, 0, avg, 1.0) for pos, fI, avg in hits])

    order("oc_function", [(10, 1, 100), (12, 2, 98), (14, 1, 96), (16, 1, 94)])
    order("oc_d0", [(10, 1, 100), (30, 1, 80)])
    order("oc_d20", [(10, 1, 100), (20, 1, 110)])
    order("oc_d21", [(10, 1, 100), (20, 1, 111)])
    order("oc_neg8", [(10, 1, 100), (12, 1, 90)])
    order("oc_neg20", [(10, 1, 100), (12, 1, 78)])
    order("oc_neg21_then_ok", [(10, 1, 100), (12, 1, 77), (15, 1, 95), (18, 1, 92)])
    order("oc_far_then_ok", [(10, 1, 60), (12, 1, 200), (20, 1, 50), (22, 1, 48)])

    # -- OTU ties: 40 OTUs (past std::sort's insertion-sort size), a negative index, repeats
    S = d.protein(130)
    # (-1 is the one negative index the device's 16-byte records hold, and the call service needs those)
    otus = [(37, 3), (12, 3), (-1, 3), (5, 3), (0, 3)] + [(o, 2) for o in (9, 33, 44, 2, 1, 30, 39, 8, 21, 6)]
    otus += [(o, 1) for o in (70, 50, 3, 4, 71, 72, 7, 34, 10, 11, 13, 14, 15, 16, 17, 18, 19, 20, 22, 23, 24,
                              25, 26, 27, 28)]
    seq_otus = [o for o, c in otus for _ in range(c)]
    d.rng.shuffle(seq_otus)
    for p, o in enumerate(seq_otus):
        d.store(S, p, 3, int(o), wt=0.5)
    d.add("otu_ties", S)
    run("otu_small_ties", [4] * 8, ois=[2, -1, 2, -1, 7, 7, 0, 5])

    keys, fI, oI, avg, wt = d.img.arrays()
    assert len(keys) + 1 < N // 2
    return (keys, fI, oI, avg, wt), N, d.seqs


# ---------------------------------------------------------------------------
RANDOM_LETTERS = "ACDE"
RANDOM_KEYS = 10000
RANDOM_BUCKETS = 25013
RANDOM_SEQS = 3000
RANDOM_SLICE = 150  # recorded and run on the device


def random_table():
    """(keys u64 ascending, fI, oI, avg, wt), num_sigs: RANDOM_KEYS of the
    4**8 8-mers over RANDOM_LETTERS, three functions that neighbouring windows
    often share, fractional weights."""
    rng = np.random.default_rng(77001)
    idx = np.sort(rng.choice(4 ** 8, RANDOM_KEYS, replace=False))
    codes = np.array([ALPHA.index(c) for c in RANDOM_LETTERS], np.uint64)
    keys = np.zeros(RANDOM_KEYS, np.uint64)
    for j in range(8):
        keys = keys * np.uint64(20) + codes[(idx >> (2 * (7 - j))) & 3]
    # the function follows the number of 'A's in the 8-mer (>= 3, <= 1, 2), which
    # changes by at most one between neighbouring windows
    n_a = sum(((idx >> (2 * j)) & 3) == 0 for j in range(8))
    fI = np.where(n_a >= 3, 1, np.where(n_a <= 1, 2, 3)).astype(np.int32)
    oI = rng.integers(-1, 7, RANDOM_KEYS).astype(np.int32)
    avg = rng.integers(0, 16, RANDOM_KEYS).astype(np.uint16)   # so the order constraint accepts and rejects
    wt = (rng.integers(1, 12, RANDOM_KEYS) / 8.0).astype(np.float32)
    return (keys, fI, oI, avg, wt), RANDOM_BUCKETS


def random_seqs(n: int = RANDOM_SEQS):
    rng = np.random.default_rng(77002)
    out = []
    for i in range(n):
        m = int(rng.integers(0, 121))
        s = rng.choice(list((RANDOM_LETTERS + "X").encode()), m, p=[.245, .245, .245, .245, .02])
        out.append((f"r{i}", bytes(s.astype(np.uint8))))
    return out


# ---------------------------------------------------------------------------
def trace(hits, params, events: Counter | None = None):
    """Replay one sequence's hits (HIT_DTYPE rows in stream order) through the
    run rules.  Returns (calls as (start, end, count, fI, weight f32) tuples,
    otu_map).  events counts the branches taken."""
    min_hits, max_gap, oc, mwh = params
    ev = events if events is not None else Counter()
    buf: list = []   # (pos, fI, oI, avg, wt) -- the first num entries of hits[]
    over = None      # hits[num] once num stopped growing at CAP - 2
    cur = 0
    carried = False
    calls, otu = [], {}

    def flush(why):
        nonlocal buf, cur, carried, over
        ev[why] += 1
        cnt, w, last = 0, np.float32(0), 0
        for i, h in enumerate(buf):
            if h[1] == cur:
                last, cnt, w = i, cnt + 1, np.float32(w + h[4])
        if cnt >= min_hits and float(w) >= mwh:
            calls.append((buf[0][0], (buf[last][0] + 7) & M32, cnt, cur, np.float32(w)))
            for h in buf[:last + 1]:
                if h[1] == cur:
                    otu[h[2]] = otu.get(h[2], 0) + 1
            if mwh > 0 and float(w) < mwh + 1 and float(w) != int(w):
                ev["weighted_accept_fraction_above"] += 1
            if len(buf) == CAP - 2:
                ev["saturated_call"] += 1
        elif cnt < min_hits:
            ev["flush_rejected_min_hits"] += 1
        else:
            ev["flush_rejected_weighted"] += 1
            if float(w) > mwh - 1 and float(w) != int(w):
                ev["weighted_reject_fraction_below"] += 1
        n = len(buf)
        if buf[n - 2][1] != cur and buf[n - 2][1] == buf[n - 1][1]:
            cur = buf[n - 1][1]
            buf = [buf[n - 2], buf[n - 1]]
            carried = True
            ev["carry_two"] += 1
        else:
            buf = []
            carried = False

    for h in hits:
        pos, fI = int(h["pos"]), int(h["function_index"]) & M32
        rec = (pos, fI, int(h["otu_index"]), int(h["avg_from_end"]), np.float32(h["function_wt"]))
        if buf and ((buf[-1][0] + max_gap) & M32) < pos:
            if max_gap == 0:
                ev["max_gap_zero_gap"] += 1
            if max_gap < 0:
                ev["max_gap_negative_gap"] += 1
            if len(buf) >= min_hits:
                flush("gap_flush")
            else:
                buf, carried = [], False
                ev["gap_reset"] += 1
        elif buf and max_gap < 0:
            ev["max_gap_negative_wrapped"] += 1
        if not buf:
            cur = fI
        ok = True
        if oc and buf:
            prev = buf[-1]
            dd = ((pos - prev[0]) - (prev[3] - rec[3])) & M32
            if fI != prev[1]:
                ok = False
                ev["order_rejected_function"] += 1
            elif dd > 20:
                ok = False
                ev["order_rejected_negative_d" if dd >= 1 << 31 else "order_rejected_d_above_20"] += 1
            else:
                ev["order_accepted"] += 1
                if dd in (0, 20):
                    ev[f"order_accepted_d{dd}"] += 1
        if not ok:
            continue
        if len(buf) < CAP - 2:
            buf.append(rec)
        else:
            over = rec  # written past the counted entries; never read back
            ev["saturated_hit"] += 1
        n = len(buf)
        if n > 1 and cur != fI and buf[n - 2][1] == buf[n - 1][1]:
            if carried and n == 4:
                ev["pair_switch_after_carry"] += 1
            flush("pair_switch")
    if len(buf) >= min_hits:
        flush("end_flush")
    return calls, otu


def walk_tally(seq: bytes, hits, table_keys, num_sigs: int, slot_of: dict, ev: Counter) -> None:
    """Window-walk and probe-chain branches of one sequence, from its bytes,
    the hits the reference reported and the table."""
    codes = [ALPHA.find(chr(c)) if c < 128 else -1 for c in seq]
    n = len(seq)
    ev[f"length_{n}"] += 1
    hit_pos = {int(h["pos"]) for h in hits}
    amb = [i for i, c in enumerate(codes) if c < 0]
    if n >= 9:
        first8 = [i for i in amb if i < 8]
        if len(first8) == 1 and not [i for i in amb if 8 <= i <= first8[0] + 8] and hits.size \
                and int(hits["pos"][0]) == first8[0] + 1:
            ev[f"ambiguous_at_window_position_{first8[0]}"] += 1
    for i in amb:
        if i >= 8 and all(c >= 0 for c in codes[i - 8:i]) and i - 8 in hit_pos:
            ev["ambiguous_enters_at_p_plus_7"] += 1
    for a, b in zip(amb, amb[1:]):
        if b == a + 1:
            ev["ambiguous_adjacent"] += 1
        elif b - a <= 8:
            ev["ambiguous_again_within_a_window"] += 1

    def key_at(p):
        w = codes[p:p + 8]
        if len(w) < 8 or min(w) < 0:
            return None
        k = 0
        for c in w:
            k = k * 20 + c
        return k

    if n >= 8:
        k = key_at(n - 8)
        assert n - 8 not in hit_pos, "the last window is never reported"
        if k is not None and k in slot_of:
            ev["last_window_stored_not_reported"] += 1
    for p in range(max(0, n - 8)):
        k = key_at(p)
        if k is None:
            continue
        home = k % num_sigs
        if k in slot_of:
            assert p in hit_pos
            s = slot_of[k]
            if s != home:
                ev["stored_after_collision_chain"] += 1
            if s < home:
                ev["chain_wraps_to_bucket_0"] += 1
        else:
            assert p not in hit_pos
            if int(table_keys[home]) <= 20 ** 8:
                ev["absent_chain_passes_stored"] += 1
                s = home
                while int(table_keys[s]) <= 20 ** 8:
                    s = (s + 1) % num_sigs
                if s < home:
                    ev["absent_chain_wraps"] += 1


REQUIRED_EVENTS = (
    [f"ambiguous_at_window_position_{j}" for j in range(8)]
    + [f"length_{n}" for n in (0, 1, 7, 8, 9, 16)]
    + ["ambiguous_enters_at_p_plus_7", "ambiguous_adjacent", "ambiguous_again_within_a_window",
       "last_window_stored_not_reported", "stored_after_collision_chain", "chain_wraps_to_bucket_0",
       "absent_chain_passes_stored", "absent_chain_wraps",
       "gap_flush", "gap_reset", "max_gap_zero_gap", "max_gap_negative_gap", "max_gap_negative_wrapped",
       "carry_two", "pair_switch", "pair_switch_after_carry", "end_flush",
       "flush_rejected_min_hits", "flush_rejected_weighted", "weighted_reject_fraction_below",
       "weighted_accept_fraction_above", "order_rejected_function", "order_rejected_d_above_20",
       "order_rejected_negative_d", "order_accepted_d0", "order_accepted_d20"])


# ---------------------------------------------------------------------------
def fastq_texts() -> list[bytes]:
    """FASTQ texts: well-formed, each error kind in each state that can raise
    it, blanks / tabs / '\\r' in ids, high bytes, truncation in every state,
    empty ids, errors on later lines."""
    ok = b"@r1 first read\nACGTTGCA\n+\nIIIIIIII\n@r2\tdef\nacgtNNRY\n+r2\n!!!!!!!!\n"
    t = [
        b"", b"\n", b"@", b"@a", b"@a\n", b"@a\nAC", b"@a\nAC\n", b"@a\nAC\n+", b"@a\nAC\n+\n", b"@a\nAC\n+\nII",
        ok, ok + b"@r3\nTTTT\n+\nIIII", ok + b"\n", ok + b"@r3 x",
        b">r1\nACGT\n", ok + b">r3\nACGT\n+\nIIII\n", b"r1\nACGT\n+\nIIII\n", ok + b"\n@r3\nAC\n+\nII\n",
        b"@r1\nAC GT\n+\nIIII\n", b"@r1\nAC\tGT\n+\nIIII\n", b"@r1\r\nACGT\r\n+\r\nIIII\r\n",
        b"@r1\nAC1T\n+\nIIII\n", b"@r1\nAC\x80T\xe9\xff\n+\nIIII\n", b"@r1\nAC*T-.\n+\nIIII\n",
        b"@r1\nACGT\nIIII\n", b"@r1\nACGT\n\n+\nIIII\n", b"@r1\nACGT\n@r2\nAC\n+\nII\n",
        b"@\nACGT\n+\nIIII\n", b"@ only a definition\nACGT\n+\nIIII\n@\t\nAC\n+\nII\n",
        b"@id\xc3\xa9\x80\xff\x01 d\nACGT\n+\nIIII\n", b"@r\rx\ty\nAC\n+\nII\n", b"@a  b\n\n+\n\n", b"@a\n\n+\n\n@b\n\n+\n\n",
        ok + b"@r3\nAC\n+\nII\n@r4\nA-C\n+\nIII\n@r5\nGG\n+\nII\n", ok + b"@r3\nAC\nII\n@r4\nGG\n+\nII\n",
        b"@r1\nACGT\n+\n@@@@\n@r2\nAC\n+\n@I\n", b"@r1\nACGT\n+ACGT\n+III\n+r2\nAC\n+\nII\n",
        b"@" + b"i" * 299 + b"\nACGT\n+\nIIII\n", b"\n\n@r1\nAC\n+\nII\n", b"@r1\nAC\n+\nII\n\n\n>x\n",
        b"@r1 d\n\n+\n\n@r2\nA\n+\nI", b"@r1\nACGT\n+\nIIII\n@r2\nAC9\n", b"@r1\nACGT\n+\nIIII\nX",
    ]
    rng = np.random.default_rng(5150)
    alphabet = list(b"@+>\n\n\nACGTacgtN I\t\r1-\x80\xff")
    for _ in range(40):   # random bytes
        t.append(bytes(rng.choice(alphabet, int(rng.integers(0, 60))).astype(np.uint8)))
    for _ in range(40):   # well-formed records with injected bad bytes
        recs = b"".join(b"@q%d%s\n%s\n+\n%s\n" % (i, b" d" if rng.random() < .3 else b"",
                                                   bytes(rng.choice(list(b"ACGTN"), m).astype(np.uint8)), b"I" * m)
                        for i, m in enumerate(rng.integers(0, 20, int(rng.integers(1, 5)))))
        b = bytearray(recs)
        for _ in range(int(rng.integers(0, 3))):
            at = int(rng.integers(0, len(b) + 1))
            b[at:at] = bytes([int(rng.choice(alphabet))])
        if rng.random() < .3:
            b = b[:int(rng.integers(0, len(b) + 1))]
        t.append(bytes(b))
    return t


# ---------------------------------------------------------------------------
def _rec(rid: bytes, bases: bytes, plus: bytes = b"") -> bytes:
    return b"@" + rid + b"\n" + bases + b"\n+" + plus + b"\n" + b"I" * len(bases) + b"\n"


# name: (bytes in front of the offending byte, the offending byte and what follows)
PLACED_PIECES = {
    "leading_gt": (b"", b">" + _rec(b"g", b"ACGTACGTACGT")),
    "garbage": (b"", b"garbage\n" + _rec(b"g", b"ACGTACGTACGT")),
    "blank_lines": (b"", b"\n\n" + _rec(b"b", b"ACGTACGTACGT")),
    "dash": (b"@d\nACGT", b"-ACGT\n+\nIIIIIIII\n"),
    "tab": (b"@t\nACGT", b"\tACGT\n+\nIIIIIIII\n"),
    "digit": (b"@n\nACGT", b"5ACGT\n+\nIIIIIIII\n"),
    "cr": (b"@c\nACGTACGT", b"\r\n+\nIIIIIIII\n"),
    "high_byte": (b"@h\nACGT", b"\xc3ACGT\n+\nIIIIIIII\n"),
    "missing_plus": (b"@m\nACGTACGT\n", b"IIIIIIII\n" + _rec(b"m2", b"ACGT")),
    "empty_id_cut": (b"@\nAC", b"-GT\n+\nIIII\n"),
    "truncated": (b"@z\nACGTAC", b"GT"),
}
PLACED_AT = (4095, 4096, 4097, 4111, 4112, 4113)  # a tile (4096-byte) edge and a lane (16-byte) edge


def placed_fastq_cases():
    return [(name, at) for name in PLACED_PIECES for at in PLACED_AT]


def placed_fastq(piece: str, at: int) -> bytes:
    """Well-formed records, then the piece with its offending byte at offset
    `at` of the text, then (but for "truncated") more well-formed records."""
    front, back = PLACED_PIECES[piece]
    room = at - len(front)
    lead = b""
    while room - len(lead) > 60:
        lead += _rec(b"L%d" % (len(lead) % 97), b"ACGTTGCAAC")
    rest = room - len(lead) - len(_rec(b"p", b""))
    assert rest >= 0
    lead += _rec(b"p", b"A" * (rest // 2), b"x" * (rest % 2))
    text = lead + front + back
    assert len(lead + front) == at
    if piece != "truncated":
        text += b"".join(_rec(b"k%d" % i, b"ACGTN" * (1 + i % 3), b"k" * (i % 2)) for i in range(10))
    return text


# ---------------------------------------------------------------------------
# Sequences just below and above the lengths at which the device changes
# scorer: 2048 windows (lane / wave in the hybrid) and 39,998 windows (wave /
# long).  A sequence of n residues has n - 8 windows.
ROUTING_LENGTHS = (2056, 2057, 40006, 40007)
ROUTING_PARAMS = [(2, 5, 0, 0), (5, 200, 0, 0), (2, 30, 0, 3), (2, 30, 1, 0), (2, -3, 0, 0)]


def routing_seqs():
    """The designed sequences end to end, repeated with random spacers of
    changing length, cut at each of ROUTING_LENGTHS: runs, switches, gaps and
    ambiguous residues against the designed table at every such length."""
    _, _, seqs = designed()
    rng = np.random.default_rng(31337)
    order = [s for _, s in seqs if s]
    parts, n = [], 0
    while n < max(ROUTING_LENGTHS):
        for i in rng.permutation(len(order)):
            spacer = random_protein(rng, int(rng.integers(0, 40))).encode()
            parts += [order[i], spacer]
            n += len(order[i]) + len(spacer)
    whole = b"".join(parts)
    return [(f"route{n}", whole[:n]) for n in ROUTING_LENGTHS]
