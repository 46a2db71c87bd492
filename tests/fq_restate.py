"""The fq path's read -> fragments step restated in plain Python, the designed
corpus that walks read edges through every translating kernel, and the wrong
restatements (mutants) that the corpus must tell from the oracle.

fragments(dna) restates DNASequence::get_possible_proteins (frames 1, 2, 3,
-1, -2, -3; code 11; a codon with a base outside ACGTU/acgtu is 'X'; the
reverse strand is the complement read backwards, frame -k from offset k-1),
split at '*', keeping the fragments longer than 10 residues.  oracle.
fq_fragments is the referee (tests/test_fq_restate.py compares the two on the
whole corpus).

The corpus' background is random G/C: a stop codon needs an A or a T on
either strand, so every frame of a background read is one run and every stop
in a read is one the builder put there (or, in the classes that say so, one
its designed bytes spell).
"""
import functools

import numpy as np

_CODE11 = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
_CLS = {c: i for i, c in enumerate("ACGT")} | {"U": 3}


def _translate_anchor(bases: bytes, anchor: int, n: int) -> str:
    """n residues from a fragment anchor: (first base) << 1 | reverse."""
    a, rev = anchor >> 1, anchor & 1
    out = []
    for i in range(n):
        if rev:
            cs = [_CLS.get(chr(bases[a - 3 * i - k]).upper()) for k in range(3)]
            cs = [None if c is None else 3 - c for c in cs]
        else:
            cs = [_CLS.get(chr(bases[a + 3 * i + k]).upper()) for k in range(3)]
        out.append("X" if None in cs else _CODE11[cs[0] * 16 + cs[1] * 4 + cs[2]])
    return "".join(out)


FRAMES = (1, 2, 3, -1, -2, -3)
STOPS_FORWARD = ("TAA", "TAG", "TGA")
STOPS_REVERSE = ("TTA", "CTA", "TCA")  # their reverse complements, read forward
SPELLINGS = STOPS_FORWARD + STOPS_REVERSE


def _class_table(bases: bytes, classes: bytes) -> bytes:
    t = bytearray(b"N" * 256)
    for b, c in zip(bases, classes):
        t[b] = c
    return bytes(t)


_CLASSES = _class_table(b"ACGTUacgtu", b"ACGTTACGTT")
_COMPLEMENT = str.maketrans("ACGT", "TGCA")  # any other class stays outside ACGT
_CODONS = {a + b + c: _CODE11[16 * i + 4 * j + k]
           for i, a in enumerate("ACGT") for j, b in enumerate("ACGT") for k, c in enumerate("ACGT")}


def frame_proteins(dna: bytes, *, classes=_CLASSES, codons=_CODONS, rev_offset=lambda k: k - 1, reversal=True,
                   edge_drop=False):
    """[(frame, protein with its '*')] of the six frames.  The keyword
    arguments are the mutants' slips; the defaults are the restatement."""
    s = dna.translate(classes).decode("ascii")
    rc = s.translate(_COMPLEMENT)
    if reversal:
        rc = rc[::-1]
    out = []
    for frame in FRAMES:
        k = abs(frame)
        m, off = (s, k - 1) if frame > 0 else (rc, rev_offset(k))
        p = [codons.get(m[i:i + 3], "X") for i in range(off, len(m) - 2, 3)]
        if edge_drop:  # q: the forward index of the codon's last forward base
            for c, aa in enumerate(p):
                q = off + 3 * c + 2 if frame > 0 else len(m) - 1 - (off + 3 * c)
                if aa == "*" and q % 64 in (63, 0):
                    p[c] = "X"
        out.append((frame, "".join(p)))
    return out


def runs_of(protein: str):
    """(first codon, codons) of every non-empty run between stops."""
    out, start = [], 0
    for tok in protein.split("*"):
        if tok:
            out.append((start, len(tok)))
        start += len(tok) + 1
    return out


def fragments(dna: bytes, keep: int = 10, **slips):
    """[(frame, fragment)] in the handler's order: the restatement."""
    return [(f, p[a:a + n]) for f, p in frame_proteins(dna, **slips) for a, n in runs_of(p) if n > keep]


def frame_runs(dna: bytes):
    """{frame: (codons of the frame, [(first codon, codons) of each run])}"""
    return {f: (len(p), runs_of(p)) for f, p in frame_proteins(dna)}


# ---- mutants: (reads, i) -> the fragments a slipped kernel would give read i ----

def _across_boundary(reads, i):
    """A frame's last codon completed with the neighbouring read's bases: the
    forward frames see the next read's first two bases, the reverse frames the
    previous read's last two (the concatenation, as far as a codon that starts
    in this read can reach)."""
    nxt = reads[i + 1][:2] if i + 1 < len(reads) else b""
    prv = reads[i - 1][-2:] if i else b""
    fwd = fragments(reads[i] + nxt)
    rev = fragments(prv + reads[i])
    return [x for x in fwd if x[0] > 0] + [x for x in rev if x[0] < 0]


def _slip(**kw):
    return lambda reads, i: fragments(reads[i], **kw)


MUTANTS = {
    "keep > 11": _slip(keep=11),
    "keep > 9": _slip(keep=9),
    "no TGA": _slip(codons=_CODONS | {"TGA": "W"}),
    "N a base": _slip(classes=_class_table(b"ACGTUacgtuNn", b"ACGTTACGTTAA")),
    "U not a base": _slip(classes=_class_table(b"ACGTacgt", b"ACGTACGT")),
    "frame -k from offset k": _slip(rev_offset=lambda k: k),
    "complement without reversal": _slip(reversal=False),
    "stop dropped at a 64-base edge": _slip(edge_drop=True),
    "stop across a read boundary": _across_boundary,
}


# ---- the corpus ----

SWEEP_LENGTHS = (140, 197, 262)
PAIR_LENGTHS = (200, 262)
BYTE_PATTERNS = ("TA?", "T?A", "?AA", "?TA", "C?A", "TC?", "G?G")
LENGTHS = tuple(range(202)) + tuple(range(255, 261)) + tuple(range(383, 388)) + (1000,)
NEIGHBOUR_ENDS = (("T", "AA"), ("TA", "A"), ("TT", "AG"), ("CT", "GA"), ("TC", "A"), ("CT", "A"))


def _gc(rng, n: int) -> bytearray:
    return bytearray(np.frombuffer(b"GC", np.uint8)[rng.integers(0, 2, n)].tobytes())


def _spell(stop: str, v: int) -> bytes:
    """A stop written as is (v 0-4 of 8), in lower case (5, 7), with U for T (6, 7)."""
    s = stop.replace("T", "U") if v >= 6 else stop
    return (s.lower() if v in (5, 7) else s).encode()


@functools.lru_cache(maxsize=None)
def corpus(seed: int = 20):
    """{class: tuple of reads (bytes)}; see the module text and each block."""
    rng = np.random.default_rng(seed)
    out = {}
    # every frame's (len - off) / 3 across 10/11 and 63/64/65, len mod 3 for the reverse frames
    out["lengths"] = tuple(bytes(_gc(rng, n)) for n in LENGTHS)
    # one stop, each spelling at every position: its last base crosses every
    # 8-base step and 64-base block edge (blocks 0..4) in every frame
    for L in SWEEP_LENGTHS:
        reads = []
        for stop in SPELLINGS:
            for p in range(L - 2):
                r = _gc(rng, L)
                r[p:p + 3] = _spell(stop, int(rng.integers(0, 8)))
                reads.append(bytes(r))
        out[f"sweep{L}"] = tuple(reads)
    # two stops with a run of exactly d codons between them, at every position
    reads = []
    for L in PAIR_LENGTHS:
        for d in (10, 11, 12):
            for stop in ("TAA", "TTA"):
                for p in range(L - 2 - 3 * (d + 1)):
                    r = _gc(rng, L)
                    r[p:p + 3] = stop.encode()
                    r[p + 3 * (d + 1):p + 3 * (d + 1) + 3] = stop.encode()
                    reads.append(bytes(r))
    out["pairs"] = tuple(reads)
    # every byte value in every place of a stop (and of a codon that is none)
    reads = []
    for b in range(256):
        for pat in BYTE_PATTERNS:
            for o in (58, 59, 60):
                r = _gc(rng, 120)
                r[o:o + 3] = bytes(b if c == "?" else ord(c) for c in pat)
                reads.append(bytes(r))
    out["every_byte"] = tuple(reads)
    # consecutive reads whose ends would spell a stop if read together, with
    # nothing, empty reads and reads of 1-2 bases between them
    reads = []
    between = ((), (b"",), (b"A",), (b"G",), (b"TA",), (b"AA",), (b"", b"C", b""))
    for n1 in (33, 64, 95):
        for tail, head in NEIGHBOUR_ENDS:
            for mid in between:
                reads.append(bytes(_gc(rng, n1)) + tail.encode())
                reads.extend(mid)
                reads.append(head.encode() + bytes(_gc(rng, 131 - n1)))
    out["neighbours"] = tuple(reads)
    return out


def designed_stops(dna: bytes):
    """(spelling, index of its last base) of every stop spelled in the read."""
    s = dna.translate(_CLASSES).decode("ascii")
    return [(s[q - 2:q + 1], q) for q in range(2, len(s)) if s[q - 2:q + 1] in SPELLINGS]


def expected(reads, fragments_of):
    """The fragment batch of the reads as the device lays it out, from
    fragments_of(read) -> [(frame, fragment)]: residues, offsets, read, frame
    and the per-(read, frame) fragment counts."""
    res, lens, read, frame = [], [], [], []
    counts = np.zeros(6 * len(reads), np.uint32)
    for r, dna in enumerate(reads):
        for f, s in fragments_of(dna):
            res.append(s)
            lens.append(len(s))
            read.append(r)
            frame.append(f)
            counts[6 * r + FRAMES.index(f)] += 1
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(np.array(lens, np.uint64))
    return {"residues": np.frombuffer("".join(res).encode(), np.uint8), "offsets": off,
            "read": np.array(read, np.uint32), "frame": np.array(frame, np.int8), "frame_counts": counts}
