"""fastq_to_protein.cc restated on the CPU, the yardstick of
the fastq_to_protein tests.

Parsing (fastq_parser.h:40-151, fastq_parser.cc:17-36, fastq_to_protein.cc:49-58)
    one byte at a time through the states start, id, defline, data, plus
    start, plus line, quality.  The id runs to the first blank; the data line
    keeps letters; a record is handed over at the quality line's newline.  An
    error -- '>' or anything but '@' where a record starts, a data byte that is
    no letter ('\\r' included), anything but '+' after the data line -- is
    reported with the line number (1 + newlines read, the offending byte
    counted) and the id in progress, and ENDS the parse, because the tool's
    error callback returns false.  At the end, by error or by end of input,
    the record in progress is handed over as it stands.  A record with an
    empty id is ignored by the tool's callback.

Translation (fastq_to_protein.cc:24-47, dna_seq.cc:9-47, dna_seq.h:28-111)
    per read and frame 1, 2, 3, -1, -2, -3: the strand (the read, or its
    reverse complement: only ACGTU/acgtu matter to code 11, U complements to
    A, every other letter stays outside them) from offset |frame| - 1,
    translated by oracle.translate11 (pinned to the reference's table),
    split at runs of '*' as boost::split with token_compress_on does, which
    is re.split(r"\\*+", p): an empty token at either end is kept and an empty
    translation is one empty token.  Tokens are numbered from 1 and those
    longer than 10 are written as ">ID:FRAME:INDEX\\nTOKEN\\n".
"""
from __future__ import annotations

import re

FRAMES = (1, 2, 3, -1, -2, -3)
_COMP = bytes.maketrans(b"ACGTUacgtu", b"TGCAAtgcaa")

START, ID, DEFLINE, DATA, PLUS_START, PLUS_LINE, QUAL = range(7)


def parse(fastq: bytes, stop_at_error: bool = True):
    """(records, error): records = [(id, bases)] as the tool's callback sees
    them (empty ids included), error = None or (text, line, id).  With
    stop_at_error False the parse goes on past errors, as under the fq
    handler (an offending byte is dropped, the state stays; the first error is
    returned), and only records ended by their quality line are listed."""
    state, line, rid, seq = START, 1, bytearray(), bytearray()
    records, error = [], None
    for c in fastq:
        ch = bytes([c])
        if ch == b"\n":
            line += 1
        err = None
        if state == START:
            if ch == b">":
                err = "Starts with >. Is this a fasta file not a fastq file?"
            elif ch != b"@":
                err = "Missing @"
            else:
                state = ID
        elif state == ID:
            if ch in (b" ", b"\t"):
                state = DEFLINE
            elif ch == b"\n":
                state = DATA
            else:
                rid += ch
        elif state == DEFLINE:
            if ch == b"\n":
                state = DATA
        elif state == DATA:
            if ch == b"\n":
                state = PLUS_START
            elif ch.isalpha() and c < 128:
                seq += ch
            else:
                err = "Bad data character '" + ch.decode("latin-1") + "'"
        elif state == PLUS_START:
            if ch != b"+":
                err = "Missing +"
            else:
                state = PLUS_LINE
        elif state == PLUS_LINE:
            if ch == b"\n":
                state = QUAL
        elif state == QUAL:
            if ch == b"\n":
                records.append((bytes(rid), bytes(seq)))
                rid, seq, state = bytearray(), bytearray(), START
        if err is not None:
            error = error or (err, line, bytes(rid))
            if stop_at_error:
                break
    if stop_at_error:  # parse_complete: the record in progress, whatever it holds
        records.append((bytes(rid), bytes(seq)))
    return records, error


def error_report(error) -> str:
    """The line the reference prints for the error (fastq_parser.h:144)."""
    text, line, rid = error
    return f"Error found: {text} at line {line} id='{rid.decode('latin-1')}'"


def strand(dna: bytes, frame: int) -> bytes:
    s = dna if frame > 0 else dna[::-1].translate(_COMP)
    return s[abs(frame) - 1:]


def tokens(dna: bytes, translate11):
    """[(frame, index, token)] of every token of the read, empty ones too."""
    out = []
    for f in FRAMES:
        p = translate11(strand(dna, f).decode("latin-1"))
        out += [(f, i, t) for i, t in enumerate(re.split(r"\*+", p), 1)]
    return out


def kept(dna: bytes, translate11):
    """[(frame, index, token)] of the tokens the tool writes."""
    return [x for x in tokens(dna, translate11) if len(x[2]) > 10]


def read_text(rid: bytes, dna: bytes, translate11) -> bytes:
    if not rid:
        return b""
    return b"".join(b">%s:%d:%d\n%s\n" % (rid, f, i, t.encode()) for f, i, t in kept(dna, translate11))


def text(fastq: bytes, translate11) -> bytes:
    """The tool's output for a FASTQ file."""
    records, _ = parse(fastq)
    return b"".join(read_text(rid, dna, translate11) for rid, dna in records)


def records_text(records, translate11) -> bytes:
    """The output for (id, bases) records already framed."""
    return b"".join(read_text(rid, dna, translate11) for rid, dna in records)


def fastq_of(records, qual: bytes = b"I") -> bytes:
    """Well-formed four-line FASTQ text of (id, bases) records."""
    return b"".join(b"@%s\n%s\n+\n%s\n" % (rid, dna, qual * len(dna)) for rid, dna in records)
