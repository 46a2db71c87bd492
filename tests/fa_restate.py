"""FastaParser::parse_char / parse_complete (fasta_parser.h:38-144,
fasta_parser.cc:30-36) restated byte by byte, and validate_fasta.cc:12-82 on
top of it: what the device parser (csrc/kgx_fa_parse.hip) and the
validate_fasta tool are tested against.  Bytes in, bytes out."""
import math

START, ID, DEFLINE, DATA, ID_OR_DATA = range(5)


def _alpha(c: int) -> bool:
    return 65 <= c <= 90 or 97 <= c <= 122  # isalpha in the C locale; bytes >= 0x80 are not letters


def walk(text: bytes):
    """The machine over text, going on past errors: (ends, errors, state, id,
    seq) with ends = [(position of the '>' that ended a record, id, seq)],
    errors = [(position, message, line, id in progress)] and the record in
    progress at the end of the text."""
    state, rid, seq, line = START, bytearray(), bytearray(), 1
    ends, errors = [], []
    for pos, c in enumerate(text):
        if c == 10:
            line += 1
        if c == 13:
            continue
        err = None
        if state == START:
            if c != 62:
                err = b"Missing >"
            else:
                state = ID
        elif state == ID:
            if c in (32, 9):
                state = DEFLINE
            elif c == 10:
                state = DATA
            else:
                rid.append(c)
        elif state == DEFLINE:
            if c == 10:
                state = DATA
        elif state == DATA:
            if c == 10:
                state = ID_OR_DATA
            elif _alpha(c) or c == 42:
                seq.append(c)
            else:
                err = b"Bad data character '" + bytes([c]) + b"'"
        else:
            if c == 62:
                ends.append((pos, bytes(rid), bytes(seq)))
                rid, seq = bytearray(), bytearray()
                state = ID
            elif c == 10:
                pass
            elif _alpha(c):
                seq.append(c)
                state = DATA
            else:
                err = b"Bad id or data character '" + bytes([c]) + b"'"
        if err is not None:
            errors.append((pos, err.decode("latin-1"), line, bytes(rid)))
    return ends, errors, state, bytes(rid), bytes(seq)


def parse(text: bytes, stop_at_error: bool = True):
    """The records of FastaParser::parse over text, parse_complete's last one
    included: ([(id, seq)], error) with error None or (message, line, id) of
    the first offending byte.  stop_at_error: the error callback returns false
    (validate_fasta.cc:35-40), so the parse ends at that byte."""
    ends, errors, _, rid, seq = walk(text)
    if errors and stop_at_error:
        ends, _, _, rid, seq = walk(text[:errors[0][0]])
    records = [(i, s) for _, i, s in ends] + [(rid, seq)]
    return records, (errors[0][1:] if errors else None)


def first_error(text: bytes):
    """(position, code, byte, newlines in text[0, position]) of the first
    offending byte, or None: kgx_fa_seqs' error fields."""
    errors = walk(text)[1]
    if not errors:
        return None
    pos, msg, line, _ = errors[0]
    code = 1 if msg.startswith("Missing") else 2 if msg.startswith("Bad data") else 3
    return pos, code, text[pos], line - 1


def lenient(text: bytes, finished: bool):
    """kgx_fa_parse without KGX_FA_STRICT: (records, consumed, newlines, error)
    with error as first_error gives it, or None when it lies at or after
    consumed."""
    ends, _, _, rid, seq = walk(text)
    records = [(i, s) for _, i, s in ends]
    consumed = ends[-1][0] if ends else 0
    if finished:
        records.append((rid, seq))
        consumed = len(text)
    e = first_error(text)
    if e is not None and e[0] >= consumed:
        e = None
    return records, consumed, text[:consumed].count(b"\n"), e


def report(lengths, error) -> str:
    """validate_fasta.cc:46-81: the tool's stdout."""
    n = len(lengths)
    if error is not None:
        return f"valid\t0\nn_seqs\t{n}\nerror_message\t{error[0]}\nerror_line\t{error[1]}\n"
    out = f"valid\t1\nn_seqs\t{n}\n"
    if n:
        total = sum(lengths)
        mean = total / n
        stddev = math.sqrt(sum((x - mean) * (x - mean) for x in lengths) / (n - 1.0)) if n > 1 else 0.0
        out += "total_size\t%d\nmean\t%.2f\nstddev\t%.2f\n" % (total, mean, stddev)
    return out


def validate_fasta(text: bytes):
    """(stdout, stderr) of validate_fasta over a file holding text: the records
    with an id are counted, the first error ends the parse and is printed."""
    records, error = parse(text, stop_at_error=True)
    lengths = [len(s) for i, s in records if i]
    err = ""
    if error is not None:
        err = f"Error found: {error[0]} at line {error[1]} id='{error[2].decode('latin-1')}'\n"
    return report(lengths, error[:2] if error else None), err


ALPHABET = b">>>>\n\n\n\n\n\r \t*-1@ACDEGKLMWYacdxX"


def random_texts(n: int = 300, max_len: int = 9000, seed: int = 0xFA):
    """n texts over '>', '\\n', '\\r', blanks, '*', '-', '1', '@' and letters in
    both cases, '>' and '\\n' weighted up; no NUL.  Half of them begin with a
    header, and the lengths favour the short ones."""
    import numpy as np
    rng = np.random.default_rng(seed)
    a = np.frombuffer(ALPHABET, np.uint8)
    out = []
    for k in range(n):
        m = int(rng.integers(0, 200)) if k % 3 else int(rng.integers(0, max_len + 1))
        body = bytes(a[rng.integers(0, len(a), m)])
        if k % 2:
            body = (b">id%d\n" % k + body)[:max_len]
        out.append(body)
    return out


HAND_CASES = [
    b"", b">", b">a", b">a\n", b">a\nAC", b">a\nAC\n", b">a\nAC\nDE\n>b\nFG\n", b"\n", b"x", b"AC\n>a\nAC\n",
    b">a def\nAC\n", b"> x\nAC\n", b">\nAC\n", b"> def\nAC\n>b\nDE\n", b">a\r\nAC\r\nDE\r\n>b\r\nFG\r\n",
    b">a\n\n\nAC\n\n>b\n\nDE\n", b">a\nAC*\nDE\n", b">a\nAC\n*DE\n", b">a\n*AC\n", b">a\n>b\nAC\n", b">a\n>b\n>c\nAC\n",
    b">a>b*c\nAC\n", b">a\nA C\n", b">a\nAC\n DE\n", b">a\nAC\n1\n", b">a\nA-C\n", b">a\nA\xc3\x84C\n", b">a\nAC\n\xffDE\n",
    b">a\tdef > * \nAC\n>b", b">a\nAC\n>b d", b">a\nAC\n>", b">a\nac\nde\n>B\nfg", b"\n\n>a\nAC\n", b"junk\n>a\nAC\n>b\nDE\n",
    b">a\nAC\r", b">a\nAC\n\r>b\nDE\n", b"\r>a\nAC\n",
]
