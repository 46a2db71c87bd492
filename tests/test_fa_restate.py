"""Pin tests/fa_restate.py, the byte machine the device FASTA parser is tested
against: its lenient records equal the oracle's FastaParser framing, and the
reference's own parser where oracle/_ref is built, on the random texts of the
GPU tests and on the hand-written cases; the rules of an offending byte and
validate_fasta's report by hand.  No GPU."""
import ctypes

import pytest

import fa_restate


def _lines(records) -> str:
    return "".join(f"{i.decode('latin-1')}\t{s.decode('latin-1')}\n" for i, s in records)


@pytest.fixture(scope="module")
def texts():
    return fa_restate.random_texts() + fa_restate.HAND_CASES


def test_lenient_records_match_oracle(oracle_lib, texts):
    for text in texts:
        records, _ = fa_restate.parse(text, stop_at_error=False)
        assert _lines(records) == oracle_lib.fasta_parse(text), text


def test_lenient_records_match_reference(oracle_lib, texts):
    ref = oracle_lib.ref_lib()
    if ref is None:
        pytest.skip("oracle/_ref is not built")
    for text in texts:
        p = ref.ref_fasta_parse(text, len(text))
        want = ctypes.string_at(p).decode("latin-1")
        ref.ref_free(p)
        records, _ = fa_restate.parse(text, stop_at_error=False)
        assert _lines(records) == want, text


def test_rules_by_hand():
    P = fa_restate.parse
    assert P(b"") == ([(b"", b"")], None)
    assert P(b">a\nAC\nDE\n>b\nFG\n") == ([(b"a", b"ACDE"), (b"b", b"FG")], None)
    # '\r' is transparent and no newline
    assert P(b">a\r\nA\rC\r\n>b\r\nFG") == ([(b"a", b"AC"), (b"b", b"FG")], None)
    # the id ends at the first blank; "> x" has an empty id
    assert P(b"> x\nAC\n>y z\nDE\n") == ([(b"", b"AC"), (b"y", b"DE")], None)
    # '>' and '*' are id bytes within an id
    assert P(b">a>b*c\nAC\n")[0] == [(b"a>b*c", b"AC")]
    # '*' is a residue in data, an error first on a later line
    assert P(b">a\nAC*\n*DE\n", False) == ([(b"a", b"AC*DE")], ("Bad id or data character '*'", 3, b"a"))
    assert P(b">a\n*AC\n") == ([(b"a", b"*AC")], None)
    # '>' straight after a header is a bad data character; the second header's letters become residues
    assert P(b">a\n>bc\nDE\n", False) == ([(b"a", b"bcDE")], ("Bad data character '>'", 2, b"a"))
    assert P(b">a\n>bc\nDE\n", True) == ([(b"a", b"")], ("Bad data character '>'", 2, b"a"))
    # anything but '>' in start, '\n' included: its line is already counted
    assert P(b"\n>a\nAC\n", False) == ([(b"a", b"AC")], ("Missing >", 2, b""))
    assert P(b"x>a\nAC\n", True) == ([(b"", b"")], ("Missing >", 1, b""))
    # the error's id is the record in progress as it stands
    assert P(b">a\nAC\n>bcd\nD-E\n", True) == ([(b"a", b"AC"), (b"bcd", b"D")], ("Bad data character '-'", 4, b"bcd"))
    assert P(b">a\nA\xc3C\n", False) == ([(b"a", b"AC")], ("Bad data character '\xc3'", 2, b"a"))
    # blank lines between data lines
    assert P(b">a\n\nAC\n\n\nDE\n")[0] == [(b"a", b"ACDE")]
    assert fa_restate.first_error(b">a\nAC\n1") == (6, 3, ord("1"), 2)
    assert fa_restate.lenient(b">a\nAC\n>b\nD", False) == ([(b"a", b"AC")], 6, 2, None)
    assert fa_restate.lenient(b">a\nAC\n>b\nD", True) == ([(b"a", b"AC"), (b"b", b"D")], 10, 3, None)
    # an error at or after consumed is not reported yet
    assert fa_restate.lenient(b">a\nAC\n>b\nD-", False)[3] is None
    assert fa_restate.lenient(b">a\nAC\n>b\nD-", True)[3] == (10, 2, ord("-"), 3)


def test_validate_fasta_by_hand():
    V = fa_restate.validate_fasta
    assert V(b"") == ("valid\t1\nn_seqs\t0\n", "")
    assert V(b">a\nACDE\n") == ("valid\t1\nn_seqs\t1\ntotal_size\t4\nmean\t4.00\nstddev\t0.00\n", "")
    assert V(b">a\nAC\n>b\nACDE\n> no id\nACDEFG\n") == \
        ("valid\t1\nn_seqs\t2\ntotal_size\t6\nmean\t3.00\nstddev\t1.41\n", "")
    assert V(b">a\nAC\n>b\nA1\n>c\nAC\n") == \
        ("valid\t0\nn_seqs\t2\nerror_message\tBad data character '1'\nerror_line\t4\n",
         "Error found: Bad data character '1' at line 4 id='b'\n")
    assert V(b"AC\n") == ("valid\t0\nn_seqs\t0\nerror_message\tMissing >\nerror_line\t1\n",
                          "Error found: Missing > at line 1 id=''\n")
