"""FASTA text to calls without the host touching a residue: kgx_fa_parse's
sequences, where the parse left them, through kgx_run_device
(Context.run_parsed) against the oracle over the oracle's own FASTA framing,
and against kgx_process_batch over the same records."""
import numpy as np
import pytest

from close_kmers_amd import synth
from helpers import pack, random_protein, synthetic_table

pytestmark = pytest.mark.gpu

PARAMS = (5, 200, 0, 0)
WANT = 7  # hits, calls, OTUs


def _text(spec):
    """About 400 proteins of 0 to 2,000 residues as FASTA text in 60-column
    lines: every other one carries a stretch of a sequence the image was built
    from, some hold '*' and lower case, some headers a definition."""
    rng = np.random.default_rng(0xFA57)
    planted, poff = synth.make_queries(spec, 200)
    out = []
    for k in range(400):
        n = 0 if k % 57 == 0 else int(rng.integers(0, 2001))
        seq = random_protein(rng, n)
        if k % 2 == 0 and n:
            at = int(rng.integers(0, n))
            piece = planted[int(poff[k // 2]):int(poff[k // 2 + 1])].tobytes().decode()
            seq = seq[:at] + piece + seq[at:]
        if k % 7 == 3 and n > 20:
            at = int(rng.integers(1, len(seq) - 1))
            seq = seq[:at] + "*" + seq[at + 1:]
        if k % 11 == 5 and n > 20:
            at = int(rng.integers(0, len(seq) - 10))
            seq = seq[:at] + seq[at:at + 10].lower() + seq[at + 10:]
        out.append(">prot%d%s\n" % (k, " some definition" if k % 5 == 0 else ""))
        # an empty sequence is a blank line: a '>' straight after a header is a bad data character
        out += [seq[i:i + 60] + "\n" for i in range(0, len(seq), 60)] or ["\n"]
    return "".join(out).encode()


def test_text_to_calls(gpu, oracle_lib):
    spec, table = synthetic_table(20000)
    text = _text(spec)
    lines = oracle_lib.fasta_parse(text).splitlines()
    records = [tuple(ln.split("\t")) for ln in lines]
    assert len(records) == 400 and records[0] == ("prot0", "")
    assert any("*" in s for _, s in records) and any(s != s.upper() for _, s in records)
    res, off = pack(records)
    want = oracle_lib.process_batch(table, res, off, params=PARAMS, want=WANT)
    assert len(want.hits) > 1000 and len(want.calls) > 50
    equal = {"hits": [], "calls": [], "otus": []}
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        prm = gpu.Params(*PARAMS)
        seqs = ctx.fa_parse(text, gpu.FA_FINISHED)
        assert (seqs.n_seqs, seqs.n_residues, seqs.error, seqs.n_seqs_no_id) == (400, len(res), 0, 0)
        got = ctx.run_parsed(seqs, prm, want=WANT)
        assert oracle_lib.diff_batch(got, want, WANT) == equal
        host = ctx.process_batch(res, off, prm, want=WANT)
        assert oracle_lib.diff_batch(host, want, WANT) == equal
        # the parse's arrays outlive the run (and the host batch): the same sequences again
        again = ctx.run_parsed(seqs, prm, want=WANT)
        assert oracle_lib.diff_batch(again, want, WANT) == equal
        h = ctx.fa_seqs_to_host(seqs)
        assert np.array_equal(h["residues"], res) and np.array_equal(h["seq_offsets"], off)
