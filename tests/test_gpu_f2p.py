"""fastq_to_protein on the GPU (kgx_fq_proteins, kgx_f2p_*, the command line)
against the CPU restatement tests/f2p_restate.py: exact bytes everywhere."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bgzf_util
import f2p_restate
from helpers import pack, synthetic_table
from tests_golden_codons import back_translate, revcomp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A11, B11 = "MKTAYIAKQRQ", "GSHMLEDPVRW"  # 11 residues each
FRAMES4 = (1, 3, -1, -2)


@pytest.fixture(scope="module")
def ctx(gpu):
    """One context over a small image for the whole module."""
    _, table = synthetic_table(20000)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as c:
        yield c


def _in_frame(prot: str, frame: int, rng) -> bytes:
    """A read whose frame `frame` translates to prot."""
    dna = "ACGT"[:abs(frame) - 1] + back_translate(prot, rng)
    return (dna if frame > 0 else revcomp(dna)).encode()


def _pack_ids(ids):
    off = np.zeros(len(ids) + 1, np.uint64)
    off[1:] = np.cumsum([len(i) for i in ids])
    return np.frombuffer(b"".join(ids), np.uint8).copy() if off[-1] else np.zeros(0, np.uint8), off


def _device(gpu, ctx, records):
    """kgx_fq_proteins over (id, bases) records: (text bytes, arrays, n_fragments)."""
    res, off = pack([("r", b) for _, b in records])
    ids, ioff = _pack_ids([i for i, _ in records])
    t = ctx.fq_proteins(res, off, ids, ioff)
    h = ctx.fq_text_to_host(t)
    assert t.n_reads == len(records) and len(h["text"]) == t.n_bytes
    return bytes(h["text"]), h, t.n_fragments


def _check_arrays(records, text, h, n, translate11):
    """token, read, frame and offsets agree with the text and the restatement."""
    off = h["offsets"].astype(np.int64)
    assert len(off) == n + 1 and off[0] == 0 and off[-1] == len(text) and np.all(np.diff(off) > 0)
    want = [(r, f, i) for r, (rid, dna) in enumerate(records) if rid
            for f, i, _ in f2p_restate.kept(dna, translate11)]
    assert list(zip(h["read"].tolist(), h["frame"].tolist(), h["token"].tolist())) == want
    for g in range(n):
        rid = records[int(h["read"][g])][0]
        head = b">%s:%d:%d\n" % (rid, int(h["frame"][g]), int(h["token"][g]))
        rec = text[off[g]:off[g + 1]]
        assert rec.startswith(head) and rec.endswith(b"\n") and rec.count(b"\n") == 2, g


def _edge_proteins():
    short = "MKT"
    cases = {
        "one": A11, "stop_first": "*" + A11, "stops_first": "***" + A11, "two_and_empty_last": A11 + "**" + B11 + "*",
        "short_then_kept": "MKT*" + B11, "stop_only": "*", "empty": "",
        "ten_dropped": A11[:10], "eleven_kept": A11, "ten_then_eleven": A11[:10] + "*" + B11,
        "all_stops": "*" * 40, "no_stop": A11 + B11 + A11,
    }
    for k in (9, 10, 99, 100):  # k short tokens before a kept one: index k + 1
        cases[f"short_{k}"] = (short + "*") * k + A11
    return cases


@pytest.mark.parametrize("frame", FRAMES4)
def test_index_and_size_edges(gpu, ctx, oracle_lib, frame):
    rng = np.random.default_rng(31)
    cases = _edge_proteins()
    records = [(f"{name}/{frame}".encode(), _in_frame(p, frame, rng)) for name, p in cases.items()]
    text, h, n = _device(gpu, ctx, records)
    assert text == f2p_restate.records_text(records, oracle_lib.translate11)
    _check_arrays(records, text, h, n, oracle_lib.translate11)
    # the cases are what they are meant to be in this frame
    want_idx = {"one": [1], "stop_first": [2], "stops_first": [2], "two_and_empty_last": [1, 2],
                "short_then_kept": [2], "stop_only": [], "empty": [], "ten_dropped": [], "eleven_kept": [1],
                "ten_then_eleven": [2], "all_stops": [], "no_stop": [1], "short_9": [10], "short_10": [11],
                "short_99": [100], "short_100": [101]}
    for r, name in enumerate(cases):
        got = [int(h["token"][g]) for g in range(n) if h["read"][g] == r and h["frame"][g] == frame]
        assert got == want_idx[name], (name, frame)


def test_read_lengths(gpu, ctx, oracle_lib):
    """The 64-base block carry, the len mod 3 of the reverse frames: stop-rich
    and IUPAC-laden reads with lower case, U/u and N, at every start alignment."""
    rng = np.random.default_rng(32)
    stoppy = np.frombuffer(b"TAAGTGATAGCTTATCAACGT", np.uint8)
    mixed = np.frombuffer(b"ACGTACGTACGTacgtNnUuRYKX", np.uint8)
    lengths = [0, 1, 2, 3, 32, 33, 34, 35, 36, 63, 64, 65, 127, 128, 129] + list(range(191, 198)) + [1000]
    records = []
    for rep in range(6):
        for L in lengths:
            pool = (stoppy, mixed, np.frombuffer(b"ACGT", np.uint8))[rep % 3]
            records.append((b"L%d.%d" % (L, rep), bytes(pool[rng.integers(0, len(pool), L)])))
    text, h, n = _device(gpu, ctx, records)
    assert text == f2p_restate.records_text(records, oracle_lib.translate11)
    _check_arrays(records, text, h, n, oracle_lib.translate11)
    assert n > 100 and int(h["token"].max()) > 3


def test_ids(gpu, ctx, oracle_lib):
    rng = np.random.default_rng(33)
    dna = [bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)]) for _ in range(8)]
    ids = [b"a", b"i" * 300, b"x:y:-1:2", b">gt>", b"", b"dup", b"dup", b"last"]
    records = list(zip(ids, dna))
    text, h, n = _device(gpu, ctx, records)
    assert text == f2p_restate.records_text(records, oracle_lib.translate11)
    _check_arrays(records, text, h, n, oracle_lib.translate11)
    assert 4 not in h["read"].tolist() and 3 in h["read"].tolist() and 5 in h["read"].tolist()
    # the neighbours of the read without an id are as they are without it
    without = records[:4] + records[5:]
    assert _device(gpu, ctx, without)[0] == text


def test_empty_batches(gpu, ctx):
    t = ctx.fq_proteins(np.zeros(0, np.uint8), np.zeros(1, np.uint64), np.zeros(0, np.uint8), np.zeros(1, np.uint64))
    assert (t.n_reads, t.n_fragments, t.n_bytes) == (0, 0, 0)
    text, h, n = _device(gpu, ctx, [(b"r1", b"ACGTACGTAC" * 3), (b"r2", b""), (b"", b"ACGT" * 50)])
    assert (text, n) == (b"", 0) and h["offsets"].tolist() == [0]


@pytest.fixture(scope="module")
def many(oracle_lib):
    """20,000 reads of 150 random ACGT bases: FASTQ text and the restatement's output."""
    rng = np.random.default_rng(0x5EED)
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (20000, 150))]
    records = [(b"read%d" % i, bytes(b[i])) for i in range(len(b))]
    return records, f2p_restate.fastq_of(records), f2p_restate.records_text(records, oracle_lib.translate11)


def _stream(gpu, ctx, blocks, part_bytes=0):
    with gpu.FastqToProtein(ctx, part_bytes) as h:
        out = [h.process(b, False) for b in blocks[:-1]] + [h.process(blocks[-1] if blocks else b"", True)]
        return b"".join(out), h.stats(), h.error()


def _cut(data: bytes, n: int):
    return [data[i:i + n] for i in range(0, len(data), n)] or [b""]


def test_many_reads_device_call(gpu, ctx, many, oracle_lib):
    records, _, want = many
    text, h, n = _device(gpu, ctx, records)
    assert text == want
    off = h["offsets"].astype(np.int64)
    assert len(off) == n + 1 and off[-1] == len(text) and np.all(np.diff(off) >= 19)
    assert n == want.count(b">") and n > 50000
    # every record's header is its arrays' (vectorised: the byte at each offset, the count)
    assert np.all(np.frombuffer(text, np.uint8)[off[:-1]] == ord(">"))
    assert np.all(np.diff(h["read"].astype(np.int64)) >= 0)


@pytest.mark.parametrize("part_bytes,block", [(0, 0), (4096, 0), (65536, 0), (0, 1000), (65536, 1000)])
def test_many_reads_streamed(gpu, ctx, many, part_bytes, block):
    records, fastq, want = many
    got, st, err = _stream(gpu, ctx, _cut(fastq, block) if block else [fastq], part_bytes)
    assert got == want
    assert err == "" and st["error_line"] == 0 and st["reads"] == len(records) and st["reads_no_id"] == 0
    assert st["text_bytes"] == len(want) and st["fragments"] == want.count(b">") and st["gzip"] == 0
    want_parts = -(-len(fastq) // part_bytes) if part_bytes else 1
    assert want_parts <= st["parts"] <= want_parts + 1
    assert st["write_ms"] > 0 and st["index_ms"] > 0 and st["parse_ms"] > 0


def test_parse_error_stops_the_file(gpu, ctx, oracle_lib):
    rng = np.random.default_rng(34)
    recs = [(b"e%d" % i, bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)])) for i in range(5)]
    third = b"@e2\n" + recs[2][1][:90] + b"-" + recs[2][1][90:] + b"\n+\n" + b"I" * 151 + b"\n"
    fastq = f2p_restate.fastq_of(recs[:2]) + third + f2p_restate.fastq_of(recs[3:])
    want = f2p_restate.records_text(recs[:2] + [(b"e2", recs[2][1][:90])], oracle_lib.translate11)
    assert want == f2p_restate.text(fastq, oracle_lib.translate11) and want.count(b">e2:") > 0
    _, error = f2p_restate.parse(fastq)
    with gpu.FastqToProtein(ctx) as h:
        cut = fastq.index(b"-") + 20
        got = h.process(fastq[:cut], False)
        assert h.process(fastq[cut:], False) == b""  # later blocks of the file yield nothing
        got += h.process(b"", True)
        assert got == want
        st = h.stats()
        assert st["error_line"] == error[1] == 10 and st["reads"] == 3
        assert h.error() == f2p_restate.error_report(error)
        # the next file on the same handle is clean
        good = f2p_restate.fastq_of(recs)
        assert h.process(good, True) == f2p_restate.records_text(recs, oracle_lib.translate11)
        assert h.stats()["error_line"] == 0 and h.error() == "" and h.stats()["reads"] == 5


def test_end_of_input_emits_the_record_in_progress(gpu, ctx, oracle_lib):
    rng = np.random.default_rng(35)
    recs = [(b"t%d" % i, bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)])) for i in range(3)]
    fastq = f2p_restate.fastq_of(recs)
    want = f2p_restate.records_text(recs, oracle_lib.translate11)
    for text in (fastq[:-1], fastq[:fastq.rindex(b"\n+")]):
        assert f2p_restate.text(text, oracle_lib.translate11) == want
        assert _stream(gpu, ctx, [text])[0] == want
        assert _stream(gpu, ctx, _cut(text, 97), 256)[0] == want


def test_gzip_bodies(gpu, ctx, many):
    _, fastq, want = many
    blocked = bgzf_util.bgzf(fastq, chunk=4000)
    got, st, _ = _stream(gpu, ctx, [blocked])
    assert got == want and st["gzip"] == 1 and st["reads"] == 20000
    assert _stream(gpu, ctx, [gzip.compress(fastq, 6)])[0] == want
    # blocks that cut members (and the sniffed header)
    assert _stream(gpu, ctx, [blocked[:2]] + _cut(blocked[2:], 150001), 1 << 20)[0] == want


def test_round_trip_into_the_protein_side(gpu, oracle_lib):
    """The tool's FASTA through the protein lookup gives the calls of the fq
    path's own fragments over the same reads, fragment for fragment."""
    from close_kmers_amd import synth
    spec, table = synthetic_table(20000)
    rng = np.random.default_rng(36)
    src = synth.ALPHA[synth.source_residue_codes(np.arange(30))].reshape(30, -1)
    reads = []
    for i in range(200):
        p = bytes(src[i % 30][int(rng.integers(0, 200)):][:60]).decode()
        d = back_translate(p, rng)
        reads.append((d if i % 2 else revcomp(d)).encode())
    records = [(b"q%d" % i, r) for i, r in enumerate(reads)]
    res, off = pack([("r", r) for r in reads])
    with gpu.Image.from_table(table) as img, gpu.Context(img) as c:
        got_text = _stream(gpu, c, [f2p_restate.fastq_of(records)])[0]
        f = c.fq_fragments(res, off)
        frag = c.run_fragments(f, gpu.Params(5, 200, 0, 0), want=3)
        n_frag = f.n_fragments
    lines = oracle_lib.fasta_parse(got_text).splitlines()
    assert len(lines) == n_frag and all(l.split("\t")[0].count(":") == 2 for l in lines)
    pres, poff = pack([tuple(l.split("\t")) for l in lines])
    want = oracle_lib.process_batch(table, pres, poff, want=3)
    assert np.array_equal(frag.call_offsets, want.call_offsets)
    assert np.array_equal(frag.hit_offsets, want.hit_offsets)
    for k in ("start", "end", "count", "function_index"):
        assert np.array_equal(frag.calls[k], want.calls[k]), k
    assert np.array_equal(frag.calls["weighted_hits"].view(np.uint32), want.calls["weighted_hits"].view(np.uint32))
    assert len(want.calls) > 50


def test_command_line(gpu, many, tmp_path):
    records, fastq, want = many
    n = 500
    want = want[:want.index(b">read%d:" % n)]
    src = tmp_path / "reads.fq"
    src.write_bytes(f2p_restate.fastq_of(records[:n - 1]) + b"@read%d\nACGT*\n" % (n - 1))
    out = tmp_path / "out.faa"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "close_kmers_amd.fastq_to_protein", str(src)]
    r = subprocess.run(cmd + ["-o", str(out), "--part-bytes", "30000"], capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, r.stderr
    want = want[:want.index(b">read%d:" % (n - 1))]
    assert out.read_bytes() == want and r.stdout == b""
    assert r.stderr.decode().strip().splitlines()[-1] == \
        f"Error found: Bad data character '*' at line {4 * (n - 1) + 2} id='read{n - 1}'"
    r = subprocess.run(cmd, capture_output=True, env=env, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr


def test_kgx_query_proteins_mode(gpu, oracle_lib):
    """kgx_query DATA_DIR FASTQ proteins over the golden fq reads."""
    from close_kmers_amd import build as kbuild
    from helpers import GOLDEN
    d = os.path.join(GOLDEN, "fq")
    src = os.path.join(d, "input.fasta")
    with open(src, "rb") as f:
        want = f2p_restate.text(f.read(), oracle_lib.translate11)
    assert want.count(b">") > 20
    r = subprocess.run([kbuild.QUERY, os.path.join(d, "data"), src, "proteins"], capture_output=True, timeout=300)
    assert r.returncode == 0 and r.stdout == want, r.stderr
