"""fastq_to_protein with the parse on the device (context option
"fq_parse_device" 1, csrc/kgx_f2p.cpp over kgx_fq_parse): the streamed
scenarios of tests/test_gpu_f2p.py, each run on one handle at the option's two
settings: the bytes are the restatement's and the same at both, and so are
reads, reads_no_id, fragments, text_bytes, error_line and error()."""
import gzip

import numpy as np
import pytest

import bgzf_util
import f2p_restate
from helpers import synthetic_table

pytestmark = pytest.mark.gpu

SAME = ("reads", "reads_no_id", "fragments", "text_bytes", "error_line", "gzip")


@pytest.fixture(scope="module")
def ctx(gpu):
    _, table = synthetic_table(20000)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as c:
        yield c
        c.set_option("fq_parse_device", 0)


@pytest.fixture(scope="module")
def many(oracle_lib):
    """3,000 reads of 150 random ACGT bases (940 KB: 230 parts of 4096 bytes, 15 of 65536, 940 blocks of
    1000): FASTQ text and the restatement's output."""
    rng = np.random.default_rng(0x5EED)
    b = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (3000, 150))]
    records = [(b"read%d" % i, bytes(b[i])) for i in range(len(b))]
    return records, f2p_restate.fastq_of(records), f2p_restate.records_text(records, oracle_lib.translate11)


def _cut(data: bytes, n: int):
    return [data[i:i + n] for i in range(0, len(data), n)] or [b""]


def _file(h, blocks):
    out = [h.process(b, False) for b in blocks[:-1]] + [h.process(blocks[-1] if blocks else b"", True)]
    return b"".join(out), h.stats(), h.error()


def _both(gpu, ctx, blocks, part_bytes=0):
    """The file through one handle at fq_parse_device 0, then 1 (the option is
    read when a file starts): the outputs agree; returns the device-parsed one."""
    with gpu.FastqToProtein(ctx, part_bytes) as h:
        ctx.set_option("fq_parse_device", 0)
        host = _file(h, blocks)
        ctx.set_option("fq_parse_device", 1)
        dev = _file(h, blocks)
        ctx.set_option("fq_parse_device", 0)
    assert dev[0] == host[0] and dev[2] == host[2]
    for k in SAME:
        assert dev[1][k] == host[1][k], k
    # parts is not compared: a device-parsed part is part_bytes of carried tail and new text (more parts
    # than the host parser's part_bytes of new text each), and one without a whole record grows (fewer)
    return dev


@pytest.mark.parametrize("part_bytes,block", [(0, 0), (4096, 0), (65536, 0), (0, 1000), (65536, 1000)])
def test_many_reads_streamed(gpu, ctx, many, part_bytes, block):
    records, fastq, want = many
    got, st, err = _both(gpu, ctx, _cut(fastq, block) if block else [fastq], part_bytes)
    assert got == want
    assert err == "" and st["error_line"] == 0 and st["reads"] == len(records) and st["reads_no_id"] == 0
    assert st["text_bytes"] == len(want) and st["fragments"] == want.count(b">") and st["gzip"] == 0
    assert st["parts"] >= (-(-len(fastq) // part_bytes) if part_bytes else 1)
    assert st["write_ms"] > 0 and st["index_ms"] > 0 and st["parse_ms"] > 0 and st["upload_ms"] > 0


def test_parts_smaller_than_a_record(gpu, ctx, many, oracle_lib):
    """part_bytes 64: every record exceeds a part, which grows until it holds one."""
    records = many[0][:300] + [(b"", b"ACGT" * 30), (b"tail", b"ACGTTGCA" * 20)]
    fastq = f2p_restate.fastq_of(records)
    want = f2p_restate.records_text(records, oracle_lib.translate11)
    for blocks in ([fastq], _cut(fastq, 1000), _cut(fastq[:-1], 37)):
        got, st, err = _both(gpu, ctx, blocks, 64)
        assert got == want and err == "" and st["reads"] == len(records) and st["reads_no_id"] == 1


def _error_file(oracle_lib):
    rng = np.random.default_rng(34)
    recs = [(b"e%d" % i, bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)])) for i in range(5)]
    third = b"@e2\n" + recs[2][1][:90] + b"-" + recs[2][1][90:] + b"\n+\n" + b"I" * 151 + b"\n"
    fastq = f2p_restate.fastq_of(recs[:2]) + third + f2p_restate.fastq_of(recs[3:])
    want = f2p_restate.records_text(recs[:2] + [(b"e2", recs[2][1][:90])], oracle_lib.translate11)
    return recs, fastq, want


@pytest.mark.parametrize("part_bytes", [0, 64, 256, 4096])
def test_parse_error_stops_the_file(gpu, ctx, oracle_lib, part_bytes):
    recs, fastq, want = _error_file(oracle_lib)
    assert want == f2p_restate.text(fastq, oracle_lib.translate11) and want.count(b">e2:") > 0
    _, error = f2p_restate.parse(fastq)
    ctx.set_option("fq_parse_device", 1)
    try:
        with gpu.FastqToProtein(ctx, part_bytes) as h:
            cut = fastq.index(b"-") + 20
            got = h.process(fastq[:cut], False)
            got += h.process(fastq[cut:], False)
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
    finally:
        ctx.set_option("fq_parse_device", 0)
    for blocks in ([fastq], _cut(fastq, 97)):
        got, st, err = _both(gpu, ctx, blocks, part_bytes)
        assert got == want and err == f2p_restate.error_report(error) and st["error_line"] == 10


def test_every_error_kind_reports_as_the_host_parser(gpu, ctx, oracle_lib):
    good = f2p_restate.fastq_of([(b"g%d" % i, b"ACGTTGCATTGACCA" * 4) for i in range(6)])
    for bad in (b">fasta\nACGT\n", b"garbage\n", b"\n\n", b"@r\nACGT\r\n+\nIIII\n", b"@r\nAC\xc3GT\n+\nIIII\n",
                b"@r\nACGT\nIIII\n", b"@\nAC-GT\n+\nIIII\n", b"@r def\nACGT\n\n+\nIIII\n"):
        fastq = good + bad + good
        _, error = f2p_restate.parse(fastq)
        for part_bytes in (0, 128):
            got, st, err = _both(gpu, ctx, _cut(fastq, 50), part_bytes)
            assert got == f2p_restate.text(fastq, oracle_lib.translate11)
            assert err == f2p_restate.error_report(error) and st["error_line"] == error[1]


def test_end_of_input_emits_the_record_in_progress(gpu, ctx, oracle_lib):
    rng = np.random.default_rng(35)
    recs = [(b"t%d" % i, bytes(np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, 150)])) for i in range(3)]
    fastq = f2p_restate.fastq_of(recs)
    want = f2p_restate.records_text(recs, oracle_lib.translate11)
    for text in (fastq[:-1], fastq[:fastq.rindex(b"\n+")]):
        assert f2p_restate.text(text, oracle_lib.translate11) == want
        assert _both(gpu, ctx, [text])[0] == want
        assert _both(gpu, ctx, _cut(text, 97), 256)[0] == want


def test_gzip_bodies(gpu, ctx, many):
    records, fastq, want = many
    blocked = bgzf_util.bgzf(fastq, chunk=4000)
    got, st, _ = _both(gpu, ctx, [blocked])
    assert got == want and st["gzip"] == 1 and st["reads"] == len(records)
    assert _both(gpu, ctx, [gzip.compress(fastq, 6)])[0] == want
    # blocks that cut members (and the sniffed header)
    assert _both(gpu, ctx, [blocked[:2]] + _cut(blocked[2:], 50001), 1 << 18)[0] == want


def test_option_values_and_error_text(gpu, ctx, monkeypatch):
    """fq_parse_device is declared after score_lean, beyond the options that
    tests/native/options_check.cpp records: its values and texts are held here."""
    set_option = gpu.lib().kgx_ctx_set_option
    for v in (0, 1):
        assert set_option(ctx.handle, b"fq_parse_device", v) == 0, gpu.last_error()
    for v in (-1, 2):
        assert set_option(ctx.handle, b"fq_parse_device", v) == gpu.KGX_EINVAL
        assert gpu.last_error() == "fq_parse_device must be 0 or 1"
    ctx.set_option("fq_parse_device", 0)
    # the environment sets a new context's default
    fastq = f2p_restate.fastq_of([(b"r", b"ACGTTGCATTGACCA" * 4)])
    for value, device in (("1", True), ("0", False), ("", False)):
        monkeypatch.setenv("KGX_FQ_PARSE_DEVICE", value)
        with gpu.Context(ctx.image) as c, gpu.FastqToProtein(c) as h:
            h.process(fastq, True)
            assert h.stats()["reads"] == 1
            assert c.stat("fq_parses") == int(device)  # texts framed on the device
    monkeypatch.setenv("KGX_FQ_PARSE_DEVICE", "2")
    with pytest.raises(Exception):
        gpu.Context(ctx.image)
    assert "KGX_FQ_PARSE_DEVICE" in gpu.last_error()
    monkeypatch.delenv("KGX_FQ_PARSE_DEVICE")
