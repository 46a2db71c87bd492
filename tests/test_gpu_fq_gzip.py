"""gzip bodies through the fq handler: kgx_fq_process, kgx_query ... fq and a
live kgx_server's POST /fq_lookup give for a .gz or BGZF body the text they
give for the FASTQ itself."""
import gzip
import os
import subprocess

import pytest

import bgzf_util as bz
from close_kmers_amd import build as kbuild
from close_kmers_amd import image_files
from helpers import GOLDEN
from test_oracle_golden import FQ_FILES, case_params

pytestmark = pytest.mark.gpu

FQ = os.path.join(GOLDEN, "fq")


def _want():
    with open(os.path.join(FQ, "expected_fq_default.txt"), "rb") as f:
        return f.read()


def _bodies():
    g = bz.golden()
    return {"plain": gzip.compress(g), "bgzf_65280": bz.bgzf(g), "bgzf_1000": bz.bgzf(g, chunk=1000)}


@pytest.fixture(scope="module")
def handler(gpu):
    table = image_files.read_image(os.path.join(FQ, "data"))
    files = {k: os.path.join(FQ, v) for k, v in FQ_FILES.items()}
    with gpu.Image.from_table(table) as img, gpu.FqHandler(img, os.path.join(FQ, "data"), **files) as fq:
        yield gpu, fq


@pytest.mark.parametrize("gunzip_device", (1, 0))
@pytest.mark.parametrize("body", ("plain", "bgzf_65280", "bgzf_1000"))
def test_fq_process_gzip_matches_golden(gpu, body, gunzip_device, monkeypatch):
    """fails without the feature: a gzip body parsed as FASTQ text is garbage"""
    monkeypatch.setenv("KGX_GUNZIP_DEVICE", str(gunzip_device))  # read when a context is created
    table = image_files.read_image(os.path.join(FQ, "data"))
    files = {k: os.path.join(FQ, v) for k, v in FQ_FILES.items()}
    with gpu.Image.from_table(table) as img, gpu.FqHandler(img, os.path.join(FQ, "data"), **files) as fq:
        assert fq.process(_bodies()[body], True) == _want()
        # the handler starts the next request afresh: text after gzip, gzip after text
        assert fq.process(bz.golden(), True) == _want()
        assert fq.process(_bodies()[body], True) == _want()


@pytest.mark.parametrize("step", (1, 17, 4096))
def test_fq_process_gzip_in_blocks(handler, step):
    """the compressed body in blocks of `step` bytes: the first block of one
    byte is held until the sniff can tell, the handler inflates whole members
    only, reads cut by a member's end are carried by the parser as in a text
    request, and the output equals the one-block output"""
    gpu, fq = handler
    gz = bz.bgzf(bz.golden(), chunk=1000)
    blocks = [gz[i:i + step] for i in range(0, len(gz), step)]
    got = b"".join(fq.process(b, i == len(blocks) - 1) for i, b in enumerate(blocks))
    assert got == _want()


def test_fq_process_bad_gzip_is_eformat_and_the_handler_goes_on(handler):
    gpu, fq = handler
    member, reason = bz.error_cases()["crc_bit"]
    with pytest.raises(gpu.KgxError) as e:
        fq.process(bz.bgzf(b"@r\nACGT\n+\nIIII\n", eof=False) + member, True)
    assert e.value.code == gpu.KGX_EFORMAT and "member 1:" in str(e.value) and f"reason {reason}" in str(e.value)
    assert fq.process(_bodies()["bgzf_1000"], True) == _want()


def test_query_tool_reads_gz(gpu, tmp_path):
    for name, body in _bodies().items():
        p = tmp_path / f"{name}.fastq.gz"
        p.write_bytes(body)
        args = [kbuild.QUERY, os.path.join(FQ, "data"), str(p), "fq"]
        args += [f"{k}={v}" for k, v in case_params("fq", "default").items()]
        r = subprocess.run(args, capture_output=True, timeout=300)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout == _want(), name


def test_server_fq_lookup_takes_gzip(gpu):
    from test_server import HEADER, Server
    srv = Server(os.path.join(FQ, "data"), family_db=True)
    try:
        text = srv.request("POST", "/fq_lookup", bz.golden())
        assert text == HEADER + _want()
        for name, body in _bodies().items():
            assert srv.request("POST", "/fq_lookup", body) == text, name
        # a corrupt body: the router's error response, not a 200 header and nothing
        member, reason = bz.error_cases()["crc_bit"]
        bad = srv.request("POST", "/fq_lookup", bz.bgzf(b"@r\nACGT\n+\nIIII\n", eof=False) + member)
        assert bad.startswith(b"HTTP/1.1 500 Failed"), bad[:80]
        assert b"Caught exception" in bad and b"CRC-32 mismatch" in bad
        assert b"200 OK" not in bad
        cut = srv.request("POST", "/fq_lookup", _bodies()["plain"][:-20])
        assert cut.startswith(b"HTTP/1.1 500 Failed") and b"cut short" in cut
        # and the server answers the next request
        assert srv.request("POST", "/fq_lookup", _bodies()["bgzf_1000"]) == text
    finally:
        srv.close()
