"""The fq handler with option "fq_body_device" (KGX_FQ_BODY_DEVICE=1 when its
context is created): a request's text framed on the device part by part, a
gzip body's blocked members inflated into the parser's text, the printed reads'
ids fetched from the device -- and the same output bytes as the host-framed
handler, the golden text and the oracle."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bgzf_util as bz
from close_kmers_amd import build as kbuild
from close_kmers_amd import image_files
from helpers import GOLDEN, data_dir_for, synthetic_table
from test_oracle_golden import FQ_FILES, case_params

pytestmark = pytest.mark.gpu

FQ = os.path.join(GOLDEN, "fq")
FILES = {k: os.path.join(FQ, v) for k, v in FQ_FILES.items()}

_BACK = {"A": "GCT", "C": "TGT", "D": "GAT", "E": "GAA", "F": "TTT", "G": "GGT", "H": "CAT", "I": "ATT",
         "K": "AAA", "L": "CTT", "M": "ATG", "N": "AAT", "P": "CCT", "Q": "CAA", "R": "CGT", "S": "TCT",
         "T": "ACT", "V": "GTT", "W": "TGG", "Y": "TAT"}


def _want():
    with open(os.path.join(FQ, "expected_fq_default.txt"), "rb") as f:
        return f.read()


@pytest.fixture(scope="module")
def golden_image(gpu):
    with gpu.Image.from_table(image_files.read_image(os.path.join(FQ, "data"))) as img:
        yield img


@pytest.fixture(scope="module")
def synthetic(gpu, oracle_lib, tmp_path_factory):
    """a synthetic image, its data directory and a source of reads that hit it"""
    from close_kmers_amd import synth
    spec, table = synthetic_table(30000)
    d = data_dir_for(str(tmp_path_factory.mktemp("fqbd")), table)
    src = synth.ALPHA[synth.source_residue_codes(np.arange(spec.n_src))].reshape(spec.n_src, -1)

    def hitting(rng, n_res=50):
        p = bytes(src[int(rng.integers(0, spec.n_src))]).decode()
        a = int(rng.integers(0, len(p) - n_res))
        return "".join(_BACK[c] for c in p[a:a + n_res])

    with gpu.Image.from_table(table) as img:
        yield img, d, hitting


def _handler(gpu, monkeypatch, img, data_dir, families=False, device=1):
    monkeypatch.setenv("KGX_FQ_BODY_DEVICE", str(device))  # read when the handler's context is created
    return gpu.FqHandler(img, data_dir, **(FILES if families else {}))


def _in_blocks(fq, body, cuts):
    return b"".join(fq.process(body[a:b], b == len(body)) for a, b in zip(cuts, cuts[1:]))


def _oracle(oracle_lib, tmp_path, data_dir, fastq):
    p = tmp_path / "reads.fq"
    p.write_bytes(fastq)
    return oracle_lib.query_text(data_dir, str(p), "fq", {})


@pytest.mark.parametrize("blocks", ("one", "three", 1, 17, 4096))
def test_golden_with_families(gpu, golden_image, monkeypatch, blocks):
    """fails without the feature: no kgx_fq_stat, and the option is unknown"""
    fastq = bz.golden()
    n = len(fastq)
    cuts = {"one": [0, n], "three": [0, n // 3 + 7, 2 * n // 3 + 3, n]}.get(blocks)
    if cuts is None:
        cuts = list(range(0, n, blocks)) + [n]
    with _handler(gpu, monkeypatch, golden_image, os.path.join(FQ, "data"), families=True) as fq:
        assert _in_blocks(fq, fastq, cuts) == _want()
        assert fq.stat("device_parts") > 0 and fq.stat("reads") > 0 and fq.stat("ids_fetched") > 0
        # the host parses only what the request's last complete record left
        assert fq.stat("host_parts") <= 1
        assert fq.stat("device_members") == 0 and fq.stat("host_members") == 0
        with pytest.raises(gpu.KgxError) as e:
            fq.stat("no_such_counter")
        assert e.value.code == gpu.KGX_EINVAL


def test_option_is_declared_and_off_by_default(gpu, golden_image, monkeypatch):
    monkeypatch.delenv("KGX_FQ_BODY_DEVICE", raising=False)
    with gpu.Context(golden_image) as ctx:
        assert ctx.get_option("fq_body_device") == 0
        ctx.set_option("fq_body_device", 1)
        assert ctx.get_option("fq_body_device") == 1
        with pytest.raises(gpu.KgxError):
            ctx.set_option("fq_body_device", 2)
    with gpu.FqHandler(golden_image, os.path.join(FQ, "data"), **FILES) as fq:
        assert fq.process(bz.golden(), True) == _want()
        assert fq.stat("device_parts") == 0 and fq.stat("host_parts") > 0 and fq.stat("ids_fetched") == 0
    monkeypatch.setenv("KGX_FQ_BODY_DEVICE", "2")
    with pytest.raises(gpu.KgxError):
        gpu.Context(golden_image)


@pytest.mark.parametrize("families", (True, False))
@pytest.mark.parametrize("part_kb", (4, 5))
def test_small_parts(gpu, oracle_lib, golden_image, monkeypatch, tmp_path, part_kb, families):
    """parts of one parser tile (4,096 bytes, the minimum) and of a tile and a
    quarter: many parts, carried text crossing the tile boundary"""
    fastq = bz.golden()
    data = os.path.join(FQ, "data")
    want = _want() if families else _oracle(oracle_lib, tmp_path, data, fastq)
    assert want.count(b"\n") > 10
    monkeypatch.setenv("KGX_FQ_PART_KB", str(part_kb))
    with _handler(gpu, monkeypatch, golden_image, data, families=families) as fq:
        assert fq.process(fastq, True) == want
        assert fq.stat("device_parts") >= len(fastq) // (part_kb << 10)
        assert 0 < fq.stat("tail_bytes_max") < 4096


def test_record_longer_than_a_part(gpu, oracle_lib, synthetic, monkeypatch, tmp_path):
    """one read of 20,000 bases between ordinary ones at parts of 4 KiB: parts
    that hold no complete record, and the room doubling until one does"""
    img, d, hitting = synthetic
    rng = np.random.default_rng(5)
    recs = []
    for i in range(120):
        seq = hitting(rng) if i != 60 else "".join(hitting(rng) for _ in range(134))[:20000]
        recs.append(f"@r{i}\n{seq}\n+\n{'I' * len(seq)}\n")
    assert len(recs[60]) > 40000
    fastq = "".join(recs).encode()
    want = _oracle(oracle_lib, tmp_path, d, fastq)
    assert b"r60\t" in want and want.count(b"\n") > 60
    monkeypatch.setenv("KGX_FQ_PART_KB", "4")
    with _handler(gpu, monkeypatch, img, d) as fq:
        assert fq.process(fastq, True) == want
        assert fq.stat("tail_bytes_max") >= 32768  # a part of 32 KiB held no complete record


def test_irregular_text(gpu, oracle_lib, synthetic, monkeypatch, tmp_path):
    img, d, hitting = synthetic
    rng = np.random.default_rng(31)
    recs = []
    for i in range(3000):
        seq = hitting(rng) if i % 3 else "".join("ACGT"[x] for x in rng.integers(0, 4, 150))
        qual = "I" * len(seq)
        head = f"r{i}"
        if i % 97 == 0:
            qual = "@" + qual[1:]          # a quality line that looks like a header
        if i % 101 == 0:
            head += "\tsome description"
        if i % 103 == 0:
            seq = seq[:40].lower() + "N1-" + seq[40:]
        if i % 113 == 5:
            head = " desc"                 # "@ desc": an empty id
        blank = "\n" if i % 107 == 0 else ""
        nl = "\r\n" if i % 109 == 0 else "\n"
        recs.append(f"{blank}@{head}{nl}{seq}{nl}+{nl}{qual}{nl}")
    body = "".join(recs)
    ends = {"no final newline": body + f"@last\n{hitting(rng)}\n+\nIIII",
            "an id and no bases": body + "@lonely"}
    monkeypatch.setenv("KGX_FQ_PART_KB", "64")
    with _handler(gpu, monkeypatch, img, d) as fq:
        for name, text in ends.items():
            fastq = text.encode()
            want = _oracle(oracle_lib, tmp_path, d, fastq)
            assert want.count(b"\n") > 1500
            assert fq.process(fastq, True) == want, name
            cuts = [0] + sorted(int(x) for x in rng.integers(1, len(fastq), 12)) + [len(fastq)]
            assert _in_blocks(fq, fastq, cuts) == want, name
        assert fq.stat("device_parts") > 20


def test_fooled_cut_text(gpu, oracle_lib, synthetic, monkeypatch, tmp_path):
    """quality lines that start with '@' and sequence lines that start with '+':
    what fools a search for record starts does not concern plain byte cuts"""
    img, d, hitting = synthetic
    rng = np.random.default_rng(77)
    recs = []
    for i in range(600):
        seq = hitting(rng)
        recs.append(f"@q{i}\n+{seq}\n+\n@{'I' * len(seq)}\n")
    fastq = "".join(recs).encode()
    want = _oracle(oracle_lib, tmp_path, d, fastq)
    assert want.count(b"\n") > 100
    with _handler(gpu, monkeypatch, img, d) as fq:
        for kb in ("16", "40"):
            monkeypatch.setenv("KGX_FQ_PART_KB", kb)
            assert fq.process(fastq, True) == want, kb


def test_empty_bodies(gpu, golden_image, monkeypatch):
    with _handler(gpu, monkeypatch, golden_image, os.path.join(FQ, "data"), families=True) as fq:
        assert fq.process(b"", True) == b""
        assert fq.process(b"\n", True) == b""
        assert fq.process(bz.golden(), True) == _want()
        assert fq.process(b"", False) == b"" and fq.process(b"", True) == b""
        assert fq.process(bz.golden(), True) == _want()


def _bodies():
    g = bz.golden()
    return {"plain": gzip.compress(g), "bgzf_65280": bz.bgzf(g), "bgzf_1000": bz.bgzf(g, chunk=1000)}


@pytest.mark.parametrize("body", ("plain", "bgzf_65280", "bgzf_1000"))
def test_gzip_bodies(gpu, golden_image, monkeypatch, body):
    gz = _bodies()[body]
    members = gpu.gunzip_scan(gz)["members"]
    with _handler(gpu, monkeypatch, golden_image, os.path.join(FQ, "data"), families=True) as fq:
        assert fq.process(gz, True) == _want()
        if body == "plain":
            assert fq.stat("device_members") == 0 and fq.stat("host_members") == 1
        else:
            assert fq.stat("device_members") == members > 1 and fq.stat("host_members") == 0
        parts = fq.stat("device_parts")
        assert parts > 0
        # text after gzip and gzip after text, on one handler
        assert fq.process(bz.golden(), True) == _want()
        assert fq.process(gz, True) == _want()
        assert fq.stat("device_parts") > 2 * parts - 1


@pytest.mark.parametrize("step", (1, 17, 4096))
def test_bgzf_in_blocks(gpu, golden_image, monkeypatch, step):
    gz = _bodies()["bgzf_1000"]
    with _handler(gpu, monkeypatch, golden_image, os.path.join(FQ, "data"), families=True) as fq:
        assert _in_blocks(fq, gz, list(range(0, len(gz), step)) + [len(gz)]) == _want()
        assert fq.stat("device_members") == gpu.gunzip_scan(gz)["members"] and fq.stat("host_members") == 0


def test_bgzf_small_parts(gpu, golden_image, monkeypatch):
    """parts of 4 KiB over members of 1,000 bytes: several members to a part,
    the carried text copied on the device from one part's buffer to the next"""
    monkeypatch.setenv("KGX_FQ_PART_KB", "4")
    gz = _bodies()["bgzf_1000"]
    with _handler(gpu, monkeypatch, golden_image, os.path.join(FQ, "data"), families=True) as fq:
        assert fq.process(gz, True) == _want()
        assert fq.stat("device_parts") >= 4 and fq.stat("tail_bytes_max") > 0


def test_bad_member_reads_as_with_the_host_path(gpu, golden_image, monkeypatch):
    member, reason = bz.error_cases()["crc_bit"]
    bad = bz.bgzf(b"@r\nACGT\n+\nIIII\n", eof=False) + member
    said = {}
    for device in (0, 1):
        with _handler(gpu, monkeypatch, golden_image, os.path.join(FQ, "data"), families=True, device=device) as fq:
            with pytest.raises(gpu.KgxError) as e:
                fq.process(bad, True)
            assert e.value.code == gpu.KGX_EFORMAT
            said[device] = str(e.value)
            assert fq.process(_bodies()["bgzf_1000"], True) == _want()  # the next request is served
            assert fq.process(bz.golden(), True) == _want()
    assert said[0] == said[1] and "member 1:" in said[1] and f"reason {reason}" in said[1]


def test_query_tool_and_server(gpu, monkeypatch, tmp_path):
    from test_server import HEADER, Server
    monkeypatch.setenv("KGX_FQ_BODY_DEVICE", "1")
    p = tmp_path / "reads.fastq.gz"
    p.write_bytes(_bodies()["bgzf_1000"])
    args = [kbuild.QUERY, os.path.join(FQ, "data"), str(p), "fq"]
    args += [f"{k}={v}" for k, v in case_params("fq", "default").items()]
    r = subprocess.run(args, capture_output=True, timeout=300, env=dict(os.environ, KGX_FQ_TIMING="1"))
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == _want()
    assert b"framed on the device" in r.stderr
    srv = Server(os.path.join(FQ, "data"), family_db=True)
    try:
        assert srv.request("POST", "/fq_lookup", bz.golden()) == HEADER + _want()
        assert srv.request("POST", "/fq_lookup", _bodies()["bgzf_1000"]) == HEADER + _want()
    finally:
        srv.close()
