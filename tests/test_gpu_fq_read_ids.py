"""kgx_fq_read_ids (csrc/kgx_fq_ids.hip): the ids of chosen reads of a device
parse, gathered on the device, against a numpy gather over the parse's own
arrays (fq_reads_to_host)."""
import numpy as np
import pytest

from helpers import synthetic_table

pytestmark = pytest.mark.gpu

# restated from csrc/kgx_fq_ids.hip: IDS_TILE chosen reads per workgroup of the
# length pass (fq_ids_len_kernel; its four waves of 64 meet in LDS), IDS_GROUP
# lanes move one id in the copy (fq_ids_copy_kernel), and one workgroup of
# SCAN_WG lanes scans the tiles' sums (fq_ids_sums_kernel), looping past
# SCAN_WG tiles
IDS_TILE, IDS_GROUP, SCAN_WG = 256, 16, 256
ID_LENGTHS = (0, 1, 15, 16, 17, 63, 64, 65, 300)
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, IDS_TILE * SCAN_WG + 300)


def _fastq(n, seed):
    """n records whose id lengths run through ID_LENGTHS (shuffled), bases of
    0-40 letters; an id of length 0 is "@ description" """
    rng = np.random.default_rng(seed)
    lens = rng.permutation(np.resize(np.array(ID_LENGTHS), n))
    alpha = np.frombuffer(b"abcdefghijklmnopqrstuvwxyz0123456789_:/.#", np.uint8)
    out = []
    for i, L in enumerate(lens):
        name = bytes(alpha[rng.integers(0, len(alpha), int(L))])
        head = name if L and i % 3 else name + b" some words"
        seq = b"ACGT" * int(rng.integers(0, 11))
        out.append(b"@" + head + b"\n" + seq + b"\n+\n" + b"I" * len(seq) + b"\n")
    return b"".join(out), lens


@pytest.fixture(scope="module")
def parsed(gpu):
    """per read count: a context, its parse and the parse's ids on the host (computed once, never changed)"""
    spec, table = synthetic_table(2000)
    with gpu.Image.from_table(table) as img:
        made = {}
        for n in COUNTS:
            ctx = gpu.Context(img)
            text, lens = _fastq(n, n)
            r = ctx.fq_parse(text)
            assert r.n_reads == n and r.n_id_bytes == int(lens.sum())
            h = ctx.fq_reads_to_host(r, ("ids", "id_offsets"))
            for a in h.values():
                a.setflags(write=False)
            made[n] = (ctx, r, h)
        yield made
        for ctx, _, _ in made.values():
            ctx.close()


def _gather(h, index):
    off = h["id_offsets"].astype(np.int64)
    parts = [h["ids"][off[r]:off[r + 1]] for r in index]
    lens = np.array([len(p) for p in parts], np.uint64)
    return (np.concatenate(parts) if parts else np.zeros(0, np.uint8)), np.concatenate([[0], np.cumsum(lens)])


def _selections(n):
    rng = np.random.default_rng(1000 + n)
    third = np.sort(rng.choice(n, size=max(1, n // 3), replace=False))
    return {"none": [], "all": np.arange(n), "every other": np.arange(0, n, 2), "first": [0], "last": [n - 1],
            "random third": third}


@pytest.mark.parametrize("n", COUNTS)
def test_read_ids_match_numpy_gather(gpu, parsed, n):
    """fails without the feature: no kgx_fq_read_ids"""
    ctx, r, h = parsed[n]
    assert int(h["id_offsets"][n]) == r.n_id_bytes  # the last id ends at n_id_bytes
    for name, index in _selections(n).items():
        got = ctx.fq_read_ids(r, index)
        ids, off = _gather(h, index)
        assert got["n"] == len(index), name
        assert np.array_equal(got["id_offsets"], off.astype(np.uint64)), name
        assert np.array_equal(got["ids"], ids), name


def test_read_ids_every_length_is_there(parsed):
    ctx, r, h = parsed[257]
    assert set(np.diff(h["id_offsets"].astype(np.int64)).tolist()) == set(ID_LENGTHS)


def test_read_ids_refuses_bad_indices_and_stale_reads(gpu, parsed):
    ctx, r, h = parsed[65]
    for bad in ([5, 4], [3, 3], [0, 65], [65]):
        with pytest.raises(gpu.KgxError) as e:
            ctx.fq_read_ids(r, bad)
        assert e.value.code == gpu.KGX_EINVAL, bad
    assert ctx.fq_read_ids(r, [0, 64])["n"] == 2  # and the context goes on


def test_read_ids_refuses_reads_of_an_earlier_parse(gpu):
    spec, table = synthetic_table(2000)
    with gpu.Image.from_table(table) as img, gpu.Context(img) as ctx:
        old = ctx.fq_parse(_fastq(70, 5)[0])
        new = ctx.fq_parse(_fastq(64, 6)[0])
        with pytest.raises(gpu.KgxError) as e:
            ctx.fq_read_ids(old, [0])
        assert e.value.code == gpu.KGX_EINVAL
        assert ctx.fq_read_ids(new, [63])["n"] == 1


def test_read_ids_nothing_after_something(parsed):
    ctx, r, h = parsed[64]
    assert ctx.fq_read_ids(r, np.arange(64))["n"] == 64
    got = ctx.fq_read_ids(r, [])
    assert got["n"] == 0 and got["ids"].size == 0 and got["id_offsets"].tolist() == [0]
