"""oracle.lookup_rollup (the batch entry of the oracle's on_hit, the function
the golden /lookup texts go through) against the interpreted restatement
_on_hit_rollup of test_gpu_tables.py, as bits, on the corpora of the two
rollup tests there: both modes, an empty mapping, hit-free and empty
sequences.  No device."""
import numpy as np
import pytest

from helpers import synthetic_table
from test_gpu_tables import _on_hit_rollup, many_ids_corpus, on_hit_corpus


@pytest.fixture(scope="module")
def world():
    return synthetic_table(60000)


def _check(oracle_lib, hoff, hk, kms, ids, family):
    orc = oracle_lib.Kmap(1 if family else 0)
    if len(kms):
        orc.add(kms, ids)
    roff, rows = oracle_lib.lookup_rollup(orc, hoff, hk, family)
    n = len(hoff) - 1
    assert len(roff) == n + 1 and roff[0] == 0 and len(rows) == int(roff[-1])
    assert rows.dtype == oracle_lib.ROLLUP_DTYPE
    most = 0
    for s in range(n):
        exp = _on_hit_rollup(hk[int(hoff[s]):int(hoff[s + 1])], orc, family)
        got = rows[int(roff[s]):int(roff[s + 1])]
        assert got["id"].tolist() == list(exp.keys()), s
        assert got["hit_count"].tolist() == [v[0] for v in exp.values()], s
        assert got["hit_total"].tolist() == [v[1] for v in exp.values()], s
        w = np.array([v[2] for v in exp.values()], np.float32)
        assert np.array_equal(got["weighted_total"].view(np.uint32), w.view(np.uint32)), s
        most = max(most, len(exp))
    return roff, rows, most


@pytest.mark.parametrize("mode", [0, 1])
def test_lookup_rollup_matches_on_hit_restatement(world, oracle_lib, mode):
    spec, table = world
    seqs, hoff, hk, res, off, kms, ids = on_hit_corpus(spec, table, oracle_lib, mode)
    hits = np.diff(hoff.astype(np.int64))
    assert (hits == 0).sum() >= 3 and b"" in seqs  # empty, 7-residue and hit-free sequences
    roff, rows, most = _check(oracle_lib, hoff, hk, kms, ids, mode == 1)
    assert most > 1 and len(rows) > 100
    assert not np.diff(roff.astype(np.int64))[hits == 0].any()
    if mode == 1:
        assert rows["weighted_total"].min() > 0 and np.array_equal(rows["hit_count"], rows["hit_total"])
    else:
        assert not rows["hit_total"].any() and not rows["weighted_total"].any()
    # an empty mapping: offsets of zeros, no rows
    roff, rows, most = _check(oracle_lib, hoff, hk, np.zeros(0, np.uint64), np.zeros(0, np.uint32), mode == 1)
    assert most == 0 and len(rows) == 0 and not roff.any()
    # no sequences at all
    roff, rows = oracle_lib.lookup_rollup(oracle_lib.Kmap(mode), np.zeros(1, np.uint64), np.zeros(0, np.uint64),
                                          mode == 1)
    assert roff.tolist() == [0] and len(rows) == 0


@pytest.mark.parametrize("family", [False, True])
def test_lookup_rollup_many_ids(world, oracle_lib, family):
    spec, table = world
    seqs, hoff, hk, res, off, kms, ids = many_ids_corpus(spec, table, oracle_lib)
    roff, rows, most = _check(oracle_lib, hoff, hk, kms, ids, family)
    assert most > 400
