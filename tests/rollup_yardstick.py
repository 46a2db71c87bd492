"""The yardstick of the /lookup rollup tests: the oracle's hits
(oracle.process_batch, want 1) through oracle.lookup_rollup, which is
LookupRequest::on_hit (lookup_request.cc:446-482) -- the function the golden
/lookup texts go through -- and the comparison every rollup test makes with
it: offsets, id, hit_count, hit_total and the bits of weighted_total, for
every sequence."""
import numpy as np


def oracle_kmap(oracle_lib, kms, ids, family):
    """kmer_to_family_id_ (set) in family mode, kmer_to_id_ (append) in peg mode"""
    orc = oracle_lib.Kmap(1 if family else 0)
    orc.add(kms, ids)
    return orc


def expected(oracle_lib, table, res, off, kms, ids, family):
    """(row offsets, rows) of the batch (res, off) over the pairs (kms, ids)"""
    r = oracle_lib.process_batch(table, res, off, want=1)
    return oracle_lib.lookup_rollup(oracle_kmap(oracle_lib, kms, ids, family), r.hit_offsets,
                                    r.hits["which_kmer"], family)


def assert_rows(got_off, got_rows, want_off, want_rows, what=""):
    got_off, want_off = np.asarray(got_off, np.uint64), np.asarray(want_off, np.uint64)
    assert len(got_off) == len(want_off), (what, len(got_off), len(want_off))
    if not np.array_equal(got_off, want_off):
        s = int(np.nonzero(np.diff(got_off.astype(np.int64)) != np.diff(want_off.astype(np.int64)))[0][0])
        raise AssertionError((what, "row count of sequence", s, int(got_off[s + 1] - got_off[s]),
                              int(want_off[s + 1] - want_off[s])))
    assert len(got_rows) == len(want_rows) == int(want_off[-1]), what
    eq = np.ones(len(want_rows), bool)
    for f in ("id", "hit_count", "hit_total"):
        eq &= got_rows[f] == want_rows[f]
    eq &= (np.ascontiguousarray(got_rows["weighted_total"]).view(np.uint32)
           == np.ascontiguousarray(want_rows["weighted_total"]).view(np.uint32))
    if not eq.all():
        r = int(np.nonzero(~eq)[0][0])
        s = int(np.searchsorted(want_off, r, side="right") - 1)
        raise AssertionError((what, "sequence", s, "row", r - int(want_off[s]), got_rows[r], want_rows[r],
                              int((~eq).sum()), "rows differ"))
