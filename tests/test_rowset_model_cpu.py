"""The host model of the row-set contract (tests/rowset_model.py), checked without a GPU: its answers against the oracle asked
another way, its bookkeeping against the expected tuples of tests/test_update.py::test_the_limit_is_shared_with_the_tail and
tests/test_append.py::test_pieces_reindex_and_limit, and the walks of tests/test_rowset_formats.py for what they must cross."""
import numpy as np
import pytest

import hvs_testlib as T
import rowset_model as R
import test_update as U

PKG = R.PKG
SEEDS, WALK_STEPS = R.WALK_SEEDS, R.WALK_STEPS                      # the walks of tests/test_rowset_formats.py::test_the_walk
N = 1 << 17


def test_expected_maps_ids_through_live_and_pads_from_the_last_live_rows():
    """5003 rows; dead: every seventh row, a block in the middle and the last 300 (the padding ids move).  The model's answer is
    compared with the oracle asked another way -- on all rows, the dead ones moved out of every predicate and far away, which
    leaves ids as they are -- distance by distance where a query has k matches, and as its matches plus the last live ids where it has fewer."""
    n, ncat = 5003, 10
    rows = T.gen_data(n, 71, T.GEN_V1, ncat)
    queries = np.concatenate([T.gen_queries(160, 72, T.GEN_V1, ncat), T.gen_queries(32, 73, T.GEN_V1, ncat, force_type=3)])
    queries[-6:-3, 0] = 7.0                                         # invalid types: all padding
    queries[-3:, 0] = -5.0
    live = np.ones(n, bool)
    live[::7] = False
    live[2000:2300] = False
    live[n - 300:] = False
    for k in (100, 8, 256):
        m = R.RowSetModel(rows, k)
        m.set_mask(live)
        lv = np.flatnonzero(live)
        pad = m.pad_ids()
        assert np.array_equal(pad, lv[::-1][:k]) and pad[0] == n - 301
        for sp in (1.0, 0.5):
            want = m.expected(queries, sp)
            per_query = m.pairs_per_query(queries, sp)
            n_live, cut, _ = PKG.mask_plan(live, k, sp)
            assert n_live == lv.size and int((lv < cut).sum()) == int(T.oracle().hvs_oracle_sn(sp, n_live))
            assert live[want].all(), "a dead id in the model's answer"
            # the other way: D with the rows at and behind the cut and the dead rows made unmatchable (type 0 matches every row:
            # those queries are compared through their distances below)
            other = rows.copy()
            gone = ~live | (np.arange(n) >= cut)
            other[gone, 0], other[gone, 1] = np.float32(-7.0), np.float32(-7.0)
            other[gone, 2:] = np.float32(1e6)
            with T.oracle_k(k):
                ref, _ = T.oracle_query(other, queries, 1.0)
                d_want = T.oracle_dists_for_ids(rows, queries, want)
                d_ref = T.oracle_dists_for_ids(rows, queries, ref)
            some_full = 0
            for q in range(queries.shape[0]):
                matches = min(int(per_query[q]), k)
                typ0 = -1.0 < queries[q, 0] < 1.0
                if typ0:
                    assert matches == k and not gone[want[q]].any()
                if matches == k or typ0:                            # every slot is a match: the same rows at the same distances
                    assert np.array_equal(d_want[q].view(np.uint32), d_ref[q].view(np.uint32)), (k, sp, q)
                    assert np.array_equal(np.sort(want[q][d_want[q] < d_want[q][-1]]), np.sort(ref[q][d_ref[q] < d_ref[q][-1]])), (k, sp, q)
                    some_full += 1
                else:           # the same matches plus live[n_live-1], live[n_live-2], ... (a multiset), in ascending distance
                    found = ref[q][~gone[ref[q]]]
                    assert found.size == matches and np.all(np.diff(d_want[q]) >= 0), (k, sp, q)
                    assert sorted(want[q].tolist()) == sorted(found.tolist() + pad[:k - matches].tolist()), (k, sp, q)
            assert some_full and (per_query < k).sum() >= 6
            assert np.array_equal(np.sort(want[-1]), np.sort(pad)) and np.array_equal(np.sort(want[-4]), np.sort(pad))   # all padding
            assert m.pairs(queries, sp) == int(per_query.sum())


def test_bookkeeping_follows_the_expected_tuples_of_the_limit_tests():
    """The sequences and the expected tuples are those of test_update.py::test_the_limit_is_shared_with_the_tail and
    test_append.py::test_pieces_reindex_and_limit (their GPU runs assert the same figures of the library)."""
    one = np.zeros((1, 1), np.float32)

    def rows(count):
        return np.repeat(one, count, axis=0)

    m = R.RowSetModel(np.zeros((N, 1), np.float32), 100, 500)
    s = U.stale_ids(300)
    m.update(s, rows(300))
    assert m.append(rows(100)) == N
    assert (m.n_stale, m.tail_limit, m.n_tail, m.n_indexed, m.reindexes) == (300, 500, 100, N, 0)
    m.update(s[::-1], rows(300))                                    # all stale already: the set does not grow
    assert (m.n_stale, m.n_tail, m.reindexes) == (300, 100, 0)
    s2 = np.setdiff1d(U.stale_ids(600), s)[:200].astype(np.uint32)
    m.update(s2, rows(200))                                         # 300 + 200 + 100 > 500
    assert (m.n_stale, m.n_tail, m.n_indexed, m.reindexes) == (0, 0, N + 100, 1)
    m.update(s[:250], rows(250))
    m.append(rows(100))                                             # 250 + 100 stay
    assert (m.n_stale, m.n_tail, m.reindexes) == (250, 100, 1)
    m.append(rows(200))                                             # 250 + 300 > 500
    assert (m.n_stale, m.n_tail, m.reindexes) == (0, 0, 2)
    assert m.stats() == (N + 400, 0, 0, 2)
    # test_append.py: the limit alone, and the default rule
    m = R.RowSetModel(np.zeros((N, 1), np.float32), 100, 512)
    m.append(rows(400))
    assert (m.n_tail, m.n_indexed, m.reindexes, m.tail_limit) == (400, N, 0, 512)
    m.append(rows(200))
    assert (m.n_tail, m.n_indexed, m.reindexes) == (0, N + 600, 1)
    m.set_tail_limit(0)
    assert m.tail_limit == max(4096, (N + 600) >> 10)
    m.reindex()                                                     # nothing to fold in: a no-op
    assert m.reindexes == 1
    # tail rows are never stale; a dead row that is updated is stale and stays dead; `patched` counts ids below n_indexed once
    m = R.RowSetModel(np.zeros((5000, 1), np.float32), 100, 1 << 30)
    m.append(rows(10))
    m.delete([3, 4, 5003])
    m.update(np.array([4, 9, 5001, 5003, 9], np.uint32), rows(5))
    assert m.stale.tolist() == [4, 9] and m.n_dead == 3 and m.patched == 2 * 3      # ids 3, 4, 9
    with pytest.raises(ValueError):
        m.delete([5010])
    with pytest.raises(ValueError):
        m.set_k(257)
    assert m.n_dead == 3 and m.k == 100
    # a compaction is a fold that also drops the mask; without a dead row it is nothing
    new_to_old = m.compact()
    assert np.array_equal(new_to_old, np.setdiff1d(np.arange(5010), [3, 4, 5003]))
    assert (m.n, m.n_dead, m.compactions) + m.stats() == (5007, 0, 1, 5007, 0, 0, 1)
    assert np.array_equal(m.compact(), np.arange(5007)) and (m.compactions, m.reindexes) == (1, 1)


@pytest.mark.parametrize("seed", SEEDS)
def test_every_walk_crosses_what_it_is_for(seed):
    """Conditions, not measurements: a seed that misses one is replaced."""
    ops = R.walk(seed, WALK_STEPS)
    assert len(ops) == WALK_STEPS
    again = R.walk(seed, WALK_STEPS)                                # seeded: the same walk every time
    assert [o[0] for o in ops] == [o[0] for o in again] and all(np.array_equal(a[1], b[1]) for a, b in zip(ops, again) if len(a) > 1)
    c = R.coverage(ops)
    print(seed, c, [o[0] for o in ops])
    assert c["append_folds"] >= 1
    assert c["update_folds"] >= 1
    assert c["compactions_with_tail_and_stale"] >= 1
    assert c["revivals_while_stale"] >= 1
    assert c["format_changes_with_all_three"] >= 2
    assert c["set_k_under_a_mask"] >= 1
    assert c["sampled_queries_under_a_mask"] >= 1
    assert c["min_live"] >= R.WALK_MIN_LIVE and c["min_n"] >= R.MIN_ROWS
    for op in ops:                                                  # the ranges of the moves
        if op[0] == "delete":
            assert 1 <= op[1].size <= 2000
        if op[0] == "append":
            assert 1 <= op[2] <= 600
        if op[0] == "update":
            assert 1 <= op[1].size <= 300
