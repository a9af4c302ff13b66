"""The inputs of tests/test_exclude_edges.py are not trivial: shown by the model alone (tests/exclude_edges.py, tests/exclude_model.py),
without a GPU."""
import numpy as np

import exclude_edges as E
import exclude_model as X


def test_many_batches_inputs_are_not_trivial():
    nodes, queries = E.workload()
    assert queries.shape[0] == E.NQ and E.NQ >= 8 * E.BATCH and E.NQ % E.BATCH != 0      # at least 8 batches, the last one ragged
    lists = E.lists()
    assert all(l.size <= X.EXCLUDE_MAX for l in lists)
    for q in range(E.NQ - 1):                                    # neighbours never share a list
        assert q % 5 == 3 or (q + 1) % 5 == 3 or lists[q].size != lists[q + 1].size or lists[q].size == 0 or (lists[q] != lists[q + 1]).any()
    for b in range(0, E.NQ - E.BATCH, E.BATCH):                   # nor do the queries at the same place of neighbouring batches
        same = sum(lists[q].size == lists[q + E.BATCH].size and (lists[q] == lists[q + E.BATCH]).all() and lists[q].size > 0 for q in range(b, b + E.BATCH) if q + E.BATCH < E.NQ)
        assert same <= 2, (b, same)
    for k in E.KS:
        with_l, plain = E.answers(k, False), E.answers(k, False, with_lists=False)
        differs = (with_l[0] != plain[0]).any(1)
        underfull = with_l[2] < k
        print("k %3d: %4d of %d answers differ from the plain ones, %4d under-full (plain: %d)" % (k, differs.sum(), E.NQ, underfull.sum(), (plain[2] < k).sum()))
        assert differs.sum() >= 0.10 * E.NQ and underfull.sum() >= 0.10 * E.NQ, (k, differs.sum(), underfull.sum())
        for rule in (0, 1, 2):                                    # every rule that names matched rows changes answers
            assert differs[rule::5].sum() >= 20, (k, rule)
        assert not differs[3::5].any() and not differs[4::5].any()
        # a list read one query, one wave or one batch off gives another answer for most queries
        for shift in (1, 64, E.BATCH):
            moved = [lists[(q + shift) % E.NQ] for q in range(E.NQ)]
            other = X.answers(E.fulls(), moved, k)
            assert ((other[0] != with_l[0]).any(1)).sum() >= 0.10 * E.NQ, (k, shift)


def test_inner_ranges_and_compaction_inputs():
    for q0, m in E.RANGES + (E.STRADDLE,):
        assert 0 < q0 and q0 + m <= E.NQ
    assert E.RANGES[0][0] % 64 != 0 and E.RANGES[1][0] % E.BATCH == 0 and E.RANGES[2][0] + E.RANGES[2][1] == E.NQ
    q0, m = E.STRADDLE
    assert q0 < E.NQ // 3 < (2 * E.NQ + 2) // 3 < q0 + m          # both owner boundaries of three GPUs lie inside
    dead, new_to_old, rows = E.compaction()
    assert dead.size == E.N // 20 and rows.shape[0] == E.N - dead.size
    lists = E.lists()[:E.NQ_COMPACT]
    named = np.unique(np.concatenate(lists))
    named = named[named < E.N]
    # the lists name rows that the compaction renumbers: the same numeric id is another row afterwards
    assert (new_to_old[named[named < rows.shape[0]]] != named[named < rows.shape[0]]).mean() > 0.9
