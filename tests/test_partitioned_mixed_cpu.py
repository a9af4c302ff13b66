"""The data sets of tests/partition_sets.py have the properties the GPU cases of tests/test_partitioned_mixed.py rely on: part
sizes on either side of the per-part thresholds, cuts with the intended relation to a quarter of a part, hand-placed categories
split over the parts as listed, under-full queries where a case relies on padding, non-finite rows in one part only, queries
far outside one part's box but inside the whole D's, a tie group with members in every part.  No GPU."""
import importlib

import numpy as np
import pytest

import hvs_testlib as T
import partition_sets as S

PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
MFMA_MIN_ROWS, INDEX_MIN_ROWS = 32768, 4096                          # kMfmaMinRows, kIndexMinRows (csrc/hvs.hip)


def build_all():
    out = {n: S.build_a(n) for n in S.A_ROW0}
    out.update(B=S.build_b(), C=S.build_c(), D=S.build_d())
    return out


@pytest.fixture(scope="module")
def sets():
    return build_all()


def sn_of(sp, n):
    return int(T.oracle().hvs_oracle_sn(sp, n))


@pytest.mark.parametrize("n, sizes, edge", [(98303, (32768, 32768, 32767), MFMA_MIN_ROWS), (65535, (32768, 32767), MFMA_MIN_ROWS),
                                            (12287, (4096, 4096, 4095), INDEX_MIN_ROWS)])
def test_part_sizes_straddle_the_thresholds(n, sizes, edge):
    row0, sn, local = PKG.partition_plan(n, len(sizes), max(S.A_KS), 1.0)
    assert tuple(np.diff(row0).tolist()) == sizes and tuple(row0.tolist()) == S.A_ROW0[n]
    assert sn == n and local.tolist() == list(sizes)
    assert all(s >= edge for s in sizes[:-1]) and sizes[-1] < edge <= n
    assert max(S.A_KS) <= sizes[-1]


@pytest.mark.parametrize("n", list(S.A_ROW0))
def test_cuts_of_set_a(n):
    """sp[1]: inside the last part, its prefix above a quarter of it; sp[2]: inside it and below a quarter; sp[3]: inside part 0"""
    P = len(S.A_ROW0[n]) - 1
    size = np.diff(S.A_ROW0[n])
    sps = S.A_SPS[n]
    assert sps[0] == 1.0
    for k in S.A_KS:
        _, sn, local = PKG.partition_plan(n, P, k, sps[1])
        assert sn == sn_of(sps[1], n) and (local[:-1] == size[:-1]).all() and size[-1] // 4 < local[-1] < size[-1]
        _, sn, local = PKG.partition_plan(n, P, k, sps[2])
        assert (local[:-1] == size[:-1]).all() and 0 < local[-1] < size[-1] // 4
        _, sn, local = PKG.partition_plan(n, P, k, sps[3])
        assert 0 < local[0] == sn < size[0] and (local[1:] == 0).all()
        assert local[0] >= size[0] // 4                             # (part 0 keeps its engine; the other parts launch nothing)


def test_hand_placed_categories(sets):
    for n in S.A_ROW0:
        a = sets[n]
        got = {c: S.matches_per_part(a["nodes"], a["row0"], c) for c in a["cats"]}
        last = len(a["row0"]) - 2
        assert got[1001][0] == 30 and got[1001][last] == 40 and sum(got[1001]) == 70
        assert got[1002][last] == 45 and sum(got[1002]) == 45
    b = sets["B"]
    for cat, counts in S.B_SPLIT.items():
        assert S.matches_per_part(b["nodes"], b["row0"], cat) == counts
    assert sorted(S.B_SPLIT.values()) == sorted([(5, 0, 60), (33, 33, 34), (0, 99, 0), (0, 0, 150)])
    assert len(b["special"]) == 12 and all((b["queries"][q, 1] in S.B_SPLIT) for q in b["special"])
    assert {q // 400 for q in b["special"]} == {0, 1, 2}
    c = sets["C"]
    assert S.matches_per_part(c["nodes"], c["row0"], 2001) == (30, 0, 50)
    assert S.matches_per_part(c["nodes"], c["row0"], 2002) == (80, 0, 150)
    assert S.matches_per_part(c["nodes"], c["row0"], 2003) == (0, 0, 60)
    assert S.matches_per_part(c["nodes"], c["row0"], 2004) == (0, 0, 30)


def test_under_full_queries_where_a_case_relies_on_padding(sets):
    for n in S.A_ROW0:
        a = sets[n]
        for sp in a["sps"]:
            m = S.passing(a["nodes"], a["queries"], sn_of(sp, n))
            for k in S.A_KS:
                assert 0 < int((m < k).sum()) < len(m), (n, sp, k)
    b = sets["B"]
    for k, sp in ((100, 1.0), (256, 1.0), (37, 0.5), (37, 1.0), (37, 0.9), (100, 0.9)):
        m = S.passing(b["nodes"], b["queries"], sn_of(sp, S.N3))
        assert 0 < int((m < k).sum()) < len(m), (k, sp)
    c = sets["C"]
    q2001, q2002 = 200, 202                                         # the type-1 queries on 2001 and 2002
    assert c["queries"][q2001, :2].tolist() == [1, 2001] and c["queries"][q2002, :2].tolist() == [1, 2002]
    m = S.passing(c["nodes"], c["queries"], S.N3)
    assert m[q2001] == 80 and m[q2002] == 230                       # under-full at k = 100; over-full at 100, under-full at 256
    for sp in c["sps"]:
        m = S.passing(c["nodes"], c["queries"], sn_of(sp, S.N3))
        assert all(0 < int((m < k).sum()) < len(m) for k in (100, 256))
        assert 30 < m[q2001] < 100 and 100 < m[q2002] < 256, "the cut must leave NaN-distance keys of part 2 in both lists"


def test_non_finite_rows_lie_in_part_2_only(sets):
    c = sets["C"]
    nodes = c["nodes"]
    big = np.abs(nodes[:, 2:]).max(1)
    with np.errstate(invalid="ignore"):
        bad = ~np.isfinite(nodes).all(1) | (big > 1e30)
    assert np.array_equal(np.flatnonzero(bad), c["bad_rows"])
    assert len(c["bad_rows"]) == 50 + 150 + 60 + 30 + 20 and c["bad_rows"].min() >= S.ROW0_3[2]
    assert int(np.isnan(nodes[:, 1]).sum()) == S.C_NAN_T
    for cat, (cnt, val) in S.C_BAD.items():
        rows = nodes[nodes[:, 0] == cat]
        hit = np.isnan(rows[:, 2:]).any(1) if np.isnan(val) else (rows[:, 2:] == np.float32(val)).any(1)
        assert int(hit.sum()) == cnt
    sn = sn_of(0.9, S.N3)
    assert S.ROW0_3[2] < sn < S.N3 and 0 < int((c["bad_rows"] < sn).sum()) < len(c["bad_rows"])
    q = c["queries"]
    assert np.isinf(q[-3, 4:]).sum() == 1 and np.isnan(q[-2, 4:]).sum() == 1 and (q[-1, 4:] == np.float32(1e30)).sum() == 1


def test_x3_queries_leave_part_0s_box_and_stay_inside_the_whole(sets):
    """Part 0's box is [-6, 6)^100 and the x 3 queries lie in [-18, 18)^100, so a component can leave part 0's [min, max] by at
    most one width of that dimension (12 of 12); "far outside" is asserted as: every x 3 query has a component more than HALF a
    width outside (|x| > 12: a third of all components; the library's test of the mid-call format change uses the same factor),
    and some reach beyond 0.95 widths.  None leaves the whole D's per-dimension [min, max], nor part 1's."""
    b = sets["B"]
    q, nodes, r = b["queries"][b["x3"], 4:], b["nodes"], b["row0"]
    ex = S.excess_over_box(q, nodes[r[0]:r[1], 2:])
    print("x 3 queries, largest excess over part 0's box in widths: min %.3f median %.3f max %.3f" % (ex.min(), np.median(ex), ex.max()))
    assert ex.min() > 0.5 and ex.max() > 0.95
    assert S.excess_over_box(q, nodes[:, 2:]).max() == 0.0
    assert S.excess_over_box(q, nodes[r[1]:r[2], 2:]).max() == 0.0
    own = S.excess_over_box(b["queries"][:400, 4:], nodes[r[0]:r[1], 2:])
    assert own.max() < 0.01, "the gen-v1 queries lie inside part 0's box (up to its sampling)"
    assert len(b["queries"]) == 1200 and len(nodes) == S.N3


def test_tie_group_of_set_d(sets):
    d = sets["D"]
    nodes, r, base = d["nodes"], d["row0"], d["base"]
    same = (nodes[:, 2:].view(np.uint32) == base[2:].view(np.uint32)).all(1)
    per_part = [int(same[r[i]:r[i + 1]].sum()) for i in range(3)]
    size1 = r[2] - r[1]
    assert per_part == [S.D_PLANTED, size1 - len(range(0, size1, 7)), S.D_PLANTED]
    assert np.array_equal(np.flatnonzero(same[:r[1]] | False), d["planted"][:S.D_PLANTED])
    q = d["queries"][d["base_query"]:d["base_query"] + 1]
    with T.oracle_k(101):
        ids, dist = T.oracle_query(nodes, q, 1.0)
    assert dist[0, 99].view(np.uint32) == dist[0, 100].view(np.uint32), "the k-th and (k+1)-th distances are bit-equal at k = 100"
    assert ids[0, 99] >= r[1] > ids[0, S.D_PLANTED - 1], "the top 100 of the base query cross the edge of parts 0 and 1"
    with T.oracle_k(100):                                            # a category query: the tie group has members from all three parts
        cq = q.copy()
        cq[0, :4] = [1, 3, -1, -1]
        ids, dist = T.oracle_query(nodes, cq, 1.0)
    assert (dist[0] == 0).all() and ids[0, 0] < r[1] <= ids[0, -1] < r[2]


def test_builders_are_deterministic(sets):
    again = build_all()
    for key, s in sets.items():
        for name in ("nodes", "queries"):
            assert np.array_equal(s[name].view(np.uint32), again[key][name].view(np.uint32)), (key, name)
        assert s["nodes"].shape[0] <= S.N3 and s["queries"].shape[0] <= 1200
