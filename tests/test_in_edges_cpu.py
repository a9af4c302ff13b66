"""The yardsticks of tests/test_in_edges.py, pinned without a GPU: the tie runs of in_edges.tie_data() are as long as claimed and
the cuts fall inside them, key_model agrees with the oracle, merged_keys_model with a hand count, and the retry / lanes workload
has the batches and the off-grid range the GPU test relies on."""
import numpy as np

import hvs_testlib as T
import in_edges as E
import in_sets as S


def parity(nodes, queries, names, got, want, k, sp, what=""):
    """test_in.parity (that module needs torch): check_parity per distinct set, each against its own rewritten copy of D"""
    names = np.array(names)
    with T.oracle_k(k):
        for name in sorted(set(names)):
            sel = np.flatnonzero(names == name)
            d2, q2 = S.rewrite(nodes, queries[sel], S.SETS[name]) if S.SETS[name] else (nodes, queries[sel])
            try:
                T.check_parity(d2, q2, got[0][sel], want[0][sel], sp, got_dists=got[1][sel])
            except AssertionError as err:
                raise AssertionError(f"{what}, set {name!r}: {err}") from None


def unpadded(want, m, k, n):
    """test_in.unpadded: the padded reference with the slots padding filled (rows n-1, n-2, ...) emptied"""
    ids, d = want[0].copy(), want[1].copy()
    for q in np.flatnonzero(m < k):
        row_i, row_d = ids[q].tolist(), d[q].tolist()
        for s in range(k - int(m[q])):
            j = row_i.index(n - 1 - s)
            del row_i[j], row_d[j]
        ids[q] = row_i + [E.EMPTY] * (k - len(row_i))
        d[q] = np.array(row_d + [np.inf] * (k - len(row_d)), np.float32)
    return ids, d


def test_tie_run_lengths_and_where_the_cuts_fall():
    nodes, queries, names, info = E.tie_data()
    sets = S.sets_of(names)
    cat = nodes[:, 0]
    for c in E.TIE_CATS:
        assert int((cat == c).sum()) == 150 and [len(x) for x in info["ids"][c]] == [30, 30, 90]
    full = E.full_keys(nodes, queries, sets, 1.0, tag="tie")
    for q, first, second in ((0, info["u"], info["w"]), (1, info["w"], info["u"])):
        assert names[q] == "tie5" and queries[q, 0] == 1.0 and np.array_equal(queries[q, 4:], first)
        keys, m = full[q]
        assert m == 750
        bits = (keys >> np.uint64(32)).astype(np.uint32)
        assert (bits[:150] == 0).all(), "150 keys at distance 0"
        assert bits[150] != 0 and (bits[150:300] == bits[150]).all() and bits[300] > bits[150], "then 150 at one other bit pattern"
        assert np.all(np.diff(keys.astype(np.uint32)[:150].astype(np.int64)) > 0) and np.all(np.diff(keys.astype(np.uint32)[150:300].astype(np.int64)) > 0)
        for k in (8, 100, 128, 129, 256):
            ids, d, _ = E.key_model(nodes, queries, sets, k, 1.0, tag="tie")
            run0, run1 = (0, 150) if k <= 150 else (150, 300)
            assert run0 < k < run1, "the cut at k falls inside a run"
            kept = ids[q, run0:k]                                            # the kept part of the cut run
            assert np.array_equal(d[q].view(np.uint32), bits[:k]) and np.array_equal(ids[q], keys[:k].astype(np.uint32))
            assert np.unique(cat[kept]).size >= 3, (q, k, np.unique(cat[kept]))
            left = keys[k:run1].astype(np.uint32)                            # ... and what the cut drops from it, larger ids all
            assert left.size and left.min() > kept.max()
    # the type-3 windows cut the runs to uneven per-category counts, one category with none
    for q, win, a, b in ((2, "A", "u", "w"), (3, "A", "w", "u"), (4, "B", "u", "w"), (5, "B", "w", "u")):
        tab = E.IN_A if win == "A" else E.IN_B
        keys, m = full[q]
        bits = (keys >> np.uint64(32)).astype(np.uint32)
        na, nb = sum(tab[a]), sum(tab[b])
        assert (bits[:na] == 0).all() and bits[na] != 0 and (bits[na:na + nb] == bits[na]).all() and bits[na + nb] > bits[na], (q, na, nb)
        per_cat = [int((cat[keys[:na].astype(np.uint32)] == c).sum()) for c in E.TIE_CATS]
        assert per_cat == tab[a] and 0 in per_cat and len(set(per_cat)) == 5, per_cat
    assert names[9] == "tie64" and full[9][1] == 750 and names[6] == "tie2" and full[6][1] == 300


def test_key_model_agrees_with_the_oracle():
    nodes, queries, names = S.data()
    sets, k = S.sets_of(names), 100
    for sp in (1.0, 0.5):
        want = S.expected(nodes, queries, names, k, sp)
        model = E.key_model(nodes, queries, sets, k, sp, tag="data")
        assert np.array_equal(model[2], want[2]), "matched rows per query"
        padded = E.pad(nodes, queries, model, k)
        parity(nodes, queries, names, padded, want, k, sp, what=f"key_model, padded, sp {sp}")
        # exact equality where no tie straddles the boundary: the k-th distance differs from the (k+1)-th
        full = E.full_keys(nodes, queries, sets, sp, tag="data")
        clear = np.array([m <= k or (keys[k - 1] >> np.uint64(32)) != (keys[k] >> np.uint64(32)) for keys, m in full])
        assert clear.sum() > 200
        inv = unpadded(want, want[2], k, nodes.shape[0])
        assert np.array_equal(model[0][clear], inv[0][clear]) and np.array_equal(model[1][clear].view(np.uint32), inv[1][clear].view(np.uint32))
    # caps and cursors: the page behind slot 5 is the one-shot answer from slot 6 on; a cap at slot 50 empties what lies beyond
    one = E.key_model(nodes, queries, sets, k, 1.0, tag="data")
    page = E.key_model(nodes, queries, sets, k - 6, 1.0, after=(one[1][:, 5], one[0][:, 5]), tag="data")
    assert np.array_equal(page[0], one[0][:, 6:]) and np.array_equal(page[1].view(np.uint32), one[1][:, 6:].view(np.uint32))
    caps = np.where(np.isinf(one[1][:, 50]), np.float32(3.0e38), one[1][:, 50])
    capped = E.key_model(nodes, queries, sets, k, 1.0, caps=caps, tag="data")
    for q in range(len(queries)):
        keep = one[1][q] <= caps[q]
        assert np.array_equal(capped[0][q, :keep.sum()], one[0][q][keep]) and (capped[0][q, keep.sum():] == E.EMPTY).all()


def test_non_finite_keys_sort_last_in_the_model():
    nodes, queries, names, special = E.nonfinite_data()
    sets = S.sets_of(names)
    ids, d, m = E.key_model(nodes, queries, sets, 100, 1.0)
    bits = d.view(np.uint32)
    q = next(i for i in range(len(queries)) if names[i] == "nf" and queries[i, 0] == 1.0)
    assert m[q] == 6
    assert ids[q, :2].tolist() in (special["plain"][2:], special["plain"][2:][::-1])
    assert ids[q, 2:5].tolist() == sorted([special["inf"][1]] + special["big"][2:]) and (bits[q, 2:5] == 0x7F800000).all()
    assert ids[q, 5] == special["nan"][1] and bits[q, 5] == E.NAN_BITS
    assert (ids[q, 6:] == E.EMPTY).all() and (bits[q, 6:] == 0x7F800000).all()
    q = next(i for i in range(len(queries)) if names[i] == "nf+" and queries[i, 0] == 1.0)
    assert m[q] == 11 and np.isfinite(d[q, :7]).all() and bits[q, 7] == 0x7F800000 and ids[q, 7] != E.EMPTY   # at k = 8: 7 finite keys, full by rows
    q = next(i for i in range(len(queries)) if names[i] == "93" and queries[i, 0] == 1.0)
    assert m[q] == 99 and np.isfinite(d[q, :95]).all() and (ids[q, :99] != E.EMPTY).all() and ids[q, 99] == E.EMPTY


def test_merged_keys_model_on_the_small_data_set():
    nodes, queries, names = S.small()
    sets = S.sets_of(names)
    cat = nodes[:, 0]
    for k in (8, 100):
        by_hand = 0
        for q, name in zip(queries, names):
            typ = q[0]
            if S.tests_c(typ) and len(S.SETS[name]):
                for c in S.categories(S.SETS[name]):                         # one list per distinct category
                    rows = (cat == c) & ((nodes[:, 1] >= q[2]) & (nodes[:, 1] <= q[3]) if int(typ) == 3 else True)
                    by_hand += min(int(rows.sum()), k)
            else:                                                            # one list, the query's own
                by_hand += min(int(T._passes(nodes, q).sum()), k)
        assert E.merged_keys_model(nodes, queries, sets, k, 1.0) == by_hand
    # ... and on a range it is the range's lists alone
    whole = E.merged_keys_model(nodes, queries, sets, 8, 1.0)
    assert E.merged_keys_model(nodes, queries, sets, 8, 1.0, 0, 30) + E.merged_keys_model(nodes, queries, sets, 8, 1.0, 30, 50) == whole


def test_the_retry_workload_makes_eight_batches_and_an_off_grid_range():
    nodes, queries, names = E.workload()
    sets = S.sets_of(names)
    nsub, sub_off, parent, value = S.plan_model(queries, sets)
    assert (len(queries), nsub) == (E.WORK_NQ, E.WORK_NSUB)
    assert nsub >= 8 * 128, "HVS_MFMA_BATCH=128 must make at least 8 batches"
    s0, s1 = int(sub_off[E.RANGE_Q0]), int(sub_off[E.RANGE_Q0 + E.RANGE_NQ])
    assert 0 < E.RANGE_Q0 and E.RANGE_Q0 + E.RANGE_NQ < len(queries)
    assert s0 % 128 and s1 % 128 and (s1 - 1) % 128 and s1 - s0 >= 4 * 128, (s0, s1)


def test_the_lifecycle_walk_is_what_it_says():
    steps = E.lifecycle()
    assert [s["step"] for s in steps] == list("abcdefg")
    base = S.data()[0]
    a, b, c, d, e, f, g = steps
    assert a["live"] is not None and np.array_equal(a["rows"], base[a["live"]]) and all(s["live"] is None for s in steps[1:])
    assert not (a["rows"][:, 0] == 1002).any() and a["rows"].shape[0] < S.N - 300 - 60
    assert int((a["rows"][:, 0] == 2).sum()) == int((base[:S.N - 300, 0] == 2).sum()) - len(np.flatnonzero(base[:, 0] == 2)[::3][np.flatnonzero(base[:, 0] == 2)[::3] < S.N - 300])
    assert np.array_equal(b["ops"][0][1], a["live"])
    assert c["rows"].shape[0] == b["rows"].shape[0] + 2000 and int((c["rows"][:, 0] == 2000).sum()) == 1
    assert int((d["rows"][:, 0] == 1003).sum()) == int((c["rows"][:, 0] == 1003).sum()) and not np.array_equal(d["rows"][:, 0], c["rows"][:, 0])
    assert f["rows"].shape[0] - e["rows"].shape[0] > 4096                   # past the default tail limit at this size
    assert not (g["rows"][:, 0] == 5).any() and g["rows"].shape[0] == f["rows"].shape[0] - int((f["rows"][:, 0] == 5).sum())
    for s in steps:
        assert not (s["rows"][:, 0] == S.VSTAR).any()
