"""Shared row sets on the GPU (include/hvs.h "shared row sets"): the k nearest rows inside a per-query bitmap, on every
engine, alone and together with caps, cursors, exclusion lists, candidate lists, the expanded resident set, row-set changes and
the multi-GPU contexts.

Expected answers come from tests/row_sets_model.py: every query's matched keys in key order (tests/after_model.py) with the keys
of rows outside the query's set dropped.  The key order is total, so every comparison is exact: ids array_equal, distance bits
array_equal.  tests/test_row_sets_cpu.py shows on the model alone that the inputs keep these tests from passing vacuously.
"""
import ctypes as C
import importlib
import os

import numpy as np
import pytest
import torch

import after_model as A
import exclude_edges as XE
import exclude_model as X
import hvs_testlib as T
import in_edges as E
import in_sets as S
import row_sets_model as R
import within_model as W

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
AUTO, EXACT, BF, I8, F16 = PKG.ENGINE_AUTO, PKG.ENGINE_EXACT_SCAN, PKG.ENGINE_MFMA_FILTER, PKG.ENGINE_MFMA_I8, PKG.ENGINE_MFMA_F16
FILTERS = (BF, I8, F16)
N = W.N
EINVAL, ESTATE = -1, -4
EMPTY, NONE = A.EMPTY, R.NONE
ZERO_EXCL = dict(excluding_queries=0, underfull_queries=0, kept_slots=0, refused_keys=0)
ZERO_CALL = dict(restricted_queries=0, underfull_queries=0, refused_keys=0, kept_slots=0)
_cache = {}


@pytest.fixture(scope="module")
def data():
    return W.data()


def sets_of():
    if "sets" not in _cache:
        _cache["sets"] = R.the_sets(N)
    return _cache["sets"]


def fulls_of(nodes, queries, sp, order="simd", tag="data"):
    ck = ("full", tag, float(sp), order)
    if ck not in _cache:
        sn = int(T.oracle().hvs_oracle_sn(sp, nodes.shape[0]))
        _cache[ck] = A.full_order(nodes, queries, sn, order)
    return _cache[ck]


def pads(nodes, queries, k, order="simd"):
    ck = ("pads", k, order)
    if ck not in _cache:
        _cache[ck] = W.pad_rows(nodes, queries, k, None, order)
    return _cache[ck]


def model(nodes, queries, sp, k, order, padding):
    """(ids, dists, kept, refused_min, the plain answers): shared by the engines of test 1 and the contexts of test 7"""
    ck = ("model", float(sp), k, order, padding)
    if ck not in _cache:
        fulls, sets, idx = fulls_of(nodes, queries, sp, order), sets_of(), R.query_sets(len(queries))
        pad_ids, pad_d = pads(nodes, queries, k, order)
        want = R.answers(fulls, sets, idx, k, None, None, None, pad_ids, pad_d, padding)
        _cache[ck] = want + (R.refused_at_least(fulls, sets, idx, want[0], want[1]) if not padding else 0,
                             A.pages(fulls, None, k, pad_ids, pad_d, padding))
    return _cache[ck]


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: ids differ in queries {np.flatnonzero((got[0] != want[0]).any(1))[:8]}"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), \
        f"{what}: distance bits differ in queries {np.flatnonzero((got[1].view(np.uint32) != want[1].view(np.uint32)).any(1))[:8]}"


def resident(e, nq, sp=1.0):
    e.query_resident(0, nq, sp)
    e.sync()
    return e.download_results(0, nq)


def gpu_u32(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.uint32).view(np.int32)).to("cuda:0")


def gpu_sets(sets):
    return torch.from_numpy(PKG.pack_row_sets(sets)[2].view(np.int64)).to("cuda:0")


def call_stats(e):
    d = e.row_sets_stats().as_dict()
    return {f: d[f] for f in ZERO_CALL}


def check_stats(e, idx, kept, k, what, refused_min=None, parts=False, sub=False):
    s = e.row_sets_stats()
    if not sub:
        assert s.restricted_queries == int((idx != NONE).sum()), (what, s.as_dict())
    assert s.underfull_queries == int((kept < k).sum()), (what, s.as_dict(), int((kept < k).sum()))
    if parts or sub:
        assert s.kept_slots >= int(kept.sum()), (what, s.as_dict(), int(kept.sum()))
    else:
        assert s.kept_slots == int(kept.sum()), (what, s.as_dict(), int(kept.sum()))
    if refused_min is not None:
        assert s.refused_keys >= refused_min, (what, s.as_dict(), refused_min)
    return s


# ---- 1. every engine x k x sampled prefix x distance order x padding, the indices attached three ways ----------------------------------
@pytest.mark.parametrize("engine", [EXACT, BF, I8, F16, AUTO])
def test_sets_on_every_engine(data, engine):
    nodes, queries = data
    nq = len(queries)
    sets, idx = sets_of(), R.query_sets(nq)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(256)
        e.load_data(nodes)
        assert e.row_sets_stats().as_dict() == dict(n_sets=0, words_per_set=0, bytes=0, **ZERO_CALL)
        e.set_row_sets(sets)
        st = e.row_sets_stats()
        assert (st.n_sets, st.words_per_set) == (R.N_SETS, N // 64) and st.bytes >= R.N_SETS * N // 8
        assert np.array_equal(e.row_sets(), sets)
        combos = [(0, k, sp) for k in (8, 100, 256) for sp in (1.0, 0.6)]
        if engine == EXACT:
            combos += [(1, k, sp) for k in (8, 100, 256) for sp in (1.0, 0.6)]
        for order, k, sp in combos:
            what = f"engine {engine} order {order} k {k} sp {sp}"
            oname = "scalar" if order else "simd"
            e.set_distance_order(order)
            e.set_k(k)
            e.set_padding(False)
            plain = e.query(queries, sp)                                    # sets loaded, no index attached: the plain answers
            want_i, want_d, want_n, refused_min, plain_want = model(nodes, queries, sp, k, oname, False)
            want = (want_i, want_d, want_n)
            same(plain, plain_want, what + " plain")
            pairs = int(e.last_timing().pairs)
            assert call_stats(e) == ZERO_CALL, what
            # the indices three ways: host, device tensor, hvs_query_in_row_sets
            e.upload_queries(queries)
            e.set_query_row_sets(idx)
            a = resident(e, nq, sp)
            same(a, want, what + " set_query_row_sets")
            assert int(e.last_timing().pairs) == pairs, what                # pairs do not look at sets
            check_stats(e, idx, want[2], k, what + " host", refused_min)
            assert e.exclude_stats().as_dict() == ZERO_EXCL, what            # keys refused by a set are counted apart
            e.upload_queries(queries)
            e.set_query_row_sets(gpu_u32(idx), stream=torch.cuda.current_stream())
            same(resident(e, nq, sp), a, what + " device")
            check_stats(e, idx, want[2], k, what + " device", refused_min)
            same(e.query(queries, sp, row_set=idx), a, what + " hvs_query_in_row_sets")
            assert int(e.last_timing().pairs) == pairs, what
            check_stats(e, idx, want[2], k, what + " hvs_query_in_row_sets", refused_min)
            # padding on: the slots the set leaves empty are padded, with rows that need not be in the set
            e.set_padding(True)
            padded = model(nodes, queries, sp, k, oname, True)
            same(resident(e, nq, sp), padded, what + " padding on")
            check_stats(e, idx, want[2], k, what + " padding on", refused_min)
            e.set_query_row_sets(None)
            same(resident(e, nq, sp), padded[4], what + " indices removed")
            assert call_stats(e) == ZERO_CALL, what
            t = e.last_timing()
            if engine == EXACT or order == 1:
                assert t.engine == EXACT, (what, t.engine)
            elif engine in FILTERS:
                assert t.engine == engine, (what, t.engine)


# ---- 2. three laws against code that shares nothing with the new code ------------------------------------------------------------------
@pytest.mark.parametrize("engine", [EXACT, BF, I8, F16, AUTO])
def test_a_small_set_equals_candidate_lists_of_its_members(data, engine):
    nodes, queries = data
    nq, k = len(queries), 100
    sets = sets_of()[[3, 4, 1]].copy()
    sets[0] &= np.arange(N) < 60000                                          # about 6000 members: within HVS_CANDIDATES_MAX
    assert 4000 < sets[0].sum() <= 8192 and 0 < sets[1].sum() <= 8192
    idx = (np.arange(nq) % 3).astype(np.uint32)
    members = [np.flatnonzero(s).astype(np.uint32) for s in sets]
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        e.upload_queries(queries)
        e.set_candidate_ids([members[int(s)] for s in idx])
        want = resident(e, nq)
        e.upload_queries(queries)
        e.set_row_sets(sets)
        e.set_query_row_sets(idx)
        same(resident(e, nq), want, f"engine {engine}")
        assert (want[0] != EMPTY).any() and (want[0][idx == 2] == EMPTY).all()


@pytest.mark.parametrize("engine", FILTERS)
def test_a_set_with_a_small_complement_equals_an_exclusion_list(data, engine):
    nodes, queries = data
    nq, k, sp = len(queries), 100, 0.6
    sn = int(T.oracle().hvs_oracle_sn(sp, N))
    out = [np.arange(7, sn, sn // 1000)[:1024].astype(np.uint32),             # spread over the prefix
           np.unique(np.concatenate([f[0][:4] for f in fulls_of(nodes, queries, sp)]))[:1024].astype(np.uint32)]   # the nearest rows of many queries
    sets = np.ones((2, N), bool)
    for s, ids in enumerate(out):
        sets[s, ids] = False
    idx = (np.arange(nq) % 2).astype(np.uint32)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        e.upload_queries(queries)
        e.set_exclude_ids([out[int(s)] for s in idx])
        want = resident(e, nq, sp)
        refused = e.exclude_stats().refused_keys
        e.set_exclude_ids(None)
        e.set_row_sets(sets)
        e.set_query_row_sets(idx)
        same(resident(e, nq, sp), want, f"engine {engine}")
        assert refused > 0 and e.row_sets_stats().refused_keys > 0 and e.exclude_stats().as_dict() == ZERO_EXCL


@pytest.mark.parametrize("engine", [EXACT, I8, AUTO])
def test_one_set_for_all_queries_equals_the_row_mask(data, engine):
    nodes, queries = data
    nq, k = len(queries), 100
    sets = sets_of()
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        for s in (2, 3, 5):
            e.set_row_mask(sets[s])
            e.upload_queries(queries)
            want = resident(e, nq)
            e.set_row_mask(None)
            e.set_row_sets(sets)
            e.set_query_row_sets(np.full(nq, s, np.uint32))
            same(resident(e, nq), want, f"engine {engine} set {s}")
            e.set_row_sets(None)


# ---- 3. edges of the key order: the run of 150 equal distances under set 6 --------------------------------------------------------------
@pytest.mark.parametrize("engine", [EXACT, I8, AUTO])
def test_the_set_cuts_a_run_of_equal_distances(engine):
    nodes, queries, _, info = E.tie_data()
    nodes = nodes.copy()
    n = nodes.shape[0]
    far = np.array([10, 11, 12, 13], np.uint32)                              # +inf and NaN distances, inside set 6 and outside it
    nodes[far[:2], 2 + 5] = np.inf
    nodes[far[2:], 2 + 6] = np.nan
    tq = R.tie_query(queries, info)
    q = np.ascontiguousarray(np.repeat(queries[tq][None, :], 8, 0))
    sets = R.the_sets(n)
    idx = np.array([6, NONE, 6, 0, 6, 1, 6, 2], np.uint32)
    fulls = A.full_order(nodes, q, n)
    assert np.isin(far, fulls[0][0][-4:]).all()                             # the last keys of the order
    run = fulls[0][0][fulls[0][1] == 0]
    in6 = int((run % 2 == 0).sum())                                          # the rows of the run that set 6 keeps
    assert run.size == 150 and 64 < in6 < 128
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(256)
        e.load_data(nodes)
        e.set_padding(False)
        e.set_row_sets(sets)
        for k in (64, 65, 128, 129, 255):
            e.set_k(k)
            e.upload_queries(q)
            e.set_query_row_sets(idx)
            want = R.answers(fulls, sets, idx, k)
            got = resident(e, len(q))
            same(got, want, f"engine {engine} k {k}")
            assert (got[1][0] == 0).sum() == min(k, in6) and (got[1][1] == 0).sum() == min(k, 150)
        # the whole order of a small set: the non-finite distances come last, only those of rows in the set
        small = np.zeros((1, n), bool)
        small[0, fulls[0][0][:20][::2]] = True
        small[0, far[[0, 2]]] = True
        e.set_k(64)
        e.set_row_sets(small)
        e.upload_queries(q)
        e.set_query_row_sets(np.zeros(len(q), np.uint32))
        got = resident(e, len(q))
        same(got, R.answers(fulls, small, np.zeros(len(q), np.uint32), 64), f"engine {engine} non-finite")
        assert list(got[0][0][10:12]) == [far[0], far[2]] and np.isinf(got[1][0][10]) and np.isnan(got[1][0][11]) and got[0][0][12] == EMPTY


# ---- 4. the query index: nine batches on both lanes, one lane, forced retries; inner ranges ---------------------------------------------
_CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path.insert(0, "tests")
import exclude_edges as XE
import row_sets_model as R
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
spec = json.loads(sys.argv[1])
nodes, queries = XE.workload()
Z = np.load(spec["expect"])
nq = XE.NQ
sets, idx = R.the_sets(XE.N), R.query_sets(nq)
runs = {}
with PKG.Engine(0) as e:
    e.set_engine(spec["engine"])
    e.load_data(nodes)
    e.set_padding(False)
    e.set_row_sets(sets)
    for path in ("host", "resident"):
        if path == "host":
            got = e.query(queries, 1.0, row_set=idx)
        else:
            e.upload_queries(queries)
            e.set_query_row_sets(idx)
            e.query_resident(0, nq, 1.0)
            e.sync()
            got = e.download_results(0, nq)
        t, s = e.last_timing(), e.row_sets_stats()
        bad = np.flatnonzero((got[0] != Z["ids"]).any(1) | (got[1].view(np.uint32) != Z["bits"]).any(1))
        runs[path] = dict(ok=bad.size == 0, bad=bad[:8].tolist(), engine=int(t.engine), retry_queries=int(t.retry_queries),
                          main_kernel_launches=int(t.main_kernel_launches), **s.as_dict())
print("RESULT " + json.dumps(runs))
"""
CASES = {
    "two lanes": {"HVS_MFMA_BATCH": "128"},
    "one lane": {"HVS_MFMA_BATCH": "128", "HVS_LANES": "0"},
    "forced retries": {"HVS_MFMA_BATCH": "128", "HVS_GUESS_PFAIL": "1"},
}


def edge_answers(k, sp=1.0, sel=None):
    ck = ("edge", k, float(sp), None if sel is None else tuple(sel))
    if ck not in _cache:
        at = range(XE.NQ) if sel is None else list(sel)
        _cache[ck] = R.answers(XE.fulls(sp, sel=sel), R.the_sets(N), R.query_sets(XE.NQ)[list(at)], k)
    return _cache[ck]


@pytest.mark.parametrize("case", list(CASES))
def test_many_batches_lanes_and_retries(case, tmp_path):
    k = 100
    want = edge_answers(k)
    idx = R.query_sets(XE.NQ)
    path = str(tmp_path / "expect.npz")
    np.savez(path, ids=want[0], bits=want[1].view(np.uint32))
    env = dict(os.environ, HVS_I8_ROTATE="0")
    for var in ("HVS_MFMA_BATCH", "HVS_LANES", "HVS_TEST_NO_SPARE", "HVS_GUESS_PFAIL", "HVS_EXACT_BATCH", "HVS_LIB", "HVS_GUESS_MID"):
        env.pop(var, None)
    env.update(CASES[case])
    r = T.run_child(_CHILD, dict(expect=path, engine=I8), env, case, timeout=120)
    for tag, got in r.items():
        what = (case, tag)
        print(what, got)
        assert got["ok"], (what, "queries with another answer:", got["bad"])
        assert got["engine"] == I8 and got["main_kernel_launches"] >= 9, (what, got)
        assert (got["restricted_queries"], got["kept_slots"], got["underfull_queries"]) == \
            (int((idx != NONE).sum()), int(want[2].sum()), int((want[2] < k).sum())), (what, got)
        assert got["refused_keys"] > 0, (what, got)
        if "HVS_GUESS_PFAIL" in CASES[case]:
            assert got["retry_queries"] > 0, (what, got)


@pytest.mark.parametrize("engine", [I8, EXACT])
def test_inner_ranges(engine):
    nodes, queries = XE.workload()
    k, NQ = 100, XE.NQ
    idx = R.query_sets(NQ)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        e.set_row_sets(R.the_sets(N))
        e.upload_queries(queries)
        e.set_query_row_sets(idx)
        for q0, m in XE.RANGES:
            before = resident(e, NQ, 0.6)
            e.query_resident(q0, m, 1.0)
            e.sync()
            s = e.row_sets_stats()
            after = e.download_results(0, NQ)
            want = edge_answers(k, 1.0, sel=range(q0, q0 + m))
            here = f"engine {engine} range ({q0}, {m})"
            same((after[0][q0:q0 + m], after[1][q0:q0 + m]), want, here)
            assert (s.restricted_queries, s.underfull_queries) == (int((idx[q0:q0 + m] != NONE).sum()), int((want[2] < k).sum())), (here, s.as_dict())
            rest = np.ones(NQ, bool)
            rest[q0:q0 + m] = False
            same((after[0][rest], after[1][rest]), (before[0][rest], before[1][rest]), here + ", the rest of the result buffer")


# ---- 5. composition -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [I8, EXACT])
def test_with_caps_cursors_and_lists(data, engine):
    nodes, queries = data
    nq, k = len(queries), 100
    sets, idx = sets_of(), R.query_sets(nq)
    fulls = fulls_of(nodes, queries, 1.0)
    page1 = R.answers(fulls, sets, idx, k)
    caps = W.choose_caps(page1[1], page1[0], first=2)
    capped = R.answers(fulls, sets, idx, k, None, caps)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        e.set_row_sets(sets)
        e.upload_queries(queries)
        e.set_query_row_sets(idx)
        e.set_max_dist2(caps)
        same(resident(e, nq), capped, "caps")
        check_stats(e, idx, capped[2], k, "caps", R.refused_at_least(fulls, sets, idx, capped[0], capped[1], caps))
        e.set_max_dist2(None)
        # cursors paged to exhaustion inside the set: no gap and no repeat
        inset = [X.drop_listed(f, c) for f, c in zip(fulls, R.complements(sets, idx))]
        P = 4
        depth = np.array([min(f[0].size, P * k) for f in inset])
        seen = [np.empty(0, np.uint32)] * nq
        lists = None
        for p in range(P):
            got = resident(e, nq)
            for q in range(nq):
                row = got[0][q][got[0][q] != EMPTY]
                assert np.array_equal(row, inset[q][0][p * k:(p + 1) * k]), (p, q)
                seen[q] = np.concatenate([seen[q], row])
            if p == 1:
                lists = [s.copy() for s in seen]                             # pages 1 and 2, for the lists below
            e.set_after_from_results()
        assert all(s.size == d for s, d in zip(seen, depth)) and (depth < P * k).any() and (depth == P * k).any()
        # exclusion lists of pages 1..2 together with the set: page 3, both refused counters positive
        e.set_after(None, None)
        e.set_exclude_ids(lists)
        want = R.answers(fulls, sets, idx, k, None, None, lists)
        same(resident(e, nq), want, "lists and sets")
        assert e.exclude_stats().refused_keys > 0 and e.row_sets_stats().refused_keys > 0
        check_stats(e, idx, want[2], k, "lists and sets")
        e.set_exclude_ids(None)
        same(resident(e, nq), page1, "lists removed, sets stay")
        # candidate lists: only the listed rows that are in the set count
        cand = [np.concatenate([f[0][:300:3], f[0][-50:]]) for f in fulls]
        e.set_candidate_ids(cand)
        want = X.answers([(f[0][np.isin(f[0], c)], f[1][np.isin(f[0], c)]) for f, c in zip(fulls, cand)], R.complements(sets, idx), k)
        same(resident(e, nq), want, "candidate lists and sets")
        check_stats(e, idx, want[2], k, "candidate lists and sets")


@pytest.mark.parametrize("engine", [AUTO, EXACT])
def test_under_category_sets(engine):
    nodes, queries, names = S.data()
    nq, k, n = len(queries), 100, nodes.shape[0]
    csets = S.sets_of(names)
    ck = ("in fulls",)
    if ck not in _cache:
        fulls = [None] * nq
        for name in sorted(set(names)):
            at = [i for i in range(nq) if names[i] == name]
            d2, q2 = S.rewrite(nodes, queries[at], S.SETS[name]) if S.SETS[name] else (nodes, queries[at])
            for i, f in zip(at, A.full_order(d2, q2, n)):
                fulls[i] = f
        _cache[ck] = fulls
    fulls = _cache[ck]
    sets, idx = R.the_sets(n), R.query_sets(nq)
    want = R.answers(fulls, sets, idx, k)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        e.set_row_sets(sets)
        e.upload_queries(queries)
        e.set_query_row_sets(idx)
        e.set_category_sets(csets)                                           # attaching category sets removes the indices
        same(resident(e, nq), A.pages(fulls, None, k), "category sets, no indices")
        assert call_stats(e) == ZERO_CALL
        e.set_query_row_sets(idx)                                            # every sub-query takes its parent's index
        same(resident(e, nq), want, "category sets and row sets")
        check_stats(e, idx, want[2], k, "category sets and row sets", R.refused_at_least(fulls, sets, idx, want[0], want[1]), sub=True)
        e.set_query_row_sets(gpu_u32(idx))
        same(resident(e, nq), want, "category sets and row sets, device")


def _one_set_per_query(n, page_ids):
    sets = np.ones((len(page_ids), n), bool)
    for q, row in enumerate(page_ids):
        sets[q, row[row != EMPTY]] = False
    return sets


def test_under_query_vectors():
    import vectors_model as V
    nodes, queries = V.data()
    vectors = V.mixed_vectors(nodes, queries)
    nq, k = len(queries), 100
    page1 = V.answers(nodes, queries, vectors, k, 1.0, padding=False)
    lists = [row[row != EMPTY] for row in page1["ids"]]
    want = V.answers(nodes, queries, vectors, k, 1.0, padding=False, depth=2 * k, exclude=lists)
    assert nq <= R.ROW_SETS_MAX
    with PKG.Engine(0) as e:
        e.set_padding(False)
        e.load_data(nodes)
        e.set_row_sets(_one_set_per_query(nodes.shape[0], page1["ids"]))     # set q: every row but query q's page 1
        e.upload_queries(queries)
        e.set_query_vectors(vectors)
        e.set_query_row_sets(np.arange(nq, dtype=np.uint32))
        got = resident(e, nq)
        assert np.array_equal(got[0], want["ids"]) and np.array_equal(got[1].view(np.uint32), want["dists"].view(np.uint32))
        assert e.row_sets_stats().refused_keys > 0


def test_under_query_clauses():
    import clauses_model as M
    nodes, queries = M.data()
    rng = np.random.default_rng(23)
    clauses, vectors = [], []
    for i, r in enumerate(queries):                                          # a window, a category, everything, under other vectors
        m = (2, 0, 3, 1)[i % 4]
        clauses.append(np.array([[2, 0, 0.2, 0.6], [1, i % M.NCAT, -1, -1], [0, 0, -1, -1]], np.float32)[:m])
        vectors.append(np.stack([r[4:] + rng.normal(0, 0.02, 100).astype(np.float32) if j & 1 else nodes[rng.integers(0, M.N), 2:]
                                 for j in range(m)]) if m else np.empty((0, 100), np.float32))
    nq, k = len(queries), 100
    page1 = M.answers(nodes, queries, clauses, vectors, k, 1.0, padding=False)
    lists = [row[row != EMPTY] for row in page1["ids"]]
    want = M.answers(nodes, queries, clauses, vectors, k, 1.0, padding=False, depth=2 * k, exclude=lists)
    assert nq <= R.ROW_SETS_MAX
    with PKG.Engine(0) as e:
        e.set_padding(False)
        e.load_data(nodes)
        e.set_row_sets(_one_set_per_query(nodes.shape[0], page1["ids"]))
        e.upload_queries(queries)
        e.set_query_clauses(clauses, vectors)
        e.set_query_row_sets(np.arange(nq, dtype=np.uint32))
        got = resident(e, nq)
        assert np.array_equal(got[0], want["ids"]) and np.array_equal(got[1].view(np.uint32), want["dists"].view(np.uint32))


# ---- 6. row-set changes under sets loaded once ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [AUTO, EXACT])
def test_row_set_changes(data, engine, monkeypatch):
    monkeypatch.setenv("HVS_COMPACT_CHUNK", "1000")                          # chunks end inside mask words
    nodes, queries = data
    nq, k = len(queries), 100
    sets, idx = sets_of(), R.query_sets(nq)
    rng = np.random.default_rng(41)
    dead = np.sort(rng.choice(N - 512, N // 20, replace=False)).astype(np.uint32)
    upd = np.sort(rng.choice(np.setdiff1d(np.arange(N - 512, dtype=np.uint32), dead), 200, replace=False)).astype(np.uint32)
    upd_rows = T.gen_data(200, 98, T.GEN_V1, W.NCAT)
    tail = T.gen_data(300, 97, T.GEN_V1, W.NCAT)
    big = T.gen_data(6000, 99, T.GEN_V1, W.NCAT)                             # more than the tail limit: the append folds

    def expect(rows, live, bits):
        f = A.full_order(rows, queries, rows.shape[0])
        if live is not None:
            f = [X.drop_listed(x, np.flatnonzero(~live).astype(np.uint32)) for x in f]
        return R.answers(f, bits, idx, k)

    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        e.set_row_sets(sets)
        e.upload_queries(queries)
        e.set_query_row_sets(idx)
        # delete, then update: bits stay with ids
        e.delete_rows(dead)
        e.update_rows(upd, upd_rows)
        now = nodes.copy()
        now[upd] = upd_rows
        live = np.ones(N, bool)
        live[dead] = False
        same(resident(e, nq), expect(now, live, sets), "delete and update")
        assert np.array_equal(e.row_sets(), sets)
        # append: new rows are in no set until assign_row_sets puts them there
        first = e.append_rows(tail)
        assert first == N
        now = np.concatenate([now, tail])
        live = np.concatenate([live, np.ones(300, bool)])
        bits = np.concatenate([sets, np.zeros((R.N_SETS, 300), bool)], 1)
        assert np.array_equal(e.row_sets(), bits)
        same(resident(e, nq), expect(now, live, bits), "append")
        new_ids = np.arange(N, N + 300, dtype=np.uint32)
        e.assign_row_sets(0, new_ids)
        e.assign_row_sets(6, np.concatenate([new_ids[::2], [N + 300, 0xFFFFFFFF, 2 * N]]).astype(np.uint32))   # ids >= n are ignored
        e.assign_row_sets(2, np.arange(0, N, 2, dtype=np.uint32)[:1000], member=False)
        bits[0, N:] = True
        bits[6, N::2] = True
        bits[2, np.arange(0, N, 2)[:1000]] = False
        assert np.array_equal(e.row_sets(), bits)
        same(resident(e, nq), expect(now, live, bits), "assign")
        # a folding append (the capacity grows: the sets are re-strided), re-index and trim
        e.append_rows(big)
        now = np.concatenate([now, big])
        live = np.concatenate([live, np.ones(6000, bool)])
        bits = np.concatenate([bits, np.zeros((R.N_SETS, 6000), bool)], 1)
        assert np.array_equal(e.row_sets(), bits)
        e.reindex()
        want = expect(now, live, bits)
        same(resident(e, nq), want, "folding append and re-index")
        e.trim_rows()
        assert np.array_equal(e.row_sets(), bits)
        same(resident(e, nq), want, "trim")
        # compaction: the sets are renumbered as the plan says, and the answers equal a fresh load of the live rows with those sets
        e.compact()
        packed = R.compact(bits, live)
        assert np.array_equal(PKG.row_sets_compact_plan(bits, live), packed)
        assert np.array_equal(e.row_sets(), packed)
        rows = np.ascontiguousarray(now[live])
        want = expect(rows, None, packed)
        same(resident(e, nq), want, "compact")
        check_stats(e, idx, want[2], k, "compact")
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(rows)
        e.set_padding(False)
        e.set_row_sets(packed)
        e.upload_queries(queries)
        e.set_query_row_sets(idx)
        same(resident(e, nq), want, "a fresh load of the live rows")


# ---- 7. context kinds -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0, 0], [0, 1]])
@pytest.mark.parametrize("partition", [False, True])
def test_context_kinds(data, partition, devices):
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs two GPUs")
    nodes, queries = data
    nq, k = len(queries), 100
    sets, idx = sets_of(), R.query_sets(nq)
    with PKG.Engine(devices=devices, partition=partition) as e:
        e.set_engine(AUTO)
        e.load_data(nodes)
        e.set_row_sets(sets)
        assert np.array_equal(e.row_sets(), sets)
        for sp in (1.0, 0.6):                                               # (0.6 ends inside part 2 of three, set 5 inside part 1)
            what = f"devices {devices} partition {partition} sp {sp}"
            want = model(nodes, queries, sp, k, "simd", False)
            e.set_padding(False)
            e.upload_queries(queries)
            e.set_query_row_sets(idx)
            same(resident(e, nq, sp), want, what + " host")
            check_stats(e, idx, want[2], k, what, want[3], parts=partition)
            e.upload_queries(queries)
            e.set_query_row_sets(gpu_u32(idx), stream=torch.cuda.current_stream())
            same(resident(e, nq, sp), want, what + " device")
            same(e.query(queries, sp, row_set=idx), want, what + " hvs_query_in_row_sets")
            e.set_padding(True)
            same(e.query(queries, sp, row_set=idx), model(nodes, queries, sp, k, "simd", True), what + " padding on")
            # a refusal on a multi-GPU context changes nothing on any GPU
            e.set_padding(False)
            bad = idx.copy()
            bad[-1] = R.N_SETS
            with pytest.raises(PKG.HvsError) as err:
                e.set_query_row_sets(bad)
            assert err.value.code == EINVAL
            same(resident(e, nq, sp), want, what + " after a refusal")
        # assign_row_sets goes to every GPU: set 1 gets the rows around every part's first row, and every query's nearest rows
        fulls = fulls_of(nodes, queries, 1.0)
        row0 = PKG.partition_plan(N, len(devices), k, 1.0)[0]
        ids = np.concatenate([[r - 1, r] for r in row0[1:len(devices)]] + [[0, N - 1]] + [f[0][:5] for f in fulls]).astype(np.uint32)
        e.assign_row_sets(1, ids)
        bits = sets.copy()
        bits[1, ids] = True
        assert np.array_equal(e.row_sets(), bits)
        want = R.answers(fulls, bits, idx, k)
        assert (want[2][idx == 1] > 0).any()
        same(resident(e, nq), want, f"devices {devices} partition {partition} assign")
        e.set_query_row_sets(None)
        same(resident(e, nq), A.pages(fulls, None, k), "removed")
        assert call_stats(e) == ZERO_CALL


# ---- 8. refusals change nothing; lifetime -----------------------------------------------------------------------------------------------------
def test_refusals_and_lifetime(data):
    nodes, queries = data
    nq, k, lib = len(queries), 100, PKG.library()
    up = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))  # noqa: E731
    u64 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    sets, idx = sets_of(), R.query_sets(nq)
    words = PKG.pack_row_sets(sets)[2]
    fulls = fulls_of(nodes, queries, 1.0)
    with PKG.Engine(0) as e:
        assert lib.hvs_set_row_sets(e._h, u64(words), R.N_SETS) == ESTATE      # before a load
        assert lib.hvs_set_query_row_sets(e._h, up(idx), nq) == ESTATE
        e.set_engine(I8)
        e.load_data(nodes)
        e.set_padding(False)
        e.upload_queries(queries)
        assert lib.hvs_set_query_row_sets(e._h, up(idx), nq) == ESTATE        # no sets loaded
        assert lib.hvs_set_query_row_sets_device(e._h, C.c_void_p(gpu_u32(idx).data_ptr()), nq, None) == ESTATE
        assert lib.hvs_assign_row_sets(e._h, 0, up(idx), nq, 1) == ESTATE
        e.set_row_sets(sets)
        page1 = R.answers(fulls, sets, idx, k)
        caps = W.choose_caps(page1[1], page1[0])
        e.set_max_dist2(caps)
        e.set_query_row_sets(idx)
        want = R.answers(fulls, sets, idx, k, None, caps)
        before = resident(e, nq)
        same(before, want, "before the refusals")
        bad = idx.copy()
        bad[17] = R.N_SETS                                                   # an index = n_sets
        d_idx, d_bad = gpu_u32(idx), gpu_u32(bad)
        many = np.zeros((257, N // 64), np.uint64)
        refused = [lib.hvs_set_query_row_sets(e._h, up(bad), nq),
                   lib.hvs_set_query_row_sets_device(e._h, C.c_void_p(d_bad.data_ptr()), nq, None),
                   lib.hvs_set_query_row_sets(e._h, up(idx), nq - 1),           # nq - 1, nq + 1
                   lib.hvs_set_query_row_sets(e._h, up(np.concatenate([idx, idx[:1]])), nq + 1),
                   lib.hvs_set_query_row_sets_device(e._h, C.c_void_p(d_idx.data_ptr()), nq + 1, None),
                   lib.hvs_set_query_row_sets_device(e._h, C.c_void_p(idx.ctypes.data), nq, None),   # a host array as a device pointer
                   lib.hvs_set_row_sets_device(e._h, C.c_void_p(words.ctypes.data), R.N_SETS, None),
                   lib.hvs_set_row_sets(e._h, u64(many), 257),                  # n_sets = 257
                   lib.hvs_assign_row_sets(e._h, R.N_SETS, up(idx), nq, 1)]
        assert refused == [EINVAL] * len(refused), refused
        assert torch.zeros(1, device="cuda:0").item() == 0                   # the runtime's error was cleared
        with pytest.raises(PKG.HvsError) as err:
            e.query(queries, 1.0, row_set=bad)                               # refused before the resident set is replaced
        assert err.value.code == EINVAL
        assert np.array_equal(e.row_sets(), sets)
        e.sync()
        same(e.download_results(0, nq), before, "the results stayed")
        same(resident(e, nq), before, "after the refusals")                 # sets, indices, caps and results stayed
        check_stats(e, idx, want[2], k, "after the refusals")
        # the device entries wait for a producer on another stream
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            big = torch.zeros(1 << 24, device="cuda:0").cumsum(0)            # keeps the stream busy in front of the producers
            d_late = gpu_u32(np.zeros(nq, np.uint32)) + torch.from_numpy(idx.view(np.int32)).to("cuda:0")
            d_sets = gpu_sets(np.zeros_like(sets)) | gpu_sets(sets)
        e.set_row_sets(d_sets, stream=side)
        e.set_max_dist2(caps)
        e.set_query_row_sets(d_late, stream=side)
        same(resident(e, nq), before, "device entries, a producer on another stream")
        del big
        # set_row_sets over attached indices drops the indices (and the results); the caps stay
        e.set_row_sets(sets)
        with pytest.raises(PKG.HvsError):
            e.set_after_from_results()                                       # (no query has a result row any more)
        plain_capped = X.answers(fulls, [np.empty(0, np.uint32)] * nq, k, None, caps)
        same(resident(e, nq), plain_capped, "the sets were replaced")
        assert call_stats(e) == ZERO_CALL
        # upload_queries drops the indices but not the sets
        e.set_query_row_sets(idx)
        e.upload_queries(queries)
        same(resident(e, nq), A.pages(fulls, None, k), "upload_queries")
        assert np.array_equal(e.row_sets(), sets) and call_stats(e) == ZERO_CALL
        e.set_query_row_sets(idx)
        same(resident(e, nq), page1, "the sets were still there")
        # the bitmaps survive new k and an engine change
        e.set_k(8)
        e.set_engine(EXACT)
        e.upload_queries(queries)
        e.set_query_row_sets(idx)
        same(resident(e, nq), R.answers(fulls, sets, idx, 8), "k and engine changed")
        # load_data drops the sets
        e.load_data(nodes)
        assert e.row_sets_stats().n_sets == 0
        assert lib.hvs_set_query_row_sets(e._h, up(idx), nq) == ESTATE
        e.upload_queries(queries)
        same(resident(e, nq), A.pages(fulls, None, 8), "after a load")
        # NULL bits: empty sets; n_sets = 0 removes them
        e.set_k(k)
        assert lib.hvs_set_row_sets(e._h, None, 3) == 0
        assert not e.row_sets().any() and e.row_sets().shape == (3, N)
        e.upload_queries(queries)
        e.set_query_row_sets(np.full(nq, 2, np.uint32))
        assert (resident(e, nq)[0] == EMPTY).all()
        e.set_row_sets(None)
        assert e.row_sets_stats().n_sets == 0
        same(resident(e, nq), A.pages(fulls, None, k), "sets removed")
