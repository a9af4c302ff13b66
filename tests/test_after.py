"""Per-query result cursors on the GPU (include/hvs.h "per-query result cursors"): the k nearest rows after a key,
page after page, on every engine.

Expected answers come from tests/after_model.py: every query's matched keys in key order (predicates by hvs_testlib._passes,
distances by the oracle's exact-order function), and the paging law on top of them.  The key order is total, so every
comparison is exact: ids array_equal, distance bits array_equal -- nothing is loosened for ties.
"""
import importlib
import json
import os

import numpy as np
import pytest
import torch

import after_model as A
import hvs_testlib as T
import within_model as W

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
AUTO, EXACT, BF, I8, F16 = PKG.ENGINE_AUTO, PKG.ENGINE_EXACT_SCAN, PKG.ENGINE_MFMA_FILTER, PKG.ENGINE_MFMA_I8, PKG.ENGINE_MFMA_F16
FILTERS = (BF, I8, F16)
N = W.N
EINVAL, ESTATE = -1, -4
EMPTY = A.EMPTY


@pytest.fixture(scope="module")
def data():
    return W.data()


_cache = {}


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


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: ids differ in queries {np.flatnonzero((got[0] != want[0]).any(1))[:8]}"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), \
        f"{what}: distance bits differ in queries {np.flatnonzero((got[1].view(np.uint32) != want[1].view(np.uint32)).any(1))[:8]}"


def resident(e, nq, sp=1.0):
    e.query_resident(0, nq, sp)
    e.sync()
    return e.download_results(0, nq)


def check_stats(e, cursors, n_after, k, what):
    a = e.after_stats()
    want = dict(cursor_queries=len(n_after), exhausted_queries=int((cursors[1] == EMPTY).sum()), underfull_queries=int((n_after < k).sum()),
                after_slots=int(n_after.sum()))
    assert a.as_dict() == want, (what, a.as_dict(), want)


def to_gpu(cursors):
    return torch.from_numpy(cursors[0]).to("cuda:0"), torch.from_numpy(cursors[1].view(np.int32)).to("cuda:0")


# ---- 1. every engine x k x sampled prefix x distance order x padding: pages 1 to 3, cursors set three ways ------------------------
@pytest.mark.parametrize("engine", [EXACT, BF, I8, F16, AUTO])
def test_pages_on_every_engine(data, engine):
    nodes, queries = data
    nq = len(queries)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(256)
        e.load_data(nodes)
        combos = [(0, k, sp) for k in (8, 100, 256) for sp in (1.0, 0.6)]
        if engine == EXACT:
            combos += [(1, k, sp) for k in (8, 100, 256) for sp in (1.0, 0.6)]
        for order, k, sp in combos:
            what = f"engine {engine} order {order} k {k} sp {sp}"
            oname = "scalar" if order else "simd"
            fulls = fulls_of(nodes, queries, sp, oname)
            pad_ids, pad_d = pads(nodes, queries, k, oname)
            e.set_distance_order(order)
            e.set_k(k)
            e.set_padding(False)
            want1 = A.pages(fulls, None, k)
            got1 = e.query(queries, sp)                                     # page 1: no cursors are set
            same(got1, want1, what + " page 1")
            pairs = int(e.last_timing().pairs)
            assert e.after_stats().as_dict() == dict(cursor_queries=0, exhausted_queries=0, underfull_queries=0, after_slots=0)
            c1 = A.last_slots(*want1[:2])
            want2 = A.pages(fulls, c1, k)
            c2 = A.last_slots(*want2[:2])
            want3 = A.pages(fulls, c2, k)
            assert (c1[1] == EMPTY).any() and (c1[1] != EMPTY).any() and want2[2].sum() > 0, what
            # page 2, the cursors three ways
            e.upload_queries(queries)
            e.set_after(*c1)
            a = resident(e, nq, sp)
            same(a, want2, what + " page 2, set_after")
            assert int(e.last_timing().pairs) == pairs, what              # pairs do not look at cursors
            check_stats(e, c1, want2[2], k, what + " page 2")
            e.upload_queries(queries)
            e.set_after(*to_gpu(c1), stream=torch.cuda.current_stream())
            same(resident(e, nq, sp), a, what + " page 2, set_after_device")
            e.upload_queries(queries)
            same(resident(e, nq, sp), want1, what + " page 1, resident")
            e.set_after_from_results()
            same(resident(e, nq, sp), a, what + " page 2, set_after_from_results")
            check_stats(e, c1, want2[2], k, what + " page 2 from results")
            # page 3: from the results again, from the host, and through hvs_query_after
            e.set_after_from_results()
            b = resident(e, nq, sp)
            same(b, want3, what + " page 3, set_after_from_results")
            check_stats(e, c2, want3[2], k, what + " page 3")
            e.set_after(*c2)
            same(resident(e, nq, sp), b, what + " page 3, set_after")
            same(e.query(queries, sp, after=c2), b, what + " page 3, hvs_query_after")
            assert int(e.last_timing().pairs) == pairs, what
            # padding on: the same cursors, the slots behind the last match padded
            e.set_padding(True)
            same(resident(e, nq, sp), A.pages(fulls, c2, k, pad_ids, pad_d, True), what + " page 3, padding on")
            check_stats(e, c2, want3[2], k, what + " page 3, padding on")
            same(e.query(queries, sp, after=c1), A.pages(fulls, c1, k, pad_ids, pad_d, True), what + " page 2, padding on, hvs_query_after")
            e.set_after(None, None)
            same(resident(e, nq, sp), A.pages(fulls, None, k, pad_ids, pad_d, True), what + " page 1, padding on")
            t = e.last_timing()
            if engine == EXACT or order == 1:
                assert t.engine == EXACT, (what, t.engine)
            elif engine in FILTERS:
                assert t.engine == engine, (what, t.engine)


# ---- 2. paging to exhaustion on 8192 rows, filter engines forced -------------------------------------------------------------------
def small_set():
    if "small" not in _cache:
        n = 8192
        nodes = T.gen_data(n, 81, T.GEN_V1, 6)
        nodes[4000:4016] = nodes[100:116]                                   # duplicate rows: the id decides
        nodes[6000:6004, 2:] = nodes[7, 2:]                                 # ... and equal vectors under other attributes
        queries = T.gen_queries(20, 82, T.GEN_V1, 6)
        queries[0, :4] = [0, -1, -1, -1]                                    # type 0: all 8192 rows, 128 pages of 64
        queries[1, :4] = [0, -1, -1, -1]
        queries[1, 4:] = nodes[100, 2:]                                     # on top of a duplicated row: distance 0 twice
        queries[2, 0] = 9.0                                                 # matches nothing
        _cache["small"] = (nodes, np.ascontiguousarray(queries))
    return _cache["small"]


@pytest.mark.parametrize("engine", FILTERS)
def test_paging_to_exhaustion(engine):
    nodes, queries = small_set()
    nq, k = len(queries), 64
    fulls = fulls_of(nodes, queries, 1.0, "simd", "small")
    longest = max(f[0].size for f in fulls)
    assert longest == 8192 and min(f[0].size for f in fulls) == 0
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(k)
        e.load_data(nodes)
        e.set_padding(False)
        e.upload_queries(queries)
        got_i, got_d = [], []
        for p in range(longest // k + 2):
            if p:
                e.set_after_from_results()
            ids, d = resident(e, nq)
            if p == 0:
                assert e.last_timing().engine == engine
            got_i.append(ids)
            got_d.append(d)
        got_i, got_d = np.concatenate(got_i, 1), np.concatenate(got_d, 1)
        for q in range(nq):
            m = fulls[q][0].size
            assert np.array_equal(got_i[q, :m], fulls[q][0]), (q, m)
            assert np.array_equal(got_d[q, :m].view(np.uint32), fulls[q][1].view(np.uint32)), (q, m)
            assert (got_i[q, m:] == EMPTY).all() and np.isinf(got_d[q, m:]).all(), (q, m)   # exhausted stays exhausted
        a = e.after_stats()
        assert (a.cursor_queries, a.exhausted_queries, a.underfull_queries, a.after_slots) == (nq, nq, nq, 0), a.as_dict()


# ---- 3. cursors belong to the resident set -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [EXACT, I8])
def test_cursors_belong_to_the_resident_set(data, engine):
    nodes, queries = data
    nq, k, lib = len(queries), 100, PKG.library()
    fp, up = PKG.engine._f32p, PKG.engine._u32p
    fulls = fulls_of(nodes, queries, 1.0)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        with pytest.raises(PKG.HvsError) as err:
            e.after_stats()                                                 # before any call
        assert err.value.code == ESTATE
        e.upload_queries(queries)
        with pytest.raises(PKG.HvsError) as err:
            e.set_after_from_results()                                      # padding is on
        assert err.value.code == ESTATE
        e.set_padding(False)
        with pytest.raises(PKG.HvsError) as err:
            e.set_after_from_results()                                      # no results yet
        assert err.value.code == ESTATE
        e.query_resident(0, nq // 2, 1.0)
        with pytest.raises(PKG.HvsError) as err:
            e.set_after_from_results()                                      # results of half the queries
        assert err.value.code == ESTATE
        plain = resident(e, nq)
        same(plain, A.pages(fulls, None, k), "no cursors after the refused calls")
        c1 = A.last_slots(*plain)
        e.set_after(*c1)
        paged = resident(e, nq)
        same(paged, A.pages(fulls, c1, k), "page 2")
        # refused calls change nothing: a wrong nq, one NULL pointer, host memory as device memory, padding on
        d, i = c1[0].ctypes.data_as(fp), c1[1].ctypes.data_as(up)
        for bad in (nq - 1, nq + 1, 0):
            assert lib.hvs_set_after(e._h, d, i, bad) == EINVAL
            assert lib.hvs_set_after_device(e._h, c1[0].ctypes.data, c1[1].ctypes.data, bad, None) == EINVAL
        assert lib.hvs_set_after(e._h, d, None, nq) == EINVAL and lib.hvs_set_after(e._h, None, i, nq) == EINVAL
        assert lib.hvs_set_after_device(e._h, c1[0].ctypes.data, None, nq, None) == EINVAL
        assert lib.hvs_set_after_device(e._h, c1[0].ctypes.data, c1[1].ctypes.data, nq, None) == EINVAL     # host memory
        assert lib.hvs_query_after(e._h, queries.ctypes.data_as(fp), d, None, None, nq, 1.0, plain[0].ctypes.data_as(up), None) == EINVAL
        e.set_padding(True)
        assert lib.hvs_set_after_from_results(e._h) == ESTATE
        e.set_padding(False)
        same(e.download_results(0, nq), paged, "results after the refused calls")
        same(resident(e, nq), paged, "cursors after the refused calls")
        # None, None removes them
        e.set_after(None, None)
        same(resident(e, nq), plain, "set_after(None, None)")
        assert e.after_stats().cursor_queries == 0
        # every call that replaces the resident set removes them
        dq = torch.from_numpy(queries).to("cuda:0")
        row_ids = np.arange(0, nq, dtype=np.uint32) * 7
        for name, replace in (("upload_queries", lambda: e.upload_queries(queries)),
                              ("set_queries_device", lambda: e.set_queries_device(dq)),
                              ("gen_queries", lambda: e.gen_queries(nq, 92, T.GEN_V1, W.NCAT)),
                              ("set_queries_from_rows", lambda: e.set_queries_from_rows(row_ids, type=1)),
                              ("query", lambda: e.query(queries, 1.0))):
            e.upload_queries(queries)
            e.set_after(*c1)
            same(resident(e, nq), paged, "cursors before " + name)
            replace()
            if name != "query":                                             # the new set has no results
                assert lib.hvs_set_after_from_results(e._h) == ESTATE, name
            now = e.download_queries(0, nq)
            got = resident(e, nq)
            assert e.after_stats().cursor_queries == 0, name
            e.upload_queries(now)                                           # the same queries through a path known to carry no cursors
            same(got, resident(e, nq), "no cursors after " + name)
            if name in ("upload_queries", "set_queries_device", "query"):
                same(got, plain, "no cursors after " + name)


# ---- 4. with caps: the cap first, then the cursor ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [EXACT, BF, I8, F16])
def test_with_caps(data, engine):
    nodes, queries = data
    nq, k = len(queries), 100
    fulls = fulls_of(nodes, queries, 1.0)
    pad_ids, pad_d = pads(nodes, queries, k)
    p1 = A.pages(fulls, None, k)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        for first in (0, 3):
            caps = W.choose_caps(p1[1], p1[0], first=first)                  # the 0th, 9th, last distance of page 1, +inf, NaN, -1, ...
            far = np.array([f[1][min(f[1].size - 1, 149)] if f[1].size else 1.0 for f in fulls], np.float32)
            caps = np.where(np.arange(nq) % 3 == 0, far, caps).astype(np.float32)    # ... and caps that cut page 2 short
            capped = [A.cap_full(f, c) for f, c in zip(fulls, caps)]
            want1 = A.pages(capped, None, k)
            c1 = A.last_slots(*want1[:2])
            want2 = A.pages(capped, c1, k)
            assert ((want2[2] > 0) & (want2[2] < k)).sum() >= 10, first
            e.set_padding(False)
            same(e.query(queries, 1.0, max_dist2=caps), want1, f"engine {engine} capped page 1")
            e.set_after_from_results()
            same(resident(e, nq), want2, f"engine {engine} capped page 2")
            check_stats(e, c1, want2[2], k, "capped page 2")
            w = e.within_stats()
            assert (w.capped_queries, w.within_slots) == (nq, int(want2[2].sum())), w.as_dict()
            same(e.query(queries, 1.0, max_dist2=caps, after=c1), want2, f"engine {engine} capped page 2, hvs_query_after")
            e.set_padding(True)
            same(resident(e, nq), A.pages(capped, c1, k, pad_ids, pad_d, True), f"engine {engine} capped page 2, padding on")
            e.set_max_dist2(None)                                             # the cursors stay
            same(resident(e, nq), A.pages(fulls, c1, k, pad_ids, pad_d, True), f"engine {engine} caps removed, cursors kept")


# ---- 5. the other context kinds: bit for bit the one-GPU context ---------------------------------------------------------------------
@pytest.mark.parametrize("engine", [EXACT, I8])
def test_replicated_and_partitioned_contexts_equal_one_gpu(data, engine):
    nodes, queries = data
    nq, k = len(queries), 100
    one = {}
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        for sp in (1.0, 0.6):
            e.set_padding(False)
            p1 = e.query(queries, sp)
            same(p1, A.pages(fulls_of(nodes, queries, sp), None, k), f"one GPU sp {sp} page 1")
            e.set_after_from_results()
            p2 = resident(e, nq, sp)
            a = e.after_stats().as_dict()
            e.set_after_from_results()
            p3 = resident(e, nq, sp)
            e.set_padding(True)
            e.set_after(*A.last_slots(*p1))
            p2_on = resident(e, nq, sp)
            one[sp] = (p1, p2, p3, p2_on, a, int(e.last_timing().pairs))
    for partition in (False, True):
        with PKG.Engine(devices=[0, 0, 0], partition=partition) as m:
            m.set_engine(engine)
            m.load_data(nodes)
            for sp in (1.0, 0.6):
                p1, p2, p3, p2_on, a, pairs = one[sp]
                c1 = A.last_slots(*p1)
                what = f"{'partitioned' if partition else 'replicated'} [0,0,0] engine {engine} sp {sp}"
                m.set_padding(False)
                same(m.query(queries, sp), p1, what + " page 1")
                m.set_after_from_results()
                same(resident(m, nq, sp), p2, what + " page 2, set_after_from_results")
                assert int(m.last_timing().pairs) == pairs, what
                s = m.after_stats().as_dict()
                assert (s["cursor_queries"], s["exhausted_queries"], s["underfull_queries"]) == \
                    (a["cursor_queries"], a["exhausted_queries"], a["underfull_queries"]), (what, s, a)
                assert s["after_slots"] == a["after_slots"] if not partition else s["after_slots"] >= a["after_slots"], (what, s, a)
                m.set_after_from_results()
                same(resident(m, nq, sp), p3, what + " page 3, set_after_from_results")
                same(m.query(queries, sp, after=c1), p2, what + " page 2, hvs_query_after")
                m.upload_queries(queries)
                m.set_after(*to_gpu(c1), stream=torch.cuda.current_stream())
                same(resident(m, nq, sp), p2, what + " page 2, set_after_device")
                for bad in (nq - 1, nq + 1):
                    assert PKG.library().hvs_set_after(m._h, c1[0].ctypes.data_as(PKG.engine._f32p), c1[1].ctypes.data_as(PKG.engine._u32p), bad) == EINVAL
                m.set_padding(True)
                assert PKG.library().hvs_set_after_from_results(m._h) == ESTATE
                same(resident(m, nq, sp), p2_on, what + " page 2, padding on")
                m.set_after(None, None)
                m.query_resident(0, nq, sp)
                m.sync()
                assert m.after_stats().cursor_queries == 0


# ---- 6. with the live-row mask, the tail and stale rows ----------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [EXACT, I8])
def test_under_a_mask_with_tail_and_stale_rows(data, engine):
    """Append, update and delete without a re-index; the pages equal the model on the equivalent fresh data set (dead rows match
    nothing there).  The cursors of page 2 name rows that are deleted before page 2 runs: a cursor is a key, not a row reference."""
    nodes, queries = data
    nq, k, sp = len(queries), 100, 1.0
    n0 = N - 3000
    rng = np.random.default_rng(5)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_tail_limit(1 << 16)
        e.load_data(nodes[:n0])
        e.append_rows(nodes[n0:])
        upd = np.sort(rng.choice(n0, 400, replace=False)).astype(np.uint32)
        new_rows = nodes[rng.choice(N, 400, replace=False)].copy()
        new_rows[:, 2:] += np.float32(0.01)
        e.update_rows(upd, new_rows)
        now = nodes.copy()
        now[upd] = new_rows
        e.set_padding(False)
        first = e.query(queries, sp)
        dead = np.unique(first[0][::3, 0][first[0][::3, 0] != EMPTY])       # the nearest row of every third query
        dead = np.concatenate([dead, np.arange(N - 40, N - 10, dtype=np.uint32)])
        e.delete_rows(dead)
        live = np.ones(N, bool)
        live[dead] = False
        fulls = A.full_order(now, queries, N)                               # the fresh data set: the rows as they are now ...
        fulls = [(f[0][live[f[0]]], f[1][live[f[0]]]) for f in fulls]       # ... without the dead ones
        assert e.append_stats().n_tail == 3000 and e.update_stats().n_stale == 400
        want1 = A.pages(fulls, None, k)
        same(e.query(queries, sp), want1, f"engine {engine} page 1")
        c1 = A.last_slots(*want1[:2])
        gone = np.unique(c1[1][(c1[1] != EMPTY)][::4])                      # the cursor rows of a quarter of the queries die now
        e.delete_rows(gone)
        live[gone] = False
        fulls = [(f[0][live[f[0]]], f[1][live[f[0]]]) for f in fulls]
        want2 = A.pages(fulls, c1, k)
        e.upload_queries(queries)
        e.set_after(*c1)
        got2 = resident(e, nq, sp)
        same(got2, want2, f"engine {engine} page 2")
        assert not np.isin(got2[0], np.concatenate([dead, gone])).any()
        check_stats(e, c1, want2[2], k, "masked page 2")
        e.set_after_from_results()
        c2 = A.last_slots(*want2[:2])
        same(resident(e, nq, sp), A.pages(fulls, c2, k), f"engine {engine} page 3")
        pad_ids = PKG.mask_plan(live, k, sp)[2]
        pad_ids, pad_d = W.pad_rows(now, queries, k, pad_ids)
        e.set_padding(True)
        same(resident(e, nq, sp), A.pages(fulls, c2, k, pad_ids, pad_d, True), f"engine {engine} page 3, padding on")
        a, u = e.append_stats(), e.update_stats()
        assert a.tail_pairs > 0 and u.stale_pairs > 0, (a.as_dict(), u.as_dict())
        assert a.n_tail == 3000 and u.n_stale == 400                        # no query re-indexed


# ---- 7. forced retries and the small-batch chunked seed -----------------------------------------------------------------------------------
_CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path.insert(0, "tests")
import after_model as A
import hvs_testlib as T
import within_model as W
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
spec = json.loads(sys.argv[1])
nodes, queries = W.data()
queries = np.ascontiguousarray(queries[spec["q0"]:spec["q1"]])
nq, k = len(queries), 100
fulls = A.full_order(nodes, queries, nodes.shape[0])
with PKG.Engine(0) as e:
    e.set_engine(spec["engine"])
    e.load_data(nodes)
    e.set_padding(False)
    ok, retry, engines = [], [], []
    got = e.query(queries, 1.0)
    want = A.pages(fulls, None, k)
    for p in range(3):
        ok.append(bool(np.array_equal(got[0], want[0]) and np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32))))
        t = e.last_timing()
        retry.append(int(t.retry_queries))
        engines.append(int(t.engine))
        cur = A.last_slots(*want[:2])
        want = A.pages(fulls, cur, k)
        if p % 2 == 0:
            e.set_after_from_results()
        else:
            e.set_after(*cur)
        e.query_resident(0, nq, 1.0)
        e.sync()
        got = e.download_results(0, nq)
    a = e.after_stats()
    out = dict(ok=ok, retry=retry, engines=engines, slots=int(a.after_slots), underfull=int(a.underfull_queries))
print("RESULT " + json.dumps(out))
"""


@pytest.mark.parametrize("case", ["forced retries", "chunked seed"])
def test_forced_retries_and_the_chunked_seed(case):
    """HVS_GUESS_PFAIL=1: reckless guesses, many queries retried with the proven threshold -- the retry batch admits behind the
    cursors too.  60 queries: the seed kernel runs in its chunked form, one place per key behind the cursor."""
    env = dict(os.environ)
    if case == "forced retries":
        env["HVS_GUESS_PFAIL"] = "1"
        spec = dict(engine=I8, q0=0, q1=241)
    else:
        spec = dict(engine=I8, q0=180, q1=240)
    r = T.run_child(_CHILD, spec, env, case, timeout=240)
    print(json.dumps(r))
    assert all(r["ok"]) and all(x == I8 for x in r["engines"]), r
    if case == "forced retries":
        assert r["retry"][0] > 0, r


# ---- 8. Engine.query_pages ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [EXACT, I8])
def test_query_pages_equals_the_oracle(data, engine):
    nodes, queries = data
    with T.oracle_k(256):
        oi, od = T.oracle_query(nodes, queries, 1.0)
    want = W.unpadded_from_padded(oi, od, W.matches(nodes, queries, N), N)
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(64)
        e.load_data(nodes)
        got = e.query_pages(queries, 4)
        assert got[0].shape == (len(queries), 256)
        same(got, want, f"engine {engine} query_pages(q, 4), k = 64")
        full = e.query(queries, 1.0)                                          # padding is back on
        assert not (full[0] == EMPTY).any()
        caps = W.choose_caps(want[1], want[0], first=1)
        capped = [A.cap_full(f, c) for f, c in zip(fulls_of(nodes, queries, 1.0), caps)]
        got = e.query_pages(queries, 2, max_dist2=caps)
        same((got[0][:, :64], got[1][:, :64]), A.pages(capped, None, 64), "query_pages with caps, page 1")
        same((got[0][:, 64:], got[1][:, 64:]), A.pages(capped, A.last_slots(got[0][:, :64], got[1][:, :64]), 64), "query_pages with caps, page 2")
