"""One context walked through every transition of the resident-query state: category sets, distance caps, result
cursors and the result range, attached, replaced and dropped in a fixed order.  tests/queryset_model.py says after every call
what is attached; every answer of the walked context must be array_equal -- ids and distance bits -- to that of a FRESH
single-GPU context given exactly that, the three per-call figures must be zero or non-zero as the model says, and
hvs_set_after_from_results must succeed exactly when the model says every query has a result row.  A second walk does the same
for what takes the staged attach: exclusion lists, candidate lists, the shared row sets and the queries' indices into them.
A third walks the expanded set's three clients -- category sets, extra query vectors, extra clauses -- through each other.

Data: in_sets.small(), 901 rows and 80 queries; padding off throughout (hvs_set_after_from_results needs it)."""
import importlib

import numpy as np
import pytest
import torch

import in_sets as S
import queryset_model as M

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
AUTO, EXACT = PKG.ENGINE_AUTO, PKG.ENGINE_EXACT_SCAN
TWO_GPUS = [0, 1]

# the walk of one GPU: every row of the table, and the pairs that matter
WALK = [
    ("upload", "Q"), ("run", 0, 80),
    ("after_from_results",), ("run", 0, 80),                               # page 2
    ("caps", "C1"), ("run", 0, 80),
    ("sets", "S"), ("after_from_results",), ("run", 0, 80),                # caps then sets: the caps and the cursors are gone
    ("caps", "C1"), ("run", 0, 80),                                        # sets then caps
    ("after_from_results",), ("run", 0, 80),                               # cursors from the merged rows
    ("bad_sets",), ("after_from_results",), ("run", 0, 80),                # a refusal changes nothing: page 3 follows
    ("set_k", 100), ("after_from_results",), ("run", 0, 80),               # k with cursors attached: they stay, the results go
    ("sets", None), ("after_from_results",), ("run", 0, 80),               # ... then detach: plain answers at k = 100
    ("sets", None), ("after_from_results",), ("run", 0, 80),               # detaching nothing is a no-op: the results are there
    ("after", None), ("caps", "C2"),
    ("run", 20, 30), ("after_from_results",),                              # a sub-range is not all results
    ("run", 60, 20), ("after_from_results",),                              # apart: replaces
    ("run", 40, 20), ("after_from_results",), ("run", 0, 40), ("after_from_results",), ("run", 0, 80),   # joined piece by piece
    ("sets", "S2"), ("caps", "C1"), ("after", "A1"), ("run", 0, 80),
    ("upload", "Q2"), ("after_from_results",), ("run", 0, 80),             # a new set with everything attached: all of it goes
    ("caps", "C1"), ("after", "A1"), ("caps", None), ("run", 10, 70),
    ("query", "Q"), ("after_from_results",), ("run", 0, 80),               # hvs_query: replaced and answered in one call
]
# the shorter half for the multi-GPU contexts (WITH_SETS: not for a row-partitioned one)
SHORT = [
    ("upload", "Q"), ("run", 0, 80), ("after_from_results",), ("run", 0, 80),
    ("caps", "C1"), ("run", 0, 80),
    ("set_k", 100), ("after_from_results",), ("run", 0, 80), ("after_from_results",), ("run", 0, 80),
    ("after", None), ("run", 20, 30), ("after_from_results",),
    ("upload", "Q2"), ("after_from_results",), ("run", 0, 80),
]
WITH_SETS = [
    ("sets", "S"), ("after_from_results",), ("caps", "C2"), ("run", 0, 80), ("after_from_results",), ("run", 0, 80),
    ("bad_sets",), ("run", 30, 40), ("sets", None), ("run", 0, 80),
    ("query", "Q"), ("after_from_results",), ("run", 0, 80),
]
# the second walk: the lists' rows of the table (tests/queryset_model.py), on one GPU ...
LISTS = [
    ("upload", "Q"), ("exclude", "E1"), ("run", 0, 80),
    ("bad_exclude",), ("run", 0, 80),                                      # a refusal changes nothing
    ("after_from_results",), ("run", 0, 80), ("after", None), ("run", 0, 80),   # cursors come and go over the lists
    ("query_sets", "I1"), ("bad_query_sets",),                             # no shared sets yet: the state is asked first
    ("row_sets", "R1"), ("after_from_results",), ("query_sets", "I1"), ("run", 0, 80),   # loading the sets drops the results
    ("bad_query_sets",), ("exclude", None), ("run", 10, 60),               # indices alone
    ("candidates", "K1"), ("caps", "C1"), ("run", 0, 80),
    ("bad_candidates",), ("after_from_results",), ("run", 0, 80),
    ("row_sets", "R2"), ("after_from_results",), ("run", 0, 80),           # the sets replaced: indices and results go, the lists stay
    ("query_sets", "I1"), ("exclude", "E2"), ("candidates", "K2"), ("run", 0, 80),   # all three
    ("set_k", 100), ("run", 0, 80),
    ("sets", "S"), ("run", 0, 80),                                         # expanded_changed drops all three
    ("candidates", "K1"), ("bad_candidates",), ("candidates", None),       # ... and refuses candidate lists while attached
    ("exclude", "E1"), ("query_sets", "I1"), ("caps", "C2"), ("run", 0, 80),   # under the expanded set: the user's, per sub-query
    ("bad_exclude",), ("bad_query_sets",), ("after_from_results",), ("run", 0, 80),
    ("sets", None), ("run", 0, 80),
    ("exclude", "E2"), ("query_sets", "I1"), ("candidates", "K1"),
    ("upload", "Q2"), ("run", 0, 80),                                      # a replaced resident set drops all three
    ("query_sets", "I1"), ("run", 0, 80), ("row_sets", None), ("run", 0, 80),
]
# ... and in a short form on the two-leaf contexts (SHORT_LISTS_SETS: not for a row-partitioned one)
SHORT_LISTS = [
    ("upload", "Q"), ("exclude", "E1"), ("run", 0, 80), ("bad_exclude",), ("after_from_results",), ("run", 0, 80),
    ("row_sets", "R1"), ("query_sets", "I1"), ("after", None), ("run", 0, 80),
    ("candidates", "K1"), ("bad_candidates",), ("bad_query_sets",), ("run", 0, 80),
    ("row_sets", "R2"), ("run", 0, 80), ("upload", "Q2"), ("run", 0, 80),
]
SHORT_LISTS_SETS = [
    ("exclude", "E2"), ("sets", "S"), ("run", 0, 80), ("candidates", "K1"),
    ("exclude", "E1"), ("query_sets", "I1"), ("run", 0, 80), ("sets", None), ("run", 0, 80),
]
# the third walk: the clients' rows of the table, on one GPU ...
P1, V1 = ("P1", False), ("V1", True)                                       # clauses' tags: (name, they bring vectors)
CLIENTS = [
    ("upload", "Q"), ("run", 0, 80), ("vectors", "X1"), ("after_from_results",), ("run", 0, 80),   # attached: the results are gone
    ("after", "A1"), ("after_from_results",), ("after", None),             # a row has several keys: cursors refused, removal allowed
    ("candidates", "K1"), ("bad_candidates",),                             # ... and candidate lists, under any client
    ("bad_vectors", "long"), ("bad_vectors", "descending"), ("sets", None), ("clauses", None),
    ("after_from_results",), ("run", 20, 30),                              # refusals and the others' detach: nothing dropped
    ("caps", "C1"), ("exclude", "E1"), ("run", 0, 80),
    ("clauses", P1), ("run", 0, 80),                                       # clauses replace vectors: caps and lists are gone
    ("candidates", "K1"), ("after_from_results",), ("run", 0, 80),         # predicate-only: a row has one key, cursors allowed
    ("vectors", None), ("sets", None), ("bad_clauses", "long"), ("bad_clauses", "descending"), ("bad_sets",), ("run", 0, 80),
    ("clauses", V1), ("after_from_results",), ("run", 0, 80),              # clauses replace clauses; with vectors: cursors refused
    ("after", "A1"), ("after_from_results",), ("exclude", "E2"), ("run", 10, 60),
    ("sets", "S"), ("caps", "C2"), ("run", 0, 80), ("after_from_results",), ("run", 0, 80),   # sets replace clauses
    ("bad_vectors", "long"), ("bad_clauses", "descending"), ("clauses", None), ("run", 0, 80),
    ("vectors", "X2"), ("candidates", "K1"), ("run", 0, 80),               # vectors replace sets
    ("vectors", None), ("after_from_results",), ("run", 0, 80),            # its own detach: dropped, plain answers
    ("vectors", None), ("clauses", None), ("sets", None), ("after_from_results",), ("run", 0, 80),   # none attached: no-ops
    ("clauses", V1), ("upload", "Q2"), ("run", 0, 80),                     # a replaced resident set drops the client
    ("vectors", "X1"), ("query", "Q"), ("after_from_results",), ("run", 0, 80),
    ("clauses", P1), ("run", 0, 80), ("clauses", None), ("run", 0, 80),
]
# ... and in a short form on the replicated two-leaf contexts
SHORT_CLIENTS = [
    ("upload", "Q"), ("vectors", "X1"), ("run", 0, 80), ("after", "A1"), ("bad_vectors", "long"), ("sets", None), ("run", 20, 30),
    ("clauses", P1), ("caps", "C1"), ("run", 0, 80), ("after_from_results",), ("bad_clauses", "descending"), ("vectors", None), ("run", 0, 80),
    ("clauses", V1), ("after_from_results",), ("candidates", "K1"), ("run", 0, 80),
    ("sets", "S"), ("bad_sets",), ("run", 0, 80), ("vectors", "X2"), ("run", 0, 80), ("vectors", None), ("run", 0, 80),
    ("clauses", V1), ("query", "Q"), ("after_from_results",), ("run", 0, 80),
]


def prepared(eng, engine, nodes, k):
    eng.set_engine(engine)
    eng.set_k(k)
    eng.load_data(nodes)
    eng.set_padding(False)
    return eng


def make_values():
    """what the tags of the walk stand for; caps and cursors are cut from the plain answers at k = 8"""
    nodes, queries, names = S.small()
    with prepared(PKG.Engine(0), EXACT, nodes, 8) as e:
        e.upload_queries(queries)
        e.query_resident(0, len(queries), 1.0)
        ids, d = e.download_results(0, len(queries))

    def caps(slot):
        c = d[:, slot].copy()
        c[np.isinf(c)] = np.float32(3.0e38)
        return c

    sets = S.sets_of(names)
    # lists: ids of the plain answers (so that they bite; empty slots, 0xFFFFFFFF, go in as they are) and random rows
    rng = np.random.default_rng(23)
    n, nq = len(nodes), len(queries)
    pick = lambda m: np.sort(rng.choice(n, m, replace=False)).astype(np.uint32)
    off = np.arange(nq + 1, dtype=np.uint32) * 2
    too_long, descending = off.copy(), off.copy()
    too_long[-1] = too_long[-2] + PKG.EXCLUDE_MAX + 1
    descending[40] = descending[39] - 1
    # the clients' values: extra vectors are rows of D; a refused CSR has one list over the limit, or one descending offset
    rows = lambda m: nodes[rng.integers(0, n, m), 2:].copy()
    preds = np.array([[2, 0, 0.2, 0.6], [1, 3, -1, -1]], np.float32)
    one, bad = np.arange(nq + 1, dtype=np.uint32), {}
    for kind, limit, width in (("vectors", PKG.VECTORS_MAX_EXTRA, 100), ("clauses", PKG.CLAUSES_MAX_EXTRA, 4)):
        too_many, down = one.copy(), one.copy()
        too_many[30:] += limit
        down[40] = down[39] - 1
        bad[kind] = {"long": (too_many, np.zeros((int(too_many[-1]), width), np.float32)), "descending": (down, np.zeros((nq, width), np.float32))}
    clients = {"X1": [rows(q % 4) for q in range(nq)], "X2": [rows((q + 2) % 4) for q in range(nq)],
               P1: ([preds[:q % 3] for q in range(nq)], None), V1: ([preds[q % 2:q % 2 + 1] for q in range(nq)], [rows(1) for q in range(nq)]),
               "bad_vectors": bad["vectors"], "bad_clauses": bad["clauses"]}
    return {**clients, "nodes": nodes, "Q": queries, "Q2": np.ascontiguousarray(queries[::-1]), "S": sets, "S2": sets[3:] + sets[:3],
            "C1": caps(4), "C2": caps(6), "A1": (d[:, 2].copy(), ids[:, 2].copy()),
            "bad": sets[:-1] + [list(range(65))],
            "E1": [ids[q, :3] for q in range(nq)], "E2": [np.concatenate([ids[q, 1:6], pick(q % 7)]) for q in range(nq)],
            "K1": [pick(150 + q) for q in range(nq)], "K2": [np.concatenate([pick(40), ids[q, :4]]) for q in range(nq)],
            "R1": rng.random((3, n)) < 0.4, "R2": rng.random((2, n)) < 0.7,
            "I1": np.array([(0, 1, 0xFFFFFFFF)[q % 3] for q in range(nq)], np.uint32),
            "bad_E": (too_long, np.zeros(int(too_long[-1]), np.uint32)), "bad_K": (descending, np.zeros(2 * nq, np.uint32)),
            "bad_I": np.array([0] * (nq - 1) + [3], np.uint32)}


@pytest.fixture(scope="module")
def values():
    return make_values()


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: ids differ in queries {np.flatnonzero((got[0] != want[0]).any(1))[:8]}"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), \
        f"{what}: distance bits differ in queries {np.flatnonzero((got[1].view(np.uint32) != want[1].view(np.uint32)).any(1))[:8]}"


def fresh_answer(engine, V, s, cursors, q0, nq):
    """queries [q0, q0 + nq) on a single-GPU context that has seen nothing but what the model says is attached"""
    with prepared(PKG.Engine(0), engine, V["nodes"], s.k) as f:
        f.upload_queries(V[s.queries])
        if s.rsets is not None:
            f.set_row_sets(V[s.rsets])
        if s.sets is not None:
            attach_client(f, s.kind, V[s.sets])
        if s.excl is not None:
            f.set_exclude_ids(V[s.excl])
        if s.cand is not None:
            f.set_candidate_ids(V[s.cand])
        if s.qsets is not None:
            f.set_query_row_sets(V[s.qsets])
        if s.caps is not None:
            f.set_max_dist2(V[s.caps])
        if s.cursors is not None:
            f.set_after(*cursors)
        f.query_resident(q0, nq, 1.0)
        f.sync()
        return f.download_results(q0, nq)


def attach_client(e, kind, value):
    """the setter of the expanded set's client `kind`; value None: its detach"""
    if kind == "clauses":
        e.set_query_clauses(*(value or (None,)))
    else:
        (e.set_category_sets if kind == "sets" else e.set_query_vectors)(value)


ATTACH = {"exclude": "set_exclude_ids", "candidates": "set_candidate_ids", "row_sets": "set_row_sets", "query_sets": "set_query_row_sets"}
REFUSED = {"bad_exclude": "bad_E", "bad_candidates": "bad_K", "bad_query_sets": "bad_I"}


def code_of(fn):
    try:
        fn()
        return M.OK
    except PKG.HvsError as err:
        return err.code


def walk(e, engine, V, calls, s=None, check_timing=True, check_sets=True):
    nq_of = {"Q": len(V["Q"]), "Q2": len(V["Q2"])}
    s = s or M.initial(e.k)
    cursors = None                                                         # the values behind s.cursors
    for i, call in enumerate(calls):
        what = f"step {i} {call} from {s}"
        op = call[0]
        got = None
        if op in ("upload", "query"):
            if op == "upload":
                rc = code_of(lambda: e.upload_queries(V[call[1]]))
            else:
                got = e.query(V[call[1]], 1.0)
                rc, q0, nq = M.OK, 0, nq_of[call[1]]
        elif op in M.CLIENTS:
            rc = code_of(lambda: attach_client(e, op, None if call[1] is None else V[call[1]]))
        elif op == "bad_sets":
            rc = code_of(lambda: e.set_category_sets(V["bad"]))
        elif op == "bad_vectors":
            rc = code_of(lambda: e.set_query_vectors(V[op][call[1]]))
        elif op == "bad_clauses":
            rc = code_of(lambda: e.set_query_clauses(V[op][call[1]]))
        elif op == "caps":
            rc = code_of(lambda: e.set_max_dist2(None if call[1] is None else V[call[1]]))
        elif op == "after":
            rc = code_of(lambda: e.set_after(*((None, None) if call[1] is None else V[call[1]])))
        elif op == "after_from_results":
            rows = e.download_results(0, s.nq) if M.full(s) else None      # (reads only: the cursors a success attaches)
            rc = code_of(e.set_after_from_results)
            assert (rc == M.OK) == (M.full(s) and not M.many_keys(s)), f"{what}: hvs_set_after_from_results returned {rc}"
        elif op == "set_k":
            rc = code_of(lambda: e.set_k(call[1]))
        elif op in ATTACH:
            rc = code_of(lambda: getattr(e, ATTACH[op])(None if call[1] is None else V[call[1]]))
        elif op in REFUSED:
            rc = code_of(lambda: getattr(e, ATTACH[op[4:]])(V[REFUSED[op]]))
        elif op == "run":
            q0, nq = call[1], call[2]
            rc = code_of(lambda: e.query_resident(q0, nq, 1.0))
            if rc == M.OK:
                e.sync()
                got = e.download_results(q0, nq)
        s, want_rc = M.step(s, call, nq_of)
        assert rc == want_rc, f"{what}: returned {rc}, the model says {want_rc}"
        if rc == M.OK and op == "after":
            cursors = None if call[1] is None else V[call[1]]
        elif rc == M.OK and op == "after_from_results":
            cursors = (rows[1][:, s.k - 1].copy(), rows[0][:, s.k - 1].copy())
        elif s.cursors is None:
            cursors = None
        if got is not None:
            same(got, fresh_answer(engine, V, s, cursors, q0, nq), what)
            w, a = e.within_stats(), e.after_stats()
            assert (w.capped_queries != 0) == (s.caps is not None), f"{what}: {w.as_dict()}"
            assert (a.cursor_queries != 0) == (s.cursors is not None), f"{what}: {a.as_dict()}"
            if check_sets:
                for kind, n in (("sets", e.in_stats()), ("vectors", e.vector_stats()), ("clauses", e.clause_stats())):
                    assert (n.sub_queries != 0) == (M.expanded(s) is not None and s.kind == kind), f"{what}: {kind} {n.as_dict()}"
            x, k = e.exclude_stats(), e.candidates_stats()
            assert (x.excluding_queries != 0) == (s.excl is not None), f"{what}: {x.as_dict()}"
            assert (k.listed_queries != 0) == (s.cand is not None), f"{what}: {k.as_dict()}"
        if check_timing:
            assert (code_of(e.within_stats) == M.OK) == s.timed, what
    return s


@pytest.mark.parametrize("engine", [EXACT, AUTO])
def test_walk(values, engine):
    with prepared(PKG.Engine(0), engine, values["nodes"], 8) as e:
        s = walk(e, engine, values, WALK)
    assert (s.k, s.queries) == (100, "Q")


@pytest.mark.parametrize("engine", [EXACT, AUTO])
def test_walk_lists(values, engine):
    with prepared(PKG.Engine(0), engine, values["nodes"], 8) as e:
        s = walk(e, engine, values, LISTS)
    assert (s.k, s.queries, s.rsets) == (100, "Q2", None)


def need_two_gpus():
    if torch.cuda.device_count() < len(set(TWO_GPUS)):
        pytest.skip("needs two GPUs")


def test_walk_replicated_on_two_gpus(values):
    need_two_gpus()
    with prepared(PKG.Engine(devices=TWO_GPUS), AUTO, values["nodes"], 8) as e:
        s = walk(e, AUTO, values, SHORT, check_timing=False)
        walk(e, AUTO, values, WITH_SETS, s, check_timing=False)


def test_walk_partitioned_in_two_parts(values):
    need_two_gpus()
    with prepared(PKG.Engine(devices=TWO_GPUS, partition=True), AUTO, values["nodes"], 8) as e:
        walk(e, AUTO, values, SHORT, check_timing=False, check_sets=False)


@pytest.mark.parametrize("devices", [[0, 0], TWO_GPUS], ids=["two leaves on GPU 0", "two GPUs"])
@pytest.mark.parametrize("partition", [False, True], ids=["replicated", "partitioned"])
def test_walk_lists_on_two_leaves(values, partition, devices):
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs two GPUs")
    with prepared(PKG.Engine(devices=devices, partition=partition), AUTO, values["nodes"], 8) as e:
        s = walk(e, AUTO, values, SHORT_LISTS, check_timing=False, check_sets=not partition)
        if not partition:
            walk(e, AUTO, values, SHORT_LISTS_SETS, s, check_timing=False)


@pytest.mark.parametrize("engine", [EXACT, AUTO])
def test_walk_clients(values, engine):
    with prepared(PKG.Engine(0), engine, values["nodes"], 8) as e:
        s = walk(e, engine, values, CLIENTS)
    assert (s.k, s.queries, M.expanded(s)) == (8, "Q", None)


@pytest.mark.parametrize("devices", [[0, 0], TWO_GPUS], ids=["two leaves on GPU 0", "two GPUs"])
def test_walk_clients_on_two_leaves(values, devices):
    if max(devices) >= torch.cuda.device_count():
        pytest.skip("needs two GPUs")
    with prepared(PKG.Engine(devices=devices), AUTO, values["nodes"], 8) as e:
        s = walk(e, AUTO, values, SHORT_CLIENTS, check_timing=False)
    assert M.expanded(s) is None


def test_partitioned_refuses_the_clients(values):
    """a row-partitioned context refuses all three clients (HVS_ESTATE) and is left as it was"""
    with prepared(PKG.Engine(devices=[0, 0], partition=True), AUTO, values["nodes"], 8) as e:
        e.upload_queries(values["Q"])
        e.query_resident(0, 80, 1.0)
        e.sync()
        before = e.download_results(0, 80)
        for kind, tag in (("sets", "S"), ("vectors", "X1"), ("clauses", V1)):
            assert code_of(lambda: attach_client(e, kind, values[tag])) == M.ESTATE, kind
        same(e.download_results(0, 80), before, "the results the refusals left")
        assert code_of(e.set_after_from_results) == M.OK                   # ... with every query's row still there
        e.query_resident(0, 80, 1.0)
        e.sync()
        same(e.download_results(0, 80), fresh_answer(AUTO, values, M.State("Q", 80, None, None, M.FROM_RESULTS, 8, (0, 80)),
                                                     (before[1][:, 7].copy(), before[0][:, 7].copy()), 0, 80), "page 2 after the refusals")
