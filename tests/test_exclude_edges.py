"""Exclusion lists where the query index can go wrong (include/hvs.h "per-query exclusion lists").  Every list form of a
kernel reads its query's list through `begin[qi]` / `count[qi]`; tests/test_exclude.py answers every call in one batch on one
lane, always over the whole resident set, so a `qi` that is batch-local, lane-local or range-local where it must be the
resident query's number reads the right list there.  Here:

* 1041 queries -- eight batches of 128 and a ragged ninth at HVS_MFMA_BATCH=128 -- whose lists differ from their neighbours' by
  q % 5, on both lanes, on one lane, without a spare lane, and under forced retries (also on the exact engine in batches of
  512); the host path and the resident path, k = 8, 100, 256, padding off and on;
* inner ranges of the resident set, on one GPU and on three-GPU contexts of both kinds;
* rows renumbered by hvs_compact under attached lists.

Expected answers come from tests/exclude_model.py on the rows of within_model.data() (tests/exclude_edges.py), exact on ids and
distance bits; tests/test_exclude_edges_cpu.py shows that the inputs make each of these mistakes visible.  The environments are
read when the library loads, so each runs in a child process under a time limit of its own; after a child that died nothing
more is started."""
import importlib
import os

import numpy as np
import pytest

import after_model as A
import exclude_edges as E
import exclude_model as X
import hvs_testlib as T

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
AUTO, EXACT, I8 = PKG.ENGINE_AUTO, PKG.ENGINE_EXACT_SCAN, PKG.ENGINE_MFMA_I8
NQ = E.NQ
ZERO_STATS = dict(excluding_queries=0, underfull_queries=0, kept_slots=0, refused_keys=0)


def same(got, want, what):
    assert np.array_equal(got[0], want[0]), f"{what}: ids differ in queries {np.flatnonzero((got[0] != want[0]).any(1))[:8]}"
    assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), \
        f"{what}: distance bits differ in queries {np.flatnonzero((got[1].view(np.uint32) != want[1].view(np.uint32)).any(1))[:8]}"


# ---- 1. many batches on both lanes ---------------------------------------------------------------------------------------------------------
_CHILD = r"""
import importlib, json, sys
import numpy as np
sys.path.insert(0, "tests")
import exclude_edges as E
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
spec = json.loads(sys.argv[1])
nodes, queries = E.workload()
Z = np.load(spec["expect"])
off, raw = Z["off"], Z["raw"]
lists = [raw[off[q]:off[q + 1]] for q in range(E.NQ)]
nq = E.NQ
result = {}
for name, engine in spec["engines"]:
    runs = {}
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.set_k(256)
        e.load_data(nodes)
        for k in E.KS:
            e.set_k(k)
            for padding in (0, 1):
                e.set_padding(bool(padding))
                tag = "%d_%d" % (k, padding)
                for path in ("host", "resident"):
                    if path == "host":
                        got = e.query(queries, 1.0, exclude=lists)
                    else:
                        e.upload_queries(queries)
                        e.set_exclude_ids(lists)
                        e.query_resident(0, nq, 1.0)
                        e.sync()
                        got = e.download_results(0, nq)
                    t, s = e.last_timing(), e.exclude_stats()
                    bad = np.flatnonzero((got[0] != Z["ids_" + tag]).any(1) | (got[1].view(np.uint32) != Z["bits_" + tag]).any(1))
                    runs[tag + "_" + path] = dict(ok=bad.size == 0, bad=bad[:8].tolist(), engine=int(t.engine), retry_queries=int(t.retry_queries),
                                                  fallback_queries=int(t.fallback_queries), main_kernel_launches=int(t.main_kernel_launches),
                                                  retry_list=int(e.last_reruns(1).size), **s.as_dict())
    result[name] = runs
print("RESULT " + json.dumps(result))
"""
CASES = {
    "one batch": {},
    "two lanes": {"HVS_MFMA_BATCH": "128"},
    "one lane": {"HVS_MFMA_BATCH": "128", "HVS_LANES": "0"},
    "no spare lane": {"HVS_MFMA_BATCH": "128", "HVS_TEST_NO_SPARE": "1"},
    "forced retries": {"HVS_MFMA_BATCH": "128", "HVS_GUESS_PFAIL": "1"},
    "forced retries, exact batches": {"HVS_MFMA_BATCH": "128", "HVS_GUESS_PFAIL": "1", "HVS_EXACT_BATCH": "512"},
}
_runs = {}


@pytest.fixture(scope="module")
def expect(tmp_path_factory):
    """the model's answers for the child processes, in a file"""
    off, raw = X.csr(E.lists())
    arrays = dict(off=off, raw=raw)
    kept = {}
    for k in E.KS:
        for padding in (0, 1):
            ids, d, n = E.answers(k, bool(padding))
            arrays["ids_%d_%d" % (k, padding)], arrays["bits_%d_%d" % (k, padding)] = ids, d.view(np.uint32)
            kept[k] = n
    path = str(tmp_path_factory.mktemp("exclude_edges") / "expect.npz")
    np.savez(path, **arrays)
    return path, kept


def child(case, path):
    if case not in _runs:
        env = dict(os.environ, HVS_I8_ROTATE="0")
        for var in ("HVS_MFMA_BATCH", "HVS_LANES", "HVS_TEST_NO_SPARE", "HVS_GUESS_PFAIL", "HVS_EXACT_BATCH", "HVS_LIB", "HVS_GUESS_MID"):
            env.pop(var, None)
        env.update(CASES[case])
        engines = [("i8", I8)] + ([("exact", EXACT)] if "HVS_EXACT_BATCH" in CASES[case] or not CASES[case] else [])
        _runs[case] = None                                                   # (a child that failed is not started again)
        _runs[case] = T.run_child(_CHILD, dict(expect=path, engines=engines), env, case, timeout=120)
    if _runs[case] is None:
        pytest.fail(f"the child process of case {case!r} failed earlier in this session")
    return _runs[case]


@pytest.mark.parametrize("case", [c for c in CASES if c != "one batch"])
def test_many_batches_lanes_and_retries(case, expect):
    """Nine batches of 1041 queries whose lists differ by q % 5: the answers equal the model's, `kept_slots` / `underfull_queries`
    equal the model's and those of the one-batch run of the same script; under HVS_GUESS_PFAIL=1 queries ARE retried, and the
    retry list is as long as the count."""
    path, kept = expect
    base = child("one batch", path)
    r = child(case, path)
    for name, runs in r.items():
        for tag, got in runs.items():
            print(case, name, tag, {f: got[f] for f in ("retry_queries", "fallback_queries", "main_kernel_launches", "kept_slots", "underfull_queries", "refused_keys")})
            k = int(tag.split("_")[0])
            what = (case, name, tag)
            assert got["ok"], (what, "queries with another answer:", got["bad"])
            assert got["engine"] == (I8 if name == "i8" else EXACT), (what, got)
            assert (got["excluding_queries"], got["kept_slots"], got["underfull_queries"]) == (NQ, int(kept[k].sum()), int((kept[k] < k).sum())), (what, got)
            one = base[name][tag]
            assert one["ok"] and (got["kept_slots"], got["underfull_queries"]) == (one["kept_slots"], one["underfull_queries"]), (what, got, one)
            assert got["retry_list"] == got["retry_queries"], (what, got)
            if name == "i8":
                assert got["main_kernel_launches"] > one["main_kernel_launches"], (what, got, one)       # the batches are small
                if "HVS_GUESS_PFAIL" in CASES[case]:
                    assert got["retry_queries"] > 0, (what, got)
            assert got["refused_keys"] > 0, (what, got)


# ---- 2. inner ranges of the resident set ---------------------------------------------------------------------------------------------------
def _inner_ranges(e, ranges, k, what):
    nodes, queries = E.workload()
    e.set_k(k)
    e.load_data(nodes)
    e.set_padding(False)
    e.upload_queries(queries)
    e.set_exclude_ids(E.lists())
    for sp, other in ((1.0, 0.6), (0.6, 1.0)):
        for q0, m in ranges:
            e.query_resident(0, NQ, other)                                   # every row of the result buffer is written ...
            e.sync()
            before = e.download_results(0, NQ)
            e.query_resident(q0, m, sp)                                      # ... then the inner range, at the other sample_proportion
            e.sync()
            s = e.exclude_stats()
            after = e.download_results(0, NQ)
            sel = range(q0, q0 + m)
            want = E.answers(k, False, sp, sel=sel)
            here = f"{what} range ({q0}, {m}) sp {sp}"
            same((after[0][q0:q0 + m], after[1][q0:q0 + m]), want, here)
            assert (s.excluding_queries, s.underfull_queries) == (m, int((want[2] < k).sum())), (here, s.as_dict())
            assert (want[0] != before[0][q0:q0 + m]).any(), here + ": the range call changes rows (the inputs are not trivial)"
            rest = np.ones(NQ, bool)
            rest[q0:q0 + m] = False
            same((after[0][rest], after[1][rest]), (before[0][rest], before[1][rest]), here + ", the rest of the result buffer")


@pytest.mark.parametrize("engine", [I8, EXACT])
def test_inner_ranges_on_one_gpu(engine):
    """query_resident(q0, m) off the wave grid, on the batch grid and at the end of the set, with lists attached to all 1041 queries:
    the range's rows are the model's rows of THOSE queries, `excluding_queries` is m, no other row of the results changes"""
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        _inner_ranges(e, E.RANGES, 100, f"engine {engine}")


@pytest.mark.parametrize("partition", [False, True])
def test_inner_ranges_on_three_gpus(partition):
    """... and on Engine(devices=[0, 0, 0]), replicated and row-partitioned, with a range that straddles both owner boundaries of
    the replicated context (queries 347 and 694)"""
    with PKG.Engine(devices=[0, 0, 0], partition=partition) as e:
        e.set_engine(AUTO)
        _inner_ranges(e, (E.RANGES[0], E.STRADDLE), 100, f"partition {partition}")


# ---- 3. compaction and trim ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("engine", [AUTO, EXACT])
def test_lists_name_the_renumbered_rows_after_a_compaction(engine):
    """What the code does ("rows renumbered": leaf_compact_commit -> HvsQuerySet::drop_results): the resident set STAYS
    through hvs_compact -- queries, caps, cursors and lists; only the results are dropped.  By the contract "an id is a row id of D
    as it is when the query runs" the lists then name the renumbered rows: the answers equal the model on the compacted rows with
    the same numeric ids, before and after hvs_trim_rows.  (The lists were made from the rows' old ids, so nine in ten of
    their entries name another row afterwards: tests/test_exclude_edges_cpu.py.)"""
    nodes, queries = E.workload()
    nq, k = E.NQ_COMPACT, 100
    queries = queries[:nq]
    lists = E.lists()[:nq]
    dead, new_to_old, rows = E.compaction()
    key = ("compacted fulls",)
    if key not in E._cache:
        E._cache[key] = A.full_order(rows, queries, rows.shape[0])
    fulls = E._cache[key]
    want = X.answers(fulls, lists, k)
    old = E.answers(k, False, sel=range(nq))
    assert (want[0] != old[0]).any(1).sum() > nq // 2
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(nodes)
        e.set_padding(False)
        e.upload_queries(queries)
        e.set_exclude_ids(lists)
        e.query_resident(0, nq, 1.0)
        e.sync()
        same(e.download_results(0, nq), old, f"engine {engine} before the compaction")
        e.delete_rows(dead)
        assert np.array_equal(e.compact(), new_to_old) and e.n == rows.shape[0]
        plan = e.exclude_plan_device()                                       # the lists are still attached, entry for entry
        assert np.array_equal(plan[3], PKG.exclude_plan(lists)[3])
        for step in ("compacted", "trimmed"):
            if step == "trimmed":
                e.trim_rows()
            e.query_resident(0, nq, 1.0)
            e.sync()
            same(e.download_results(0, nq), want, f"engine {engine} {step}")
            s = e.exclude_stats()
            assert (s.excluding_queries, s.kept_slots, s.underfull_queries) == (nq, int(want[2].sum()), int((want[2] < k).sum())), (step, s.as_dict())
            assert s.refused_keys >= X.refused_at_least(fulls, lists, want[0], want[1]) > 0, (step, s.as_dict())
        e.set_exclude_ids(None)
        e.query_resident(0, nq, 1.0)
        e.sync()
        same(e.download_results(0, nq), A.pages(fulls, None, k)[:2], f"engine {engine} lists removed")
        assert e.exclude_stats().as_dict() == ZERO_STATS
