"""Row-set state x tile-format state on the GPU (DESIGN 3.9a x 3.4a): deletes, appends, updates, re-indexes and compactions on
contexts whose tile format changes under them -- forced through hvs_set_engine, planned and probed by HVS_ENGINE_AUTO, demoted
in mid-call -- and with rotated INT8 tiles.

Every step of every scenario runs on an engine and on the host model of tests/rowset_model.py side by side.  After every
query: the oracle's answer on the model's live rows (distances bit-equal, ids tie-aware, no dead id in any slot),
hvs_timing.pairs, and n_indexed / n_tail / n_stale / reindexes of hvs_append_stats / hvs_update_stats against the model's, so
that a silent re-index cannot pass for a tail or stale scan.  The library is compared with itself only where "the context of
a fresh load" is the claim.  Measured values are printed, never asserted; what is asserted is derived in the model (pairs,
patched, the stats tuples) or set by include/hvs.h (the flags, the engine a forced setting runs).

Recorded on the MI355X (engines: 1 exact, 2 BF16, 3 INT8, 4 FP16):
* B: HVS_ENGINE_AUTO answers Q with engine 3 (INT8, flags 0) after the load; the FAR call of 512 queries at n = 40 000 is enough
  for the demotion on one GPU and on two parts (256 queries each, all of them without a usable INT8 bound): engine 4, flags 2,
  fallback_queries 0, retry_queries 0; after hvs_reindex and after hvs_compact AUTO is back at engine 3, as the fresh load is.
* C: 30 000 rows after the compaction: engine 1, as the fresh load; n = 35 000 on the index over 30 000: engine 3 (the filter, on
  the plan no probe has checked, with a tail of 5000 rows behind it), flags 0; after hvs_reindex: engine 3, as the fresh load.
* E: hvs_set_engine(FP16) with non-finite stale rows in D: engine 1 (no format has a usable bound: orderings only); finite again
  and hvs_set_engine(INT8): engine 3.
* G: with HVS_GUESS_PFAIL=1 a probed load plans engine 4, so the child loads without the probe (engine 3, 23 of Q's 102 queries
  retried); the FAR call: engine 4, flags 2, fallback 0, retry 0 -- every FAR query goes to the exact list at once, so at this
  shape no retry batch precedes the demotion; the Q0 call behind it retries 4.
* Each test takes under a second.

Shown once by hand (MI355X), sensitivity:
* build_tiles returning HVS_OK instead of patch_tiles(c): test_forced_formats_... fails at the first format change,
  set_engine(FP16), on `tiles_patched == model.patched` (0 against 6060); printed beside it: dead_survivors 1877,
  stale_survivors 20; the answers stay right (64 of 64 identical to the oracle's).
* Read off the code, not run: before probe_format invalidated the last call's timing, hvs_last_timing after a re-index under
  AUTO returned the probe's counters under the earlier call's name.  Run: before the masked / sampled pair counts moved in front of hvs_k_prep, scenario B's
  FAR call reported hvs_timing.pairs 59 094 (the tail's and the stale rows' alone) against 6 643 142: hvs_k_prep empties the range
  of a query without a usable bound, and the counts read the ranges after it; before hvs_compact freed the live-row counts on
  its no-index path, test_first_index_after_a_compaction_below_4096_rows reported pairs 12 884 961 850 against 187 603 (5604
  counts written into buffers of 5004).
"""
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import hvs_testlib as T
import rowset_model as R
import test_append as A

pytestmark = pytest.mark.gpu
PKG = R.PKG
AUTO, EXACT, BF16, I8, F16 = R.AUTO, R.EXACT, R.BF16, R.I8, R.F16
FILTERS = R.FILTERS
N, NCAT, NFAR = 40_000, 5, 512
LIMIT = A.FAR                                                      # a tail limit no scenario but the walk reaches
FORMAT_CHANGED, I8_ROTATED = 2, 4                                  # HVS_TIMING_* (include/hvs.h)
ESTATE = -4

_stopped = []                                                      # a HIP error ends the GPU work of this module


def _start():
    if _stopped:
        pytest.fail("not started: " + _stopped[0])


_data = {}


def make_data(profile=T.GEN_V1):
    """N base rows and 300 to append, 5000 more for the crossing of 32768, 400 replacement rows, a pool for the walks; Q: 96
    mixed queries and six of invalid type, Q0: 64 of type 0, FAR: NFAR mixed queries three times as far out."""
    if profile not in _data:
        d = types.SimpleNamespace()
        d.nodes = T.gen_data(N + 300, 91, profile, NCAT)
        d.more = T.gen_data(5000, 95, profile, NCAT)
        d.repl = T.gen_data(400, 173, profile, NCAT)
        d.pool = T.gen_data(R.WALK_POOL, 177, profile, NCAT)
        d.Q = T.gen_queries(102, 92, profile, NCAT)
        d.Q[-6:-3, 0] = 7.0                                         # invalid types: nothing matches, the answer is all padding
        d.Q[-3:, 0] = -5.0
        d.Q0 = T.gen_queries(64, 93, profile, NCAT, force_type=0)
        d.FAR = T.gen_queries(NFAR, 94, profile, NCAT)
        d.FAR[:, 4:] *= np.float32(3.0)                             # far outside the data's box
        d.near = np.unique(T.oracle_query(d.nodes[:N], d.Q0)[0][:, 0])   # each Q0 query's nearest base row
        _data[profile] = d
    return _data[profile]


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def engine_on(devices):
    return PKG.Engine(devices=devices) if devices else PKG.Engine(0)


class Both:
    """one context and the model of it: every move goes to both, every query is checked against the model"""

    def __init__(self, e, engine, rows, limit=LIMIT):
        _start()
        self.e = e
        e.set_engine(engine)
        e.set_tail_limit(limit)
        e.load_data(rows)
        self.m = R.RowSetModel(rows, 100, limit)
        self.same_stats()

    def __enter__(self):
        return self

    def __exit__(self, typ, exc, tb):
        if isinstance(exc, PKG.HvsError) and exc.code == -3:
            _stopped.append(str(exc))
        self.e.close()

    def same_stats(self):
        e, m = self.e, self.m
        a, u = e.append_stats(), e.update_stats()
        got = (a.n_indexed, a.n_tail, u.n_stale, a.reindexes)
        assert got == m.stats(), (got, m.stats())
        assert (e.n, e.n_live, e.k, a.tail_limit, u.limit) == (m.n, m.n_live, m.k, m.tail_limit, m.tail_limit)
        assert e.compact_stats().compactions == m.compactions

    def delete(self, ids):
        self.e.delete_rows(ids)
        self.m.delete(ids)
        self.same_stats()

    def set_mask(self, live):
        self.e.set_row_mask(live)
        self.m.set_mask(live)
        assert np.array_equal(self.e.row_mask(), self.m.live)
        self.same_stats()

    def append(self, rows):
        assert self.e.append_rows(rows) == self.m.append(rows)
        self.same_stats()

    def update(self, ids, rows):
        self.e.update_rows(ids, rows)
        self.m.update(ids, rows)
        self.same_stats()

    def reindex(self):
        self.e.reindex()
        self.m.reindex()
        self.same_stats()

    def compact(self):
        got, want = self.e.compact(), self.m.compact()
        assert np.array_equal(got, want)
        self.same_stats()

    def trim(self):
        self.e.trim_rows()
        self.same_stats()

    def set_k(self, k):
        self.e.set_k(k)
        self.m.set_k(k)

    def query(self, queries, sp=1.0, what=""):
        ids, dists = self.e.query(queries, sp)
        t = self.e.last_timing()
        st = self.m.check(queries, ids, dists, sp)                  # (asserts "no dead id in any slot" before it maps ids)
        want = self.m.pairs(queries, sp)
        print(what, "nq", len(queries), "k", self.m.k, "sp", sp, st, "ran", t.engine, "flags", t.flags, "retry", t.retry_queries, "fallback",
              t.fallback_queries, "pairs", t.pairs, want, "stats", self.m.stats())
        assert t.pairs == want, (t.pairs, want)
        self.same_stats()
        return t

    def tombstones(self, q0, strict=True, survivors=True, what=""):
        """type-0 queries, each passing at least 256 k live rows: once a query's threshold is finite no dead and no stale row
        reaches the re-scoring front end (tests/test_row_mask.py, test_tombstones_keep_dead_rows_out_of_the_survivor_lists)"""
        m = self.m
        assert (T.passing_rows_per_query(m.rows[m.live], q0) >= 256 * m.k).all()
        t = self.query(q0, 1.0, what + " Q0")
        ms, us = self.e.mask_stats(), self.e.update_stats()
        print(what, "mask", ms.as_dict(), "update", us.as_dict(), "model patched", m.patched)
        assert (ms.n_dead, ms.n_live) == (m.n_dead, m.n_live)
        assert ms.tiles_patched == m.patched, (ms.tiles_patched, m.patched)
        if survivors:
            assert ms.dead_survivors == 0
        if strict:
            assert us.stale_survivors == 0
            assert t.fallback_queries == 0
        return t


def mutate(b, d):
    """delete 3000 base rows, each Q0 query's nearest among them; append 300; update 40 indexed rows (10 of them dead) and 3 of
    the tail"""
    rng = np.random.default_rng(5)
    others = rng.permutation(np.setdiff1d(np.arange(N), d.near))[:3000 - d.near.size]
    dead = np.concatenate([d.near, others]).astype(np.uint32)
    b.delete(dead)
    b.append(d.nodes[N:])
    live_ids = np.setdiff1d(np.arange(N), dead)
    upd = np.concatenate([rng.choice(live_ids, 30, replace=False), rng.choice(others, 10, replace=False), [N + 1, N + 150, N + 299]]).astype(np.uint32)
    b.update(upd, d.repl[:43])
    assert b.m.stats() == (N, 300, 40, 0) and b.m.n_dead == 3000 and b.m.patched == 2 * 3030
    return dead, upd


# ---- A. forced formats over one context with dead, tail and stale rows ---------------------------------------------------------
def test_forced_formats_over_one_context_with_dead_tail_and_stale_rows(monkeypatch):
    """hvs_set_engine I8 -> F16 -> BF16 -> EXACT -> I8 on a context with 3000 dead, 300 tail and 40 stale rows: the rebuild in
    run_queries (build_tiles_chain) is the only thing that keeps dead and stale rows out of the new tiles, and only tiles_patched,
    dead_survivors and stale_survivors show it.  Then, in F16: a revival (the same format is rebuilt), k = 256 and 8, sp = 0.5."""
    monkeypatch.setenv("HVS_I8_ROTATE", "0")
    d = make_data()
    with Both(PKG.Engine(0), I8, d.nodes[:N]) as b:
        dead, upd = mutate(b, d)
        for engine in (I8, F16, BF16, EXACT, I8):
            b.e.set_engine(engine)
            t = b.query(d.Q, 1.0, f"A set_engine({engine})")
            assert (t.engine, t.flags) == (engine, 0)
            t = b.tombstones(d.Q0, what=f"A set_engine({engine})")
            assert (t.engine, t.flags) == (engine, 0)
            assert b.m.reindexes == 0 and b.e.append_stats().reindexes == 0      # nothing was folded
        b.e.set_engine(F16)
        b.query(d.Q, 1.0, "A F16")
        rng = np.random.default_rng(6)
        dead_stale = np.intersect1d(dead, b.m.stale)
        assert dead_stale.size == 10
        back = np.concatenate([dead_stale[:6], rng.choice(np.setdiff1d(dead, dead_stale), 494, replace=False)])
        live = b.m.live.copy()
        live[back] = True
        b.set_mask(live)                                            # 500 rows come back, six of them stale
        assert b.m.patched == 2 * (3030 - 494)
        t = b.query(d.Q, 1.0, "A revived")
        assert (t.engine, t.flags) == (F16, 0)
        t = b.tombstones(d.Q0, what="A revived")
        assert (t.engine, t.flags) == (F16, 0)
        b.delete(np.arange(N + 290, N + 300))                       # the last rows are dead: the padding ids move
        for k in (256, 8):
            b.set_k(k)
            ids, _ = b.e.query(d.Q[-6:], 1.0)                       # invalid types: all padding
            assert (np.sort(ids, axis=1) == np.sort(b.m.pad_ids())).all() and b.m.pad_ids()[0] == N + 289
            t = b.query(d.Q, 1.0, f"A k = {k}")
            assert (t.engine, t.flags) == (F16, 0)
        t = b.query(d.Q, 0.5, "A sp = 0.5")
        assert t.engine == F16                                      # (half the live rows: above the quarter below which the exact engine answers)


# ---- B. AUTO: probe, demotion, compaction --------------------------------------------------------------------------------------
def scenario_b(d, devices, first_load_unprobed=False):
    """`first_load_unprobed`: HVS_PLAN_PROBE=0 (read per index build) while the data set is loaded, so that the plan is the model's
    INT8 whatever a probe would say; every later index build probes as usual."""
    if first_load_unprobed:
        os.environ["HVS_PLAN_PROBE"] = "0"
    try:
        b = Both(engine_on(devices), AUTO, d.nodes[:N])
    finally:
        if first_load_unprobed:
            del os.environ["HVS_PLAN_PROBE"]
    with b:
        t = b.query(d.Q, 1.0, "B load under AUTO")
        print("B: AUTO answers with engine", t.engine, "flags", t.flags)
        assert t.engine in FILTERS
        mutate(b, d)
        # demotion in mid-call: the re-run of the demoted list scans the tail and the stale rows, under the mask
        t = b.query(d.FAR, 1.0, "B FAR")
        print("B: FAR", NFAR, "queries: engine", t.engine, "flags", t.flags, "fallback", t.fallback_queries, "retry", t.retry_queries)
        assert t.flags & FORMAT_CHANGED, t.as_dict()
        assert t.engine in (F16, BF16)
        assert b.m.stats() == (N, 300, 40, 0)
        demoted = t.engine
        t = b.tombstones(d.Q0, strict=False, what="B after FAR")
        assert (t.engine, t.flags) == (demoted, 0)
        # hvs_reindex under the mask: the planner's probe runs a real filter batch under it
        b.reindex()
        assert b.m.stats() == (N + 300, 0, 0, 1)
        ms, a, u = b.e.mask_stats(), b.e.append_stats(), b.e.update_stats()
        print("B after hvs_reindex, before any query:", ms.as_dict(), a.as_dict(), u.as_dict())
        assert ms.tiles_patched == 2 * b.m.n_dead == b.m.patched
        assert (ms.dead_survivors, a.tail_pairs, a.tail_admitted, u.stale_pairs, u.stale_admitted, u.stale_survivors) == (0, 0, 0, 0, 0, 0)
        with pytest.raises(PKG.HvsError) as err:                    # nor does the probe's batch pass for the caller's last call
            b.e.last_timing()
        assert err.value.code == ESTATE
        t = b.query(d.Q, 1.0, "B reindexed")
        b.tombstones(d.Q0, strict=False, what="B reindexed")
        # hvs_compact: the context of a fresh load of the live rows, the planner's choice included
        b.compact()
        assert b.m.stats() == (b.m.n, 0, 0, 2) and b.m.n == N + 300 - 3000
        with engine_on(devices) as f:
            f.set_tail_limit(LIMIT)
            f.load_data(b.m.rows)                                   # AUTO
            for k in (100, 256):
                b.set_k(k)
                f.set_k(k)
                for sp in (1.0, 0.5):
                    for name, q in (("Q", d.Q), ("FAR[:64]", d.FAR[:64]), ("Q0", d.Q0)):
                        got, want = b.e.query(q, sp), f.query(q, sp)
                        tg, tw = b.e.last_timing(), f.last_timing()
                        print("B compacted / fresh", k, sp, name, "engine", tg.engine, tw.engine, "flags", tg.flags, tw.flags)
                        assert same(got, want), (k, sp, name)
                        assert (tg.engine, tg.flags, tg.pairs) == (tw.engine, tw.flags, tw.pairs), (k, sp, name)
            b.set_k(100)
        b.query(d.Q, 1.0, "B compacted")


@pytest.mark.parametrize("devices", [None, [0, 0]], ids=["one GPU", "two parts on GPU 0"])
def test_auto_probe_demotion_reindex_and_compaction(devices, monkeypatch):
    """Load under AUTO, the delete / append / update of A, a call far outside the data's box (demotion in mid-call with a tail and
    stale rows), hvs_reindex under the mask (the probe leaves nothing in the figures), hvs_compact (byte-equal to a fresh AUTO
    load of the live rows, engine and flags call by call)."""
    monkeypatch.delenv("HVS_I8_ROTATE", raising=False)
    scenario_b(make_data(), devices)


# ---- C. crossing 32768 under AUTO, and the first index under a mask ---------------------------------------------------------------
def test_crossing_32768_under_auto(monkeypatch):
    """40 000 rows -> compaction to 30 000 (AUTO answers with the exact engine, as a fresh load does) -> 5000 appended (n = 35 000 on
    an index over 30 000 that no probe has seen: whichever engine runs, the oracle's answers) -> hvs_reindex (a fresh load of the
    35 000)."""
    monkeypatch.delenv("HVS_I8_ROTATE", raising=False)
    d = make_data()

    def equals_fresh(b, what):
        with PKG.Engine(0) as f:
            f.set_tail_limit(LIMIT)
            f.load_data(b.m.rows)
            for q in (d.Q, d.Q0):
                got, want = b.e.query(q, 1.0), f.query(q, 1.0)
                tg, tw = b.e.last_timing(), f.last_timing()
                print("C", what, "engine", tg.engine, tw.engine, "flags", tg.flags, tw.flags)
                assert same(got, want) and (tg.engine, tg.flags, tg.pairs) == (tw.engine, tw.flags, tw.pairs), what
            return tg.engine

    with Both(PKG.Engine(0), AUTO, d.nodes[:N]) as b:
        b.delete(np.random.default_rng(7).choice(N, 10_000, replace=False))
        b.compact()
        assert b.e.n == 30_000 and b.m.stats() == (30_000, 0, 0, 1)
        assert equals_fresh(b, "compacted to 30 000") == EXACT
        b.query(d.Q, 1.0, "C 30 000")
        b.append(d.more)
        assert b.e.n == 35_000 and b.m.stats() == (30_000, 5000, 0, 1)
        t = b.query(d.Q, 1.0, "C 35 000 on an index over 30 000")
        print("C: n = 35 000, n_indexed = 30 000 under AUTO: engine", t.engine, "flags", t.flags)
        b.query(d.Q0, 1.0, "C 35 000 on an index over 30 000, Q0")
        b.reindex()
        assert b.m.stats() == (35_000, 0, 0, 2)
        print("C: after hvs_reindex of the 35 000 rows: engine", equals_fresh(b, "35 000 re-indexed"))
        b.query(d.Q, 1.0, "C 35 000 re-indexed")


def test_first_index_under_a_mask(monkeypatch):
    """3000 rows under EXACT have no index; 200 deleted, 100 appended, then hvs_set_engine(I8) builds the first one -- not through
    leaf_reindex / index_data -- over all rows, mask re-applied.  Below the model's 4096 rows: the expectations are stated here."""
    monkeypatch.setenv("HVS_I8_ROTATE", "0")
    _start()
    d = make_data()
    import test_row_mask as M
    cur, live = d.nodes[:3100].copy(), np.ones(3100, bool)
    dead = np.random.default_rng(8).choice(3000, 200, replace=False)
    live[dead] = False
    with A.fresh(EXACT, cur[:3000]) as e:
        assert (e.append_stats().n_indexed, e.append_stats().n_tail) == (0, 0)
        e.delete_rows(dead)
        assert e.append_rows(cur[3000:]) == 3000
        assert (e.append_stats().n_indexed, e.append_stats().n_tail, e.n, e.n_live) == (0, 0, 3100, 2900)
        e.set_engine(I8)
        for k in (100, 256):
            e.set_k(k)
            ids, dists = e.query(d.Q, 1.0)
            t, a, ms = e.last_timing(), e.append_stats(), e.mask_stats()
            print("C (ii) k", k, "ran", t.engine, a.as_dict(), ms.as_dict())
            assert t.engine == I8
            assert (a.n_indexed, a.n_tail) == (3100, 0)
            assert ms.tiles_patched == 2 * 200
            M.check(cur, d.Q, live, ids, dists, 1.0, k)
            assert t.pairs == int(M.matches_in_live_prefix(cur, d.Q, live, 1.0).sum())
        e.set_k(100)
        more = d.nodes[3100:3150]
        assert e.append_rows(more) == 3100
        cur, live = np.concatenate([cur, more]), np.concatenate([live, np.ones(50, bool)])
        for sp in (1.0, 0.5):
            ids, dists = e.query(d.Q, sp)
            a = e.append_stats()
            assert (a.n_indexed, a.n_tail) == (3100, 50)
            M.check(cur, d.Q, live, ids, dists, sp, 100)
            assert e.last_timing().pairs == int(M.matches_in_live_prefix(cur, d.Q, live, sp).sum())


def test_first_index_after_a_compaction_below_4096_rows(monkeypatch):
    """An I8 context of 5003 rows under a mask answers a call (the live-row counts along its orderings are made: 5004 entries), goes
    to EXACT and is compacted to 3003 rows: no index.  2600 appended rows later hvs_set_engine(I8) builds one over 5603 rows, under
    a mask again: the counts must have room for the new orderings."""
    monkeypatch.setenv("HVS_I8_ROTATE", "0")
    _start()
    d = make_data()
    import test_row_mask as M
    rng = np.random.default_rng(9)
    with A.fresh(I8, d.nodes[:5003]) as e:
        dead = rng.choice(5003, 2000, replace=False)
        live = np.ones(5003, bool)
        live[dead] = False
        e.delete_rows(dead)
        ids, dists = e.query(d.Q, 1.0)
        assert e.last_timing().engine == I8
        M.check(d.nodes[:5003], d.Q, live, ids, dists, 1.0, 100)
        e.set_engine(EXACT)
        new_to_old = e.compact()
        cur = d.nodes[:5003][new_to_old]
        assert (e.n, e.append_stats().n_indexed) == (3003, 0)
        assert e.append_rows(d.more[:2600]) == 3003
        cur = np.concatenate([cur, d.more[:2600]])
        live = np.ones(5603, bool)
        live[::9] = False
        e.set_row_mask(live)
        assert (e.n, e.append_stats().n_indexed, e.append_stats().n_tail) == (5603, 0, 0)
        e.set_engine(I8)
        for sp in (1.0, 0.5):
            ids, dists = e.query(d.Q, sp)
            t, a, ms = e.last_timing(), e.append_stats(), e.mask_stats()
            assert t.engine == I8 and (a.n_indexed, a.n_tail) == (5603, 0) and ms.tiles_patched == 2 * int((~live).sum())
            M.check(cur, d.Q, live, ids, dists, sp, 100)
            assert t.pairs == int(M.matches_in_live_prefix(cur, d.Q, live, sp).sum())


# ---- D. rotated INT8 tiles through re-index and compaction ---------------------------------------------------------------------
@pytest.mark.parametrize("profile", [T.GEN_V1, T.GEN_PCA], ids=["v1", "pca"])
def test_rotated_int8_tiles_through_reindex_and_compaction(profile, monkeypatch):
    """HVS_I8_ROTATE=1 (read per data set): hvs_reindex and hvs_compact recompute centre and scale of the rotated vectors
    (hvs_k_minmax_rot) over rows that were appended and updated since the load.  Uniform rows, and the PCA-like law the rotation
    exists for."""
    monkeypatch.setenv("HVS_I8_ROTATE", "1")
    d = make_data(profile)
    with Both(PKG.Engine(0), I8, d.nodes[:N]) as b:
        mutate(b, d)
        t = b.query(d.Q, 1.0, "D")
        assert t.engine == I8 and t.flags & I8_ROTATED
        t = b.tombstones(d.Q0, strict=False, survivors=False, what="D")
        assert t.engine == I8 and t.flags & I8_ROTATED
        b.reindex()
        t = b.query(d.Q, 1.0, "D reindexed")
        assert t.engine == I8 and t.flags & I8_ROTATED
        b.tombstones(d.Q0, strict=False, survivors=False, what="D reindexed")
        b.compact()
        t = b.query(d.Q, 1.0, "D compacted")
        assert t.engine == I8 and t.flags & I8_ROTATED
        with A.fresh(I8, b.m.rows) as f:
            for sp in (1.0, 0.5):
                for q in (d.Q, d.Q0):
                    got, want = b.e.query(q, sp), f.query(q, sp)
                    tg, tw = b.e.last_timing(), f.last_timing()
                    assert same(got, want) and (tg.engine, tg.flags, tg.pairs) == (tw.engine, tw.flags, tw.pairs), sp


# ---- E. non-finite contents of a stale row at a rebuild ----------------------------------------------------------------------
def test_non_finite_stale_rows_at_a_rebuild(monkeypatch):
    """Five indexed rows are updated to inf / nan contents: stale, the INT8 tiles stay.  hvs_set_engine(F16) then rebuilds from D
    as it is now (kept as it was, not judged -- the engine that runs is printed); the answers are the oracle's
    throughout."""
    monkeypatch.setenv("HVS_I8_ROTATE", "0")
    d = make_data()
    ids = np.array([11, 7_000, 20_001, 33_333, N - 1], np.uint32)
    bad = d.repl[:5].copy()
    bad[0, 7], bad[1, 52], bad[2, 101], bad[3, 1], bad[4, 0] = np.inf, -np.inf, np.nan, np.nan, np.inf
    with Both(PKG.Engine(0), I8, d.nodes[:N]) as b:
        b.update(ids, bad)
        assert b.m.stats() == (N, 0, 5, 0)
        t = b.query(d.Q, 1.0, "E stale non-finite rows")
        assert t.engine == I8
        b.query(d.Q0, 1.0, "E stale non-finite rows, Q0")
        b.e.set_engine(F16)
        t = b.query(d.Q, 1.0, "E set_engine(F16)")
        print("E: set_engine(F16) with non-finite stale rows in D: engine", t.engine, "flags", t.flags)
        b.query(d.Q, 0.5, "E set_engine(F16), sp = 0.5")
        b.update(ids, d.repl[5:10])                                 # finite again (still stale)
        b.e.set_engine(I8)
        t = b.query(d.Q, 1.0, "E finite again, set_engine(I8)")
        print("E: finite again, set_engine(I8): engine", t.engine, "flags", t.flags)
        b.reindex()
        assert b.m.stats() == (N, 0, 0, 1)
        t = b.query(d.Q, 1.0, "E reindexed")
        assert t.engine == I8
        b.query(d.Q0, 1.0, "E reindexed, Q0")


# ---- F. the walk ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", R.WALK_SEEDS)
def test_the_walk(seed, monkeypatch):
    """rowset_model.walk(seed, 30) on one context with the tail limit 1000 (folds happen by the rule).  The stats after every op, the
    oracle and `pairs` after every query op, and after every hvs_set_engine the Q0 figures of A when a filter answered
    (dead_survivors, stale_survivors and fallback_queries where Q0's precondition, 256 k live rows, holds)."""
    monkeypatch.delenv("HVS_I8_ROTATE", raising=False)
    d = make_data()
    with Both(PKG.Engine(0), AUTO, d.nodes[:N], R.WALK_LIMIT) as b:
        for i, op in enumerate(R.walk(seed, R.WALK_STEPS)):
            kind, what = op[0], f"F {seed} op {i} {op[0]}"
            if kind == "delete":
                b.delete(op[1])
            elif kind == "revive":
                b.set_mask(op[1])
            elif kind == "append":
                b.append(R.pool_rows(d.pool, op[1], op[2]))
            elif kind == "update":
                b.update(op[1], R.pool_rows(d.pool, op[2], op[1].size))
            elif kind in ("reindex", "compact", "trim"):
                getattr(b, kind)()
            elif kind == "set_k":
                b.set_k(op[1])
            elif kind == "query":
                b.query(d.Q, op[1], what)
            else:
                assert kind == "set_engine"
                b.e.set_engine(op[1])
                t = b.query(d.Q0, 1.0, what + f"({op[1]}) Q0")
                if op[1] != AUTO:
                    assert t.engine == op[1], "the requested engine did not run"
                if t.engine in FILTERS:
                    ms, us = b.e.mask_stats(), b.e.update_stats()
                    assert ms.tiles_patched == b.m.patched, (what, ms.tiles_patched, b.m.patched)
                    if b.m.n_live >= 256 * b.m.k:
                        assert (ms.dead_survivors, us.stale_survivors, t.fallback_queries) == (0, 0, 0), what
            b.same_stats()
            print(what, "stats", b.m.stats(), "n", b.m.n, "dead", b.m.n_dead, "k", b.m.k)


# ---- G. one child process: many batches on two lanes, retry batches before the demotion -------------------------------------------
_CHILD = r"""
import sys
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import test_rowset_formats as F
F.scenario_b(F.make_data(), None, first_load_unprobed=True)
print('SUBPROCESS-OK')
"""


def test_scenario_b_with_small_batches_and_failing_guesses():
    """HVS_MFMA_BATCH=256 HVS_EXACT_BATCH=512 HVS_GUESS_PFAIL=1 (read when the library is loaded, hence the child): the FAR call is
    two batches on two lanes, and guessed thresholds fail, so retry batches run before the demotion.  Under HVS_GUESS_PFAIL=1 the
    planner's probe sees its guesses fail and plans FP16 tiles at the load (recorded above), from which nothing can be demoted: the
    child loads with the probe off (INT8 by the model) and probes at every later index build."""
    _start()
    env = dict(os.environ, HVS_MFMA_BATCH="256", HVS_EXACT_BATCH="512", HVS_GUESS_PFAIL="1")
    env.pop("HVS_I8_ROTATE", None)
    try:
        r = subprocess.run([sys.executable, "-c", _CHILD], capture_output=True, text=True, env=env, cwd=T.REPO, timeout=600)
    except subprocess.TimeoutExpired:
        _stopped.append("the child process of scenario B ran into its time limit")
        pytest.fail(_stopped[-1])
    print(r.stdout[-6000:])
    if r.returncode < 0 or r.returncode > 128:
        _stopped.append("the child process of scenario B exited %d" % r.returncode)
    assert r.returncode == 0 and "SUBPROCESS-OK" in r.stdout, "exit %d\n" % r.returncode + r.stdout[-3000:] + r.stderr[-3000:]
