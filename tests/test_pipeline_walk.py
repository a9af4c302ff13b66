"""One context walked through the states of the host <-> device copy pipeline of hvs_query and hvs_load_data: the
rings of pinned staging slots as they are first made, grown, rebuilt for a larger k, wrapped and bypassed, and the lanes'
hand-over when a call is many batches long.

Every hvs_query answer is compared BIT FOR BIT, ids and distances, with the resident path's answer on the same context
(upload_queries, query_resident, download_results).  Before each host call the resident query buffer is overwritten with other
queries, so a batch that runs before its input was staged cannot compare equal by accident, and the caller's arrays are
pre-filled with 0xDEADBEEF / -1, so a row that was never drained cannot either.  A sample of 32 queries per step is checked
against the oracle as well.

D: 40 000 gen-v1 rows (above the filter engines' minimum, so a filter engine answers); k starts at 100.  The steps, in order on
ONE context -- each reaches a state of the pipe its predecessors did not:
  1. no reserve; 1 000 queries, pageable in and out, ids only: result slot 0 is small (4 096 queries);
  2. the same with distances: the distance slot is allocated after the id slot;
  3. 70 001 queries with distances: slot 0 grows to a whole slot, slot 1 is partial;
  4. set_k(200) and 5 000 queries (the result slots are rebuilt for the larger k; list capacity 512); set_k(100) and 70 001
     queries (slots sized for 200, copies strided by 100); the same 70 001 queries once more with a result cursor each;
  5. 300 000 queries, pageable in, pinned out: the input ring wraps (5 pieces over 4 slots), the output ring is bypassed; two
     queries with an inf component, in the first and the last piece, are answered by the exact engine and fetched again;
  6. the same, pinned in, pageable out: the output ring wraps and is drained from inside the copy-out;
  7. 70 001 queries, ids pinned and distances pageable: the mixed case takes the staged path;
  8. load_data of 300 000 pageable rows (more than the ring's 4 x 65 536 x 104 floats: the upload wraps), download_data equals
     the source; the same from a pinned copy; 1 000 queries after each load;
  9. a second context with reserve(300 000) before its first call repeats step 5: the same answers;
 10. Engine(devices=[0, 0]) under both gather modes, 140 000 queries (two pieces per leaf), one inf query in the second leaf's
     range (under the peer gather its row leaves through the row-by-row branch): the single-GPU answers.

The walk runs in a child process (the batch size and the lane switch are read when the library loads): with the default batch
size, with HVS_MFMA_BATCH=16384 -- steps 5, 6 and 9 are then many batches on two lanes -- and with that and HVS_LANES=0."""
import os

import pytest

import hvs_testlib as T

pytestmark = pytest.mark.gpu
CHILD_TIMEOUT = 300

_CHILD = r"""
import importlib, json, sys, time, numpy as np, torch
sys.path.insert(0, 'tests'); sys.path.insert(0, '.')
import hvs_testlib as T
PKG = importlib.import_module('project---hybrid-vector-search-queries_amd')
FILTERS = (PKG.ENGINE_MFMA_I8, PKG.ENGINE_MFMA_F16, PKG.ENGINE_MFMA_FILTER)
N, NQ, NCAT, NROWS = 40_000, 300_000, 20, 300_000
nodes = T.gen_data(N, 61, T.GEN_V1, NCAT)
Q = T.gen_queries(NQ, 62, T.GEN_V1, NCAT)
POISON = T.gen_queries(NQ, 63, T.GEN_V1, NCAT)
QINF = Q.copy(); QINF[70, 8] = np.inf; QINF[NQ - 1, 9] = np.inf       # first and last of the 5 pieces
Q140 = Q[:140_000].copy(); Q140[100_000, 8] = np.inf                   # in the second leaf's range
obs, clock = [], [time.time()]

def pinned(shape, dt):
    return torch.empty(shape, dtype=dt).pin_memory().numpy()

def pinned_copy(a):
    p = pinned(a.shape, torch.float32); p[:] = a
    return p

def out_arrays(nq, k, dists, pin_ids, pin_dists):
    ids = pinned((nq, k), torch.int32).view(np.uint32) if pin_ids else np.empty((nq, k), np.uint32)
    ids[:] = 0xDEADBEEF
    d = None
    if dists:
        d = pinned((nq, k), torch.float32) if pin_dists else np.empty((nq, k), np.float32)
        d[:] = -1
    return ids, d

def resident(e, q, after=None):
    e.upload_queries(q)
    if after is not None: e.set_after(*after)
    e.query_resident(0, len(q), 1.0); e.sync()
    return e.download_results(0, len(q))

def same(step, ids, d, want):
    bad = np.nonzero((ids != want[0]).any(axis=1))[0]
    assert bad.size == 0, '%s: ids differ from the resident path in %d queries, first %d' % (step, bad.size, bad[0])
    if d is not None:
        bad = np.nonzero((d.view(np.uint32) != want[1].view(np.uint32)).any(axis=1))[0]
        assert bad.size == 0, '%s: distances differ from the resident path in %d queries, first %d' % (step, bad.size, bad[0])

def sample(nq, *extra):
    return np.unique(np.r_[np.linspace(0, nq - 1, 32 - len(extra)).astype(np.int64), np.array(extra, np.int64)])

def oracle_check(step, data, q, ids, d, k=100, sel=None, ref_cut=None):
    sel = sample(len(q)) if sel is None else sel
    with T.oracle_k(ref_cut[2] if ref_cut else k):
        ref, _ = T.oracle_query(data, q[sel])
    if ref_cut: ref = np.ascontiguousarray(ref[:, ref_cut[0]:ref_cut[1]])
    with T.oracle_k(k):
        T.check_parity(data, q[sel], ids[sel], ref, got_dists=None if d is None else d[sel])

def note(step, **kw):
    now = time.time()
    obs.append(dict(step=step, seconds=round(now - clock[0], 2), **kw)); clock[0] = now
    print('step', obs[-1], flush=True)

def host(e, step, q, want, dists=True, pin_in=False, pin_ids=False, pin_dists=False, after=None, fallback=0, poison=True):
    # one hvs_query of `q` on a context whose resident buffer holds other queries; `want`: the resident path's answer
    if poison: e.upload_queries(POISON[:len(q)])
    ids, d = out_arrays(len(q), e.k, dists, pin_ids, pin_dists)
    e.query(pinned_copy(q) if pin_in else q, 1.0, want_dists=dists, out_ids=ids, out_dists=d, after=after)
    t = e.last_timing()
    assert t.nq == len(q) and t.engine in FILTERS, (step, t.as_dict())
    assert t.fallback_queries == fallback, (step, t.fallback_queries, fallback)
    same(step, ids, d, want)
    note(step, nq=len(q), k=e.k, launches=int(t.main_kernel_launches), fallback=int(t.fallback_queries), retried=int(t.retry_queries))
    return ids, d

with PKG.Engine(0) as e:
    e.load_data(nodes)
    q1k, q5k, q70k = Q[:1000], Q[:5000], Q[:70_001]
    w1k = resident(e, q1k)
    ids, _ = host(e, '1 small, ids only', q1k, w1k, dists=False)
    oracle_check('1', nodes, q1k, ids, None)
    ids, d = host(e, '2 small, with distances', q1k, w1k)
    oracle_check('2', nodes, q1k, ids, d)
    w70k = resident(e, q70k)
    ids, d = host(e, '3 two pieces', q70k, w70k)
    oracle_check('3', nodes, q70k, ids, d)

    e.set_k(200)
    ids, d = host(e, '4.1 k = 200', q5k, resident(e, q5k))
    assert ids.shape == (5000, 200)
    oracle_check('4.1', nodes, q5k, ids, d, k=200)
    e.set_k(100)
    ids, d = host(e, '4.2 k back to 100', q70k, resident(e, q70k))
    same('4.2 against step 3', ids, d, w70k)
    cursor = (d[:, 49].copy(), ids[:, 49].copy())
    ids, d = host(e, '4.3 with cursors', q70k, resident(e, q70k, after=cursor), after=cursor)
    every = np.nonzero(q70k[:, 0] == 0)[0]                            # (no predicate: rows 50..149 exist, no padding)
    oracle_check('4.3', nodes, q70k, ids, d, sel=every[np.linspace(0, every.size - 1, 32).astype(np.int64)], ref_cut=(50, 150, 200))

    winf = resident(e, QINF)
    sel_inf = sample(NQ, 70)
    ids5, d5 = host(e, '5 input ring wraps, pinned out', QINF, winf, pin_ids=True, pin_dists=True, fallback=2)
    oracle_check('5', nodes, QINF, ids5, d5, sel=sel_inf)
    ids, d = host(e, '6 pinned in, output ring wraps', QINF, winf, pin_in=True, fallback=2)
    oracle_check('6', nodes, QINF, ids, d, sel=sel_inf)
    ids, d = host(e, '7 ids pinned, distances pageable', q70k, w70k, pin_ids=True)
    oracle_check('7', nodes, q70k, ids, d)
    w140 = resident(e, Q140)

    rows = T.gen_data(NROWS, 71, T.GEN_V1, NCAT)
    assert rows.size > 4 * 65536 * 104
    for tag, src in (('8 load from pageable rows', rows), ('8 load from pinned rows', pinned_copy(rows))):
        e.load_data(src)
        back = e.download_data(0, NROWS)
        assert np.array_equal(back.view(np.uint32), rows.view(np.uint32)), tag
        del back
        note(tag, n=NROWS)
        ids, d = host(e, tag + ', queries', q1k, resident(e, q1k))
    oracle_check('8', rows, q1k, ids, d)
    del rows

with PKG.Engine(0) as e:
    e.load_data(nodes)
    e.reserve(NQ)
    ids, d = host(e, '9 reserved context', QINF, (ids5, d5), pin_ids=True, pin_dists=True, fallback=2, poison=False)
    oracle_check('9', nodes, QINF, ids, d, sel=sel_inf)
del ids5, d5, winf

with PKG.Engine(devices=[0, 0]) as e:
    e.load_data(nodes)
    for mode in (0, 1):
        e.set_gather(mode)
        e.upload_queries(POISON[:len(Q140)])
        ids, d = out_arrays(len(Q140), 100, True, False, False)
        e.query(Q140, 1.0, out_ids=ids, out_dists=d)
        same('10 gather mode %d' % mode, ids, d, w140)
        t = e.last_timing()
        note('10 two virtual ranks, gather mode %d' % mode, nq=int(t.nq), fallback=int(t.fallback_queries))
    oracle_check('10', nodes, Q140, ids, d, sel=sample(len(Q140), 100_000))
print('RESULT ' + json.dumps(obs))
"""

MODES = {"default_batch": {}, "batch_16384": {"HVS_MFMA_BATCH": "16384"}, "batch_16384_one_lane": {"HVS_MFMA_BATCH": "16384", "HVS_LANES": "0"}}


@pytest.mark.parametrize("mode", list(MODES))
def test_walk(mode):
    env = dict(os.environ)
    for name in ("HVS_MFMA_BATCH", "HVS_LANES", "HVS_TEST_NO_SPARE"):
        env.pop(name, None)
    env.update(MODES[mode])
    obs = T.run_child(_CHILD, {}, env, "pipeline-walk-" + mode, CHILD_TIMEOUT)
    for o in obs:
        print(o)
    steps = [o["step"] for o in obs]
    assert len(steps) == 16 and steps[0].startswith("1 ") and steps[-1].endswith("gather mode 1"), steps
    by = {o["step"]: o for o in obs}
    if mode != "default_batch":      # 300 000 queries in batches of at most 16 384: 19 batches or more, a filter launch each at least
        for s in ("5 input ring wraps, pinned out", "6 pinned in, output ring wraps", "9 reserved context"):
            assert by[s]["launches"] >= 19, by[s]
