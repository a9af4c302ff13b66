"""Inputs and expectations of tests/test_exclude_edges.py: exclusion lists where the index `qi` with which a kernel
reads `begin[qi]` / `count[qi]` can go wrong -- many batches on both lanes, inner ranges of the resident set, renumbered rows.

Everything expected comes from tests/exclude_model.py on the rows of within_model.data() (N = 2^17): full(q) by
after_model.full_order (predicates from hvs_testlib._passes, distances from the oracle's exact-order function), exact on ids and
on distance bits.  Nothing here reads a GPU.

The queries: the 241 of within_model.data() and 800 more gen-v1 queries of all four types, every second of them narrowed to a
type-3 window of 20 to 400 rows (so that lists leave answers under-full), 1041 in all -- eight batches of 128 and a ragged ninth.  Query q takes list rule q % 5, so that neighbours never share a list
and a list read at a batch-local or lane-local index gives another answer:
  0  keys 1..100 of full(q)         1  keys 1..1000          2  every second key of the first 600
  3  1024 ids that match nothing (rows failing the predicate, then ids >= n)               4  empty
"""
import numpy as np

import after_model as A
import exclude_model as X
import hvs_testlib as T
import within_model as W

N, NCAT = W.N, W.NCAT
NQ = 1041
KS = (8, 100, 256)
EMPTY = A.EMPTY
BATCH = 128
_cache = {}


def workload():
    """(nodes, queries): within_model.data() and 800 more queries of the same law"""
    if "work" not in _cache:
        nodes, queries = W.data()
        more = T.gen_queries(NQ - len(queries), 95, T.GEN_V1, NCAT)
        # every second one a narrow type-3 query (a T window of 20 to 400 of its category's ~13 100 rows): a list of 100 to 1000
        # of the nearest keys then leaves fewer than k rows, or none
        rng = np.random.default_rng(96)
        for i in range(0, len(more), 2):
            l = rng.uniform(0.02, 0.9)
            more[i, 0:4] = 3.0, float(i % NCAT), l, l + rng.uniform(0.0015, 0.03)
        _cache["work"] = (nodes, np.ascontiguousarray(np.concatenate([queries, more])))
    return _cache["work"]


def fulls(sp=1.0, rows=None, tag="work", sel=None):
    """full(q) of every query (or of queries `sel`) on the sampled prefix of `rows` (default: the workload's)"""
    key = ("fulls", tag, float(sp), None if sel is None else tuple(sel))
    whole = ("fulls", tag, float(sp), None)
    if key not in _cache and whole in _cache:
        _cache[key] = [_cache[whole][q] for q in sel]
    if key not in _cache:
        nodes, queries = workload()
        rows = nodes if rows is None else rows
        sn = int(T.oracle().hvs_oracle_sn(sp, rows.shape[0]))
        _cache[key] = A.full_order(rows, queries if sel is None else queries[list(sel)], sn)
    return _cache[key]


def lists():
    """one raw list per query, rule q % 5, from full(q) at sample_proportion 1"""
    if "lists" not in _cache:
        nodes, queries = workload()
        out = []
        for q, (ids, _) in enumerate(fulls()):
            rule = q % 5
            if rule == 0:
                lst = ids[:100]
            elif rule == 1:
                lst = ids[:1000]
            elif rule == 2:
                lst = ids[:600:2]
            elif rule == 3:
                fail = np.flatnonzero(~T._passes(nodes, queries[q]))[:X.EXCLUDE_MAX].astype(np.uint32)
                lst = np.concatenate([fail, np.arange(N, N + X.EXCLUDE_MAX - fail.size, dtype=np.uint32)])
            else:
                lst = ids[:0]
            out.append(np.ascontiguousarray(lst, np.uint32))
        _cache["lists"] = out
    return _cache["lists"]


def pads(k, rows=None, tag="work"):
    key = ("pads", tag, k)
    if key not in _cache:
        nodes, queries = workload()
        _cache[key] = W.pad_rows(nodes if rows is None else rows, queries, k)
    return _cache[key]


def answers(k, padding, sp=1.0, sel=None, rows=None, tag="work", with_lists=True):
    """(ids, dists, kept) of the queries `sel` (default: all) under their lists, by exclude_model.answers"""
    key = ("answers", tag, k, padding, float(sp), None if sel is None else tuple(sel), with_lists)
    if key not in _cache:
        f = fulls(sp, rows, tag, sel)
        at = range(NQ) if sel is None else list(sel)
        lst = [lists()[q] if with_lists else lists()[q][:0] for q in at]
        pad_ids, pad_d = pads(k, rows, tag)
        _cache[key] = X.answers(f, lst, k, None, None, pad_ids, pad_d[list(at)], padding)
    return _cache[key]


# ---- inner ranges of the resident set: (q0, m); the last one straddles both owner boundaries of a three-GPU replicated context
RANGES = ((1, 63), (128, 128), (NQ - 65, 65))
STRADDLE = (NQ // 3 - 40, NQ // 3 + 90)


# ---- compaction: 5 % of the rows die; the first 241 queries carry their lists through it
NQ_COMPACT = 241


def compaction():
    """(dead ids, new_to_old, the compacted rows)"""
    if "compact" not in _cache:
        nodes, _ = workload()
        rng = np.random.default_rng(31)
        dead = np.sort(rng.choice(N, N // 20, replace=False)).astype(np.uint32)
        live = np.ones(N, bool)
        live[dead] = False
        new_to_old = np.flatnonzero(live).astype(np.uint32)
        _cache["compact"] = (dead, new_to_old, np.ascontiguousarray(nodes[new_to_old]))
    return _cache["compact"]
