"""Host model of the per-query distance caps (include/hvs.h "per-query distance caps"), and the inputs the cap
tests share.

The contract, restated: the matched rows of a query in key order (distance bits, then id) have the rows within the cap as a
prefix, so the capped answer is the UNCAPPED, UNPADDED answer with every slot where not (dist <= cap) made empty, and with
padding on the empty slots are then filled from the pad list (rows n-1, n-2, ..., or the last live ids under a mask) and the k
keys are put in key order again (pad rows may be nearer than matched ones).  A NaN distance is within no cap; a NaN or
negative cap matches nothing.
"""
import numpy as np

import hvs_testlib as T

EMPTY = np.uint32(0xFFFFFFFF)
N, NCAT = 1 << 17, 10     # the data set of tests/test_partitioned.py: large enough for the filter engines to run


def _keys(ids, dists):
    bits = np.ascontiguousarray(dists, np.float32).view(np.uint32).astype(np.uint64)
    bits = np.where(np.isnan(dists), np.uint64(0x7FC00000), bits)
    return (bits << np.uint64(32)) | ids.astype(np.uint64)


def capped_row(ids, dists, cap, pad_ids=None, pad_dists=None, padding=True):
    """One uncapped, unpadded answer row (k slots; empty = 0xFFFFFFFF / +inf) -> (ids, dists, n_within) of the capped row."""
    ids = np.asarray(ids, np.uint32)
    dists = np.asarray(dists, np.float32)
    k = ids.size
    cap = np.float32(cap)
    with np.errstate(invalid="ignore"):
        keep = (ids != EMPTY) & (dists <= cap)
    if np.isnan(cap) or cap < 0:
        keep[:] = False
    n_in = int(keep.sum())
    out_ids = np.full(k, EMPTY, np.uint32)
    out_d = np.full(k, np.inf, np.float32)
    out_ids[:n_in], out_d[:n_in] = ids[keep], dists[keep]
    keys = np.full(k, np.uint64(0xFFFFFFFFFFFFFFFF), np.uint64)
    keys[:n_in] = _keys(out_ids[:n_in], out_d[:n_in])
    if padding:
        m = k - n_in
        out_ids[n_in:], out_d[n_in:] = np.asarray(pad_ids, np.uint32)[:m], np.asarray(pad_dists, np.float32)[:m]
        out_d[n_in:][np.isnan(out_d[n_in:])] = np.float32(np.nan)
        keys[n_in:] = _keys(out_ids[n_in:], out_d[n_in:])
    order = np.argsort(keys, kind="stable")
    out_d = out_d[order]
    nan = np.isnan(out_d)
    out_d.view(np.uint32)[nan] = 0x7FC00000       # the engines' keys carry one NaN
    return out_ids[order], out_d, n_in


def capped_answers(ids, dists, caps, pad_ids=None, pad_dists=None, padding=True):
    """capped_row over a whole answer: ids / dists [nq][k] uncapped and unpadded, caps [nq]; pad_ids [k] (the same rows pad every
    query), pad_dists [nq][k].  -> (ids, dists, n_within[nq])"""
    out_i, out_d, n_in = np.empty_like(ids), np.empty_like(dists), np.zeros(len(ids), np.int64)
    for q in range(len(ids)):
        out_i[q], out_d[q], n_in[q] = capped_row(ids[q], dists[q], caps[q], pad_ids, None if pad_dists is None else pad_dists[q], padding)
    return out_i, out_d, n_in


def choose_caps(dists, ids, first=0):
    """Caps from each query's own uncapped, unpadded distances, so that boundaries are hit exactly.  Query q takes rule
    (q + first) % 8 of: the 0th, 9th and last matched distance bit-exact (`<=` keeps that slot and its ties), nextafter below
    the 0th (nothing within), twice the last (all within), +inf, NaN, -1.  A query that matched fewer rows takes the last one it
    has; one that matched none takes 1.0 in place of a distance."""
    k = dists.shape[1]
    caps = np.empty(len(dists), np.float32)
    for q in range(len(dists)):
        m = int((ids[q] != EMPTY).sum())
        d = dists[q][:m]
        d = d[np.isfinite(d)]
        at = (lambda j: d[min(j, d.size - 1)]) if d.size else (lambda j: np.float32(1.0))
        rule = (q + first) % 8
        caps[q] = (at(0), at(9), at(k - 1), np.nextafter(at(0), np.float32(-np.inf), dtype=np.float32), np.float32(2.0) * at(k - 1),
                   np.float32(np.inf), np.float32(np.nan), np.float32(-1.0))[rule]
    return caps


def caps_below_nearest(dists, ids):
    """nextafter below every query's nearest distance: no row is within any cap."""
    one = np.where(ids[:, 0] != EMPTY, dists[:, 0], np.float32(1.0)).astype(np.float32)
    one = np.where(np.isfinite(one), one, np.float32(1.0)).astype(np.float32)
    return np.nextafter(one, np.float32(-np.inf), dtype=np.float32)


def unpadded_from_padded(ids, dists, matches, n_total):
    """The oracle pads: its row holds min(matches, k) matched rows and the pad rows n-1, n-2, ... in key order.  -> the row without
    the pad rows (which pad slot of equal keys is dropped does not matter), matched rows first, then empty slots."""
    k = ids.shape[1]
    out_i = np.full_like(ids, EMPTY)
    out_d = np.full_like(dists, np.inf)
    for q in range(len(ids)):
        m = min(int(matches[q]), k)
        keep = np.ones(k, bool)
        for pad in range(n_total - 1, n_total - 1 - (k - m), -1):
            at = np.flatnonzero(keep & (ids[q] == pad))
            keep[at[-1]] = False
        out_i[q, :m], out_d[q, :m] = ids[q][keep], dists[q][keep]
    return out_i, out_d


def pad_rows(nodes, queries, k, pad_ids=None, order="simd"):
    """(pad_ids[k], pad_dists[nq][k]): rows n-1, n-2, ... (or the given ids) and their exact-order distances to every query."""
    n = nodes.shape[0]
    if pad_ids is None:
        pad_ids = np.arange(n - 1, n - 1 - k, -1).astype(np.uint32)
    with T.oracle_k(k):
        d = T.oracle_dists_for_ids(nodes, queries, np.tile(np.asarray(pad_ids, np.uint32), (len(queries), 1)), order)
    return np.asarray(pad_ids, np.uint32), d


# ---- the data set and queries of the cap tests: gen-v1 rows with hand-placed categories (the pools of tests/test_partitioned.py),
# 224 mixed gen-v1 queries, 12 on the placed categories, 5 that match nothing or have non-finite components
def data():
    nodes = T.gen_data(N, 91, T.GEN_V1, NCAT)
    rng = np.random.default_rng(11)
    body = [(0, 43691), (43691, 87382), (87382, N - 256)]
    for cat, counts in ((1001, (5, 0, 60)), (1002, (33, 33, 34)), (1003, (0, 99, 0)), (1006, (50, 50, 50)), (1007, (3, 0, 0))):
        for cnt, (a, b) in zip(counts, body):
            free = np.flatnonzero(nodes[a:b, 0] < 1000) + a
            nodes[rng.choice(free, cnt, replace=False), 0] = np.float32(cat)
    free = np.flatnonzero(nodes[N - 100:, 0] < 1000) + N - 100
    nodes[rng.choice(free, 40, replace=False), 0] = np.float32(1005)      # pad rows duplicate matches
    queries = T.gen_queries(224, 92, T.GEN_V1, NCAT)
    special = T.gen_queries(12, 93, T.GEN_V1, NCAT)
    for i, cat in enumerate((1001, 1002, 1003, 1004, 1005, 1006)):
        special[2 * i, :4] = [1, cat, -1, -1]
        special[2 * i + 1, :4] = [3, cat, 0.05, 0.95]
    special[7, :4] = [1, 1007, -1, -1]                                     # three matches
    bad = T.gen_queries(5, 94, T.GEN_V1, NCAT)
    bad[0, 0], bad[1, 0], bad[2, 0] = 7.0, -5.0, np.nan                    # invalid types: nothing matches
    bad[3, 4 + 10] = np.inf                                                # every distance +inf
    bad[4, 4 + 20] = np.nan                                                # every distance NaN
    return nodes, np.ascontiguousarray(np.concatenate([queries, special, bad]))


def matches(nodes, queries, sn):
    return np.array([int(T._passes(nodes[:sn], q).sum()) for q in queries])
