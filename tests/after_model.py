"""Host model of the per-query result cursors (include/hvs.h "per-query result cursors").

The contract, restated.  full(q) is every matched key of query q -- rows of the sampled prefix that pass its predicate -- in key
order: distance bits ascending (one NaN, 0x7FC00000, above +inf), then id.  The answer with cursor c is the first k keys of
full(q) that are strictly greater than c, then padding rows (or empty slots, 0xFFFFFFFF / +inf, with padding off), the k slots
in key order.  A cursor whose id is 0xFFFFFFFF is exhausted and matches nothing.  The key order is total, so every comparison
made with this model is exact equality of ids and of distance bits: nothing is loosened for ties.

The reference shares nothing with the code under test: predicates from hvs_testlib._passes, distances from the oracle's
exact-order function.
"""
import numpy as np

import hvs_testlib as T

EMPTY = np.uint32(0xFFFFFFFF)
EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
NAN_BITS = 0x7FC00000


def keys_of(ids, dists):
    """(dist bits with the canonical NaN) << 32 | id"""
    d = np.ascontiguousarray(dists, np.float32)
    bits = np.where(np.isnan(d), np.uint32(NAN_BITS), d.view(np.uint32)).astype(np.uint64)
    return (bits << np.uint64(32)) | np.asarray(ids, np.uint32).astype(np.uint64)


def cursor_key(after_dist, after_id):
    """The cursor's key, or None for an exhausted cursor."""
    if int(after_id) == 0xFFFFFFFF:
        return None
    return int(keys_of(np.array([after_id], np.uint32), np.array([after_dist], np.float32))[0])


def _dists(nodes, q, ids, order):
    """exact-order distances of one query to the rows `ids`, through the oracle in rows of at most 256 ids"""
    m = ids.size
    if m == 0:
        return np.empty(0, np.float32)
    c = int(min(256, max(8, m)))
    rows = -(-m // c)
    grid = np.zeros(rows * c, np.uint32)
    grid[:m] = ids
    with T.oracle_k(c):
        d = T.oracle_dists_for_ids(nodes, np.tile(np.ascontiguousarray(q, np.float32), (rows, 1)), grid.reshape(rows, c), order)
    return d.ravel()[:m]


def full_order(nodes, queries, sn, order="simd"):
    """Per query (ids, dists) of ALL its matched rows among rows [0, sn), in key order; NaN distances carry the canonical bits."""
    counts = T.passing_rows_per_query(nodes[:sn], queries)
    out = []
    for qi, q in enumerate(queries):
        ids = np.flatnonzero(T._passes(nodes[:sn], q)).astype(np.uint32)
        valid = -1.0 < q[0] < 4.0
        assert not valid or ids.size == counts[qi], (qi, ids.size, counts[qi])
        d = _dists(nodes, q, ids, order)
        d = d.copy()
        d.view(np.uint32)[np.isnan(d)] = NAN_BITS
        at = np.argsort(keys_of(ids, d), kind="stable")
        out.append((ids[at], d[at]))
    return out


def page(full, cursor, k, pads=None, padding=False):
    """The law: full = (ids, dists) of one query in key order, cursor = (after_dist, after_id) or None for "no cursor",
    pads = (pad_ids[k], pad_dists[k]).  -> (ids[k], dists[k], n_after)."""
    ids, d = full
    keys = keys_of(ids, d)
    if cursor is None:
        first = 0
    else:
        ck = cursor_key(*cursor)
        first = ids.size if ck is None else int(np.searchsorted(keys, np.uint64(ck), "right"))
    take = min(k, ids.size - first)
    out_i = np.full(k, EMPTY, np.uint32)
    out_d = np.full(k, np.inf, np.float32)
    out_k = np.full(k, EMPTY_KEY, np.uint64)
    out_i[:take], out_d[:take], out_k[:take] = ids[first:first + take], d[first:first + take], keys[first:first + take]
    if padding and take < k:
        m = k - take
        out_i[take:] = np.asarray(pads[0], np.uint32)[:m]
        out_d[take:] = np.asarray(pads[1], np.float32)[:m]
        out_d[take:].view(np.uint32)[np.isnan(out_d[take:])] = NAN_BITS
        out_k[take:] = keys_of(out_i[take:], out_d[take:])
        at = np.argsort(out_k, kind="stable")
        out_i, out_d = out_i[at], out_d[at]
    return out_i, out_d, take


def pages(fulls, cursors, k, pad_ids=None, pad_dists=None, padding=False):
    """page() over all queries: cursors = None or (dists[nq], ids[nq]); pad_dists [nq][k].  -> (ids[nq][k], dists[nq][k], n_after[nq])"""
    nq = len(fulls)
    out_i, out_d, n = np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32), np.zeros(nq, np.int64)
    for q in range(nq):
        cur = None if cursors is None else (cursors[0][q], cursors[1][q])
        out_i[q], out_d[q], n[q] = page(fulls[q], cur, k, None if not padding else (pad_ids, pad_dists[q]), padding)
    return out_i, out_d, n


def last_slots(ids, dists):
    """The cursors that continue behind an UNPADDED page: its last slots."""
    return np.ascontiguousarray(dists[:, -1], np.float32), np.ascontiguousarray(ids[:, -1], np.uint32)


def cap_full(full, cap):
    """full(q) under a distance cap (the cap first, then the cursor): the keys with dist <= cap, none for a NaN or negative cap"""
    ids, d = full
    cap = np.float32(cap)
    with np.errstate(invalid="ignore"):
        keep = d <= cap
    if np.isnan(cap) or cap < 0:
        keep = np.zeros(ids.size, bool)
    return ids[keep], d[keep]
