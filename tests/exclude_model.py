"""Host model of the per-query exclusion lists (include/hvs.h "per-query exclusion lists").

The contract, restated.  full(q) is every matched key of query q in key order (tests/after_model.py: predicates from
hvs_testlib._passes, distances from the oracle's exact-order function).  The answer under a list is: full(q) cut by the cap if
there is one, with every key whose id is listed dropped, then the page of k slots behind the cursor (after_model.page), padded
or with empty slots.  Pad rows are taken whether listed or not.  A listed id is only compared with row ids, so ids that name no
matched row -- 0xFFFFFFFF, ids >= n, ids behind the sampled prefix, rows failing the predicate -- change nothing.

The model shares nothing with the engines.  normalise() is the plain-numpy form of hvs_exclude_plan.
"""
import numpy as np

import after_model as A

EMPTY = A.EMPTY
EXCLUDE_MAX = 1024


def csr(lists):
    """(offsets[nq + 1], ids) of a list of per-query id sequences"""
    rows = [np.asarray(r, np.uint32).ravel() for r in lists]
    off = np.zeros(len(rows) + 1, np.uint32)
    if rows:
        off[1:] = np.cumsum([r.size for r in rows])
    return off, (np.concatenate(rows).astype(np.uint32) if rows else np.empty(0, np.uint32))


def normalise(lists, row0=0, n_rows=0xFFFFFFFF):
    """Per query np.unique of the ids it keeps -- not 0xFFFFFFFF, inside [row0, row0 + n_rows) -- minus row0.
    -> (kept, begin[nq], count[nq], ids) laid out as hvs_exclude_plan lays them out: query q's list at begin[q] = its raw
    offset, the rest of its raw extent 0xFFFFFFFF; or None for a list longer than EXCLUDE_MAX."""
    off, raw = csr(lists)
    nq = len(lists)
    if any(len(r) > EXCLUDE_MAX for r in lists):
        return None
    begin, count = off[:nq].copy(), np.zeros(nq, np.uint32)
    ids = np.full(raw.size, EMPTY, np.uint32)
    for q in range(nq):
        r = raw[off[q]:off[q + 1]].astype(np.int64)
        keep = (r != 0xFFFFFFFF) & (r >= row0) & (r < int(row0) + int(n_rows))
        u = np.unique(r[keep] - row0).astype(np.uint32)
        count[q] = u.size
        ids[off[q]:off[q] + u.size] = u
    return int(count.sum()), begin, count, ids


def drop_listed(full, listed):
    """full = (ids, dists) in key order without the keys whose id is in `listed`"""
    ids, d = full
    keep = ~np.isin(ids, np.asarray(listed, np.uint32))
    return ids[keep], d[keep]


def answers(fulls, lists, k, cursors=None, caps=None, pad_ids=None, pad_dists=None, padding=False):
    """-> (ids[nq][k], dists[nq][k], kept[nq]): kept = the non-pad slots of every query"""
    nq = len(fulls)
    out_i, out_d, n = np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32), np.zeros(nq, np.int64)
    for q in range(nq):
        f = fulls[q] if caps is None else A.cap_full(fulls[q], caps[q])
        f = drop_listed(f, lists[q])
        cur = None if cursors is None else (cursors[0][q], cursors[1][q])
        out_i[q], out_d[q], n[q] = A.page(f, cur, k, None if not padding else (pad_ids, pad_dists[q]), padding)
    return out_i, out_d, n


def refused_at_least(fulls, lists, got_ids, got_dists, caps=None, cursors=None):
    """Lower bound of hvs_exclude_info.refused_keys: listed rows that are matched keys of their query (within cap, behind the
    cursor) strictly nearer than the answer's last kept key -- each of them was admitted by every other test of the pass that
    gave the answer, so each was refused at least once."""
    total = 0
    for q in range(len(fulls)):
        kept = got_ids[q] != EMPTY
        if not kept.any():
            continue
        last = A.keys_of(got_ids[q][kept], got_dists[q][kept]).max()
        f = fulls[q] if caps is None else A.cap_full(fulls[q], caps[q])
        keys = A.keys_of(*f)
        sel = np.isin(f[0], np.asarray(lists[q], np.uint32)) & ((keys >> np.uint64(32)) < (last >> np.uint64(32)))
        if cursors is not None:
            ck = A.cursor_key(cursors[0][q], cursors[1][q])
            sel &= (keys > np.uint64(ck)) if ck is not None else False
        total += int(sel.sum())
    return total


# ---- list shapes the normalisation must get right, at lengths on both sides of every wave and power-of-two boundary ----
LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024)
N_ROWS = 5000          # "n" of the shapes below: ids >= N_ROWS name no row of today


def shaped_lists(length, rng):
    """One list of `length` raw entries in each shape the normalisation must get right."""
    base = rng.choice(N_ROWS, max(length, 1), replace=False).astype(np.uint32)[:length]
    mixed = base.copy()
    mixed[::3] = EMPTY                                                      # 0xFFFFFFFF mixed in
    beyond = base.copy()
    beyond[1::2] = beyond[1::2] + np.uint32(N_ROWS)                         # ids >= n
    few = rng.choice(base, length) if length else base                      # duplicates in random order
    return [np.full(length, 77, np.uint32),                                 # all equal
            np.sort(base)[::-1].copy(),                                     # strictly descending
            np.sort(base),                                                  # already sorted
            mixed, beyond, few, base]


def all_shapes():
    """every shape at every length of LENGTHS: the lists of the normalisation tests, on the host and on the device"""
    rng = np.random.default_rng(5)
    return [lst for length in LENGTHS for lst in shaped_lists(length, rng)]


# ---- the lists the GPU tests attach (tests/test_exclude.py, test 1): query i takes rule i % 8 ----
def rule_lists(fulls, nodes_n, sn, k, passes_none):
    """`passes_none(q)`: ids of up to 400 rows of [0, sn) that FAIL query q's predicate."""
    lists = []
    for i, (ids, _) in enumerate(fulls):
        rule = i % 8
        if rule == 0:
            lst = np.empty(0, np.uint32)
        elif rule == 1:
            lst = ids[:1]
        elif rule == 2:
            lst = ids[:k]
        elif rule == 3:
            lst = ids[:EXCLUDE_MAX][::-1]                                   # descending: the device sorts
        elif rule == 4:
            lst = ids[:2 * k:2]
        elif rule == 5:
            beyond = np.arange(nodes_n, nodes_n + 312, dtype=np.uint32)       # ids >= n
            behind = np.arange(sn, min(nodes_n, sn + 312), dtype=np.uint32)   # ids behind the sampled prefix (none when sn == n)
            fail = np.asarray(passes_none(i), np.uint32)[:400]
            lst = np.concatenate([beyond, behind, fail])
            lst = np.concatenate([lst, np.arange(2 * nodes_n, 2 * nodes_n + EXCLUDE_MAX - lst.size, dtype=np.uint32)])
        elif rule == 6:
            lst = ids if ids.size <= EXCLUDE_MAX else ids[:3]
        else:
            page1 = np.full(k, EMPTY, np.uint32)                              # the unpadded page 1, empty slots left in
            m = min(k, ids.size)
            page1[:m] = ids[:m]
            lst = np.concatenate([[EMPTY], page1, page1[:3]])                 # ... an empty slot in front, and duplicates
        lists.append(np.ascontiguousarray(lst, np.uint32))
    return lists
