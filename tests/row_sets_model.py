"""Host model of the shared row sets (include/hvs.h "shared row sets"), and the sets the GPU tests attach.

The contract, restated.  full(q) is every matched key of query q in key order (tests/after_model.py).  A context holds bitmaps
over the rows of D; query q carries a set index or NONE (0xFFFFFFFF).  The answer is that of the exclusion lists' model
(tests/exclude_model.py) with one clause swapped: from full(q), cut by the cap, the keys whose row is OUTSIDE q's set are dropped
(with the keys of q's exclusion list, if there is one), then the page of k slots behind the cursor follows, padded or with empty
slots.  Pad rows are taken whether in the set or not.  An empty set matches nothing; NONE restricts nothing.

The model shares nothing with the engines.  compact() is the plain-numpy form of hvs_row_sets_compact_plan.
"""
import numpy as np

import after_model as A
import exclude_model as X

EMPTY = A.EMPTY
NONE = np.uint32(0xFFFFFFFF)
ROW_SETS_MAX = 256


def outside(sets, s):
    """ids of the rows that are NOT in set s (none for NONE)"""
    if s == NONE:
        return np.empty(0, np.uint32)
    return np.flatnonzero(~sets[int(s)]).astype(np.uint32)


def complements(sets, idx, lists=None):
    """per query the ids its set keeps out, with the query's own exclusion list where there is one"""
    comp = {int(s): outside(sets, s) for s in np.unique(idx)}
    return [comp[int(idx[q])] if lists is None else np.concatenate([comp[int(idx[q])], np.asarray(lists[q], np.uint32)]) for q in range(len(idx))]


def answers(fulls, sets, idx, k, cursors=None, caps=None, lists=None, pad_ids=None, pad_dists=None, padding=False):
    """-> (ids[nq][k], dists[nq][k], kept[nq]): kept = the non-pad slots of every query"""
    return X.answers(fulls, complements(sets, idx, lists), k, cursors, caps, pad_ids, pad_dists, padding)


def refused_at_least(fulls, sets, idx, got_ids, got_dists, caps=None, cursors=None):
    """Lower bound of hvs_row_sets_info.refused_keys, written as the exclusion model's: rows outside the query's set that are
    matched keys of their query (within cap, behind the cursor) strictly nearer than the answer's last kept key."""
    return X.refused_at_least(fulls, complements(sets, idx), got_ids, got_dists, caps, cursors)


def compact(sets, live):
    """the sets after a compaction under the mask `live`: the columns of the live rows, in order"""
    return np.ascontiguousarray(np.asarray(sets, bool)[:, np.asarray(live, bool)])


# ---- the sets the GPU tests attach over within_model.data(): N rows ----
def id_hash(n):
    """a fixed 32-bit mix of the row id (no engine code is involved)"""
    x = np.arange(n, dtype=np.uint64)
    x = (x * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(2246822519)) & np.uint64(0xFFFFFFFF)
    x ^= x >> np.uint64(13)
    return x.astype(np.uint32)


N_SETS = 7


def the_sets(n):
    """set 0 all rows, 1 no row, 2 about a half, 3 about a tenth, 4 about 0.1 % (by the id hash), 5 ids < n / 3, 6 every second id"""
    h = id_hash(n)
    ids = np.arange(n)
    sets = np.zeros((N_SETS, n), bool)
    sets[0] = True
    sets[2] = h % 2 == 0
    sets[3] = (h >> 3) % 10 == 0
    sets[4] = (h >> 7) % 1000 == 0
    sets[5] = ids < n // 3
    sets[6] = ids % 2 == 0
    return sets


def query_sets(nq):
    """query i takes set i % 8, with 7 -> NONE"""
    idx = (np.arange(nq) % 8).astype(np.uint32)
    idx[idx == 7] = NONE
    return idx


def tie_query(queries, info):
    """the query of tests/in_edges.py's tie data that matches every row and lies ON the vector u: a run of 150 distances 0"""
    at = [i for i in info["on_u"] if queries[i, 0] == 0]
    assert len(at) == 1
    return at[0]
