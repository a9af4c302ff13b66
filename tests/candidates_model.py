"""Host model of the per-query candidate lists (include/hvs.h "per-query candidate lists").

The contract, restated.  full(q) is every matched key of query q in key order (tests/after_model.py: predicates from
hvs_testlib._passes, distances from the oracle's exact-order function).  The answer under a candidate list is: full(q) with only
the keys whose id IS listed kept, cut by the cap if there is one, less the keys of the exclusion list if there is one, then the
page of k slots behind the cursor (after_model.page), padded or with empty slots.  Pad rows are taken whether listed or not.  A
listed id is only compared with row ids, so ids that name no matched row -- 0xFFFFFFFF, ids >= n, ids behind the sampled prefix,
rows failing the predicate -- contribute nothing, and an empty list matches nothing.

The model shares nothing with the code under test.  normalise() is the plain-numpy form of hvs_candidates_plan.
"""
import numpy as np

import after_model as A
import exclude_model as X

EMPTY = A.EMPTY
CANDIDATES_MAX = 8192
csr = X.csr


def normalise(lists, row0=0, n_rows=0xFFFFFFFF):
    """exclude_model.normalise with the limit CANDIDATES_MAX"""
    off, raw = csr(lists)
    nq = len(lists)
    if any(len(r) > CANDIDATES_MAX for r in lists):
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


def keep_listed(full, listed):
    """full = (ids, dists) in key order with only the keys whose id is in `listed`: the mirror of exclude_model.drop_listed"""
    ids, d = full
    keep = np.isin(ids, np.asarray(listed, np.uint32))
    return ids[keep], d[keep]


def answers(fulls, lists, k, cursors=None, caps=None, pad_ids=None, pad_dists=None, padding=False, excludes=None):
    """-> (ids[nq][k], dists[nq][k], kept[nq], passing[nq]): kept = the non-pad slots of every query, passing = its listed
    matched rows before cap, exclusion and cursor (hvs_candidates_info.passing_ids)"""
    nq = len(fulls)
    out_i, out_d = np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32)
    n, passing = np.zeros(nq, np.int64), np.zeros(nq, np.int64)
    for q in range(nq):
        f = keep_listed(fulls[q], lists[q])
        passing[q] = f[0].size
        if caps is not None:
            f = A.cap_full(f, caps[q])
        if excludes is not None:
            f = X.drop_listed(f, excludes[q])
        cur = None if cursors is None else (cursors[0][q], cursors[1][q])
        out_i[q], out_d[q], n[q] = A.page(f, cur, k, None if not padding else (pad_ids, pad_dists[q]), padding)
    return out_i, out_d, n, passing


def scanned(lists):
    """hvs_candidates_info.scanned_ids of a one-GPU or replicated context: the normalised entries of all lists"""
    return int(normalise(lists)[0])


# ---- list shapes the normalisation must get right (exclude_model.shaped_lists) at lengths on both sides of every wave, block and
# power-of-two boundary of hvs_k_norm_candidates ----
LENGTHS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 4095, 4096, 4097, 8191, 8192)
N_ROWS = 20000         # "n" of the shapes below: ids >= N_ROWS name no row of today


def shaped_lists(length, rng):
    """exclude_model.shaped_lists over N_ROWS rows"""
    base = rng.choice(N_ROWS, max(length, 1), replace=False).astype(np.uint32)[:length]
    mixed = base.copy()
    mixed[::3] = EMPTY
    beyond = base.copy()
    beyond[1::2] = beyond[1::2] + np.uint32(N_ROWS)
    few = rng.choice(base, length) if length else base
    return [np.full(length, 77, np.uint32), np.sort(base)[::-1].copy(), np.sort(base), mixed, beyond, few, base]


def all_shapes():
    rng = np.random.default_rng(17)
    return [lst for length in LENGTHS for lst in shaped_lists(length, rng)]


# ---- the lists the GPU tests attach (tests/test_candidates.py, test 1): query i takes rule i % 8 ----
MIX_LENGTHS = (15, 16, 17, 63, 64, 65)


def rule_lists(fulls, nodes_n, sn, k, passes_none):
    """`passes_none(q)`: ids of up to 400 rows of [0, sn) that FAIL query q's predicate."""
    lists = []
    for i, (ids, _) in enumerate(fulls):
        rule = i % 8
        fail = np.asarray(passes_none(i), np.uint32)[:400]
        if rule == 0:
            lst = np.empty(0, np.uint32)
        elif rule == 1:
            lst = ids[:1]
        elif rule == 2:
            lst = ids[:k]
        elif rule == 3:
            lst = np.sort(ids[:CANDIDATES_MAX])[::-1]                         # 8192 entries descending: the device sorts
            if lst.size < CANDIDATES_MAX:                                     # (few matches: filled up with rows that fail)
                fill = np.setdiff1d(np.arange(min(sn, CANDIDATES_MAX * 2), dtype=np.uint32), lst)[:CANDIDATES_MAX - lst.size]
                lst = np.sort(np.concatenate([lst, fill]).astype(np.uint32))[::-1]
        elif rule == 4:
            lst = ids[::2][:CANDIDATES_MAX]
        elif rule == 5:
            beyond = np.arange(nodes_n, nodes_n + 312, dtype=np.uint32)       # ids >= n
            behind = np.arange(sn, min(nodes_n, sn + 312), dtype=np.uint32)   # ids behind the sampled prefix (none when sn == n)
            lst = np.concatenate([beyond, behind, fail, [EMPTY, EMPTY]])
        elif rule == 6:
            page1 = np.full(k, EMPTY, np.uint32)                              # an unpadded result row, empty slots left in
            m = min(k, ids.size, 40)
            page1[:m] = ids[:m]
            lst = np.concatenate([[EMPTY], page1, page1[:3]])                 # ... an empty slot in front, and duplicates
        else:
            length = MIX_LENGTHS[(i // 8) % len(MIX_LENGTHS)]                 # matches mixed with non-matches
            m = min(ids.size, (length + 1) // 2)
            none = np.concatenate([fail, np.arange(2 * nodes_n, 2 * nodes_n + length, dtype=np.uint32)])   # (a type-0 query fails no row)
            lst = np.concatenate([ids[:3 * m:3][:m], none[:length]])[:length]
            lst = lst[np.argsort((lst.astype(np.uint64) * 2654435761) % 1000003, kind="stable")]   # in no order
        lists.append(np.ascontiguousarray(lst, np.uint32))
    return lists


# ---- the data of the cut tests (tests/test_candidates.py, test 2): one type-0 query and lists whose keys ARRIVE in a chosen order.
# A list is scanned in id order, so the rows of a block of consecutive ids are re-arranged by their distance to the query:
# ascending, descending, or with a run of TIE_RUN copies of one row placed across the scan's first cut (arrival CAP, the buffer's
# size: 256 for k <= 128, else 512) AND across slot k of the answer (TIE_RUN / 2 of the run rank in front of slot k).
CUT_N, CUT_KS, CUT_LENGTHS, TIE_RUN = 60000, (100, 128, 129, 256), (600, 8192), 150


def cut_cap(k):
    return 256 if k <= 128 else 512


def cut_data():
    """-> (nodes, query[1][104], {name: ids}, {name: (first, last) arrival positions of the tie run}); names are
    ("asc" | "desc", length) and ("tie", k, length)"""
    import hvs_testlib as T
    nodes = T.gen_data(CUT_N, 171, T.GEN_V1, 10).copy()
    query = np.ascontiguousarray(T.gen_queries(1, 172, T.GEN_V1, 10))
    query[0, :4] = [0, -1, -1, -1]
    d = A._dists(nodes, query[0], np.arange(CUT_N, dtype=np.uint32), "simd")
    rng = np.random.default_rng(173)
    lists, runs, start = {}, {}, 0
    for length in CUT_LENGTHS:
        for name in ("asc", "desc") + tuple(("tie", k) for k in CUT_KS):
            ids = np.arange(start, start + length, dtype=np.uint32)
            start += length
            by_dist = ids[np.argsort(d[ids], kind="stable")]
            if name == "asc":
                src = by_dist
            elif name == "desc":
                src = by_dist[::-1]
            else:
                k = name[1]
                front = k - TIE_RUN // 2                                      # rows in front of the run in key order
                first = cut_cap(k) - TIE_RUN // 2                             # the run's first arrival position
                rest = rng.permutation(np.concatenate([by_dist[:front], by_dist[front + 1:length - TIE_RUN + 1]]))
                src = np.concatenate([rest[:first], np.full(TIE_RUN, by_dist[front], np.uint32), rest[first:]])
                runs[name + (length,)] = (first, first + TIE_RUN - 1)
            assert src.size == length
            nodes[ids] = nodes[src].copy()
            lists[(name, length) if isinstance(name, str) else name + (length,)] = ids
    assert start <= CUT_N
    return nodes, query, lists, runs
