"""Host model of query clauses (include/hvs.h "query clauses"), shared by tests/test_clauses_cpu.py and
tests/test_clauses.py.

The contract, restated.  User query q has the clause list K(q): its own row (four attribute floats and vector), then its extras,
each [type, v, l, r] with a vector of its own or, for predicate-only clauses, the query's.  The key of a row for q is the
smallest key (distance bits, id) over the clauses it passes; the answer is the first k rows in that order among the rows of the
sampled live prefix that pass at least one clause, then the usual padding, a pad row reporting its smallest distance over the
vectors of K(q).

The model takes, per clause, the ORACLE's depth-k answer (T.oracle_query under T.oracle_k), empties the slots past the count of
rows that pass that clause (the oracle pads), and applies the definition in numpy: union, smallest key per id, first k, padding
(vectors_model's merge_one and finish: the arithmetic is that of multi-vector queries).  `stream` restates the merge's streaming
rule with its threshold and yields the four counters of hvs_clauses_stats.  Nothing here comes from the library.
"""
import numpy as np

import hvs_testlib as T
import vectors_model as V

EMPTY = V.EMPTY
MAX_EXTRA = 255
NDIM = V.NDIM
keys_of, key_ids, key_dists, merge_one, finish, pad_rows = V.keys_of, V.key_ids, V.key_dists, V.merge_one, V.finish, V.pad_rows


def check(offsets):
    """hvs_clauses_check in numpy: nsub = offsets[nq] + nq, or None where it refuses"""
    off = np.asarray(offsets, np.int64).ravel()
    if off.size == 0 or off[0] != 0:
        return None
    m = np.diff(off)
    if (m < 0).any() or (m > MAX_EXTRA).any():
        return None
    nsub = int(off[-1]) + off.size - 1
    return None if nsub >= 0xFFFFFFFF else nsub


def csr(clauses, vectors=None):
    """(offsets[nq + 1], attrs[total, 4], vecs[total, 100] or None) of per-query clause lists"""
    rows = [np.asarray(a, np.float32).reshape(-1, 4) for a in clauses]
    off = np.zeros(len(rows) + 1, np.uint32)
    if rows:
        off[1:] = np.cumsum([r.shape[0] for r in rows])
    attrs = np.ascontiguousarray(np.concatenate(rows) if rows else np.empty((0, 4)), np.float32)
    vecs = None
    if vectors is not None:
        vecs = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float32).reshape(-1, NDIM) for v in vectors]), np.float32)
    return off, attrs, vecs


def sub_queries(queries, clauses, vectors=None):
    """the expansion: (rows [nsub, 104], sub_off[nq + 1]) -- sub-query 0 of query q is q's row, sub-query 1 + j its row with floats
    0..3 replaced by extra clause j and, with `vectors`, floats 4.. by that clause's vector"""
    out, sub = [], [0]
    for i, q in enumerate(np.asarray(queries, np.float32)):
        a = np.asarray(clauses[i], np.float32).reshape(-1, 4)
        block = np.repeat(q[None, :], 1 + a.shape[0], axis=0)
        block[1:, :4] = a
        if vectors is not None:
            block[1:, 4:] = np.asarray(vectors[i], np.float32).reshape(-1, NDIM)
        out.append(block)
        sub.append(sub[-1] + block.shape[0])
    return np.ascontiguousarray(np.concatenate(out), np.float32), np.array(sub, np.int64)


def unpadded_lists(nodes, subq, depth, sp=1.0, live=None, engine="canonical"):
    """the unpadded depth-`depth` list of every row of `subq` (ordinary queries): (ids [n, depth] global, EMPTY in unmatched slots;
    dists, +inf there; counts of passing rows).  The oracle runs on the live rows and its ids are mapped back."""
    nodes = np.ascontiguousarray(nodes, np.float32)
    lv = np.arange(nodes.shape[0]) if live is None else np.flatnonzero(live)
    rows = np.ascontiguousarray(nodes[lv])
    with T.oracle_k(depth):
        ids, d = T.oracle_query(rows, np.ascontiguousarray(subq, np.float32), sp, engine=engine)
    sn = int(T.oracle().hvs_oracle_sn(sp, rows.shape[0]))
    ids, d = ids.copy(), d.copy()
    nl = rows.shape[0]
    counts = np.empty(len(subq), np.int64)
    for j in range(len(subq)):
        cnt = counts[j] = int(T._passes(rows[:sn], subq[j]).sum())
        if cnt >= depth:
            continue
        row_i, row_d = ids[j].tolist(), d[j].tolist()                      # the oracle padded: rows nl-1, nl-2, ... sorted in with the matches
        for s in range(depth - cnt):
            at = row_i.index(nl - 1 - s)
            del row_i[at], row_d[at]
        ids[j] = row_i + [0] * (depth - cnt)
        d[j] = row_d + [np.inf] * (depth - cnt)
    out = lv[ids].astype(np.uint32)
    for j in range(len(subq)):
        if counts[j] < depth:
            out[j, counts[j]:] = EMPTY
    return out, d.astype(np.float32), counts


def stream(ids, dists, k):
    """The merge's streaming rule for ONE query's lists (m x k, ascending, EMPTY last), restated: the lists are read in order, 64
    slots (a chunk) at a time, into a buffer of cap = 256 (k <= 128) or 512 keys.  Before a chunk that might not fit (held + 64 >
    cap) the buffer is de-duplicated by id and, if the chunk still might not fit, cut to its k smallest keys: the largest key kept
    becomes the threshold tau.  A loaded key is admitted only if strictly below tau; after a chunk with a slot that was empty or
    not below tau the rest of the list is not loaded.  Once more de-duplicated at the end, then the k smallest.
    -> (keys in order, read_keys, duplicate_keys, bounded_keys, skipped_chunks)"""
    cap = 256 if k <= 128 else 512
    none = np.uint64(0xFFFFFFFFFFFFFFFF)                                # "no key": above every key
    buf = np.empty(0, np.uint64)                                        # the keys held, duplicates of an id included
    tau = none
    read = dups = bounded = skipped = 0

    def dedup(buf):
        b = np.sort(buf)                                                # by key: the first of an id is its smallest
        _, first = np.unique(key_ids(b), return_index=True)
        return b[first], buf.size - first.size

    m, depth = ids.shape
    assert depth == k
    chunks = (k + 63) // 64
    for j in range(m):
        kj = keys_of(ids[j], dists[j])
        have = ids[j] != EMPTY
        for ch in range(chunks):
            if buf.size + 64 > cap:
                buf, n = dedup(buf)
                dups += n
                if buf.size + 64 > cap:
                    buf = np.sort(buf)[:k]
                    tau = buf[-1]
            e = slice(ch * 64, min(k, ch * 64 + 64))
            admit = have[e] & (kj[e] < tau)
            read += int(have[e].sum())
            bounded += int((have[e] & ~admit).sum())
            buf = np.concatenate([buf, kj[e][admit]])
            if not admit.all():
                skipped += chunks - 1 - ch
                break
    if m > 1:
        buf, n = dedup(buf)
        dups += n
    return np.sort(buf)[:k], read, dups, bounded, skipped


def pad_dists(nodes, vecs, pad_ids, order="simd"):
    """a pad row's smallest distance over the vectors `vecs` of a query's clauses (by key: NaN above +inf)"""
    vecs = np.unique(np.asarray(vecs, np.float32).reshape(-1, NDIM), axis=0)
    out = np.empty(len(pad_ids), np.float32)
    for s, i in enumerate(pad_ids):
        d = np.array([T.oracle_dist(nodes[i, 2:], v, order) for v in vecs], np.float32)
        out[s] = key_dists(np.sort(keys_of(np.full(d.size, i), d))[:1])[0]
    return out


def answers(nodes, queries, clauses, vectors, k, sp=1.0, padding=True, live=None, engine="canonical", depth=None, caps=None, exclude=None):
    """-> dict(ids [nq, k], dists, kept [nq], read_keys, duplicate_keys, bounded_keys, skipped_chunks, underfull, pairs, lists): the
    model's answer and the figures hvs_clauses_stats must report.  depth / caps / exclude as vectors_model.answers has them."""
    depth = k if depth is None else depth
    order = "scalar" if engine == "baseline" else "simd"
    subq, sub_off = sub_queries(queries, clauses, vectors)
    ids, d, counts = unpadded_lists(nodes, subq, depth, sp, live, engine)
    pid = pad_rows(nodes, k, live)
    nq = len(queries)
    out_i, out_d = np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32)
    kept = np.zeros(nq, np.int64)
    fig = np.zeros(4, np.int64)
    underfull = 0
    for q in range(nq):
        li, ld = ids[sub_off[q]:sub_off[q + 1]].copy(), d[sub_off[q]:sub_off[q + 1]].copy()
        if caps is not None or exclude is not None:                       # what each sub-query's list looks like under them
            for j in range(li.shape[0]):
                ok = li[j] != EMPTY
                if caps is not None:
                    ok &= ld[j] <= np.float32(caps[q])
                if exclude is not None:
                    ok &= ~np.isin(li[j], np.asarray(exclude[q], np.uint32))
                n_ok = min(int(ok.sum()), k)
                li[j] = np.concatenate([li[j][ok][:k], np.full(depth - n_ok, EMPTY)])
                ld[j] = np.concatenate([ld[j][ok][:k], np.full(depth - n_ok, np.inf, np.float32)])
        li, ld = li[:, :k], ld[:, :k]
        for j in range(li.shape[0]):                                      # the engines' lists are in key order, ties by id
            o = np.argsort(np.where(li[j] == EMPTY, np.uint64(0xFFFFFFFFFFFFFFFF), keys_of(li[j], ld[j])), kind="stable")
            li[j], ld[j] = li[j][o], ld[j][o]
        keys, _, _ = merge_one(li, ld)
        skeys, *f = stream(li, ld, k)
        assert np.array_equal(skeys, keys[:k]), ("the streaming rule lost a row", q)
        fig += f
        pads = None
        if padding and keys.size < k:
            pads = (pid, pad_dists(nodes, subq[sub_off[q]:sub_off[q + 1], 4:], pid, order))
        out_i[q], out_d[q], kept[q] = finish(keys, k, pads, padding)
        underfull += int(kept[q] < k)
    return dict(ids=out_i, dists=out_d, kept=kept, read_keys=int(fig[0]), duplicate_keys=int(fig[1]), bounded_keys=int(fig[2]),
                skipped_chunks=int(fig[3]), underfull=underfull, pairs=int(counts.sum()), lists=(ids, d, sub_off))


def brute(nodes, queries, clauses, vectors, k, sp=1.0, order="simd"):
    """The definition without sub-lists: per query the k smallest of min over the clauses a row passes of key(row, clause's vector),
    over ALL rows of the prefix -> (ids, dists) unpadded (EMPTY / +inf).  Small inputs only."""
    n = nodes.shape[0]
    sn = int(T.oracle().hvs_oracle_sn(sp, n))
    subq, sub_off = sub_queries(queries, clauses, vectors)
    out_i, out_d = np.full((len(queries), k), EMPTY, np.uint32), np.full((len(queries), k), np.inf, np.float32)
    for q in range(len(queries)):
        best = {}
        for j in range(sub_off[q], sub_off[q + 1]):
            rows = np.flatnonzero(T._passes(nodes[:sn], subq[j]))
            kv = keys_of(rows, np.array([T.oracle_dist(nodes[r, 2:], subq[j, 4:], order) for r in rows], np.float32))
            for r, key in zip(rows.tolist(), kv.tolist()):
                best[r] = min(best.get(r, key), key)
        top = np.array(sorted(best.values())[:k], np.uint64)
        out_i[q, :top.size], out_d[q, :top.size] = key_ids(top), key_dists(top)
    return out_i, out_d


def product(q_rows, sets, vectors):
    """product_clauses in plain python: -> (q_out, clauses, vecs) per query -- the c (1 + m) clauses of a type-1 / 3 query with a
    non-empty set, category by category (categories truncated to int32, distinct, ascending), own vector first; else the 1 + m
    vector clauses.  The first clause is the query's own row."""
    q_out = np.array(q_rows, np.float32, copy=True)
    clauses, vecs = [], []
    for p, q in enumerate(q_rows):
        t = float(q[0])
        tests_c = -1.0 < t < 4.0 and int(t) in (1, 3) and len(sets[p]) > 0
        cats = sorted({float(np.float32(int(s))) for s in sets[p]}) if tests_c else [float(q[1])]
        own = [q[4:]] + [v for v in np.asarray(vectors[p], np.float32).reshape(-1, NDIM)]
        a, v = [], []
        for cat in cats:
            for vec in own:
                a.append([q[0], cat, q[2], q[3]])
                v.append(vec)
        q_out[p, 1] = a[0][1]
        clauses.append(np.array(a[1:], np.float32).reshape(-1, 4))
        vecs.append(np.array(v[1:], np.float32).reshape(-1, NDIM))
    return q_out, clauses, vecs


# ---- the data set of the GPU tests (tests/test_clauses.py) ---------------------------------------------------------------------
N, NCAT = 12288, 10
_cache = {}


def data():
    """(nodes, queries): 12288 gen-v1 rows (an index and filter tiles exist: > 4096) with hand-placed categories 1001 (5 rows),
    1002 (99) and 1003 (150) in front of the last 256 rows; 96 gen-v1 queries of mixed types"""
    if "data" not in _cache:
        nodes = T.gen_data(N, 91, T.GEN_V1, NCAT)
        rng = np.random.default_rng(29)
        for cat, cnt in ((1001, 5), (1002, 99), (1003, 150)):
            V._place(nodes, rng, cat, cnt, 0, N - 256)
        _cache["data"] = (nodes, T.gen_queries(96, 92, T.GEN_V1, NCAT))
    return _cache["data"]
