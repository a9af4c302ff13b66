"""Host model of multi-vector queries (include/hvs.h "multi-vector queries"), shared by tests/test_vectors_cpu.py and
tests/test_vectors.py.

The contract, restated.  User query q has the vectors V(q): its own and its extras.  The key of a row for q is the smallest key
(distance bits, id) over V(q); the answer is the first k rows in that order among the rows that pass q's predicate in the
sampled live prefix, then the usual padding with a pad row reporting its smallest distance over V(q).

The model takes, for each query and each vector, the ORACLE's depth-k answer (T.oracle_query under T.oracle_k), empties the slots
past the count of rows that pass (the oracle pads), and applies the definition in numpy: union, smallest key per id in the u64
key order, first k, padding.  That depth-k lists suffice is the lemma of DESIGN 3.15; tests/test_vectors_cpu.py checks it against
a brute force over every row.  Nothing here comes from the library.
"""
import numpy as np

import hvs_testlib as T

EMPTY = np.uint32(0xFFFFFFFF)
MAX_EXTRA = 63
NDIM = 100


def keys_of(ids, dists):
    """the engines' u64 keys: distance bits (one canonical NaN, above +inf), then id"""
    d = np.ascontiguousarray(dists, np.float32)
    bits = d.view(np.uint32).astype(np.uint64)
    bits[np.isnan(d)] = 0x7FC00000
    return (bits << np.uint64(32)) | np.asarray(ids, np.uint64)


def key_ids(keys):
    return (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def key_dists(keys):
    return (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)


def csr(vectors):
    """(offsets[nq + 1], vecs[total, 100]) of a list of per-query [m_i, 100] arrays"""
    rows = [np.asarray(v, np.float32).reshape(-1, NDIM) for v in vectors]
    off = np.zeros(len(rows) + 1, np.uint32)
    if rows:
        off[1:] = np.cumsum([r.shape[0] for r in rows])
    return off, np.ascontiguousarray(np.concatenate(rows) if rows else np.empty((0, NDIM)), np.float32)


def check(offsets):
    """hvs_vectors_check in numpy: nsub = offsets[nq] + nq, or None where it refuses"""
    off = np.asarray(offsets, np.int64).ravel()
    if off.size == 0 or off[0] != 0:
        return None
    m = np.diff(off)
    if (m < 0).any() or (m > MAX_EXTRA).any():
        return None
    nsub = int(off[-1]) + off.size - 1
    return None if nsub >= 0xFFFFFFFF else nsub


def sub_queries(queries, vectors):
    """the expansion: (rows [nsub, 104], sub_off[nq + 1]) -- sub-query j of query q is q's row with floats 4.. replaced by vector j"""
    out, sub = [], [0]
    for q, v in zip(np.asarray(queries, np.float32), vectors):
        v = np.asarray(v, np.float32).reshape(-1, NDIM)
        block = np.repeat(q[None, :], 1 + v.shape[0], axis=0)
        block[1:, 4:] = v
        out.append(block)
        sub.append(sub[-1] + block.shape[0])
    return np.ascontiguousarray(np.concatenate(out), np.float32), np.array(sub, np.int64)


def sub_lists(nodes, queries, vectors, depth, sp=1.0, live=None, engine="canonical"):
    """Per query the unpadded depth-`depth` lists of its vectors: (ids [nsub, depth] global, EMPTY in unmatched slots; dists,
    +inf there; sub_off).  The oracle runs on the live rows and its ids are mapped back."""
    nodes = np.ascontiguousarray(nodes, np.float32)
    lv = np.arange(nodes.shape[0]) if live is None else np.flatnonzero(live)
    rows = np.ascontiguousarray(nodes[lv])
    subq, sub_off = sub_queries(queries, vectors)
    with T.oracle_k(depth):
        ids, d = T.oracle_query(rows, subq, sp, engine=engine)
    sn = int(T.oracle().hvs_oracle_sn(sp, rows.shape[0]))
    d = d.copy()
    nl = rows.shape[0]
    for q in range(len(queries)):
        cnt = int(T._passes(rows[:sn], queries[q]).sum())
        if cnt >= depth:
            continue
        for j in range(sub_off[q], sub_off[q + 1]):                        # the oracle padded: rows nl-1, nl-2, ... sorted in with the matches
            row_i, row_d = ids[j].tolist(), d[j].tolist()
            for s in range(depth - cnt):
                at = row_i.index(nl - 1 - s)                               # (a pad row that is also a match: equal keys, either goes)
                del row_i[at], row_d[at]
            ids[j] = row_i + [0] * (depth - cnt)
            d[j] = row_d + [np.inf] * (depth - cnt)
    out = lv[ids].astype(np.uint32)
    for q in range(len(queries)):
        cnt = int(T._passes(rows[:sn], queries[q]).sum())
        if cnt < depth:
            out[sub_off[q]:sub_off[q + 1], cnt:] = EMPTY
    return out, d, sub_off


def merge_one(ids, dists):
    """union of one query's lists (m x depth), smallest key per id, in key order -> (keys, merged_keys, duplicates)"""
    have = ids.ravel() != EMPTY
    keys = np.sort(keys_of(ids.ravel()[have], dists.ravel()[have]))
    _, first = np.unique(key_ids(keys), return_index=True)             # (sorted by key: the first of an id is its smallest)
    out = np.sort(keys[first])
    return out, int(keys.size), int(keys.size - out.size)


def stream_stats(ids, dists, k):
    """-> (merged_keys, duplicate_keys) of ONE query's lists (m x k) as the contract defines them (include/hvs.h): the lists are read
    in order, 64 slots at a time, into a buffer of cap = 256 (k <= 128) or 512 keys; before a step that might not fit (held + 64 >
    cap) the buffer is de-duplicated by id and, if the step still might not fit, cut to its k smallest keys; once more at the
    end.  A key is a duplicate when the buffer holds its id with a key at least as small at a de-duplication."""
    cap = 256 if k <= 128 else 512
    held = {}                                                           # id -> smallest key held
    pending = []                                                        # keys appended since the last de-duplication
    seen = dups = 0

    def dedup():
        nonlocal dups
        for key in pending:
            i = int(key) & 0xFFFFFFFF
            if i in held:
                dups += 1
                held[i] = min(held[i], int(key))
            else:
                held[i] = int(key)
        pending.clear()

    m, depth = ids.shape
    for j in range(m):
        kj = keys_of(ids[j], dists[j])
        for off in range(0, depth, 64):
            if len(held) + len(pending) + 64 > cap:
                dedup()
                if len(held) + 64 > cap:
                    for key in sorted(held.values())[k:]:
                        del held[key & 0xFFFFFFFF]
            step = kj[off:off + 64][ids[j, off:off + 64] != EMPTY]
            pending.extend(step.tolist())
            seen += step.size
    if m > 1:
        dedup()
    return seen, dups


def pad_rows(nodes, k, live=None):
    """the padding ids: the last k live rows, descending (n-1, n-2, ... with every row live)"""
    lv = np.arange(nodes.shape[0]) if live is None else np.flatnonzero(live)
    return lv[::-1][:k].astype(np.uint32)


def pad_dists(nodes, query, vecs, pad_ids, order="simd"):
    """a pad row's smallest distance over the query's vectors (by key: NaN above +inf)"""
    allv = np.concatenate([np.asarray(query, np.float32)[None, 4:], np.asarray(vecs, np.float32).reshape(-1, NDIM)])
    out = np.empty(len(pad_ids), np.float32)
    for s, i in enumerate(pad_ids):
        d = np.array([T.oracle_dist(nodes[i, 2:], v, order) for v in allv], np.float32)
        out[s] = key_dists(np.sort(keys_of(np.full(d.size, i), d))[:1])[0]
    return out


def finish(keys, k, pads, padding):
    """the first k keys, then the pad rows (ids, dists) or empty slots, sorted by key with ties by slot -> (ids, dists, kept)"""
    keys = keys[:k]
    kept = keys.size
    ids, d = key_ids(keys), key_dists(keys)
    if kept < k:
        if padding:
            ids = np.concatenate([ids, pads[0][:k - kept]])
            d = np.concatenate([d, pads[1][:k - kept]])
        else:
            ids = np.concatenate([ids, np.full(k - kept, EMPTY)])
            d = np.concatenate([d, np.full(k - kept, np.inf, np.float32)])
        allk = keys_of(ids, d)
        allk[ids == EMPTY] = np.uint64(0xFFFFFFFFFFFFFFFF)
        order = np.argsort(allk, kind="stable")
        ids, d = ids[order], d[order]
    return ids.astype(np.uint32), d.astype(np.float32), kept


def answers(nodes, queries, vectors, k, sp=1.0, padding=True, live=None, engine="canonical", depth=None, caps=None, exclude=None):
    """-> dict(ids [nq, k], dists, kept [nq], merged_keys, duplicate_keys, underfull, lists) -- the model's answer and the figures
    hvs_vectors_stats must report.  `depth`: the oracle's depth (default k; deeper for exclusion lists: a page behind listed rows).
    caps: one per query (rows whose smallest distance exceeds it leave); exclude: one id list per query (applied to every
    sub-list, as the sub-queries apply their parent's)."""
    depth = k if depth is None else depth
    order = "scalar" if engine == "baseline" else "simd"
    ids, d, sub_off = sub_lists(nodes, queries, vectors, depth, sp, live, engine)
    pid = pad_rows(nodes, k, live)
    nq = len(queries)
    out_i, out_d = np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32)
    kept = np.zeros(nq, np.int64)
    merged = dups = underfull = 0
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
        keys, _, _ = merge_one(li, ld)
        s, dd = stream_stats(li, ld, k)
        merged += s
        dups += dd
        pads = None
        if padding and keys.size < k:
            pads = (pid, pad_dists(nodes, queries[q], vectors[q], pid, order))
        out_i[q], out_d[q], kept[q] = finish(keys, k, pads, padding)
        underfull += int(kept[q] < k)
    return dict(ids=out_i, dists=out_d, kept=kept, merged_keys=merged, duplicate_keys=dups, underfull=underfull,
                lists=(ids, d, sub_off))


def brute(nodes, queries, vectors, k, sp=1.0, order="simd"):
    """The definition without sub-lists: per query the k smallest of min_j key(row, v_j) over ALL passing rows of the prefix ->
    (ids, dists) unpadded (EMPTY / +inf).  One oracle distance per (row, vector): small inputs only."""
    n = nodes.shape[0]
    sn = int(T.oracle().hvs_oracle_sn(sp, n))
    out_i, out_d = np.full((len(queries), k), EMPTY, np.uint32), np.full((len(queries), k), np.inf, np.float32)
    for q, (row, vecs) in enumerate(zip(queries, vectors)):
        rows = np.flatnonzero(T._passes(nodes[:sn], row))
        if not rows.size:
            continue
        allv = np.concatenate([row[None, 4:], np.asarray(vecs, np.float32).reshape(-1, NDIM)])
        best = None
        for v in allv:
            kv = keys_of(rows, np.array([T.oracle_dist(nodes[r, 2:], v, order) for r in rows], np.float32))
            best = kv if best is None else np.minimum(best, kv)
        best = np.sort(best)[:k]
        out_i[q, :best.size], out_d[q, :best.size] = key_ids(best), key_dists(best)
    return out_i, out_d


def distinct_min_dists(keys, upto):
    """no equal-distance tie among the first `upto` merged keys (the rule of the GPU tests: no query is left out)"""
    bits = (keys[:upto] >> np.uint64(32))
    return bool((np.diff(bits.astype(np.int64)) != 0).all())


# ---- the data set of the GPU tests (tests/test_vectors.py), checked for ties on the CPU (tests/test_vectors_cpu.py) ------------------
N, NCAT = 32768, 10
PLACED = {1001: 5, 1002: 99, 1003: 100, 1004: 150}
M_CYCLE = (0, 1, 3, 1, 0, 3, 1, 63)                                      # extras per query, cycling
_cache = {}


def _place(nodes, rng, cat, count, a, b):
    free = np.flatnonzero(nodes[a:b, 0] < 1000) + a
    ids = np.sort(rng.choice(free, count, replace=False))
    nodes[ids, 0] = np.float32(cat)
    return ids


def data():
    """(nodes, queries): 32768 gen-v1 rows (an index and filter tiles exist) with hand-placed categories of 5, 99, 100 and 150 rows
    in front of the last 256 rows; 200 gen-v1 queries of mixed types plus a type-1 and a type-3 query on every placed category"""
    if "data" not in _cache:
        nodes = T.gen_data(N, 81, T.GEN_V1, NCAT)
        rng = np.random.default_rng(23)
        for cat, cnt in PLACED.items():
            _place(nodes, rng, cat, cnt, 0, N - 256)
            assert int((nodes[:, 0] == cat).sum()) == cnt
        gen = T.gen_queries(200, 82, T.GEN_V1, NCAT)
        hand = T.gen_queries(2 * len(PLACED), 83, T.GEN_V1, NCAT)
        for i, cat in enumerate(PLACED):
            hand[2 * i, :4] = [1, cat, -1, -1]
            hand[2 * i + 1, :4] = [3, cat, 0.02, 0.98]
        _cache["data"] = (nodes, np.ascontiguousarray(np.concatenate([gen, hand])))
    return _cache["data"]


def mixed_vectors(nodes, queries, seed=5):
    """m(q) cycling through M_CYCLE: odd extras lie near the query's own vector (overlapping neighbourhoods: the same rows under
    several vectors, at different distances), even ones are vectors of random rows of D (other neighbourhoods)"""
    rng = np.random.default_rng(seed)
    out = []
    for i, q in enumerate(queries):
        m = M_CYCLE[i % len(M_CYCLE)]
        v = np.empty((m, NDIM), np.float32)
        for j in range(m):
            if j & 1:
                v[j] = q[4:] + rng.normal(0.0, 0.01, NDIM).astype(np.float32)
            else:
                v[j] = nodes[rng.integers(0, nodes.shape[0]), 2:] + np.float32(0.001) * rng.standard_normal(NDIM).astype(np.float32)
        out.append(v)
    return out


def perturbed_queries():
    """test 4: indices into data()'s queries -- gen-v1 queries of every type, and the queries on the 99-row and the 150-row
    category (lists with empty slots at k = 128 / 256)"""
    return np.array([0, 1, 2, 3, 4, 5, 202, 203, 206, 207])


def perturbed_copies(queries, m=63):
    """test 4: every extra is the query's own vector with ONE component moved -- the same neighbourhood, every distance different
    (tests/test_vectors_cpu.py checks that it is)"""
    out = []
    for q in queries:
        v = np.repeat(q[None, 4:], m, axis=0).astype(np.float32)
        for j in range(m):
            v[j, (7 * j) % NDIM] += np.float32(2.5) + np.float32(0.03125) * np.float32(j)
        out.append(v)
    return out


def far_vectors(nodes, queries, seed=9):
    """test 5: three extras per query taken from far-apart rows of D -- other neighbourhoods, no row under two vectors"""
    rng = np.random.default_rng(seed)
    return [nodes[rng.choice(nodes.shape[0], 3, replace=False), 2:].copy() for _ in queries]
