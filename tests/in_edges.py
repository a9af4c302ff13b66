"""Category sets at the merge's edges: what tests/test_in_edges_cpu.py and tests/test_in_edges.py share -- data with long runs of
equal distances spread over several categories, the canonical answer stated in numpy with oracle distances (key_model), the
exact value of hvs_in_info.merged_keys, and the row-set walk of the lifecycle test.  Nothing here touches a GPU."""
import numpy as np

import hvs_testlib as T
import in_sets as S

EMPTY = 0xFFFFFFFF
NAN_BITS = 0x7FC00000
N = S.N
TIE_CATS = [1101, 1102, 1103, 1104, 1105]
NF_CATS = [1201, 1202]
# the sets of this file, by name, beside those of in_sets (S.expected and test_in.parity look names up in S.SETS)
SETS = {
    "tie5": list(TIE_CATS),
    "tie2": [1101, 1103],
    "tie64": list(TIE_CATS) + list(range(3000, 3059)),   # 64 distinct values, the five tie categories among them
    "nf": list(NF_CATS),                                 # six rows, four of them at a non-finite distance
    "nf+": list(NF_CATS) + [1001],                       # eleven rows, seven at a finite distance
}
S.SETS.update(SETS)
_cache = {}

# ---- 1. tie runs ------------------------------------------------------------------------------------------------------------------------
RUN, PLAIN = 30, 90                                      # per category: 30 rows at u, 30 at w, 90 with their generated vectors
WINDOWS = {"A": (0.2, 0.6), "B": (0.65, 0.9)}            # the T windows of the type-3 tie queries
# rows of each category's u-run / w-run whose T lies in window A, in window B (the rest in neither): T = 0.45 / 0.7 / 0.95
IN_A = {"u": [30, 17, 0, 9, 23], "w": [12, 30, 5, 0, 21]}
IN_B = {"u": [0, 13, 30, 4, 7], "w": [3, 0, 25, 30, 9]}


def tie_data():
    """(nodes, queries, names, info): S.data()'s rows with five more categories of 150 rows each, their ids interleaved; per
    category 30 rows hold the vector u, 30 the vector w (u with one component a few ulps away), 90 keep theirs.  info: u, w,
    ids[cat] = (u-rows, w-rows, plain rows), and the query indices by kind."""
    if "tie" in _cache:
        return _cache["tie"]
    nodes = S.data()[0].copy()
    rng = np.random.default_rng(23)
    u = T.gen_data(1, 501, T.GEN_V1, S.NCAT)[0, 2:].copy()
    ids = {}
    for ci, cat in enumerate(TIE_CATS):
        placed = rng.permutation(S._place(nodes, rng, cat, 2 * RUN + PLAIN, 0, N - 400))
        ids[cat] = (np.sort(placed[:RUN]), np.sort(placed[RUN:2 * RUN]), np.sort(placed[2 * RUN:]))
        for run, rows in zip("uw", ids[cat][:2]):
            a, b = IN_A[run][ci], IN_B[run][ci]
            assert a + b <= RUN
            t = np.full(RUN, 0.95, np.float32)
            t[:a] = np.float32(0.45)
            t[a:a + b] = np.float32(0.7)
            nodes[rows, 1] = t
            for name, (lo, hi) in WINDOWS.items():
                want = (IN_A if name == "A" else IN_B)[run][ci]
                assert int(((t >= np.float32(lo)) & (t <= np.float32(hi))).sum()) == want, (cat, run, name)
    u_rows = np.concatenate([ids[c][0] for c in TIE_CATS])
    w_rows = np.concatenate([ids[c][1] for c in TIE_CATS])
    order = np.argsort(np.concatenate([ids[c][0] for c in TIE_CATS]), kind="stable")
    cats_by_id = np.repeat(TIE_CATS, RUN)[order]
    assert (np.diff(cats_by_id) < 0).sum() > 20, "the u-rows' ids are sorted by category: the merge would not choose across lists"
    # queries: the generated vectors first, then the ones on u and on w
    gen = T.gen_queries(40, 502, T.GEN_V1, S.NCAT)
    head = [  # (type, l, r, set, vector: "u" / "w" / None = generated)
        (1, -1, -1, "tie5", "u"), (1, -1, -1, "tie5", "w"), (3, 0.2, 0.6, "tie5", "u"), (3, 0.2, 0.6, "tie5", "w"),
        (3, 0.65, 0.9, "tie5", "u"), (3, 0.65, 0.9, "tie5", "w"), (1, -1, -1, "tie2", "u"), (1, -1, -1, "tie2", "w"),
        (3, 0.2, 0.6, "tie2", "u"), (1, -1, -1, "tie64", "u"), (3, 0.0, 1.0, "tie5", "u"), (3, 0.0, 1.0, "tie64", "w"),
    ]
    head += [(1, -1, -1, "tie5", None)] * 8 + [(3, 0.0, 1.0, "tie5", None)] * 4 + [(3, 0.2, 0.6, "tie5", None)] * 4
    head += [(1, -1, -1, "tie2", None)] * 3 + [(3, 0.1, 0.9, "tie2", None)] * 2 + [(1, -1, -1, "tie64", None)] * 2
    head += [(0, -1, -1, "tie5", "u"), (2, 0.2, 0.6, "tie5", "w"), (0, -1, -1, "tie2", None), (1, -1, -1, "empty", "u"), (1, -1, -1, "150", None)]
    assert len(head) == 40
    queries, names = gen.copy(), []
    for i, (typ, lo, hi, name, vec) in enumerate(head):
        queries[i, :4] = [typ, 1101 if name != "150" else 2, lo, hi]
        names.append(name)
    queries = np.ascontiguousarray(queries, np.float32)
    # w: u with one component three ulps away.  A query ON u or w tells the two apart (0 against the square of the step); one
    # with a generated vector far away usually rounds both to one distance and sees a single run of 300 (split counts them)
    w = u.copy()
    w[41] = (w[41:42].view(np.uint32) + np.uint32(3)).view(np.float32)[0]
    q = queries.copy()
    for i, h in enumerate(head):
        if h[4] is not None:
            q[i, 4:] = u if h[4] == "u" else w
    two = np.zeros((2, T.DCOLS), np.float32)
    two[0, 2:], two[1, 2:] = u, w
    with T.oracle_k(8):
        d = T.oracle_dists_for_ids(two, q, np.tile(np.array([0, 1] * 4, np.uint32), (len(q), 1)))
    on = [i for i, h in enumerate(head) if h[4] is not None]
    assert (d[on, 0] != d[on, 1]).all() and (np.minimum(d[on, 0], d[on, 1]) == 0).all()
    split = int((d[:, 0] != d[:, 1]).sum())
    nodes[u_rows, 2:] = u
    nodes[w_rows, 2:] = w
    info = dict(u=u, w=w, split=split, ids=ids, on_u=[i for i, h in enumerate(head) if h[4] == "u"], on_w=[i for i, h in enumerate(head) if h[4] == "w"])
    _cache["tie"] = (nodes, np.ascontiguousarray(q), names, info)
    return _cache["tie"]


# ---- 2. the canonical answer ---------------------------------------------------------------------------------------------------------------
KEEP = 2048                                              # keys kept per query by full_keys (k <= 256: eight pages, and more)


def effective(q_row, values):
    return bool(len(values)) and S.tests_c(q_row[0])


def _dists(nodes, q_row, ids):
    """oracle distances (the hot path's order) of one query to rows `ids`, in slices of 256"""
    m = ids.size
    if m == 0:
        return np.zeros(0, np.float32)
    rows = (m + 255) // 256
    padded = np.zeros(rows * 256, np.uint32)
    padded[:m] = ids
    with T.oracle_k(256):
        d = T.oracle_dists_for_ids(nodes, np.repeat(q_row[None, :], rows, 0), padded.reshape(rows, 256))
    return d.ravel()[:m]


def key_bits(d):
    """the distance half of the builder's keys (hvs_make_key): the f32 bits, every NaN the canonical one"""
    d = np.ascontiguousarray(d, np.float32)
    return np.where(np.isnan(d), np.uint32(NAN_BITS), d.view(np.uint32)).astype(np.uint32)


def full_keys(nodes, queries, sets, sp, tag=None):
    """per query: (its first KEEP matched keys in key order -- (distance bits << 32) | id, ascending --, the number of matched
    rows).  Matched: in the sampled prefix and passing the set predicate (S.rewrite + T._passes)."""
    ck = ("full", tag, float(sp))
    if tag is not None and ck in _cache:
        return _cache[ck]
    n = nodes.shape[0]
    sn = int(T.oracle().hvs_oracle_sn(sp, n))
    out = [None] * len(queries)
    groups = {}
    for i, (q, s) in enumerate(zip(queries, sets)):
        key = tuple(np.asarray(s, np.float32).view(np.uint32).tolist()) if effective(q, s) else ()
        groups.setdefault(key, []).append(i)
    for key, members in groups.items():
        d2 = S.rewrite(nodes[:sn], queries[:0], sets[members[0]])[0] if key else nodes[:sn]
        for i in members:
            q2 = queries[i].copy()
            if key:
                q2[1] = S.VSTAR
            ids = np.flatnonzero(T._passes(d2, q2)).astype(np.uint32)
            keys = (key_bits(_dists(nodes, queries[i], ids)).astype(np.uint64) << np.uint64(32)) | ids.astype(np.uint64)
            out[i] = (np.sort(keys)[:KEEP], int(ids.size))
    if tag is not None:
        _cache[ck] = out
    return out


def key_model(nodes, queries, sets, k, sp, caps=None, after=None, tag=None):
    """(ids, dists, m): the canonical answer with padding off -- per query the first k matched keys in key order (those within
    the cap and strictly after the cursor (dists, ids), where given), then 0xFFFFFFFF / +inf; m = matched rows in the prefix
    (caps and cursors are not looked at).  The builder's documented order (hvs_device.h, the paging law of include/hvs.h) in
    numpy with oracle distances: independent of every kernel.  `tag` caches the sorted keys (as S.expected's does)."""
    full = full_keys(nodes, queries, sets, sp, tag)
    nq = len(queries)
    ids = np.full((nq, k), EMPTY, np.uint32)
    bits = np.full((nq, k), 0x7F800000, np.uint32)
    for i, (keys, m) in enumerate(full):
        truncated = m > keys.size
        if caps is not None:                             # dist <= cap in IEEE arithmetic: NaN is within no cap
            d = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
            with np.errstate(invalid="ignore"):
                keys = keys[d <= np.float32(caps[i])]
        if after is not None:
            if int(after[1][i]) == EMPTY:
                keys = keys[:0]
            else:
                c = (np.uint64(key_bits(np.float32(after[0][i]).reshape(1))[0]) << np.uint64(32)) | np.uint64(int(after[1][i]))
                keys = keys[keys > c]
        if after is not None and truncated and keys.size < k:
            raise AssertionError("key_model: paged past the %d keys kept per query" % KEEP)
        keys = keys[:k]
        ids[i, :keys.size] = keys.astype(np.uint32)
        bits[i, :keys.size] = (keys >> np.uint64(32)).astype(np.uint32)
    return ids, bits.view(np.float32), np.array([m for _, m in full], np.int64)


def pad(nodes, queries, model, k):
    """key_model's answer with padding on, the way test_in.unpadded inverts it: slot m + s of a query with m < k matches takes
    row n - 1 - s; the row is then in key order, pad rows among the matches (the merge sorts once, ties by slot)."""
    ids, d, m = model[0].copy(), model[1].copy(), model[2]
    n = nodes.shape[0]
    for q in np.flatnonzero(m < k):
        mm = int(m[q])
        pid = (n - 1 - np.arange(k - mm)).astype(np.uint32)
        pd = _dists(nodes, queries[q], pid)
        keys = np.concatenate([(key_bits(d[q, :mm]).astype(np.uint64) << np.uint64(32)) | ids[q, :mm].astype(np.uint64),
                               (key_bits(pd).astype(np.uint64) << np.uint64(32)) | pid.astype(np.uint64)])
        keys = keys[np.argsort(keys, kind="stable")]
        ids[q] = keys.astype(np.uint32)
        d[q] = (keys >> np.uint64(32)).astype(np.uint32).view(np.float32)
    return ids, d


def sub_matches(nodes, queries, sets, sp, tag=None):
    """matches of every sub-query (S.plan_model) in the prefix (cached by `tag`, as S.expected is)"""
    ck = ("sub", tag, float(sp))
    if tag is not None and ck in _cache:
        return _cache[ck]
    n = nodes.shape[0]
    sn = int(T.oracle().hvs_oracle_sn(sp, n))
    nsub, sub_off, parent, value = S.plan_model(queries, sets)
    c, out = nodes[:sn, 0], np.zeros(nsub, np.int64)
    one = {}
    for j in range(nsub):
        p = int(parent[j])
        q = queries[p].copy()
        if effective(q, sets[p]):
            q[1] = value[j]
            if np.isnan(value[j]):
                continue                                 # a set without a usable value matches nothing
        key = (p, q[1].tobytes())
        if key not in one:
            one[key] = int(T._passes(nodes[:sn], q).sum())
        out[j] = one[key]
    if tag is not None:
        _cache[ck] = (out, sub_off)
    return out, sub_off


def merged_keys_model(nodes, queries, sets, k, sp, q0=0, nq=None, tag=None):
    """hvs_in_info.merged_keys of a call over user queries [q0, q0 + nq) without caps and cursors: the non-empty slots over all
    sub-query lists, sum of min(matches of the sub-query in the prefix, k)"""
    m, sub_off = sub_matches(nodes, queries, sets, sp, tag)
    nq = len(queries) - q0 if nq is None else nq
    return int(np.minimum(m[sub_off[q0]:sub_off[q0 + nq]], k).sum())


# ---- 3. the retry / lanes workload -------------------------------------------------------------------------------------------------------
TILES = 2                                                # S.data()'s queries, this many times over
WORK_NQ, WORK_NSUB = 472, 1878                           # what that gives (tests/test_in_edges_cpu.py re-derives both)
RANGE_Q0, RANGE_NQ = 37, 300                             # "a range that starts and ends inside": user queries [37, 337)


def workload():
    """(nodes, queries, names) of test_retries_small_batches_and_lanes"""
    nodes, queries, names = S.data()
    return nodes, np.ascontiguousarray(np.tile(queries, (TILES, 1))), list(names) * TILES


# ---- 4. the row-set walk --------------------------------------------------------------------------------------------------------------------
def lifecycle():
    """The operations of test_row_set_lifecycle_with_sets_attached on S.data()'s rows, in order, and what each step leaves:
    a list of dicts -- step, ops = [(name, args...)], rows = the array a fresh load equal to the context would hold, live = the
    ascending live ids where a mask is in force (the context still speaks the old ids: rows = old[live]) or None."""
    if "life" in _cache:
        return _cache["life"]
    base = S.data()[0]
    steps = []
    # (a) delete category 1002, every third row of category 2 and the last 300 rows
    dead = np.concatenate([np.flatnonzero(base[:, 0] == 1002), np.flatnonzero(base[:, 0] == 2)[::3], np.arange(N - 300, N)])
    dead = np.unique(dead).astype(np.uint32)
    live = np.setdiff1d(np.arange(N), dead).astype(np.uint32)
    rows = np.ascontiguousarray(base[live])
    steps.append(dict(step="a", ops=[("delete", dead)], rows=rows, live=live))
    # (b) compact
    steps.append(dict(step="b", ops=[("compact", live)], rows=rows, live=None))
    # (c) append 2000 rows: some of categories 1001 and 5, one of the new category 2000 (which only the set "64" names)
    extra = T.gen_data(2000, 84, T.GEN_V1, S.NCAT)
    extra[::40, 0] = 1001.0
    extra[7::50, 0] = 5.0
    extra[777, 0] = 2000.0
    rows = np.ascontiguousarray(np.concatenate([rows, extra]))
    steps.append(dict(step="c", ops=[("append", extra)], rows=rows, live=None))
    # (d) one indexed row into category 1003, one row of category 1003 out of it
    n_indexed = rows.shape[0] - 2000
    into = int(np.flatnonzero(rows[:5000, 0] == 8)[3])
    out = int(np.flatnonzero(rows[:n_indexed, 0] == 1003)[11])
    rows = rows.copy()
    rows[into, 0], rows[out, 0] = 1003.0, 8.0
    steps.append(dict(step="d", ops=[("update", np.array([into, out], np.uint32), rows[[into, out]].copy())], rows=rows, live=None))
    # (e) reindex
    steps.append(dict(step="e", ops=[("reindex",)], rows=rows, live=None))
    # (f) an append past the tail limit (4096 rows at this size): the append itself folds the index
    more = T.gen_data(4200, 85, T.GEN_V1, S.NCAT)
    more[3::60, 0] = 1006.0
    rows = np.ascontiguousarray(np.concatenate([rows, more]))
    steps.append(dict(step="f", ops=[("append_folding", more)], rows=rows, live=None))
    # (g) delete the whole of category 5, compact, trim
    gone = np.flatnonzero(rows[:, 0] == 5).astype(np.uint32)
    keep = np.setdiff1d(np.arange(rows.shape[0]), gone).astype(np.uint32)
    rows = np.ascontiguousarray(rows[keep])
    steps.append(dict(step="g", ops=[("delete", gone), ("compact", keep), ("trim",)], rows=rows, live=None))
    _cache["life"] = steps
    return steps


# ---- 5. non-finite distances -------------------------------------------------------------------------------------------------------------
def nonfinite_data():
    """(nodes, queries, names, special): a copy of S.data()'s rows with six rows put into the categories 1002 and 1003 of the set
    "93" -- one with a +inf component, one with a NaN, two with components of +-3e19 (finite rows whose distance overflows to
    +inf), two ordinary ones -- and six more of the same kinds in two fresh categories, which the sets "nf" and "nf+" name."""
    if "nf" in _cache:
        return _cache["nf"]
    nodes = S.data()[0].copy()
    rng = np.random.default_rng(29)
    free = np.flatnonzero(nodes[:N - 400, 0] < 1000)
    rows = rng.choice(free, 12, replace=False)           # (not sorted: the kinds' ids interleave)
    special = {}
    for half, cats in ((rows[:6], [1002, 1003]), (rows[6:], NF_CATS)):
        nodes[half, 0] = np.array([cats[0], cats[1], cats[0], cats[1], cats[0], cats[1]], np.float32)
        nodes[half[0], 2 + 17] = np.inf
        nodes[half[1], 2 + 60] = np.nan
        nodes[half[2], 2 + 3] = np.float32(3e19)
        nodes[half[3], 2 + 99] = np.float32(-3e19)
        for kind, r in zip(["inf", "nan", "big", "big", "plain", "plain"], half):
            special.setdefault(kind, []).append(int(r))
    base_q, base_names = S.data()[1], S.data()[2]
    pick = [i for i in range(len(base_q)) if S.tests_c(base_q[i, 0])][:30] + [i for i in range(len(base_q)) if not S.tests_c(base_q[i, 0])][:6]
    queries = np.ascontiguousarray(base_q[pick])
    cycle = ["93", "nf", "nf+"]
    names = [cycle[i % 3] for i in range(len(pick))]
    _cache["nf"] = (nodes, queries, names, special)
    return _cache["nf"]
