"""Category sets: what tests/test_in_cpu.py and tests/test_in.py share -- a numpy restatement of hvs_in_plan, the fresh-value
rewrite of D that turns a set query into a plain one for the oracle, and the data set of the GPU tests."""
import numpy as np

import hvs_testlib as T

VSTAR = np.float32(7777.0)   # a category no data set here uses
N, NCAT = 65536, 10
PLACED = {1001: 5, 1002: 60, 1003: 33, 1004: 99, 1005: 0, 1006: 150}


def tests_c(t):
    """the engines' reading of a type float: does the query compare C?"""
    t = np.float32(t)
    return bool(-1.0 < t < 4.0) and int(t) in (1, 3)


def categories(values):
    """the distinct categories a set names, ascending: values truncate as the engines' v does, NaN and values outside int32 drop"""
    v = np.asarray(values, np.float32).ravel()
    v = v[(v >= np.float32(-2147483648.0)) & (v < np.float32(2147483648.0))]
    return np.unique(np.trunc(v).astype(np.float32) + np.float32(0.0))      # (-0.0 + 0.0 = +0.0)


def _as_lists(sets):
    if isinstance(sets, tuple):
        off, vals = np.asarray(sets[0], np.int64), np.asarray(sets[1], np.float32)
        if off.size == 0 or off[0] != 0 or (np.diff(off) < 0).any() or off[-1] > vals.size:
            return None
        return [vals[off[i]:off[i + 1]] for i in range(off.size - 1)]
    return [np.asarray(s, np.float32) for s in sets]


def plan_model(q_rows, sets):
    """(nsub, sub_offsets, parent, value) as hvs_in_plan defines them, or None where it refuses"""
    sets = _as_lists(sets)
    if sets is None:
        return None
    sub, parent, value = [0], [], []
    for p, s in enumerate(sets):
        cats = categories(s)
        if cats.size > 64:
            return None
        if len(s) and (q_rows is None or tests_c(q_rows[p, 0])):
            vals = list(cats) if cats.size else [np.float32(np.nan)]
        else:
            vals = [q_rows[p, 1] if q_rows is not None else np.float32(np.nan)]
        parent += [p] * len(vals)
        value += vals
        sub.append(len(parent))
    return len(parent), np.array(sub, np.uint32), np.array(parent, np.uint32), np.array(value, np.float32)


def rewrite(nodes, queries, values):
    """(D', Q'): every C of the set rewritten to VSTAR, every query that compares C asking for VSTAR -- a plain query on D' is
    the set query on D (include/hvs.h "category sets")"""
    assert not (nodes[:, 0] == VSTAR).any()
    d = nodes.copy()
    d[np.isin(nodes[:, 0], categories(values)), 0] = VSTAR
    q = np.ascontiguousarray(queries, np.float32).copy()
    for row in q:
        if tests_c(row[0]):
            row[1] = VSTAR
    return d, q


def _place(nodes, rng, cat, count, a, b):
    free = np.flatnonzero(nodes[a:b, 0] < 1000) + a
    ids = np.sort(rng.choice(free, count, replace=False))
    nodes[ids, 0] = np.float32(cat)
    return ids


# the distinct sets of the GPU tests, by name
SETS = {
    "two": [2, 5],
    "five": [0, 3, 4, 7, 9],
    "65": [1001, 1002],                                  # 65 rows: padded at k = 100
    "93": [1002, 1003, 1005],                            # 93 rows
    "132": [1003, 1004, 1005],                           # over k = 100, under 256
    "none": [1005],                                      # nothing: all padding
    "twice": [3, 3, 0.0, -0.0, 3.5],                     # categories 0 and 3, each named more than once
    "64": [1001, 2] + list(range(2000, 2062)),           # 64 distinct values, most of them absent
    "150": [1005, 1006],                                 # the paging union
    "ties": [1002, 1006],                                # holds two rows with one vector, one in each category
    "empty": [],
    "s45": [1001, 1002],                                 # of the small data set: 45 rows
    "s75": [1005, 1003, 1002, 1001],                     # ... 75 rows
}
SMALL_N = 901                                            # no index below 4096 rows: every engine setting runs the plain exact scan
SMALL_PLACED = {1001: 5, 1002: 40, 1003: 30, 1005: 0}
_cache = {}


def data():
    """(nodes, queries, names): names[i] = the set of query i (a key of SETS).  224 gen-v1 queries -- the types 1 and 3 among them
    cycle through the sets, the others carry one too and must not notice -- plus hand-made ones."""
    if "data" in _cache:
        return _cache["data"]
    nodes = T.gen_data(N, 81, T.GEN_V1, NCAT)
    rng = np.random.default_rng(17)
    ids = {cat: _place(nodes, rng, cat, cnt, 0, N - 400) for cat, cnt in PLACED.items()}
    for cat, cnt in PLACED.items():
        assert int((nodes[:, 0] == cat).sum()) == cnt
    nodes[ids[1006][40], 2:] = nodes[ids[1002][10], 2:]                      # one vector in two categories of "ties"
    gen = T.gen_queries(224, 82, T.GEN_V1, NCAT)
    cycle = ["two", "five", "65", "93", "132", "none", "twice", "64", "empty", "150"]
    names = [cycle[i % len(cycle)] for i in range(224)]
    hand = T.gen_queries(12, 83, T.GEN_V1, NCAT)
    hand[0, :4] = [1, 1001, -1, -1]
    hand[1, :4] = [3, 1001, 0.05, 0.95]
    hand[2, :4] = [3, 4, 0.2, 0.6]
    hand[3, :4] = [0, -1, -1, -1]
    hand[4, :4] = [2, -1, 0.3, 0.5]
    hand[5, :4] = [7, 3, -1, -1]                                           # invalid type: matches nothing, with or without a set
    hand[6, :4] = [1, 3e9, -1, -1]                                         # its own v is unusable: the set replaces it
    hand[7, :4] = [1, 2, -1, -1]
    hand[7, 4:] = nodes[ids[1002][10], 2:]                                 # on top of the shared vector: distance 0 twice
    hand[8, :4] = [1.5, 2, -1, -1]                                         # read as type 1
    hand[9, :4] = [3, 2, 0.0, 1.0]
    hand[10, :4] = [1, 2, -1, -1]
    hand[11, :4] = [np.nan, 2, -1, -1]
    hnames = ["132", "65", "five", "two", "five", "two", "two", "ties", "93", "150", "empty", "two"]
    queries = np.ascontiguousarray(np.concatenate([gen, hand]))
    _cache["data"] = (nodes, queries, names + hnames)
    return _cache["data"]


def small():
    """(nodes, queries, names) of the second data set: 901 rows, 10 gen-v1 categories of about 90 rows each and hand-placed ones,
    so that unions land under, between and over k = 8, 100, 256 -- and the last 256 rows, the padding, hold matches of every set"""
    if "small" in _cache:
        return _cache["small"]
    nodes = T.gen_data(SMALL_N, 91, T.GEN_V1, NCAT)
    rng = np.random.default_rng(19)
    for cat, cnt in SMALL_PLACED.items():
        _place(nodes, rng, cat, cnt, 0, SMALL_N)
        assert int((nodes[:, 0] == cat).sum()) == cnt
    gen = T.gen_queries(72, 92, T.GEN_V1, NCAT)
    cycle = ["two", "five", "s45", "s75", "none", "twice", "64", "empty"]
    names = [cycle[i % len(cycle)] for i in range(72)]
    hand = T.gen_queries(8, 93, T.GEN_V1, NCAT)
    hand[0, :4] = [1, 1001, -1, -1]
    hand[1, :4] = [3, 1002, 0.05, 0.95]
    hand[2, :4] = [1, 3e9, -1, -1]
    hand[3, :4] = [3, 4, 0.2, 0.8]
    hand[4, :4] = [0, -1, -1, -1]
    hand[5, :4] = [2, -1, 0.3, 0.5]
    hand[6, :4] = [7, 3, -1, -1]
    hand[7, :4] = [1, 2, -1, -1]
    hnames = ["s75", "s45", "s45", "five", "two", "five", "two", "none"]
    _cache["small"] = (nodes, np.ascontiguousarray(np.concatenate([gen, hand])), names + hnames)
    return _cache["small"]


def sets_of(names):
    return [SETS[x] for x in names]


def expected(nodes, queries, names, k, sp, engine="canonical", tag="data"):
    """the oracle on the rewritten copy of D: one run per distinct set, padding on.  Returns (ids, dists, m) with m[q] = the
    rows of the prefix that pass query q's set predicate (their sum is hvs_timing.pairs)."""
    ck = (tag, k, float(sp), engine)
    if ck in _cache:
        return _cache[ck]
    n = nodes.shape[0]
    sn = int(T.oracle().hvs_oracle_sn(sp, n))
    ids = np.zeros((len(queries), k), np.uint32)
    d = np.zeros((len(queries), k), np.float32)
    m = np.zeros(len(queries), np.int64)
    names = np.array(names)
    with T.oracle_k(k):
        for name in sorted(set(names)):
            sel = np.flatnonzero(names == name)
            d2, q2 = rewrite(nodes, queries[sel], SETS[name]) if SETS[name] else (nodes, queries[sel])
            ids[sel], d[sel] = T.oracle_query(d2, q2, sp, engine=engine)
            m[sel] = [int(T._passes(d2[:sn], q).sum()) for q in q2]
    _cache[ck] = (ids, d, m)
    return _cache[ck]
