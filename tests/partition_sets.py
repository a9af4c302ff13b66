"""Data sets on which the parts of a row-partitioned context DIFFER (include/hvs.h "row-partitioned context"): each
part is a leaf context that decides from its own rows which engine, index and tile format it uses, so a D whose row ranges differ
in size, box, law, finiteness or ties makes the parts take different paths.  Built deterministically (numpy default_rng with fixed
seeds, hvs_testlib.gen_*); every set comes with the properties the GPU cases of tests/test_partitioned_mixed.py rely on, and
tests/test_partitioned_mixed_cpu.py checks those properties without a GPU.

A  row counts that straddle the per-part thresholds (32768: filter engines under AUTO; 4096: an index at all)
B  "mixed": part 0 gen-v1, part 1 gen-v1 with the vectors x 3, part 2 clustered; a third of the queries from each law
C  non-finite rows in part 2 only
D  one part of equal distances, the same vector planted in the two others: ties across part edges
"""
import numpy as np

import hvs_testlib as T

NCAT = 10
N3 = 110592                                                          # 3 x 36864: sets B, C, D
ROW0_3 = (0, 36864, 73728, 110592)

# ---- A ----------------------------------------------------------------------------------------------------------------------
A_ROW0 = {98303: (0, 32768, 65536, 98303), 65535: (0, 32768, 65535), 12287: (0, 4096, 8192, 12287)}
# per n: 1.0; a cut inside the last part with that part's prefix above a quarter of its rows; one below a quarter; one inside part 0
A_SPS = {98303: (1.0, 0.87, 0.70, 0.2), 65535: (1.0, 0.87, 0.55, 0.2), 12287: (1.0, 0.87, 0.70, 0.2)}
A_KS = (100, 256)
A_CATS = {1001: 70, 1002: 45}                                        # both under 100 matches: padded at either k


def _place(nodes, rng, cat, counts, pools):
    """`counts[i]` rows of ordinary category, drawn from rows [a, b) = pools[i], become category `cat`; returns their ids"""
    out = []
    for cnt, (a, b) in zip(counts, pools):
        free = np.flatnonzero(nodes[a:b, 0] < 1000) + a
        ids = np.sort(rng.choice(free, cnt, replace=False))
        nodes[ids, 0] = np.float32(cat)
        out.append(ids)
    return np.concatenate(out)


def _pools(row0):
    return [(row0[r], row0[r + 1]) for r in range(len(row0) - 1)]


def _cat_queries(base, cats):
    """queries 2i (type 1) and 2i + 1 (type 3, T in [0.05, 0.95]) on cats[i]; the vectors are those of `base`"""
    q = base[:2 * len(cats)].copy()
    for i, cat in enumerate(cats):
        q[2 * i, :4] = [1, cat, -1, -1]
        q[2 * i + 1, :4] = [3, cat, 0.05, 0.95]
    return q


def build_a(n):
    row0 = A_ROW0[n]
    nodes = T.gen_data(n, 101 + n % 7, T.GEN_V1, NCAT)
    rng = np.random.default_rng(n)
    pools = _pools(row0)
    _place(nodes, rng, 1001, (30,) + (0,) * (len(pools) - 2) + (40,), pools)    # first and last part
    _place(nodes, rng, 1002, (0,) * (len(pools) - 1) + (45,), pools)            # the last part only
    queries = T.gen_queries(200, 102 + n % 7, T.GEN_V1, NCAT)
    special = T.gen_queries(2, 103, T.GEN_V1, NCAT)
    special[0, :4] = [1, 1001, -1, -1]
    special[1, :4] = [3, 1002, 0.0, 1.0]
    return dict(name=f"A{n}", nodes=nodes, queries=np.ascontiguousarray(np.concatenate([queries, special])), row0=row0,
                sps=A_SPS[n], cats=dict(A_CATS))


# ---- B ----------------------------------------------------------------------------------------------------------------------
B_SPLIT = {2001: (5, 0, 60), 2002: (33, 33, 34), 2003: (0, 99, 0), 2004: (0, 0, 150)}
B_X3 = slice(400, 800)                                               # the queries of part 1's law


def build_b():
    nodes = T.gen_data(N3, 111, T.GEN_V1, NCAT)
    nodes[ROW0_3[1]:ROW0_3[2], 2:] *= np.float32(3.0)
    nodes[ROW0_3[2]:] = T.gen_data(ROW0_3[3] - ROW0_3[2], 111, T.GEN_CLUSTER, NCAT, row0=ROW0_3[2])
    rng = np.random.default_rng(11)
    for cat, counts in B_SPLIT.items():
        _place(nodes, rng, cat, counts, _pools(ROW0_3))
    q1 = T.gen_queries(400, 112, T.GEN_V1, NCAT)
    q3 = T.gen_queries(400, 113, T.GEN_V1, NCAT)
    q3[:, 4:] *= np.float32(3.0)
    part1 = nodes[ROW0_3[1]:ROW0_3[2], 2:]
    q3[:, 4:] = np.clip(q3[:, 4:], part1.min(0), part1.max(0))       # inside part 1's box, so inside the whole D's
    qc = T.gen_queries(400, 114, T.GEN_CLUSTER, NCAT)
    queries = np.ascontiguousarray(np.concatenate([q1, q3, qc]))
    special = []                                                     # a dozen: every hand-placed category under every law
    for j in range(3):
        for i, cat in enumerate(B_SPLIT):
            q = 400 * j + 10 + i
            queries[q, :4] = [1, cat, -1, -1] if (i + j) % 2 == 0 else [3, cat, 0.02, 0.98]
            special.append(q)
    return dict(name="B", nodes=nodes, queries=queries, row0=ROW0_3, x3=B_X3, cats=dict(B_SPLIT), special=special)


# ---- C ----------------------------------------------------------------------------------------------------------------------
C_BAD = {2001: (50, np.nan), 2002: (150, np.nan), 2003: (60, np.inf), 2004: (30, 3e38)}   # part 2: rows, their bad component
C_FINITE = {2001: 30, 2002: 80}                                       # part 0: finite rows of the same categories
C_NAN_T = 20


def build_c():
    nodes = T.gen_data(N3, 121, T.GEN_V1, NCAT)
    rng = np.random.default_rng(12)
    pools = _pools(ROW0_3)
    bad_rows = []
    for cat, (cnt, val) in C_BAD.items():
        ids = _place(nodes, rng, cat, (0, 0, cnt), pools)
        nodes[ids, 2 + rng.integers(0, 100, cnt)] = np.float32(val)
        bad_rows.append(ids)
    for cat, cnt in C_FINITE.items():
        _place(nodes, rng, cat, (cnt, 0, 0), pools)
    free = np.flatnonzero(nodes[ROW0_3[2]:, 0] < 1000) + ROW0_3[2]
    nan_t = np.sort(rng.choice(free, C_NAN_T, replace=False))
    nodes[nan_t, 1] = np.nan
    queries = T.gen_queries(200, 122, T.GEN_V1, NCAT)
    special = _cat_queries(T.gen_queries(8, 123, T.GEN_V1, NCAT), list(C_BAD))
    odd = T.gen_queries(3, 124, T.GEN_V1, NCAT)
    odd[0, 4 + 10], odd[1, 4 + 20], odd[2, 4 + 30] = np.inf, np.nan, 1e30
    return dict(name="C", nodes=nodes, queries=np.ascontiguousarray(np.concatenate([queries, special, odd])), row0=ROW0_3,
                bad_rows=np.sort(np.concatenate(bad_rows + [nan_t])), cats={c: C_BAD[c][0] + C_FINITE.get(c, 0) for c in C_BAD},
                sps=(1.0, 0.9))


# ---- D ----------------------------------------------------------------------------------------------------------------------
D_PLANTED = 60


def build_d():
    nodes = T.gen_data(N3, 131, T.GEN_V1, NCAT)
    base = T.gen_data(1, 3)[0]
    a, b = ROW0_3[1], ROW0_3[2]
    i = np.arange(b - a)
    nodes[a:b] = base
    nodes[a:b, 0] = i % NCAT
    nodes[a:b, 1] = ((i % 1000) / 1000.0).astype(np.float32)
    nodes[a:b:7, 2:] += np.float32(0.5)
    rng = np.random.default_rng(13)
    planted = np.sort(np.concatenate([rng.choice(np.arange(lo, hi), D_PLANTED, replace=False) for lo, hi in ((0, a), (b, N3))]))
    nodes[planted, 2:] = base[2:]
    queries = T.gen_queries(65, 132, T.GEN_V1, NCAT)
    queries[64, :4] = [0, -1, -1, -1]
    queries[64, 4:] = base[2:]
    return dict(name="D", nodes=nodes, queries=np.ascontiguousarray(queries), row0=ROW0_3, base=base, planted=planted, base_query=64)


# ---- properties ---------------------------------------------------------------------------------------------------------------
def matches_per_part(nodes, row0, cat):
    return tuple(int((nodes[row0[r]:row0[r + 1], 0] == cat).sum()) for r in range(len(row0) - 1))


def passing(nodes, queries, sn):
    """rows of [0, sn) that pass each query's predicate"""
    return np.array([int(T._passes(nodes[:sn], q).sum()) for q in queries])


def excess_over_box(queries_vec, rows_vec):
    """per query: the largest distance of a component outside the rows' per-dimension [min, max], in units of that dimension's width"""
    lo, hi = rows_vec.min(0), rows_vec.max(0)
    out = np.maximum(np.maximum(lo - queries_vec, queries_vec - hi), 0)
    return (out / (hi - lo)).max(1)
