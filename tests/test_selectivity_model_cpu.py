"""The host model of the filters' selectivity (tests/selectivity_model.py) against the header it restates, against itself,
and the conditions that make the GPU assertions of tests/test_filter_selectivity.py sharp -- evaluated by the model alone, for
every GPU case, format and regime:

  (a) at most 5 % of a case's queries sit on a grid edge of the guess table (excluded from the count assertions);
  (b) the bracket is narrow: sum hi - sum lo <= 0.2 % of sum lo;
  (c) a band 25 % too wide is visible: the model with the band x 1.25 gives a sum lo at least 10 bracket widths above the
      production sum hi (FP16 is not admitted, see test_conditions_of_the_gpu_cases);
  (d) no query's list takes more keys at one level than a batch of the case's size gets in a context that reserved
      RESERVE_NQ queries, nor a group more survivor entries (the proven threshold appends ~1500 keys per type-0 query at a
      radix-16 level, above the 1024 of a fresh context: such a query would be retried whatever its thresholds);
  (e) the reckless run's retry set is non-empty and under half of the queries.

These are properties of the inputs: a GPU assertion that rests on them cannot be vacuous.
"""
import os
import subprocess

import numpy as np
import pytest

import bound_model as BM
import hvs_testlib as T
import selectivity_model as SM


@pytest.fixture(scope="module")
def header_tables(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("levels") / "selectivity_levels.out")
    subprocess.run(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O1", "-std=c++17", "-w",
                    os.path.join(T.REPO, "tests", "selectivity_levels.hip"), "-o", exe], check=True, capture_output=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    return [line.split() for line in r.stdout.splitlines()]


PLANS = [None, [2, 2], [4, 8, 32]]


def test_levels_equal_the_headers(header_tables):
    seen = {"L": 0, "B": 0, "S": 0}
    for f in header_tables:
        n, p = int(f[1]), int(f[2])
        L = SM.levels(n, plan=PLANS[p])
        seen[f[0]] += 1
        if f[0] == "L":
            K = int(f[4])
            radix = [int(x) for x in f[6:6 + K + 1]]
            stride = [int(x) for x in f[6 + K + 2:]]
            print("n=%d plan=%s K=%d radices %s strides %s" % (n, PLANS[p], K, radix[1:], stride))
            assert (L.K, L.radix, L.stride) == (K, radix, stride), (n, p, L.K, L.radix, L.stride)
        elif f[0] == "B":
            assert int(L.block_level(int(f[3]))) == int(f[4]), f
        else:
            level, a, b, want = (int(x) for x in f[3:7])
            assert L.seen_before(level, a, b) == want, f
    assert seen["L"] == 15 and seen["B"] == 120 and seen["S"] > 400, seen
    L = SM.levels(32768)
    assert (L.K, L.radix[1:], L.stride) == (2, [16, 4], [64, 4, 1])
    L = SM.levels(70001)
    assert (L.K, L.radix[1:], L.stride) == (3, [2, 16, 4], [128, 64, 4, 1])


@pytest.mark.parametrize("n,plan", [(4113, None), (70001, None), (32768, [4, 8, 32]), (300001, [2, 2])])
def test_seen_before_against_brute_force(n, plan):
    L = SM.levels(n, plan=plan)
    lvl = L.block_level(np.arange(n) // 32)
    rng = np.random.default_rng(n)
    for t in range(200):
        a = int(rng.integers(0, n))
        b = min(n, a + int(rng.integers(0, 400) if t % 2 else rng.integers(0, n)))
        if t == 0:
            a, b = 0, n
        for level in range(L.K + 2):
            assert L.seen_before(level, a, b) == int((lvl[a:b] < level).sum()), (n, plan, level, a, b)


def test_orderings_and_ranges_against_the_predicate():
    case = SM.CASES[0]
    nodes, queries = SM.case_data(case)
    o = SM.orderings(nodes)
    assert sorted(o.perm_ct.tolist()) == list(range(case.n)) and sorted(o.perm_t.tolist()) == list(range(case.n))
    unaligned = 0
    for q in queries:
        ordn, a, b = o.query_range(q)
        ids = (o.perm_t if ordn else o.perm_ct)[a:b]
        assert np.array_equal(np.sort(ids), np.nonzero(T._passes(nodes, q))[0])
        unaligned += (a % 32 != 0) or (b % 32 != 0)
    assert unaligned >= 60          # every range but the type-0 ones starts or ends inside a block
    tied = nodes.copy()
    tied[5, :2] = tied[9, :2]
    with pytest.raises(AssertionError):
        SM.orderings(tied)
    fixed = SM.dedupe_ct(tied)
    SM.orderings(fixed)
    assert (fixed != tied).sum() == 1 and fixed[9, 1] == np.nextafter(tied[9, 1], np.float32(np.inf))


@pytest.fixture(scope="module")
def ref_topk():
    out = {}

    def get(case):
        key = (case.name,)
        if key not in out:
            nodes, queries = SM.case_data(case)
            with T.oracle_k(case.k):
                out[key] = T.oracle_query(nodes, queries, case.sp)
        return out[key]
    return get


@pytest.mark.parametrize("fmt", [BM.PLAIN_I8, BM.ROT_I8, BM.BF16])
def test_walk_is_consistent(fmt, ref_topk):
    """n = 32768: lo <= hi; with proven thresholds no query fails; every query's final held set is the oracle's top-k (also
    behind a failed guess and its retry); counts are at least the true top-k rows outside level 0, and monotone in the band."""
    case = SM.CASES[0]
    nodes, queries = SM.case_data(case)
    P = SM.case_prep(case, fmt)
    L = SM.levels(case.n)
    ref_ids, ref_d = ref_topk(case)
    for regime in ("proven", "default", "reckless"):
        w = SM.case_walk(case, fmt, regime)
        assert (w["lo"] <= w["hi"]).all() and (w["retry_lo"] <= w["retry_hi"]).all()
        if regime == "proven":
            assert not w["retry"].any()
        for q in range(P.nq):
            held = w["held"][q]
            m = min(case.k, held.size)
            assert np.array_equal(held[:m].view(np.uint32), ref_d[q, :m].view(np.uint32)), (regime, q)
            ordn, a, b = P.ranges[q]
            if b - a >= case.k:
                assert m == case.k
                pos = np.empty(case.n, np.int64)
                pos[(P.ord.perm_t if ordn else P.ord.perm_ct)] = np.arange(case.n)
                outside0 = int((L.block_level(pos[ref_ids[q]] // 32) > 0).sum())
                got = w["retry_lo"][q].sum() if w["retry"][q] else w["lo"][q].sum()
                assert got >= outside0, (regime, q, got, outside0)
        tot = [SM.totals(SM.case_walk(case, fmt, regime, s), ~w["excluded"]) for s in (1.0, 1.1, SM.MUTANT_SCALE)]
        assert tot[0][0] <= tot[1][0] <= tot[2][0] and tot[0][1] <= tot[1][1] <= tot[2][1], (regime, tot)
        per_q = [SM.case_walk(case, fmt, regime, s)["lo"] for s in (1.0, SM.MUTANT_SCALE)]
        assert (per_q[0] <= per_q[1]).all()


def test_conditions_of_the_gpu_cases():
    """Conditions (a) to (e) of the module docstring, for every case, format and regime of the GPU test.

    FP16 meets (c) on no generated law at these sizes -- its band is small against the spread of the distances: the band x 1.25
    lifts sum lo by 2.1 / 1.6 / 1.4 bracket widths (proven / default / reckless) on GEN_PCA rows and by 1.8 / 1.6 / 1.9 on
    GEN_CLUSTER rows (whose bracket, 0.21 % / 0.27 % of sum lo under guessed thresholds, also misses (b)); gen-v1 rows give
    less.  FP16 therefore keeps its production assertions, on GEN_PCA rows, and is left out of the mutant run."""
    print()
    cap = SM.list_capacity(SM.RESERVE_NQ, SM.NQ_MAIN + SM.NQ_NARROW)
    assert cap == 4096
    for case in SM.CASES:
        nodes, queries = SM.case_data(case)
        nq = queries.shape[0]
        for fmt in case.fmts:
            P = SM.case_prep(case, fmt)
            if case.name == "out":
                clipped = np.asarray(P.info["clip"]) > 0.0
                assert int(P.hopeless.sum()) == 4 and int((clipped & ~P.hopeless).sum()) >= 12
            else:
                assert not P.hopeless.any()
            for regime in case.regimes:
                w = SM.case_walk(case, fmt, regime)
                m = SM.case_walk(case, fmt, regime, SM.MUTANT_SCALE)
                keep = ~w["excluded"]
                lo, hi = SM.totals(w)
                mlo, mhi = SM.totals(m, keep)
                width = hi - lo
                lift = (mlo - hi) / max(width, 1)
                print("%-7s %-6s %-8s excluded %d retried %2d exact %d  lo %7d hi %7d width %.4f %%  band x %.2f: lo %7d = hi + %6.1f widths  "
                      "longest list %d" % (case.name, fmt, regime, int(w["excluded"].sum()), int(w["retry"].sum()), int(w["exact"].sum()), lo, hi,
                                           100.0 * width / lo, SM.MUTANT_SCALE, mlo, lift, max(w["cand"].max(), w["retry_cand"].max())))
                assert w["excluded"].sum() <= 0.05 * nq, "(a)"
                assert width <= 0.002 * lo, "(b)"
                if fmt != BM.FP16:
                    assert mlo >= hi + 10 * width and width > 0, "(c)"
                    assert np.array_equal(m["retry"], w["retry"]) and not m["overflow"].any()
                assert not w["overflow"].any() and w["cand"].max() <= cap and w["retry_cand"].max() <= 3072, "(d)"
                assert (w["hi"] + 62).sum(0).max() <= SM.HVS_GROUP * cap, "(d) survivor entries of a group (<= survivors in the blocks its ranges touch)"
                if regime == "proven":
                    assert not w["retry"].any()
                    # ... which a fresh context's lists would not hold (why the GPU test reserves)
                    assert case.k < 100 or w["cand"].max() > SM.HVS_FCAP
                if regime == "reckless":
                    assert 0 < w["retry"].sum() < nq / 2, "(e)"
