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

The attached cells of the GPU test (selectivity_model.ATTACH_MATRIX: distance caps, result cursors, a row mask) get the same
treatment: the walk without attachments is the committed one to the unit, its held keys are the answers the features' own
host models give, (a), (b), (d) hold, and (c'), (e'), (g), (h), (i) of test_conditions_of_the_attached_gpu_cases; (f) each
wrong reading of the code that selectivity_model.WRONG names would leave the bracket or change the retry set somewhere.
The Prepared objects and walks come from selectivity_model's caches, shared by all tests of the module.

Exclusion lists (selectivity_model.EXCL_ATTACH) are the fourth attachment: their cells meet (a), (b), (d), (c') and
(e') -- (e") for the lists -- like the others, and test_conditions_of_the_list_cells adds (j) the walk under ex_p1 IS the walk
under after_p2, array for array, and (k) what the model says of `refused_keys`.

Shared row sets (selectivity_model.RSET_ATTACH) are the fifth: their cells meet (a), (b), (d), (e') and the walks'
consistency like the others, and the tests at the end of this module add (l) sets that restrict no query are the committed walk,
(m) the laws of the empty and the all-ones set, (n) the walk under rs_page1 IS the walk under ex_p1 with the set's counter in
place of the list's, (o) to (s) of test_conditions_of_the_set_cells; the five wrong rules of the sets are part of (f).
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


# --------------------------------------------------------------------------- the attachments: caps, cursors, a row mask

def test_no_attachment_is_the_committed_walk():
    """caps = after = live = None: the totals of the table in tests/test_filter_selectivity.py's docstring, to the unit; a cap of
    +inf on every query, a cursor in front of every key and a mask without a dead row change nothing either."""
    case = SM.CASES[0]
    nodes, queries = SM.case_data(case)
    want = {"proven": (193545, 193551, 0), "default": (39470, 39473, 0), "reckless": (57937, 57943, 21)}
    nq = queries.shape[0]
    for regime, (lo, hi, retried) in want.items():
        w = SM.case_walk(case, BM.PLAIN_I8, regime)
        assert SM.totals(w) == (lo, hi) and int(w["retry"].sum()) == retried and not w["excluded"].any(), (regime, SM.totals(w))
        r = SM.REGIMES[regime]
        # (a mask without a dead row is no mask: hvs_ctx::rs.n_dead == 0 runs the plain kernels)
        same = SM.walk(BM.PLAIN_I8, nodes, queries, case.k, case.sp, r["guess"], r["pfail"], r["mid"], 1.0,
                       SM.list_capacity(SM.RESERVE_NQ, nq), prep=SM.case_prep(case, BM.PLAIN_I8), caps=np.full(nq, np.inf, np.float32),
                       after=(np.zeros(nq, np.float32), np.zeros(nq, np.uint32)), live=np.ones(case.n, bool))
        for name in ("lo", "hi", "cand", "retry_lo", "retry_hi", "retry", "dead_hi"):
            assert np.array_equal(same[name], w[name]), (regime, name)
        assert all(np.array_equal(x, y) for x, y in zip(same["held_keys"], w["held_keys"]))


def _cell_walks(with_exact=False):
    """[(case, fmt, regime, attachment name, attachment, walk)] of every cell the GPU test runs under attachments; with_exact: also
    the cells of a case that sends queries to the exact engine (`out`)."""
    return [(case, fmt, regime, name, SM.attachment(case, name), SM.case_walk(case, fmt, regime, attach=name))
            for case, fmt, regime, name in SM.attach_cells() if with_exact or not SM.case_prep(case, fmt).hopeless.any()]


def test_attached_walks_are_consistent():
    """Every attached cell: lo <= hi, dead <= all, proven thresholds retry nobody, no dead survivor without a mask, and the final
    held keys are bit for bit what the laws of tests/within_model.py and tests/after_model.py give on full(q) of the live rows
    (SM.expected_keys) -- also behind a failed guess and its retry.  Under `mask` alone the distances also equal the oracle's
    answer on D[live] wherever k live rows match (ids mapped back through `live`)."""
    oracle_checked, expected = set(), {}
    for case, fmt, regime, name, att, w in _cell_walks():
        for p in ("", "retry_"):
            assert (w[p + "lo"] <= w[p + "hi"]).all() and (w[p + "dead_lo"] <= w[p + "dead_hi"]).all(), (case.name, fmt, regime, name)
            assert (w[p + "dead_hi"] <= w[p + "hi"]).all() and (w[p + "dead_lo"] <= w[p + "lo"]).all()
            if "live" not in att:
                assert not w[p + "dead_hi"].any()
        if regime == "proven":
            assert not w["retry"].any(), (case.name, fmt, name)
        assert not w["exact"].any()
        if (case.name, name) not in expected:
            expected[(case.name, name)] = SM.expected_keys(case, att)
        want = expected[(case.name, name)]
        for q, (got, exp) in enumerate(zip(w["held_keys"], want)):
            assert np.array_equal(got, exp), (case.name, fmt, regime, name, q, got.size, exp.size)
        if name == "mask" and case.sp == 1.0 and case.name not in oracle_checked:
            oracle_checked.add(case.name)
            nodes, queries = SM.case_data(case)
            back = np.flatnonzero(att["live"])
            with T.oracle_k(case.k):
                ref_ids, ref_d = T.oracle_query(nodes[back], queries, case.sp)
            full = 0
            for q, exp in enumerate(want):
                if exp.size == case.k:
                    full += 1
                    assert np.array_equal(SM.key_dists(exp).view(np.uint32), ref_d[q].view(np.uint32)), (case.name, q)
                    assert np.array_equal(np.sort(SM.key_ids(exp)), np.sort(back[ref_ids[q]])) or \
                        np.unique(ref_d[q]).size < case.k, (case.name, q)
            assert full >= 100


def test_conditions_of_the_attached_gpu_cases():
    """Conditions (a), (b), (d) as above and (c'), (e'), (g), (h), (i) of the attachments, for every attached cell of the GPU test:

      (c') the band x 1.25 lifts sum lo by at least 10 bracket widths above the production sum hi, for the non-FP16 formats under
           cap_kth, after_p2, mask and ex_p1, with the same retry set;
      (e') under `reckless` every attachment except cap_mixed -- every list attachment: (e") -- retries more than 0 and fewer than
           half of the queries;
      (g)  under `mask`, in every regime, some dead row is a survivor (sum dead_hi > 0): `dead_survivors` is not asserted to be 0;
      (h)  cap_mixed has at least 8 queries of each of its eight kinds;
      (i)  after_deep has at least 4 exhausted cursors and at least 4 more queries whose page behind the cursor is under-full."""
    print()
    for case, fmt, regime, name, att, w in _cell_walks(with_exact=True):
        nq = SM.case_data(case)[1].shape[0]
        keep = ~w["excluded"]
        cap = SM.list_capacity(SM.RESERVE_NQ, int(keep.sum()))
        lo, hi = SM.totals(w)
        dlo, dhi = SM.totals(w, what="dead_")
        width = hi - lo
        line = "%-7s %-6s %-8s %-10s excluded %d retried %2d  lo %7d hi %7d width %.4f %%  dead [%d, %d]  longest list %d / %d" % (
            case.name, fmt, regime, name, int(w["excluded"].sum()), int(w["retry"].sum()), lo, hi, 100.0 * width / max(lo, 1), dlo, dhi,
            w["cand"].max(), w["retry_cand"].max())
        assert w["excluded"].sum() <= 0.05 * nq, "(a) " + line
        if lo >= 1000:
            assert width <= 0.002 * lo, "(b) " + line
        assert not w["overflow"].any() and w["cand"].max() <= cap, "(d) " + line
        nretry = int(w["retry"][keep].sum())
        assert nretry == 0 or w["retry_cand"].max() <= SM.list_capacity(SM.RESERVE_NQ, nretry), "(d) retry batch " + line
        if name not in SM.RSET_ATTACH:      # (the set cells: (q) of test_conditions_of_the_set_cells counts entries, not survivors)
            assert (w["hi"] + 62)[keep].sum(0).max() <= SM.HVS_GROUP * cap, "(d) survivor entries of a group " + line
        if fmt != BM.FP16 and name in ("cap_kth", "after_p2", "mask", "ex_p1"):
            m = SM.case_walk(case, fmt, regime, SM.MUTANT_SCALE, attach=name)
            mlo, mhi = SM.totals(m, keep)
            line += "  band x %.2f: lo %7d = hi + %.1f widths" % (SM.MUTANT_SCALE, mlo, (mlo - hi) / max(width, 1))
            assert mlo >= hi + 10 * width and width > 0, "(c') " + line
            assert np.array_equal(m["retry"], w["retry"]) and not m["overflow"].any(), "(c') " + line
        print(line)
        if regime == "reckless" and name != "cap_mixed":
            assert 0 < w["retry"].sum() < nq / 2, "(e') " + line
        if name == "mask":
            assert dhi > 0, "(g) " + line
        if "cap_kind" in att:
            assert (np.bincount(att["cap_kind"], minlength=8) >= 8).all(), "(h)"
        if name == "after_deep":
            exhausted = att["after"][1] == 0xFFFFFFFF
            underfull = np.array([x.size < case.k for x in w["held_keys"]])
            assert exhausted.sum() >= 4 and (underfull & ~exhausted).sum() >= 4, "(i) %d %d" % (exhausted.sum(), (underfull & ~exhausted).sum())


def test_each_wrong_rule_is_seen():
    """(f) Each wrong rule of selectivity_model.WRONG shows on at least one (case, format, regime) of the matrix: its sum bracket
    is disjoint from the right rule's by at least 10 bracket widths, or its retry set differs."""
    print()
    where = {"cap": ("cap_kth", "cap_mixed", "cap_after", "all"), "after": ("after_p2", "after_deep", "cap_after", "all"), "mask": ("mask", "all"),
             "excl": SM.EXCL_ATTACH, "set": SM.RSET_ATTACH}
    # a list rule must show in the regime where the GPU test would meet it: with thresholds as shipped, resp. where queries are retried
    must_show_under = {"excl_in_lists": "default", "excl_seed_only": "default", "excl_retry_dropped": "reckless",
                       "set_in_lists": "default", "set_seed_only": "default", "set_retry_dropped": "reckless"}
    for wrong in SM.WRONG:
        seen = []
        for case, fmt, regime, name in SM.attach_cells():
            if name not in where[wrong.split("_")[0]] or regime != must_show_under.get(wrong, regime):
                continue
            if wrong == "set_before_list" and name not in ("rs_list", "rs_all"):
                continue
            if wrong.startswith("set_") and len(seen) >= 2:      # (seen: the other cells' walks under the rule are left out)
                break
            w = SM.case_walk(case, fmt, regime, attach=name)
            x = SM.case_walk(case, fmt, regime, attach=name, wrong=wrong)
            keep = ~w["excluded"]
            (lo, hi), (xlo, xhi) = SM.totals(w), SM.totals(x, keep)
            gap = max(xlo - hi, lo - xhi) / max(hi - lo, 1)
            retry_differs = not np.array_equal(w["retry"][keep], x["retry"][keep])
            if wrong == "set_before_list":
                # the order of the two tests moves no key and no threshold: it shows in the two refused-keys sums, which the GPU
                # test compares for equality
                sums = [(int(v["refused"][keep].sum()), int(v["set_refused"][keep].sum())) for v in (x, w)]
                assert (xlo, xhi) == (lo, hi) and not retry_differs
                if sums[0][0] != sums[1][0] and sums[0][1] != sums[1][1]:
                    seen.append("%s/%s/%s/%s: refused, set_refused %s against %s" % (case.name, fmt, regime, name, sums[0], sums[1]))
            elif gap >= 10 or retry_differs:
                seen.append("%s/%s/%s/%s: [%d, %d] against [%d, %d] (%.0f widths)%s" % (
                    case.name, fmt, regime, name, xlo, xhi, lo, hi, gap, ", retry set differs: %d against %d" % (
                        x["retry"][keep].sum(), w["retry"][keep].sum()) if retry_differs else ""))
        print("%-18s seen in %2d cells, e.g. %s" % (wrong, len(seen), seen[0] if seen else "-"))
        assert seen, wrong


# --------------------------------------------------------------------------- the fourth attachment: exclusion lists

def test_list_cells_with_an_exact_fallback_are_consistent():
    """The `out` cells (four far queries without a usable INT8 bound): what test_attached_walks_are_consistent asks, of the queries
    the filter answers; the far ones take no part in any level and the model counts nothing for them."""
    cells = [c for c in _cell_walks(with_exact=True) if c[5]["exact"].any()]
    assert sorted((c[0].name, c[2], c[3]) for c in cells) == [("out", rg, name) for rg in ("proven", "reckless") for name in ("ex_p1", "rs_half")]
    for case, fmt, regime, name, att, w in cells:
        assert not w["set_refused"][w["exact"]].any() and (name != "rs_half" or (att["sets"][1][w["exact"]] != SM.SET_NONE).any())
        for p in ("", "retry_"):
            assert (w[p + "lo"] <= w[p + "hi"]).all() and not w[p + "dead_hi"].any()
        if regime == "proven":
            assert not w["retry"].any()
        assert int(w["exact"].sum()) == 4 and not (w["retry"] & w["exact"]).any()
        assert not w["refused"][w["exact"]].any() and not w["hi"][w["exact"]].any()
        fulls = SM.case_fulls(case)
        assert all(fulls[q].size >= case.k for q in np.flatnonzero(w["exact"])), "the far queries list matched rows: the sink must refuse"
        for q, (got, exp) in enumerate(zip(w["held_keys"], SM.expected_keys(case, att))):
            assert w["exact"][q] or np.array_equal(got, exp), (regime, q, got.size, exp.size)


def test_conditions_of_the_list_cells():
    """(j) for every case, format and regime the walk under ex_p1 equals the walk under after_p2 in lo, hi, cand, fails, overflow,
           both retry brackets and the held keys: excluding page 1 re-scores what the page-2 cursor re-scores;
       (k) `refused` summed over a cell is positive for every list attachment, and under ex_p1 with proven thresholds it is k times
           the number of queries with at least k matches plus the match counts of the others (each listed key is asked for once:
           tau never falls below the k-th unlisted key, which lies behind all of them);
       the raw lists of ex_deep put the sort and the de-duplication in the path of those counts."""
    print()
    for case in SM.CASES:
        fulls = SM.case_fulls(case)
        for fmt in case.fmts:
            exact = SM.case_prep(case, fmt).hopeless
            for regime in case.regimes:
                a, x = SM.case_walk(case, fmt, regime, attach="after_p2"), SM.case_walk(case, fmt, regime, attach="ex_p1")
                for name in ("lo", "hi", "cand", "fails", "overflow", "retry", "retry_lo", "retry_hi", "retry_cand", "excluded"):
                    assert np.array_equal(a[name], x[name]), ("(j)", case.name, fmt, regime, name)
                assert all(np.array_equal(p, q) for p, q in zip(a["held_keys"], x["held_keys"])), ("(j)", case.name, fmt, regime)
                assert not a["refused"].any()
                if regime == "proven":
                    want = sum(min(case.k, fulls[q].size) for q in range(len(fulls)) if not exact[q])
                    assert int(x["refused"].sum()) == want > 0, ("(k)", case.name, fmt, int(x["refused"].sum()), want)
    for case, fmt, regime, name, att, w in _cell_walks(with_exact=True):
        if name in SM.EXCL_ATTACH:
            print("%-7s %-6s %-8s %-10s refused %6d  listed %6d" % (case.name, fmt, regime, name, int(w["refused"].sum()), sum(x.size for x in att["excl"])))
            assert w["refused"].sum() > 0, ("(k)", case.name, fmt, regime, name)
    raw = SM.attachment(SM.CASES[0], "ex_deep")["excl"]
    import exclude_model as XM
    assert all(r.size <= XM.EXCLUDE_MAX for r in raw)
    doubled = sum(np.unique(r).size < r.size for r in raw)
    descending = sum(r.size > 3 and r[0] != 0xFFFFFFFF and (np.diff(SM.key_ids(SM.case_fulls(SM.CASES[0])[q][:3])[::-1]) != 0).all() for q, r in enumerate(raw))
    assert doubled >= 70 and descending >= 70 and sum((r == 0xFFFFFFFF).any() for r in raw) >= 70, (doubled, descending)
    assert sum(r.size == XM.EXCLUDE_MAX for r in raw) >= 20


# --------------------------------------------------------------------------- the fifth attachment: shared row sets

def _set_cells():
    return [c for c in _cell_walks(with_exact=True) if c[3] in SM.RSET_ATTACH]


def test_unrestricted_sets_are_the_committed_walk():
    """(l) sets=None is the committed walk (test_no_attachment_is_the_committed_walk pins its totals); sets whose every index is
    0xFFFFFFFF -- the EXCL forms with `if (s == 0xFFFFFFFFu) return true;` -- reproduce it array for array and refuse nothing."""
    case = SM.CASES[0]
    nodes, queries = SM.case_data(case)
    nq = queries.shape[0]
    member = np.random.default_rng(7).random((3, case.n)) < 0.3
    for regime in ("proven", "default", "reckless"):
        w = SM.case_walk(case, BM.PLAIN_I8, regime)
        r = SM.REGIMES[regime]
        same = SM.walk(BM.PLAIN_I8, nodes, queries, case.k, case.sp, r["guess"], r["pfail"], r["mid"], 1.0, SM.list_capacity(SM.RESERVE_NQ, nq),
                       prep=SM.case_prep(case, BM.PLAIN_I8), sets=(member, np.full(nq, SM.SET_NONE, np.uint32)))
        for name in ("lo", "hi", "cand", "ent", "retry_lo", "retry_hi", "retry_cand", "retry", "fails", "excluded"):
            assert np.array_equal(same[name], w[name]), (regime, name)
        assert all(np.array_equal(x, y) for x, y in zip(same["held_keys"], w["held_keys"]))
        assert not same["set_refused"].any() and not same["refused"].any() and not w["set_refused"].any()


def test_laws_of_the_edge_sets():
    """(m) rs_edges, every cell: a query on the all-ones set (shipped with dirty bits past n) or without a restriction walks exactly
    as without an attachment; a query on the empty set admits nothing -- no list takes a key, tau never moves, nothing is retried,
    every row of the range is a survivor at every level >= 1 -- and its set_refused is the rows of the range in the sampled prefix,
    once (one pass)."""
    cells = [c for c in _set_cells() if c[3] == "rs_edges"]
    assert {c[0].name for c in cells} == {"v1_32k", "v1_70k"}
    for case, fmt, regime, name, att, w in cells:
        P, L = SM.case_prep(case, fmt), SM.levels(case.n)
        plain = SM.case_walk(case, fmt, regime)
        idx = att["sets"][1]
        empty, free = idx == 0, idx != 0
        assert empty.sum() >= 30 and (idx == 1).sum() >= 30 and (idx == SM.SET_NONE).sum() >= 30
        for field in ("lo", "hi", "cand", "ent", "retry_lo", "retry_hi", "retry_cand", "retry", "fails"):
            assert np.array_equal(w[field][free], plain[field][free]), (case.name, fmt, regime, field)
        assert all(np.array_equal(w["held_keys"][q], plain["held_keys"][q]) for q in np.flatnonzero(free))
        assert not w["set_refused"][free].any()
        assert not w["cand"][empty].any() and not w["retry"][empty].any() and not w["retry_hi"][empty].any()
        for q in np.flatnonzero(empty):
            ordn, a, b = P.ranges[q]
            ids = (P.ord.perm_t if ordn else P.ord.perm_ct)[a:b]
            rows = np.bincount(L.block_level(np.arange(a, b) // 32), minlength=L.K + 1)
            assert np.array_equal(w["lo"][q], rows[1:]) and np.array_equal(w["hi"][q], rows[1:]), (case.name, fmt, regime, q)
            assert w["held_keys"][q].size == 0 and w["set_refused"][q] == int((ids < w["sn"]).sum()) > 0, (case.name, fmt, regime, q)
        words = SM.packed_sets(case, "rs_edges")
        bits = np.unpackbits(words.view(np.uint8), axis=1, bitorder="little")
        assert not bits[0].any() and bits[1].all()
        assert case.n % 64 == 0 or bits.shape[1] > case.n, "the 70001-row case has bits past n"
    assert SM.packed_sets(SM.case_by_name("v1_70k"), "rs_edges").shape[1] * 64 - 70001 == 15


def test_rs_page1_is_the_twin_of_ex_p1():
    """(n) for every case, format and regime the walk under rs_page1 -- one set per query, the complement of its page 1 -- equals the
    walk under ex_p1 (and so under after_p2: (j)) in lo, hi, cand, fails, overflow, both retry brackets and the held keys, and the
    set refuses key for key what the list refuses."""
    for case in SM.CASES:
        for fmt in case.fmts:
            for regime in case.regimes:
                x, s = SM.case_walk(case, fmt, regime, attach="ex_p1"), SM.case_walk(case, fmt, regime, attach="rs_page1")
                for name in ("lo", "hi", "cand", "ent", "fails", "overflow", "retry", "retry_lo", "retry_hi", "retry_cand", "excluded"):
                    assert np.array_equal(x[name], s[name]), ("(n)", case.name, fmt, regime, name)
                assert all(np.array_equal(p, q) for p, q in zip(x["held_keys"], s["held_keys"])), ("(n)", case.name, fmt, regime)
                assert np.array_equal(s["set_refused"], x["refused"]) and not s["refused"].any() and not x["set_refused"].any()
                assert s["set_refused"].sum() > 0


def test_conditions_of_the_set_cells():
    """Per cell of the GPU test with row sets, beside (a), (b), (d), (e') of test_conditions_of_the_attached_gpu_cases:

      (o) set_refused summed over the cell is positive; under `reckless` at least 6 queries are retried and at least 6 are not; in
          rs_ranges at least 4 queries have fewer than k members to answer with and at least 4 have k;
      (p) the queries left out (`excluded`) are exactly those of the case without an attachment: the grid edge depends on the
          range only;
      (q) no query overflows its list at list_capacity(RESERVE_NQ, 112), and the survivor entries of all queries together (`ent`
          + 8 per query and level for the rows of the two edge blocks outside its range) stay within HVS_GROUP lists -- the
          empty-set queries' runs of survivors take an eighth of their length in entries;
      (r) rs_list: both counters positive and at least 100 keys asked for that are listed AND outside the set;
      (s) in the cells of the band x 1.25 build the model's bracket for that band lies strictly above the production bracket."""
    print()
    seen = set()
    for case, fmt, regime, name, att, w in _set_cells():
        seen.add(name)
        keep = ~w["excluded"]
        plain = SM.case_walk(case, fmt, regime)
        cap = SM.list_capacity(SM.RESERVE_NQ, int(keep.sum()))
        members = np.array([x.size for x in SM.expected_keys(case, att)])
        answered = keep & ~w["exact"]
        line = "%-7s %-6s %-8s %-9s retried %2d  set_refused %7d refused %6d both %5d  entries %6d / %6d  under-full %3d empty %2d  longest list %4d / %4d" % (
            case.name, fmt, regime, name, int(w["retry"][keep].sum()), int(w["set_refused"][keep].sum()), int(w["refused"][keep].sum()),
            int(w["both"][keep].sum()), (w["ent"] + 8)[keep].sum(0).max(), (w["retry_ent"] + 8)[w["retry"] & keep].sum(0).max(initial=0),
            int((members < case.k).sum()), int((members == 0).sum()), w["cand"].max(), w["retry_cand"].max())
        print(line)
        assert w["set_refused"][keep].sum() > 0 and not w["set_refused"][w["exact"]].any(), "(o) " + line
        if regime == "reckless":
            assert w["retry"][answered].sum() >= 6 and (~w["retry"])[answered].sum() >= 6, "(o) " + line
        if name == "rs_ranges":
            assert (members < case.k).sum() >= 4 and (members >= case.k).sum() >= 4, "(o) " + line
        assert np.array_equal(w["excluded"], plain["excluded"]), "(p) " + line
        assert not w["overflow"].any() and w["cand"].max() <= cap == 4096, "(q) " + line
        assert (w["ent"] + 8)[keep].sum(0).max() <= SM.HVS_GROUP * cap, "(q) " + line
        nretry = int(w["retry"][keep].sum())
        if nretry:
            assert (w["retry_ent"] + 8)[w["retry"] & keep].sum(0).max() <= SM.HVS_GROUP * SM.list_capacity(SM.RESERVE_NQ, nretry), "(q) " + line
        if "excl" in att:
            assert w["refused"][keep].sum() > 0, "(r) " + line
        if name == "rs_list":
            assert w["both"][keep].sum() >= 100, "(r) " + line
    assert seen == set(SM.RSET_ATTACH)
    wide = [c for c in SM.attach_cells(wide=True) if c[3] in SM.RSET_ATTACH]
    assert len(wide) == 2
    for case, fmt, regime, name in wide:
        w, m = SM.case_walk(case, fmt, regime, attach=name), SM.case_walk(case, fmt, regime, SM.MUTANT_SCALE, attach=name)
        (lo, hi), (mlo, mhi) = SM.totals(w), SM.totals(m, ~w["excluded"])
        print("%-7s %-6s %-8s %-9s production [%d, %d]  band x %.2f [%d, %d]" % (case.name, fmt, regime, name, lo, hi, SM.MUTANT_SCALE, mlo, mhi))
        assert mlo > hi, "(s)"
        assert np.array_equal(m["retry"], w["retry"]) and np.array_equal(m["set_refused"], w["set_refused"])
