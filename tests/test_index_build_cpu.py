"""The case set of tests/index_model.py without a GPU: tests/device_index.hip cross-compiles, its --host dump (hvs_make_levels,
hvs_storage_to_block, hvs_attr_key and its inverse) is the model's restatement, every wrong rule of the model changes an
expected output word of some case -- so the GPU comparison of tests/test_index_build.py would tell it from the right rule --
and the cases reach the levels, blocks, class populations and bin counts they are there for."""
import subprocess

import numpy as np
import pytest

import index_model as M


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("index_host")
    exe, out = str(tmp / "device_index.out"), str(tmp / "host.bin")
    M.build_harness(exe)                                   # (for gfx950: the device code is compiled whatever mode is run)
    r = subprocess.run([exe, "--host", out], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout + r.stderr
    return M.read_results(out, M.host_names())


def test_host_struct_sizes_and_case_list(host):
    assert host["SIZES"].tolist() == [4 * M.QUANT_WORDS, 4 * M.BOUNDS_WORDS, 4 * M.LEVELS_WORDS]
    assert host["CASE_N"].tolist() == list(M.CASE_N) == [c.n for c in M.cases()]


def test_host_levels_and_storage_order(host):
    for c, n in enumerate(M.CASE_N):
        L = M.levels(n)
        assert np.array_equal(host["c%d_LEVELS" % c], L.words()), "hvs_make_levels(%d)" % n
        assert np.array_equal(host["c%d_BLOCKS" % c], L.blocks), "hvs_storage_to_block, n = %d" % n
        assert sorted(L.blocks.tolist()) == list(range(L.nblk))


def test_host_attr_keys(host):
    f = M.host_floats().view(np.float32)
    assert np.array_equal(host["KEYS"], M.attr_key(f))
    assert np.array_equal(host["KEYS_INV"], M.attr_key_inv(host["KEYS"]).view(np.uint32))
    fin = ~np.isnan(f)
    order = np.argsort(f[fin], kind="stable")
    assert np.all(np.diff(host["KEYS"][fin][order].astype(np.int64)) >= 0), "the keys do not preserve the order"
    assert np.all(host["KEYS"][~fin] == 0xFFFFFFFF) and host["KEYS"][fin].max() < 0xFFFFFFFF
    back = host["KEYS_INV"].view(np.float32)
    assert np.array_equal(back[fin], np.where(f[fin] == 0, np.float32(0), f[fin])) and not np.signbit(back[fin][f[fin] == 0]).any()


def test_shapes():
    """the smallest n at which each level rule can go wrong, derived from the level table itself"""
    L1, L31, L33, L = (M.levels(n) for n in (1, 31, 33, 4100))
    assert (L1.nblk, L31.nblk, L33.nblk) == (1, 1, 2) and L1.K == L31.K == L33.K == 0
    assert L.K >= 2 and len(set(L.radix[1:L.K + 1])) >= 2, "three levels, two different radices"
    assert L.n % 32 != 0, "a partial last block"
    assert L.blocks[-1] != L.nblk - 1, "the last storage index is not the last block"
    case = M.cases()[M.BATCH_CASE]
    assert set(L.level_of.tolist()) == set(range(L.K + 1)), "every level holds blocks"
    for o in range(2):      # the partial block's valid rows differ between the orderings: each builder run places other rows there
        last = case.perm[o][(L.nblk - 1) * 32:]
        assert last.size == L.n % 32 and np.unique(last).size == last.size
    assert not np.array_equal(case.perm[0][(L.nblk - 1) * 32:], case.perm[1][(L.nblk - 1) * 32:])


def test_data_edges():
    cs = M.cases()
    big = cs[M.BATCH_CASE]
    C, Tt = big.D[:, 0], big.D[:, 1]
    assert (np.signbit(C) & (C == 0)).any() and (~np.signbit(C) & (C == 0)).any(), "C = -0.0 beside +0.0"
    assert np.isnan(Tt).any()
    ct = big.keys()[0]
    assert np.unique(ct).size < ct.size, "duplicate (C, T) pairs"
    qz = big.quant(False)
    dq = M.i8_rows(qz)[0]
    assert dq.max() == 127 and dq.min() == -127, "both box extremes"
    assert (big.V.min(0) == big.V.max(0)).any(), "a constant dimension"
    assert cs[0].quant(False).sd == 1.0 and cs[1].quant(False).sd == 1.0, "all rows equal: scale 1"
    assert not np.array_equal(big.quant(True).kmax[:100], qz.kmax[:100]), "the rotated box differs from the plain one"
    f16 = cs[2].V
    assert (np.abs(f16) == np.float32(2.0 ** -14)).any() and (np.abs(f16) > 65504).any() and (np.abs(f16) < 2.0 ** -14).any()
    assert cs[3].quant(False).sd == 0.0 and cs[3].quant(True).sd == 0.0, "non-finite data: no INT8 format"
    # dead rows: first block, partial last block, a block all dead, blocks with none -- in the (C, T) ordering
    dead_pos = big.dead[big.perm[0]]
    per_block = np.add.reduceat(dead_pos.astype(int), np.arange(0, big.n, 32))
    assert 0 < per_block[0] < 32 and 0 < per_block[-1] and (per_block == 32).any() and (per_block == 0).any()


def test_near_integer_inits_are_rare():
    """the looser rule for the rotated builder's inits (floor of a sum known to 1e-12) cannot hide a wrong floor"""
    for c, case in enumerate(M.cases()):
        if M.runs(c, "rot"):
            assert M.near_integer_share(case) < 0.01, case.name


def test_batch_cases():
    B = M.batch()
    pops = set()
    for f in B.forms:
        pops |= set(int(x) for x in f["counts"])
    assert {0, 1, 31, 32, 33} <= pops, pops
    lay = B.layout(B.forms[0])["LAYOUT"]
    used_ct = int(np.sum(-(-B.forms[0]["counts"][:4].astype(int) // 32) * 32))
    assert lay[4] == 512 and used_ct % 512 != 0, "the type-2 part is pushed to the next multiple of 512 slots"
    assert B.forms[0]["nslots"] <= 2048 and lay[5] <= B.forms[0]["nslots"]
    bins = set()
    for counts in [f["counts"] for f in B.forms] + list(M.SYN_COUNTS):
        bins |= set(M.nbins_of(int(x)) for x in counts)
    # 4096 bins would need 2^33 queries of one class: the clamp is out of a 32-bit population's reach, 2896 is the most
    assert 1 in bins and 2 in bins and 3 in bins and max(bins) == M.nbins_of(0xFFFFFFFF) == 2896
    f = B.forms[0]
    width = f["qb"].astype(int) - f["qa"].astype(int)
    assert (width == 0).any() and (width == 1).any() and (width == B.n).any(), "ranges: empty, one row, the whole ordering"
    assert set(f["rank"].tolist()) == {0, 1, 2, 3, 4}


def _outputs(section, rules):
    """the expected words of a section under a set of rules, as one dict"""
    out = {}
    if section == "keys":
        for c, case in enumerate(M.cases()):
            out[c] = np.concatenate([x.view(np.uint32) for x in case.keys(rules)[:2]])
    elif section == "quant":
        for c, case in enumerate(M.cases()):
            out[c] = np.concatenate([case.quant(r, rules).words() for r in (False, True)])
    elif section in ("tiles", "patch"):
        for c, case in enumerate(M.cases()):
            for b in (M.BUILDERS if section == "tiles" else M.PATCH_FORMATS):
                if M.runs(c, b):
                    m = M.build_model(case, b, rules, dead=case.dead if section == "patch" else None)
                    out[c, b] = np.concatenate(m.tiles + m.norms)
    elif section == "prep":
        for si, ps in enumerate(M.prep_sets()):
            for b in M.BUILDERS:
                for v in (2, 6):
                    m = M.prep_model(ps, b, v, rules)[0]
                    out[si, b, v] = np.concatenate([np.ascontiguousarray(m[f]).view(np.uint32).ravel() for f in M.PREP_FIELDS])
    else:
        B = M.batch()
        for i, f in enumerate(B.with_rules(rules)):
            lay = B.layout(f, rules)
            out[i] = np.concatenate([f["qa"], f["qb"]] + [lay[x] for x in ("QID", "RANK", "RA", "RB", "LAYOUT")])
    return out


@pytest.mark.parametrize("section,rule", [(s, r) for s, rs in M.RULES.items() for r in rs])
def test_wrong_rule_changes_an_expected_word(section, rule):
    right, wrong = _outputs(section, frozenset()), _outputs(section, frozenset([rule]))
    assert any(not np.array_equal(right[k], wrong[k]) for k in right), "no case tells %s from the right rule" % rule


def test_prep_cases():
    """the query and cap edges of the prep section, from the model's own figures"""
    B, (s0, s1) = M.batch(), M.prep_sets()
    slot = {nm: int(np.nonzero(s0.lay["QID"] == qi)[0][0]) for nm, qi in B.edge.items()}
    for b in ("i8x16", "rot"):
        m, ex, info = M.prep_model(s0, b, 6)
        clip, rest, hopeless = info["clip"], info["rest"], info["hopeless"]
        with np.errstate(invalid="ignore"):
            margin = (np.abs(clip - 4.0 * rest) > 1e-6 * (clip + rest)) | (clip == 0.0)       # (no clip term: 0 <= 4 x rest whatever the sums)
        assert margin[s0.real & ~np.isnan(clip)].all(), "a query at the edge of hopelessness: the rotated sums could fall either way"
        if b == "i8x16":
            for nm in ("just_outside", "just_outside_t2"):
                assert 0.0 < clip[slot[nm]] <= 4.0 * rest[slot[nm]] and not hopeless[slot[nm]]
            assert 2.0 * rest[slot["between_2x_4x"]] < clip[slot["between_2x_4x"]] <= 4.0 * rest[slot["between_2x_4x"]]
            assert clip[slot["centre"]] == 0.0 and not hopeless[slot["centre"]]
            for nm in ("far_outside", "nan", "huge", "past_half"):
                assert hopeless[slot[nm]], nm
            th = m["THETA"].view(np.int32)
            assert (th[s0.real] == -0x7FFFFFFF).any() and (th == 0x7FFFFFFF)[slot["huge"]], "both clamps of thetai"
            assert 0 < hopeless.sum() < s0.real.sum() / 2
    for b in ("bf16", "f16"):
        _, _, info = M.prep_model(s0, b, 6)
        assert info["hopeless"][slot["nan"]] and info["hopeless"][slot["huge"]]
        assert info["hopeless"][slot["past_half"]] == (b == "f16")
    caps = s0.caps[s0.qi[s0.real]]
    assert np.isinf(caps).any() and (caps == -1).any() and (caps == 0).any() and ((caps > 0) & (caps < 1.2e-38)).any()
    last_real = np.nonzero(s0.real[:-1] & ~s0.real[1:])[0]
    assert np.isfinite(s0.caps[s0.qi[last_real]]).any(), "a finite cap beside a padding slot"
    # the ties of rint: on the all-equal rows the scale is 1 and the queries sit exactly half a step off the grid
    qz = s1.case.quant(False)
    t = (s1.Q[:, 4:].astype(np.float64) - qz.center[:100]) * qz.inv_sd
    assert qz.sd == 1.0 and (np.abs(t - np.floor(t)) == 0.5).any() and (np.abs(t) > 127.5).any()
