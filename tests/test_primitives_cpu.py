"""The case set of tests/primitives_model.py, checked without a GPU: that it can tell every wrong rule from the right one, that
its select lists reach the branches they were built for, that its distance and predicate models are the oracle's, and that the
harness (tests/device_primitives.hip) still compiles against the device headers -- a changed signature fails here."""
import ctypes as C

import numpy as np
import pytest

import hvs_testlib as T
import primitives_model as M

SECTIONS = M.sections()


def _differs(section, rules):
    """does the model under `rules` differ from the model in a word both define?"""
    base, other = section.expected(), section.expected(frozenset(rules))
    for name, (v0, m0) in base.items():
        v1, m1 = other[name]
        if v0.size != v1.size or np.any((v0 != v1) & m0 & m1):
            return True
    return False


@pytest.mark.parametrize("section,rule", [(s, r) for s, rs in M.RULES.items() for r in rs])
def test_every_wrong_rule_changes_an_expected_output(section, rule):
    assert _differs(SECTIONS[section], [rule]), "no case of section %s tells rule %s from the right one" % (section, rule)


def test_rank_ties_by_slot_descending_cannot_be_observed():
    """equal keys write equal ids and distances, whichever slot takes the lower rank: no output depends on the tie order"""
    assert not _differs(SECTIONS["pad_rank"], M.UNOBSERVABLE_RULES["pad_rank"])


def test_cases_cover_every_section_and_blob():
    assert set(SECTIONS) == set(M.RULES) | {"cut"}
    outs = set()
    for s in SECTIONS.values():
        exp = s.expected()
        assert set(exp) <= set(s.labels), s.name
        outs |= set(exp)
    assert outs == set(M.OUT_BLOBS)


@pytest.mark.parametrize("nk", [4, 8])
def test_select_lists_reach_every_last_digit_width_and_both_rank_edges(nk):
    """A host trace of the histogram descent's control flow, used for this coverage condition only (the expected results are a
    sort's)."""
    sel = [p for p in SECTIONS["select"].parts if p.nk == nk][0]
    traces = [(c, sel.trace(i)) for i, c in enumerate(sel.cases)]
    top = [(c, t) for c, t in traces if c[0] == "top_bit"]
    ends_at_0 = [t for _, t in top if t[-1]["lo"] == 0]
    assert len(ends_at_0) == len(top), "the pair x, x ^ 1 at ranks keep, keep + 1 takes the descent to bit 0"
    assert {t[-1]["width"] for t in ends_at_0} == set(range(1, 9))
    assert {t[0]["hi"] % 8 for t in ends_at_0} == set(range(8))
    assert {t[0]["hi"] for _, t in top} == set(range(3 if nk == 4 else 7, 64)), "every top differing bit the key count allows"
    steps = [s for _, t in traces for s in t]
    assert any(s["first"] and s["rem"] > 1 for s in steps) and any(s["last"] and s["rem"] > 1 for s in steps)
    assert any(s["bucket0"] for s in steps) and any(s["top_bucket"] and s["width"] == 8 for s in steps)
    assert any(t[0]["rem"] == 1 for _, t in traces), "rem == 1 on the first step"
    edge = {c[1]: t[0] for c, t in traces if c[0] == "edge"}
    assert edge["first"]["first"] and edge["last"]["last"] and edge["bucket0"]["bucket0"] and edge["highest"]["top_bucket"] and edge["single"]["rem"] == 1
    counts = {(c[2].size, c[3]) for c, _ in traces}
    assert set(M.select_counts(nk)) <= counts
    assert any(cnt == keep + 1 for cnt, keep in counts) and any(cnt == sel.cap for cnt, keep in counts)
    for fam in ("top_bit", "edge", "one_dist", "realistic", "special"):
        assert any(c[0] == fam for c, _ in traces), fam
    # the contract's precondition, and the dirty tail: every word behind cnt is smaller than every valid key (or 0 beside the key 0)
    for (fam, p, keys, keep), row in zip(sel.cases, sel.lists):
        assert np.unique(keys).size == keys.size and keep < keys.size <= sel.cap
        tail = row[keys.size:]
        assert np.all((tail < keys.min()) | (tail == 0)), (fam, p)


def test_distance_model_is_the_oracle_on_every_family():
    lib = T.oracle()
    seen = {}
    for fam in M.DIST_FAMILIES:
        d, q = M.dist_family(fam)
        simd, scal = M.dist_simd_order(d, q), M.dist_scalar_order(d, q)
        for i in range(d.shape[0]):
            for mine, fn in ((simd, lib.hvs_oracle_dist_simd_order), (scal, lib.hvs_oracle_dist_scalar_order)):
                want = np.float32(fn(T._fp(np.ascontiguousarray(d[i])), T._fp(np.ascontiguousarray(q[i]))))
                assert M.canon_bits(mine[i]) == M.canon_bits(want), (fam, i, mine[i], want)
        seen[fam] = (simd, scal)
    tiny = np.float32(1.17549435e-38)
    assert np.all((seen["tiny"][0] > 0) & (seen["tiny"][0] < tiny)) and np.all((seen["tiny"][1] > 0) & (seen["tiny"][1] < tiny))
    assert np.all(np.isposinf(seen["overflow"][0])) and np.all(np.isposinf(seen["overflow"][1]))
    near = seen["near_overflow"][0]
    assert np.isposinf(near).any() and np.isfinite(near).any(), "a scale at which some results overflow and some do not"
    assert np.isnan(seen["non_finite"][0]).any() and np.isinf(seen["non_finite"][0]).any()
    for fam in ("uniform", "wide", "known_answer"):
        assert (M.f32_bits(seen[fam][0]) != M.f32_bits(seen[fam][1])).any(), "the two orders differ in bits: " + fam


def test_predicate_table_is_the_oracle():
    lib = T.oracle()
    p = SECTIONS["predicate"]
    want = p.expected()["PRED_PASS"][0].reshape(p.Q.shape[0], p.rows.shape[0])
    for i, q in enumerate(p.Q):
        qq = np.ascontiguousarray(q)
        for j, row in enumerate(p.rows):
            assert int(lib.hvs_oracle_predicate(T._fp(np.ascontiguousarray(row)), T._fp(qq))) == int(want[i, j]), (q, row)
    assert want.any() and not want.all()
    o = p.expected()["ORD"][0].astype(np.int64)
    assert np.all(np.diff(o) > 0), "hvs_ordered_u32 is strictly monotone over the table's floats, -0 in front of +0"


def test_blob_files_round_trip(tmp_path):
    path = str(tmp_path / "b.bin")
    arrays = [np.arange(5, dtype=np.uint32), np.arange(3, dtype=np.uint64) << np.uint64(40), np.zeros(0, np.uint32), np.ones((2, 3), np.float32)]
    M.write_blobs(path, arrays)
    raw = np.fromfile(path, np.uint32)
    assert raw[0] == M.MAGIC and raw[1] == 4
    for i, a in enumerate(arrays):
        off, ln = int(raw[2 + 2 * i]), int(raw[3 + 2 * i])
        assert off % 2 == 0 and np.array_equal(raw[off:off + ln], np.ascontiguousarray(a).view(np.uint32).ravel())


def test_harness_cross_compiles_for_gfx950(tmp_path):
    M.build_harness(str(tmp_path / "device_primitives.out"))
