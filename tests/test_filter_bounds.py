"""The filter bounds on data that makes them tight (the sets and the f64 model: tests/bound_model.py).

Every answer of the filter engines rests on one inequality: a pair is dropped when its matrix-core estimate lies below
theta (`hvs_k_merge`).  On random data the band that theta subtracts is far from tight (the 300 nearest rows of 300 gen-v1
queries over 6 x 10^4 rows use at most 0.27 of it in every format), so a band several times too small would pass every
parity test.  These tests run the adversarial sets of bound_model -- a row in each query's true top-k that uses
0.94-0.998 of the band, k decoys right behind it -- through

* the production library: every filter engine (BF16, FP16, INT8 in both operand layouts, rotated INT8 on the rotated set)
  answers bit for bit what the oracle answers, with the requested engine, no query sent to the exact engine and the INT8
  tiles cut from the vectors the test asked for;
* mutant builds of the same source whose band is too small (-DHVS_MUTANT_BAND_SCALE / -DHVS_MUTANT_DROP, see hvs_k_merge):
  each must give wrong answers on the set built for what it breaks.  That shows the first half would notice a wrong band.

Every library runs in a child process of its own (HVS_LIB, HVS_I8_SHAPE are read at load), one at a time, under a time limit;
a child that dies or times out fails its test and no further child is started.

Not covered: rho (mutant bit 8).  What it bounds is the rounding of -|d|^2/2 to f32 and into three 16-bit pieces, relative
2^-24 of |d|^2/2, against Cauchy-Schwarz terms of relative 2^-9 (BF16) or 2^-12 (FP16) of |q||d| -- plus, in FP16, an
allowance for flushed denormal pieces.  On the float sets it is under 10^-3 of the band (test_bound_model.py,
test_rho_carries_no_usable_share); no set built here lets dropping it change an answer, so there is no DROP=8 mutant to
run.  mu is covered by mfma_bound_check.hip.

Wrong queries per mutant, of 64 per set (MI355X; the production library: none):
  BAND_SCALE=0.9   a 56, b 56, d 56, e 56         DROP=1 (E_D)   a 56, d 56, e 56
  BAND_SCALE=0.5   c 55                           DROP=2 (e_q)   a 63, d 64, e 64
                                                  DROP=4 (clip)  b 63
"""
import importlib
import os

import numpy as np
import pytest

import bound_model as BM
import hvs_testlib as T

pytestmark = pytest.mark.gpu
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
BF, F16, I8 = PKG.ENGINE_MFMA_FILTER, PKG.ENGINE_MFMA_F16, PKG.ENGINE_MFMA_I8
CHILD_TIMEOUT = 300

# mutant -> (compile flags, [(set, engine, HVS_I8_ROTATE)] that must give at least one wrong query)
MUTANTS = {
    "band_scale_0.9": (["-DHVS_MUTANT_BAND_SCALE=0.9"],
                       [("a_int8", I8, "0"), ("b_int8_clipped", I8, "0"), ("d_f16", F16, None), ("e_bf16", BF, None)]),
    "band_scale_0.5": (["-DHVS_MUTANT_BAND_SCALE=0.5"], [("c_int8_rotated", I8, "1")]),
    "drop_E_D": (["-DHVS_MUTANT_DROP=1"], [("a_int8", I8, "0"), ("d_f16", F16, None), ("e_bf16", BF, None)]),
    "drop_e_q": (["-DHVS_MUTANT_DROP=2"], [("a_int8", I8, "0"), ("d_f16", F16, None), ("e_bf16", BF, None)]),
    "drop_clip": (["-DHVS_MUTANT_DROP=4"], [("b_int8_clipped", I8, "0")]),
}

_CHILD = r"""
import importlib, json, os, sys, numpy as np
sys.path.insert(0, '.')
PKG = importlib.import_module('project---hybrid-vector-search-queries_amd')
spec = json.loads(sys.argv[1])
out = {}
for name, engine, rot in spec['runs']:
    z = np.load(os.path.join(spec['dir'], name + '.npz'))
    if rot is None:
        os.environ.pop('HVS_I8_ROTATE', None)
    else:
        os.environ['HVS_I8_ROTATE'] = rot
    with PKG.Engine(0) as e:
        e.set_engine(engine)
        e.load_data(z['nodes'])
        ids, d = e.query(z['queries'], 1.0)
        t = e.last_timing()
    tag = '%s-%d-%s' % (name, engine, rot)
    np.savez(os.path.join(spec['out'], tag + '.npz'), ids=ids, dists=d)
    out[tag] = dict(engine=int(t.engine), fallback=int(t.fallback_queries), retry=int(t.retry_queries), flags=int(t.flags),
                    rescored=int(t.rescored_pairs))
print('RESULT ' + json.dumps(out))
"""


def _tag(name, engine, rot):
    return "%s-%d-%s" % (name, engine, rot)


@pytest.fixture(scope="module")
def sets(tmp_path_factory):
    d = tmp_path_factory.mktemp("bound_sets")
    out = {}
    for s in BM.all_sets():
        ref_ids, ref_d = T.oracle_query(s.nodes, s.queries)
        np.savez(d / (s.name + ".npz"), nodes=s.nodes, queries=s.queries)
        out[s.name] = (s, ref_ids, ref_d)
    return d, out


@pytest.fixture(scope="module")
def mutant_libs(tmp_path_factory):
    """The mutant builds, compiled in parallel: engine.HIPCC_FLAGS plus the switch."""
    return T.build_variant_libs(tmp_path_factory.mktemp("mutants"), {name: flags for name, (flags, _) in MUTANTS.items()})


def _run_child(sets, runs, lib=None, shape="16"):
    data_dir, _ = sets
    out_dir = data_dir / ("out_%s_%s" % (os.path.basename(lib) if lib else "production", shape))
    out_dir.mkdir(exist_ok=True)
    env = dict(os.environ, HVS_I8_SHAPE=shape)
    env.pop("HVS_I8_ROTATE", None)
    if lib:
        env["HVS_LIB"] = lib
    else:
        env.pop("HVS_LIB", None)
    timing = T.run_child(_CHILD, dict(dir=str(data_dir), out=str(out_dir), runs=runs), env, lib or "production", CHILD_TIMEOUT)
    res = {}
    for name, engine, rot in runs:
        tag = _tag(name, engine, rot)
        z = np.load(out_dir / (tag + ".npz"))
        res[tag] = (z["ids"], z["dists"], timing[tag])
    return res


def _wrong_queries(ref_d, dists):
    """Queries whose distance sequence differs from the oracle's in any bit (a dropped neighbour changes it)."""
    return np.nonzero((np.sort(dists, axis=1).view(np.uint32) != ref_d.view(np.uint32)).any(axis=1))[0]


def _production_runs(shape):
    runs = []
    for name in ("a_int8", "b_int8_clipped", "c_int8_rotated", "d_f16", "e_bf16"):
        runs.append((name, I8, "0"))
        if shape == "16":
            runs += [(name, BF, None), (name, F16, None)]
    if shape == "16":
        runs.append(("c_int8_rotated", I8, "1"))
    return runs


@pytest.mark.parametrize("shape", ["16", "32"])
def test_production_library_is_exact_on_tight_bands(sets, shape):
    """Every filter engine on every adversarial set: bit-identical to the oracle, the requested engine ran, no exact fallback,
    the INT8 tiles cut from the vectors asked for (HVS_TIMING_I8_ROTATED)."""
    runs = _production_runs(shape)
    res = _run_child(sets, runs, shape=shape)
    _, data = sets
    for name, engine, rot in runs:
        s, ref_ids, ref_d = data[name]
        ids, dists, t = res[_tag(name, engine, rot)]
        print(shape, name, engine, rot, t)
        assert t["engine"] == engine, (name, engine, rot, t)
        assert t["fallback"] == 0, (name, engine, rot, t)
        if engine == I8:
            assert bool(t["flags"] & 4) == (rot == "1"), (name, rot, t)
        assert np.array_equal(dists.view(np.uint32), ref_d.view(np.uint32)), (name, engine, rot, _wrong_queries(ref_d, dists)[:8])
        T.check_parity(s.nodes, s.queries, ids, ref_ids, got_dists=dists)


@pytest.mark.parametrize("mutant", list(MUTANTS))
def test_mutant_band_gives_wrong_answers(sets, mutant_libs, mutant):
    """A build whose band is too small (or lacks one term) drops true neighbours on the set built for it: the production test
    above would fail on such a library."""
    _, runs = MUTANTS[mutant]
    res = _run_child(sets, runs, lib=mutant_libs[mutant])
    _, data = sets
    counts = {}
    for name, engine, rot in runs:
        _, _, ref_d = data[name]
        ids, dists, t = res[_tag(name, engine, rot)]
        counts[(name, engine, rot)] = len(_wrong_queries(ref_d, dists))
        print(mutant, name, engine, rot, "wrong queries", counts[(name, engine, rot)], t)
    assert all(c > 0 for c in counts.values()), (mutant, counts)
