"""The index build kernels and the batch layout kernels of csrc/hvs_filter.h, each launched on its own on the GPU
(tests/device_index.hip, in the grid and block shapes csrc/hvs.hip uses) and compared with the host models of
tests/index_model.py: hvs_k_attr_keys; hvs_k_quant_reset, hvs_k_minmax, hvs_k_minmax_rot and hvs_k_quant_params; the four tile
builders on both orderings (hvs_k_build_tiles in BF16 and F16, hvs_k_build_tiles_i8, _i8x16 and _i8x16_rot); hvs_k_patch_tiles
run twice under one mask; hvs_k_plan_stats with step 1 and 7; hvs_k_count_classes, hvs_k_query_keys2 and hvs_k_layout in the
q0 + range form and the list form, the layout from the production grid, from one workgroup and from three; hvs_k_prep.

Exactness (index_model.py states it in full): word for word, except values behind a device sqrt (at or above the exact f64
value, at most one f32 ulp above the model's rounded-up value) and order-dependent f64 sums (relative 1e-12, an accumulator
init from one of them floor(v) for a v that close to the model's).

The harness is built once per session and run once, in one process; a run that ends non-zero or runs out of time fails every
section's test with its output attached, and nothing is run again.

hvs_k_prep<false> and <true> run in BF16, F16, I8, I8X16 and rotated I8X16, with for_filter and count_pairs 0 and 1, over
arrays pre-filled with 0xEE, on the range form's layout and on one group of queries over the all-equal rows (scale 1: exact ties
of rint).  theta / thetai are the model's formula on the device's own stored qn, normq, eq, nqb and HvsBounds.

Beyond the three classes: the rotated formats' sums (hvs_k_build_tiles_i8x16_rot's row sums, rotated hvs_k_prep's qn, nb2, e2
and clip term) are LDS atomicAdd sums of 128 terms in any order, so the values rounded up from them (e_d8, n_d8, eq, nqb, the
clip term in normq) are compared within the f64 summation bound on both sides: at or above exact (1 - 1e-12), at most one ulp
above the rounded-up model (1 + 1e-12).  tests/test_index_build_cpu.py asserts that no query lies that close to the edge of
hopelessness.

Measured on an MI355X host: the harness compiles in 2.2 s and runs in 0.3 s of wall time, 0.23 s inside the program, most of it
the runtime's start: keys 8.6 ms (with the first launch), quant 0.8 ms, tiles 8.6 ms, patch 6.4 ms, plan 0.4 ms, batch 1.9 ms,
prep 33 ms (80 launches).  The whole module takes 3.4 s.  RUN_TIMEOUT_S leaves the same wide margin as tests/test_primitives.py:
the tested code is a few hundred trivial launches, so the margin hides nothing.  Of the 173130 values behind a device sqrt or
rounded up from an order-dependent sum (37 row bounds of the builders, 37 of hvs_k_plan_stats, the rest eq, nqb and normq of
hvs_k_prep) none differed from the model.  Nothing else differed either: no file of csrc/ changed.
"""
import os
import subprocess
import time

import numpy as np
import pytest

import index_model as M

pytestmark = pytest.mark.gpu

RUN_TIMEOUT_S = 120


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """-> dict(got={blob name: words} or None, log=text, tally=SqrtTally)"""
    tmp = tmp_path_factory.mktemp("index_build")
    exe, cases, results = str(tmp / "device_index.out"), str(tmp / "cases.bin"), str(tmp / "results.bin")
    compile_s = M.build_harness(exe)
    M.write_cases(cases)
    t0 = time.time()
    try:
        r = subprocess.run([exe, cases, results], capture_output=True, text=True, timeout=RUN_TIMEOUT_S)
    except subprocess.TimeoutExpired as e:
        return dict(got=None, log="the harness ran out of time (%d s):\n%s\n%s" % (RUN_TIMEOUT_S, e.stdout, e.stderr))
    log = "compile %.1f s, run %.1f s\n%s%s" % (compile_s, time.time() - t0, r.stdout, r.stderr[-4000:])
    print(log)
    if r.returncode != 0 or not os.path.exists(results):
        return dict(got=None, log="the harness exited %d:\n%s" % (r.returncode, log))
    return dict(got=M.read_results(results, M.out_names()), log=log, tally=M.SqrtTally())


def _got(run, name):
    assert run["got"] is not None, run["log"]
    assert "section %-10s" % name in run["log"], run["log"]
    return run["got"]


def test_struct_sizes(run):
    """the model's word offsets into HvsQuant, HvsBounds and HvsLevels are the device's"""
    assert run["got"] is not None, run["log"]
    assert run["got"]["SIZES"].tolist() == [4 * M.QUANT_WORDS, 4 * M.BOUNDS_WORDS, 4 * M.LEVELS_WORDS]


def test_keys(run):
    """hvs_k_attr_keys: keys_ct, keys_t, ids"""
    diff = M.check_keys(_got(run, "keys"))
    assert diff is None, diff


def test_quant(run):
    """the whole HvsQuant, plain and rotated, non-finite data included"""
    diff = M.check_quant(_got(run, "quant"))
    assert diff is None, diff


def test_tiles(run):
    """every tile word, norms, blockpos and the HvsBounds raised from zero, per builder and ordering"""
    diff = M.check_tiles(_got(run, "tiles"), run["tally"])
    print("sqrt-class values so far: %d compared, %d differ from the model" % (run["tally"].compared, run["tally"].differed))
    assert diff is None, diff


def test_patch(run):
    """tombstones in the first and the partial last block, a block with no dead row, a block all dead; idempotence"""
    diff = M.check_patch(_got(run, "patch"))
    assert diff is None, diff


def test_plan(run):
    diff = M.check_plan(_got(run, "plan"), run["tally"])
    print("sqrt-class values so far: %d compared, %d differ from the model" % (run["tally"].compared, run["tally"].differed))
    assert diff is None, diff


def test_batch(run):
    """class counts, query keys under real and synthetic populations, ranges, and the slot layout from 2, 1 and 3 workgroups"""
    diff = M.check_batch(_got(run, "batch"))
    assert diff is None, diff


def test_prep(run):
    """hvs_k_prep<false> and <true> in five formats, for_filter and count_pairs 0 and 1, over dirty arrays: every field of
    HvsBatch the kernel writes, all of bfrag, the pair counter; theta / thetai from the device's own stored norms and bounds"""
    diff = M.check_prep(_got(run, "prep"), run["tally"])
    print("sqrt-class values so far: %d compared, %d differ from the model" % (run["tally"].compared, run["tally"].differed))
    assert diff is None, diff


def test_cross_check(run):
    """the device's tiles and B fragments, decoded by the model's layout maps, give tests/bound_model.py's S (I8X16) and est
    (BF16, F16)"""
    diff = M.cross_check(_got(run, "prep"))
    assert diff is None, diff
