"""The wave-level device primitives of csrc/hvs_device.h and csrc/hvs_kernels.h, each run on its own on the GPU
(tests/device_primitives.hip) and compared word for word with the host models of tests/primitives_model.py: both forms of
hvs_wave_select_prune, the merge tail (make_room, final_cut, pad, rank_write), the keep functions with their counters, the
admission tests, hvs_gather_list_keys, hvs_wave_dedup_ids, the four distance forms, and the query parse and predicate.

The harness is built once per session and run once, in one process; a run that ends non-zero or runs out of time fails every
section's test with its output attached, and nothing is run again.

Measured on an MI355X host: the harness compiles in 1.9 s (4.4 s on a slower build machine) and runs in 0.3 s of wall time,
0.24 s of it inside the program and 0.17 s of that the first launch with the runtime's start; every later section takes
0.3 to 1.5 ms.  The whole module takes 3 s.  RUN_TIMEOUT_S leaves a wide margin: the tested code is a handful of trivial
launches, so the margin hides nothing.
"""
import os
import subprocess
import time

import numpy as np
import pytest

import primitives_model as M

pytestmark = pytest.mark.gpu

RUN_TIMEOUT_S = 120


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """-> dict(got={blob name: words} or None, log=text)"""
    tmp = tmp_path_factory.mktemp("primitives")
    exe, cases, results = str(tmp / "device_primitives.out"), str(tmp / "cases.bin"), str(tmp / "results.bin")
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
    return dict(got=M.read_blobs(results, M.OUT_BLOBS), log=log)


def _check(run, name):
    assert run["got"] is not None, run["log"]
    assert "section %-10s" % name in run["log"], run["log"]
    diff = M.compare(M.sections()[name], run["got"])
    assert diff is None, diff


def test_select(run):
    """hvs_wave_select_prune<4|8>: histogram form with and without compaction, bit-serial form in LDS and in global memory"""
    _check(run, "select")


def test_make_room_and_final_cut(run):
    _check(run, "cut")


def test_pad_and_rank_write(run):
    _check(run, "pad_rank")


def test_keep_functions_and_admission_tests(run):
    """hvs_keep_within / _after / _unlisted with every counter slot, hvs_excluded and hvs_in_row_set on their own"""
    _check(run, "keep")


def test_gather_list_keys(run):
    _check(run, "gather")


def test_dedup_ids(run):
    _check(run, "dedup")


def test_distance_forms(run):
    """the plain, packed, LDS-pipelined and sequential forms on the same pairs, as key bits"""
    _check(run, "dist")
    got, lab = run["got"], M.sections()["dist"].labels["DIST_PLAIN"]
    for other in ("DIST_PK", "DIST_LDS"):
        bad = np.nonzero(got["DIST_PLAIN"] != got[other])[0]
        assert bad.size == 0, "dist: %s differs from the plain form at %s" % (other, lab[int(bad[0])])


def test_parse_predicate_and_ordered_u32(run):
    _check(run, "predicate")
    o = run["got"]["ORD"].astype(np.int64)
    assert np.all(np.diff(o) > 0), "hvs_ordered_u32 is not strictly monotone over the table (-0 in front of +0)"
