#!/usr/bin/env python3
"""Query rate under category sets (include/hvs.h "category sets"): D = 10^7 gen-v1 rows with 100 categories, 262 144
type-1 user queries, every query with a set of m = 1, 2, 4, 8, 16 distinct categories (its own v and the m - 1 that follow it).
Measured: host wall time of query_resident + sync, best of --reps after one warm-up call.  The yardstick is the SAME build answering
the same m x 262 144 plain type-1 queries with padding off -- the expanded set, built by hand on the host -- which no set
function touches.  Recorded: user queries/s, sub-queries/s, the plain rate, expand_ms, merge_ms and the merge's share of the
call.  Writes the table to profiles/in_rate.txt.

    python scripts/in_rate.py [--n 10000000] [--nq 262144] [--m 1,2,4,8,16] [--reps 3] [--engine 0] [--label TEXT] [--out FILE]
"""
import argparse
import importlib
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NCAT = 100


def commit(tree):
    try:
        r = subprocess.run(["git", "-C", tree, "describe", "--always", "--dirty"], capture_output=True, text=True)
        return r.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def best_wall(e, nq, reps):
    """(best wall seconds, its timing) of query_resident + sync over `reps` calls after one warm-up"""
    best, best_t = None, None
    for i in range(reps + 1):
        t0 = time.perf_counter()
        e.query_resident(0, nq, 1.0)
        e.sync()
        dt = time.perf_counter() - t0
        if i and (best is None or dt < best):
            best, best_t = dt, e.last_timing()
    return best, best_t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", type=int, default=262_144)
    ap.add_argument("--m", default="1,2,4,8,16")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engine", type=int, default=0)
    ap.add_argument("--label", default=None, help="what to call the tree in the table (default: its commit)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "in_rate.txt"))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
    ms = [int(x) for x in a.m.split(",")]
    lines = [f"in_rate: {a.label or 'commit ' + commit(REPO)}, n = {a.n}, ncat = {NCAT}, nq = {a.nq} type-1 user queries (gen-v1), k = 100, "
             f"engine setting {a.engine}, wall time of query_resident + sync, best of {a.reps}",
             f"{'m':>3} {'sub-queries':>11} {'sets ms':>9} {'user q/s':>10} {'sub q/s':>10} {'plain ms':>9} {'plain q/s':>10} {'sets/plain':>10} "
             f"{'expand ms':>9} {'merge ms':>9} {'merge share':>11} {'underfull':>9} {'pairs equal':>11}"]
    with PKG.Engine(0) as e:
        e.set_engine(a.engine)
        e.set_k(100)
        e.gen_data(a.n, 1, ncat=NCAT)
        e.gen_queries(a.nq, 2, ncat=NCAT, force_type=1)
        users = e.download_queries(0, a.nq)
        v = users[:, 1].astype(np.int64)
        for m in ms:
            vals = ((v[:, None] + np.arange(m)[None, :]) % NCAT).astype(np.float32)      # m distinct categories, the query's own first
            off = (np.arange(a.nq + 1, dtype=np.uint64) * m).astype(np.uint32)
            # under sets (padding on: the merge pads once)
            e.set_padding(True)
            e.upload_queries(users)
            e.set_category_sets((off, np.ascontiguousarray(vals.ravel())))
            e.reserve(a.nq)
            wall, t = best_wall(e, a.nq, a.reps)
            st = e.in_stats()
            assert st.sub_queries == a.nq * m, st.as_dict()
            # the expanded set by hand, padding off
            plain = np.repeat(users, m, axis=0)
            plain[:, 1] = np.sort(vals, axis=1).ravel()                                   # (hvs_in_plan's order: ascending)
            e.set_padding(False)
            e.upload_queries(plain)
            e.reserve(a.nq * m)
            pwall, pt = best_wall(e, a.nq * m, a.reps)
            del plain
            lines.append(f"{m:>3} {a.nq * m:11d} {wall * 1e3:9.2f} {a.nq / wall:10.0f} {a.nq * m / wall:10.0f} {pwall * 1e3:9.2f} "
                         f"{a.nq * m / pwall:10.0f} {(a.nq * m / wall) / (a.nq * m / pwall):10.3f} {st.expand_ms:9.3f} {st.merge_ms:9.3f} "
                         f"{st.merge_ms / (wall * 1e3):11.3f} {st.underfull_queries:9d} {str(int(t.pairs) == int(pt.pairs)):>11}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
