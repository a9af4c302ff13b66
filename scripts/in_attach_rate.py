#!/usr/bin/env python3
"""Wall time of ATTACHING category sets (include/hvs.h "category sets from device memory"): the same context, the
same sets, once through hvs_set_category_sets (a host CSR: the plan is host arithmetic, then uploaded) and once through
hvs_set_category_sets_device (the CSR already in device memory: the plan kernels).  D = 10^6 gen-v1 rows with 100 categories,
262 144 type-1 user queries, every query with m = 1, 4, 16 distinct categories (its own v and the m - 1 that follow it), and
m = 16 once more with every value four times in the raw set.  Each timed attach starts from a context without sets (the
detach is not timed); best of --reps.  Recorded beside it: expand_ms of each path (for the device path it includes the plan
kernels) and, for reference, the wall time of query_resident + sync of the same set.  Writes the table to
profiles/in_attach_rate.txt.

    python scripts/in_attach_rate.py [--n 1000000] [--nq 262144] [--reps 3] [--engine 0] [--label TEXT] [--out FILE]
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
CASES = ((1, 1), (4, 1), (16, 1), (16, 4))                   # (distinct categories per query, times each value is repeated)


def commit(tree):
    try:
        r = subprocess.run(["git", "-C", tree, "describe", "--always", "--dirty"], capture_output=True, text=True)
        return r.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def best_attach(e, sets, reps):
    """best wall seconds of set_category_sets(sets) on a context without sets"""
    best = None
    for _ in range(reps):
        e.set_category_sets(None)
        t0 = time.perf_counter()
        e.set_category_sets(sets)
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best


def query_wall(e, nq):
    t0 = time.perf_counter()
    e.query_resident(0, nq, 1.0)
    e.sync()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--nq", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engine", type=int, default=0)
    ap.add_argument("--label", default=None, help="what to call the tree in the table (default: its commit)")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "in_attach_rate.txt"))
    a = ap.parse_args()
    sys.path.insert(0, REPO)
    import torch
    PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
    lines = [f"in_attach_rate: {a.label or 'commit ' + commit(REPO)}, n = {a.n}, ncat = {NCAT}, nq = {a.nq} type-1 user queries (gen-v1), k = 100, "
             f"engine setting {a.engine}, wall time of the attach from a context without sets, best of {a.reps}; query ms: query_resident + sync",
             f"{'m':>3} {'x':>2} {'raw values':>10} {'sub-queries':>11} {'host attach ms':>14} {'device attach ms':>16} {'host/device':>11} "
             f"{'host expand ms':>14} {'device expand ms':>16} {'query ms':>9} {'plans equal':>11}"]
    with PKG.Engine(0) as e:
        e.set_engine(a.engine)
        e.set_k(100)
        e.gen_data(a.n, 1, ncat=NCAT)
        e.gen_queries(a.nq, 2, ncat=NCAT, force_type=1)
        v = e.download_queries(0, a.nq)[:, 1].astype(np.int64)
        for m, rep in CASES:
            vals = ((v[:, None] + np.arange(m)[None, :]) % NCAT).astype(np.float32)      # m distinct categories, the query's own first
            vals = np.ascontiguousarray(np.tile(vals, (1, rep)).ravel())                 # ... the whole list `rep` times
            off = (np.arange(a.nq + 1, dtype=np.uint64) * (m * rep)).astype(np.uint32)
            dev = (torch.from_numpy(off.view(np.int32)).to("cuda:0"), torch.from_numpy(vals).to("cuda:0"))
            torch.cuda.synchronize()
            e.set_category_sets((off, vals))                                             # (buffers grow here, outside the timing)
            e.reserve(a.nq)
            query_wall(e, a.nq)
            host = best_attach(e, (off, vals), a.reps)
            qwall = query_wall(e, a.nq)
            st_h = e.in_stats()
            plan_h = e.in_plan_device()
            device = best_attach(e, dev, a.reps)
            query_wall(e, a.nq)
            st_d = e.in_stats()
            plan_d = e.in_plan_device()
            assert st_h.sub_queries == st_d.sub_queries == a.nq * m, (st_h.as_dict(), st_d.as_dict())
            equal = plan_h[0] == plan_d[0] and all(np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(plan_h[1:], plan_d[1:]))
            lines.append(f"{m:>3} {rep:>2} {vals.size:10d} {a.nq * m:11d} {host * 1e3:14.2f} {device * 1e3:16.2f} {host / device:11.1f} "
                         f"{st_h.expand_ms:14.3f} {st_d.expand_ms:16.3f} {qwall * 1e3:9.2f} {str(equal):>11}")
            print(lines[-1], flush=True)
            del dev
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
