#!/usr/bin/env python3
"""Query rate under per-query distance caps (include/hvs.h "per-query distance caps"): queries/s through Engine at
D = 10^7 (gen-v1, mixed query types) without caps, with caps at each query's k-th distance (the same answers), at its 10th
distance and just below its nearest distance (nothing within), next to what the caps change elsewhere: re-scored pairs, retried
queries, exact-engine fallbacks and the figures of hvs_within_stats.  The caps are taken from the queries' own uncapped answers.
Writes the table, with the commit it ran at, to profiles/within_rate.txt.

    python scripts/within_rate.py [--n 10000000] [--nq 262144] [--reps 3] [--engine 0] [--out profiles/within_rate.txt]
"""
import argparse
import importlib
import os
import subprocess
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
EMPTY = 0xFFFFFFFF


def commit():
    try:
        r = subprocess.run(["git", "-C", REPO, "describe", "--always", "--dirty"], capture_output=True, text=True)
        return r.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engine", type=int, default=PKG.ENGINE_AUTO)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "within_rate.txt"))
    a = ap.parse_args()
    lines = [f"within_rate: commit {commit()}, n = {a.n}, nq = {a.nq} (gen-v1, mixed types), engine setting {a.engine}, best of {a.reps}",
             f"{'caps':>16} {'queries/s':>11} {'query ms':>9} {'ran':>4} {'rescored':>11} {'retry':>6} {'fallback':>9} {'underfull':>10} "
             f"{'within_slots':>13}"]
    with PKG.Engine(0) as e:
        e.set_engine(a.engine)
        e.gen_data(a.n, 1)
        e.gen_queries(a.nq, 2)
        e.reserve(a.nq)
        k = e.k
        # the queries' own uncapped, unpadded answers: where the caps come from
        e.set_padding(False)
        e.query_resident(0, a.nq, 1.0)
        e.sync()
        ids, d = e.download_results(0, a.nq)
        e.set_padding(True)
        have = (ids != EMPTY) & np.isfinite(d)
        m = have.sum(1)
        rows = np.arange(a.nq)

        def at(j):  # the j-th matched distance, or the last one a query has, or 1.0 for a query without any
            return np.where(m > 0, d[rows, np.clip(np.minimum(j, m - 1), 0, k - 1)], np.float32(1.0)).astype(np.float32)

        settings = (("none", None), ("k-th distance", at(k - 1)), ("10th distance", at(9)),
                    ("below nearest", np.nextafter(at(0), np.float32(-np.inf), dtype=np.float32)))
        for name, caps in settings:
            e.set_max_dist2(caps)
            best = None
            for _ in range(a.reps + 1):                      # the first run warms the workspace up
                e.query_resident(0, a.nq, 1.0)
                e.sync()
                t = e.last_timing()
                if best is None or t.query_ms < best.query_ms:
                    best = t
            w = e.within_stats()
            if name == "k-th distance":                      # the same answers as without caps (padding on both times)
                got = e.download_results(0, a.nq, want_dists=False)
                e.set_max_dist2(None)
                e.query_resident(0, a.nq, 1.0)
                e.sync()
                assert np.array_equal(got, e.download_results(0, a.nq, want_dists=False)), "caps at the k-th distance changed the answers"
            lines.append(f"{name:>16} {a.nq / (best.query_ms * 1e-3):11.0f} {best.query_ms:9.2f} {best.engine:4d} {best.rescored_pairs:11d} "
                         f"{best.retry_queries:6d} {best.fallback_queries:9d} {w.underfull_queries:10d} {w.within_slots:13d}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
