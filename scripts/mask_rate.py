#!/usr/bin/env python3
"""Query rate under a live-row mask: queries/s through Engine at D = 10^7 (gen-v1, mixed query types) with 0 %, 10 %, 50 %
and 90 % of the rows deleted at random, next to what the mask costs elsewhere: exact-engine fallbacks, retried queries,
re-scored pairs and the dead survivors the re-scoring front end had to drop (hvs_mask_info).  Writes the table, with the
commit it ran at, to profiles/mask_rate.txt.

    python scripts/mask_rate.py [--n 10000000] [--nq 262144] [--reps 3] [--engine 0] [--out profiles/mask_rate.txt]
"""
import argparse
import importlib
import os
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")


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
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "mask_rate.txt"))
    a = ap.parse_args()
    lines = [f"mask_rate: commit {commit()}, n = {a.n}, nq = {a.nq} (gen-v1, mixed types), engine setting {a.engine}, best of {a.reps}",
             f"{'deleted':>8} {'n_live':>9} {'mask ms':>8} {'queries/s':>11} {'ran':>4} {'fallback':>9} {'retry':>6} {'rescored':>11} "
             f"{'dead_surv':>10} {'patched':>9}"]
    rng = np.random.default_rng(1)
    with PKG.Engine(0) as e:
        e.set_engine(a.engine)
        e.gen_data(a.n, 1)
        e.gen_queries(a.nq, 2)
        e.reserve(a.nq)
        order = rng.permutation(a.n).astype(np.uint32)
        for frac in (0.0, 0.1, 0.5, 0.9):
            dead = order[:int(frac * a.n)]
            t0 = time.perf_counter()
            e.set_row_mask(None)
            if dead.size:
                e.delete_rows(dead)
            mask_ms = (time.perf_counter() - t0) * 1e3
            best = None
            for _ in range(a.reps + 1):                      # the first run warms the workspace up
                e.query_resident(0, a.nq, 1.0)
                e.sync()
                t = e.last_timing()
                if best is None or t.query_ms < best.query_ms:
                    best = t
            m = e.mask_stats()
            lines.append(f"{100 * frac:7.0f}% {m.n_live:9d} {mask_ms:8.1f} {a.nq / (best.query_ms * 1e-3):11.0f} {best.engine:4d} "
                         f"{best.fallback_queries:9d} {best.retry_queries:6d} {best.rescored_pairs:11d} {m.dead_survivors:10d} "
                         f"{m.tiles_patched:9d}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
