#!/usr/bin/env python3
"""The FP16 bound of scanned row sets: every row once with hvs_set_row_set_scan_filter at 0 and once at 1,
the modes ALTERNATING inside one session, on the data of scripts/row_set_scan_rate.py (D rows generated on the device, mixed
queries, one set drawn by a hash of the row id, the scan limit above its population).

    python scripts/row_set_scan_filter_rate.py [--rows 10000000] [--queries 262144] [--reps 3] [--out FILE]

Per row and mode: the query ms of every run (after one warm-up per mode) and their median, the device time of the kernels, and for
mode 1 rescored_pairs / passing_pairs: the share of the passing pairs whose exact distance was still evaluated."""
import argparse
import importlib
import os
import statistics
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
from row_set_scan_rate import hashed  # noqa: E402  (scripts/ is sys.path[0] when this file is run)


def once(e, nq, mode):
    e.set_row_set_scan_filter(mode)
    e.query_resident(0, nq, 1.0)
    e.sync()
    return e.last_timing()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default="profiles/row_set_scan_filter_rate.txt")
    args = ap.parse_args()
    n, nq, k = args.rows, args.queries, 100
    with open(args.out, "w") as out, PKG.Engine(0) as e:
        e.gen_data(n, 1)
        e.gen_queries(nq, 2)
        h = hashed(n, 0)
        line = f"D = {n} rows, {nq} mixed queries, k = {k}; modes alternate, {args.reps} runs each after a warm-up each"
        print(line, flush=True)
        out.write(line + "\n")
        for f in (0.001, 0.01, 0.1, 0.2, 0.3):
            sets = (h < f)[None, :]
            e.set_row_sets(sets)
            e.set_query_row_sets(np.zeros(nq, np.uint32))
            e.set_row_set_scan_limit(int(sets.sum()))
            ms, last = {0: [], 1: []}, {}
            for rep in range(args.reps + 1):
                for mode in (0, 1):
                    t = once(e, nq, mode)
                    assert e.row_set_scan_stats().scanned_queries == nq
                    if rep:
                        ms[mode].append(t.query_ms)
                    last[mode] = t
            for mode in (0, 1):
                t = last[mode]
                line = (f"f = {f:<6} mode {mode}  query ms {' '.join(f'{x:9.2f}' for x in ms[mode])}  median {statistics.median(ms[mode]):9.2f}"
                        f"  kernels {t.main_kernel_ms:9.2f} ms  passing {t.pairs}  bounded {t.scanned_pairs if mode else 0}  rescored {t.rescored_pairs}"
                        f"  rescored/passing {t.rescored_pairs / max(t.pairs, 1):.4f}")
                print(line, flush=True)
                out.write(line + "\n")
                out.flush()
            line = f"f = {f:<6} mode 1 / mode 0 = {statistics.median(ms[1]) / statistics.median(ms[0]):.3f}"
            print(line, flush=True)
            out.write(line + "\n")
        e.set_row_set_scan_filter(0)


if __name__ == "__main__":
    main()
