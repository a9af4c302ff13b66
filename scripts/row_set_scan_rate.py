#!/usr/bin/env python3
"""Scanned row sets: the rows of 6.1f once with the scan limit at 0 (the path of DESIGN 3.18) and once with
it above the set's population.  D rows generated on the device, mixed queries, sets drawn by a hash of the row id.

    python scripts/row_set_scan_rate.py [--rows 10000000] [--queries 262144] [--reps 3] [--slow-reps 1] [--out FILE]

Per case: query ms (best of --reps after a warm-up; a run whose warm-up took more than a second gets --slow-reps),
the device time of the two scan kernels, the time of the first call after the limit changed less a warm call (member lists and
query grouping), scanned_pairs, and the rate of the gather: member rows the items read x 408 bytes over the kernels' time.
Dense cases run first: the sparse limit-0 runs change the tile format for later calls."""
import argparse
import importlib
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")


def hashed(n, salt):
    x = (np.arange(n, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(29)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    return ((x >> np.uint64(40)).astype(np.float64)) / float(1 << 24)


def timed(e, nq, reps):
    best, t = None, None
    for _ in range(reps):
        e.query_resident(0, nq, 1.0)
        e.sync()
        t = e.last_timing()
        best = t.query_ms if best is None else min(best, t.query_ms)
    return best, t


def case(e, name, sets, idx, nq, k, args, out):
    e.set_row_sets(sets)
    e.set_query_row_sets(idx)
    pop = int(sets.sum(1).max())
    rows = []
    for limit in (0, pop):
        e.set_row_set_scan_limit(limit)
        t0 = time.perf_counter()
        e.query_resident(0, nq, 1.0)                                          # warm-up; with the limit on it builds lists and groups
        e.sync()
        first_ms = (time.perf_counter() - t0) * 1e3
        ms, t = timed(e, nq, args.slow_reps if first_ms > 1000.0 else args.reps)   # (runs of seconds each are timed --slow-reps times)
        st = e.row_set_scan_stats()
        line = f"{name:<28} limit {limit:>9}  query {ms:10.2f} ms  kernels {t.main_kernel_ms:10.2f} ms  retry {t.retry_queries:>7} exact {t.fallback_queries:>7}"
        if limit:
            items, _ = PKG.row_set_scan_plan(np.bincount(idx, minlength=len(sets)), sets.sum(1), k, 0, 512)
            gathered = int((items[:, 4].astype(np.int64) - items[:, 3]).sum()) * 408
            line += (f"  first call {first_ms - ms:8.2f} ms over a warm one  items {st.items} chunks {st.member_chunks} scanned_pairs {st.scanned_pairs}"
                     f"  gather {gathered / (t.main_kernel_ms * 1e-3) / 1e9:7.1f} GB/s  {nq / (ms * 1e-3) / 1e6:6.3f} M queries/s")
            assert st.scanned_queries == nq, st.as_dict()
        rows.append(ms)
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--queries", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--slow-reps", type=int, default=1)
    ap.add_argument("--out", default="profiles/row_set_scan_rate.txt")
    args = ap.parse_args()
    n, nq, k = args.rows, args.queries, 100
    with open(args.out, "w") as out, PKG.Engine(0) as e:
        e.gen_data(n, 1)
        e.gen_queries(nq, 2)
        e.query_resident(0, nq, 1.0)
        e.sync()
        base, _ = timed(e, nq, args.reps)
        line = f"D = {n} rows, {nq} mixed queries, k = {k}; baseline without sets {base:.2f} ms"
        print(line, flush=True)
        out.write(line + "\n")
        h = hashed(n, 0)
        one = np.zeros(nq, np.uint32)
        for f in (0.5, 0.4, 0.3, 0.2, 0.1, 0.01, 0.001):                       # (0.4 .. 0.2: where the two paths cross)
            case(e, f"one set, f = {f}", (h < f)[None, :], one, nq, k, args, out)
        many = np.stack([hashed(n, 1000 + s) < 0.01 for s in range(64)])
        case(e, "64 sets, f = 0.01", many, (np.arange(nq) % 64).astype(np.uint32), nq, k, args, out)
        # the skewed call: 64 queries on a set of 10 % of the rows, with and without chunking (one chunk: HVS_SET_SCAN_CHUNK = all rows)
        e.gen_queries(64, 3)
        big = (h < 0.1)[None, :]
        for chunk in ("", str(n)):
            os.environ["HVS_SET_SCAN_CHUNK"] = chunk
            if not chunk:
                os.environ.pop("HVS_SET_SCAN_CHUNK")
            case(e, f"64 queries, f = 0.1, {'one chunk' if chunk else 'chunked'}", big, np.zeros(64, np.uint32), 64, k, args, out)
        os.environ.pop("HVS_SET_SCAN_CHUNK", None)


if __name__ == "__main__":
    main()
