#!/usr/bin/env python3
"""Query rate with appended rows behind the index: queries/s through Engine at D = 10^7 (gen-v1, mixed query types) with a
tail of 0, limit / 4, limit and 4 x limit rows (limit = the default tail limit, max(4096, n_indexed / 1024)), next to the
tail scan's own counters (hvs_append_info), the cost of one append of 10^3 rows and of the re-index.  Writes the table, with
the commit it ran at, to profiles/append_rate.txt.  The tail = 0 line is what the same command gives on a build without
hvs_append_rows (`--baseline`: only that line, through the API both builds have).

    python scripts/append_rate.py [--n 10000000] [--nq 262144] [--reps 3] [--engine 0] [--baseline] [--limit ROWS] [--out profiles/append_rate.txt]
"""
import argparse
import importlib
import os
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")


def commit():
    try:
        r = subprocess.run(["git", "-C", REPO, "describe", "--always", "--dirty"], capture_output=True, text=True)
        return r.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def best_of(e, nq, reps):
    best = None
    for _ in range(reps + 1):                                # the first run warms the workspace up
        e.query_resident(0, nq, 1.0)
        e.sync()
        t = e.last_timing()
        if best is None or t.query_ms < best.query_ms:
            best = t
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engine", type=int, default=PKG.ENGINE_AUTO)
    ap.add_argument("--baseline", action="store_true", help="tail = 0 only, without the append API")
    ap.add_argument("--limit", type=int, default=0, help="measure around this limit instead of the default one")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "append_rate.txt"))
    a = ap.parse_args()
    lines = [f"append_rate: commit {commit()}, n = {a.n}, nq = {a.nq} (gen-v1, mixed types), engine setting {a.engine}, best of {a.reps}",
             f"{'tail':>8} {'n_indexed':>10} {'queries/s':>11} {'vs tail 0':>9} {'ran':>4} {'fallback':>9} {'retry':>6} {'tail_pairs':>13} "
             f"{'admitted':>10}"]
    with PKG.Engine(0) as e:
        e.set_engine(a.engine)
        e.gen_data(a.n, 1)
        e.gen_queries(a.nq, 2)
        e.reserve(a.nq)
        if a.baseline:
            t = best_of(e, a.nq, a.reps)
            lines.append(f"{0:8d} {a.n:10d} {a.nq / (t.query_ms * 1e-3):11.0f} {'':>9} {t.engine:4d} {t.fallback_queries:9d} {t.retry_queries:6d}")
        else:
            limit = a.limit or e.append_stats().tail_limit
            more = e.download_data(0, 4 * limit)            # rows to append: copies of the first ones (ids differ, nothing else)
            e.set_tail_limit(1 << 31)                        # the tails below are measured, not folded in
            e.reserve_rows(a.n + 4 * limit + 1000)
            rate0, have = None, 0
            for tail in (0, limit // 4, limit, 4 * limit):
                if tail > have:
                    e.append_rows(more[have:tail])
                    have = tail
                t, s = best_of(e, a.nq, a.reps), e.append_stats()
                assert s.n_tail == tail
                rate = a.nq / (t.query_ms * 1e-3)
                rate0 = rate0 or rate
                lines.append(f"{tail:8d} {s.n_indexed:10d} {rate:11.0f} {100 * (rate / rate0 - 1):+8.1f}% {t.engine:4d} {t.fallback_queries:9d} "
                             f"{t.retry_queries:6d} {s.tail_pairs:13d} {s.tail_admitted:10d}")
                print(lines[-1], flush=True)
            t0 = time.perf_counter()
            e.append_rows(more[:1000])
            append_ms = (time.perf_counter() - t0) * 1e3
            t0 = time.perf_counter()
            e.reindex()
            wall_ms = (time.perf_counter() - t0) * 1e3
            s = e.append_stats()
            lines.append(f"tail limit {limit} rows{'' if a.limit else ' (the default)'}; one append of 1000 rows (room reserved): {append_ms:.2f} ms; re-index over "
                         f"{s.n_indexed} rows: {s.reindex_ms:.1f} ms on the device, {wall_ms:.1f} ms wall")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
