#!/usr/bin/env python3
"""Cost and gain of hvs_compact at D = 10^7 (gen-v1 rows, mixed query types).  For the dead sets 1 %, 10 % and 50 % random and
one contiguous block of 10 %: the device time of the row move (hvs_compact_info.move_ms), of its gathers and of its copies back
(HVS_TRACE's line of hvs_compact), the time a plain device-to-device hipMemcpyAsync takes in this process for the bytes the
gathers read (the source rows from the first dead id on) and for the bytes the copies move, the index build (reindex_ms), and
the query rate under the mask before the compaction, after it, and on a fresh load of D[live].  Writes the table, with the
commit it ran at, to profiles/compact_rate.txt.

    python scripts/compact_rate.py [--n 10000000] [--nq 262144] [--reps 3] [--engine 0] [--out profiles/compact_rate.txt]
"""
import argparse
import importlib
import os
import re
import subprocess
import sys
import tempfile

os.environ["HVS_TRACE"] = "1"                                # read when the library is loaded: hvs_compact reports its two phases
import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")
ROW_BYTES = 408


def commit():
    try:
        r = subprocess.run(["git", "-C", REPO, "describe", "--always", "--dirty"], capture_output=True, text=True)
        return r.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def best_rate(e, nq, reps):
    best = None
    for _ in range(reps + 1):                                # the first run warms the workspace up
        e.query_resident(0, nq, 1.0)
        e.sync()
        t = e.last_timing()
        if best is None or t.query_ms < best.query_ms:
            best = t
    return nq / (best.query_ms * 1e-3), best


def memcpy_ms(nbytes, reps=3):
    """best device time of one device-to-device copy of nbytes (torch's copy of a contiguous tensor is a hipMemcpyAsync)"""
    if nbytes == 0:
        return 0.0
    src = torch.empty(nbytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty_like(src)
    best = None
    for _ in range(reps + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        dst.copy_(src)
        b.record()
        b.synchronize()
        best = a.elapsed_time(b) if best is None else min(best, a.elapsed_time(b))
    del src, dst
    torch.cuda.empty_cache()
    return best


def compact_traced(e):
    """e.compact() with the library's stderr line caught: (map, gathers ms, copies ms)"""
    sys.stderr.flush()
    saved = os.dup(2)
    with tempfile.TemporaryFile(mode="w+b") as tmp:
        os.dup2(tmp.fileno(), 2)
        try:
            new_to_old = e.compact()
        finally:
            os.dup2(saved, 2)
            os.close(saved)
        tmp.seek(0)
        text = tmp.read().decode(errors="replace")
    m = re.search(r"hvs_compact .*gathers ([0-9.]+) ms, copies ([0-9.]+) ms", text)
    return new_to_old, (float(m.group(1)) if m else float("nan")), (float(m.group(2)) if m else float("nan"))


def dead_sets(n):
    rng = np.random.default_rng(3)
    return [("1 % random", rng.choice(n, n // 100, replace=False)), ("10 % random", rng.choice(n, n // 10, replace=False)),
            ("50 % random", rng.choice(n, n // 2, replace=False)), ("10 % block", np.arange(n // 3, n // 3 + n // 10))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engine", type=int, default=PKG.ENGINE_AUTO)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "compact_rate.txt"))
    a = ap.parse_args()
    lines = [f"compact_rate: commit {commit()}, n = {a.n}, nq = {a.nq} (gen-v1, mixed types), engine setting {a.engine}, best of {a.reps}, "
             f"HVS_COMPACT_CHUNK = {os.environ.get('HVS_COMPACT_CHUNK', '65536 (default)')}",
             "times in ms; memcpy(read) / memcpy(moved): one device-to-device hipMemcpyAsync of the bytes the gathers read / the copies move",
             f"{'dead set':>12} {'n_live':>9} {'chunks':>6} {'move':>8} {'gathers':>8} {'copies':>8} {'memcpy(read)':>12} {'memcpy(moved)':>13} "
             f"{'gather/memcpy':>13} {'reindex':>8} {'q/s masked':>11} {'q/s after':>11} {'q/s fresh':>11} {'after/fresh':>11}"]
    for name, dead in dead_sets(a.n):
        with PKG.Engine(0) as e:
            e.set_engine(a.engine)
            e.gen_data(a.n, 1)
            e.gen_queries(a.nq, 2)
            e.reserve(a.nq)
            e.delete_rows(dead.astype(np.uint32))
            masked, _ = best_rate(e, a.nq, a.reps)
            _, gather_ms, copy_ms = compact_traced(e)
            s, r = e.compact_stats(), e.append_stats()
            after, t_after = best_rate(e, a.nq, a.reps)
            rows = e.download_data(0, e.n)
            queries = e.download_queries(0, a.nq)
        read_ms = memcpy_ms((s.n_before - s.first_moved) * ROW_BYTES)
        moved_ms = memcpy_ms(s.rows_moved * ROW_BYTES)
        with PKG.Engine(0) as f:
            f.set_engine(a.engine)
            f.load_data(rows)
            f.upload_queries(queries)
            f.reserve(a.nq)
            fresh, t_fresh = best_rate(f, a.nq, a.reps)
        assert t_after.pairs == t_fresh.pairs and t_after.engine == t_fresh.engine
        lines.append(f"{name:>12} {s.n_after:9d} {s.chunks:6d} {s.move_ms:8.2f} {gather_ms:8.2f} {copy_ms:8.2f} {read_ms:12.2f} {moved_ms:13.2f} "
                     f"{gather_ms / read_ms:13.2f} {r.reindex_ms:8.1f} {masked:11.0f} {after:11.0f} {fresh:11.0f} {after / fresh:11.3f}")
        print(lines[-1], flush=True)
        del rows, queries
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
