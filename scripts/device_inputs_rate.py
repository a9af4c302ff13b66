#!/usr/bin/env python3
"""Device-resident inputs against the host paths they replace: host wall times through Engine at D = 10^7 (gen-v1) with
262144 mixed queries, best of 3, for
  queries   upload_queries (pageable numpy) + query_resident + sync + download_results
            against set_queries_device + query_resident + export_results_device + a stream wait (torch tensors in and out),
  load      load_data (pageable numpy) against load_data_device,
  from-rows download_data + a numpy rebuild of [type, v, l, r, x] rows + upload_queries against set_queries_from_rows.
Writes the table, with the commit it ran at, to profiles/device_inputs_rate.txt.  No threshold: the figures are recorded
against the host path of the same build.

    python scripts/device_inputs_rate.py [--n 10000000] [--nq 262144] [--reps 3] [--engine 0] [--out profiles/device_inputs_rate.txt]
"""
import argparse
import importlib
import os
import subprocess
import sys
import time

import numpy as np
import torch  # before the library: one HIP runtime per process

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
PKG = importlib.import_module("project---hybrid-vector-search-queries_amd")


def commit():
    try:
        r = subprocess.run(["git", "-C", REPO, "describe", "--always", "--dirty"], capture_output=True, text=True)
        return r.stdout.strip() or "unknown"
    except OSError:
        return "unknown"


def best_ms(fn, reps):
    best = None
    for _ in range(reps + 1):                                # the first run warms buffers and staging slots up
        t0 = time.perf_counter()
        fn()
        ms = (time.perf_counter() - t0) * 1e3
        best = ms if best is None else min(best, ms)
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=10_000_000)
    ap.add_argument("--nq", type=int, default=262_144)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--engine", type=int, default=PKG.ENGINE_AUTO)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "device_inputs_rate.txt"))
    a = ap.parse_args()
    n, nq = a.n, a.nq
    lines = [f"device_inputs_rate: commit {commit()}, n = {n}, nq = {nq} (gen-v1, mixed types), engine setting {a.engine}, host wall time, best of {a.reps}",
             f"{'':<10} {'host path ms':>13} {'device path ms':>15} {'ratio':>7}"]

    def row(name, host_ms, dev_ms, note):
        lines.append(f"{name:<10} {host_ms:13.2f} {dev_ms:15.2f} {host_ms / dev_ms:6.1f}x   {note}")
        print(lines[-1], flush=True)

    torch.cuda.init()
    stream = torch.cuda.current_stream().cuda_stream
    with PKG.Engine(0) as e:
        e.set_engine(a.engine)
        e.gen_data(n, 1)
        e.gen_queries(nq, 2)
        e.reserve(nq)
        k = e.k
        q_host = e.download_queries(0, nq)
        q_dev = torch.from_numpy(q_host).cuda()
        out_ids = torch.empty((nq, k), dtype=torch.int32, device="cuda")
        out_d = torch.empty((nq, k), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        got = {}

        # -- queries
        def host_queries():
            e.upload_queries(q_host)
            e.query_resident(0, nq, 1.0)
            e.sync()
            got["host"] = e.download_results(0, nq)

        def device_queries():
            e.set_queries_device(q_dev)
            e.query_resident(0, nq, 1.0)
            e.export_results_device(0, nq, out_ids.data_ptr(), out_d.data_ptr())
            e.stream_wait(stream)
            torch.cuda.current_stream().synchronize()

        h, d = best_ms(host_queries, a.reps), best_ms(device_queries, a.reps)
        assert np.array_equal(out_ids.cpu().numpy().view(np.uint32), got["host"][0]), "the two paths disagree"
        assert np.array_equal(out_d.cpu().numpy().view(np.uint32), got["host"][1].view(np.uint32)), "the two paths disagree"
        row("queries", h, d, f"{nq} queries in, ids and distances out ({nq * (PKG.engine.QCOLS + 2 * k) * 4 / 1e6:.0f} MB over PCIe on the host path)")

        # -- from rows
        ids = np.random.default_rng(3).integers(0, n, nq).astype(np.uint32)
        typ, dt = 3, np.float32(0.05)

        def host_from_rows():
            rows = e.download_data(0, n)[ids]
            q = np.empty((nq, PKG.engine.QCOLS), np.float32)
            q[:, 0], q[:, 1], q[:, 2], q[:, 3] = typ, rows[:, 0], rows[:, 1] - dt, rows[:, 1] + dt
            q[:, 4:] = rows[:, 2:]
            e.upload_queries(q)
            got["q"] = q

        def device_from_rows():
            e.set_queries_from_rows(ids, type=typ, dt=float(dt))

        h, d = best_ms(host_from_rows, a.reps), best_ms(device_from_rows, a.reps)
        assert np.array_equal(e.download_queries(0, nq).view(np.uint32), got["q"].view(np.uint32)), "the two paths disagree"
        row("from-rows", h, d, f"{nq} random ids, type 3, dt 0.05 (the host path downloads all {n} rows to pick from)")

        # -- load
        d_host = e.download_data(0, n)
        d_dev = torch.from_numpy(d_host).cuda()
        torch.cuda.synchronize()
        h = best_ms(lambda: e.load_data(d_host), a.reps)
        d = best_ms(lambda: e.load_data_device(d_dev), a.reps)
        assert np.array_equal(e.download_data(n - 1000, 1000).view(np.uint32), d_host[n - 1000:].view(np.uint32))
        row("load", h, d, f"{n} rows, {n * PKG.engine.DCOLS * 4 / 1e9:.2f} GB, index build and planner probe included in both")
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
