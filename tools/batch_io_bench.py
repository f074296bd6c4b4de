#!/usr/bin/env python3
"""Batched sets as files, file to file: many fragment CSVs in, one output CSV
per set out (DESIGN.md "Batched sets as files").

~50M rows at cfg3's density written as 16384, 1024 and 64 CSV files (a set's
genome length is 3 Gbp x rows / 50M; every set has its own seed) in a scratch
directory, page cache warm.  Three routes alternate in this process, each run
from the files to the files:

  a  host       what `rk_repkiller --batch` does, driven through the library:
                rk_db_load_csv on 16 threads, the columns copied into one host
                SoA, rk_classify_batch, a serial loop of rk_db_write_csv
  b  device     rk_dbset_load_csv_device, rk_classify_dbset, the host save per
                set (rk_dbset_write_csv)
  c  device_save  rk_dbset_load_csv_device with all nine columns resident,
                rk_classify_dbset_to_csv

Route a's code is what every earlier build has, so the yardstick is timed on
this same build in the same job.  Every output of every run is hashed and
compared with route a's.  Every figure is a median over the runs with its
spread (min, max).

  python tools/batch_io_bench.py [--total 50000000] [--splits 16384,1024,64]
                                 [--runs 3] [--tmp DIR]
                                 [--out profiles/batch_csv_device.json]

Results of the splits given are merged into --out (other splits already there
are kept), so the shapes can be measured in separate jobs.
"""
from __future__ import annotations

import argparse
import ctypes
import hashlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402,F401  (one shared HIP runtime)

import repkiller_amd as rk  # noqa: E402

CFG3_ROWS, CFG3_GENOME = 50_000_000, 3_000_000_000
THREADS = 16


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 22), b""):
            h.update(blk)
    return h.digest()


def hash_all(pool, paths):
    """One digest over the digests of all files, in order, and their total size."""
    h = hashlib.sha256()
    for d in pool.map(sha256_file, paths):
        h.update(d)
    return h.hexdigest(), sum(os.path.getsize(p) for p in paths)


def write_inputs(pool, d, total, nsets):
    rows = total // nsets
    genome = max(1000, CFG3_GENOME * rows // CFG3_ROWS)

    def one(k):
        p = os.path.join(d, f"in{k:05d}.csv")
        rk.write_input_csv(p, rk.synth(rows, genome, seed=1000 + k), genome, genome)
        return p

    return list(pool.map(one, range(nsets))), rows, genome


def route_host(ctx, pool, ins, outs):
    lib = rk.load_library()
    t0 = time.perf_counter()

    def load(p):
        h = ctypes.c_void_p()
        rk._check(lib.rk_db_load_csv(p.encode(), ctypes.byref(h)))
        return h

    dbs = list(pool.map(load, ins))
    t1 = time.perf_counter()
    ns = len(dbs)
    views = [rk.FragsSoA() for _ in dbs]
    lx, ly = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    off = np.zeros(ns + 1, np.uint64)
    a, b, c = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_uint64()
    for k, h in enumerate(dbs):
        lib.rk_db_view(h, ctypes.byref(views[k]), ctypes.byref(a), ctypes.byref(b),
                       ctypes.byref(c))
        lx[k], ly[k] = a.value, b.value
        off[k + 1] = off[k] + np.uint64(views[k].n)
    n = int(off[-1])
    x, y, ln = np.empty(n, np.uint64), np.empty(n, np.uint64), np.empty(n, np.uint64)
    st = np.empty(n, np.uint8)
    for k, v in enumerate(views):
        o, m = int(off[k]), int(v.n)
        if m:
            ctypes.memmove(x.ctypes.data + 8 * o, v.x_start, 8 * m)
            ctypes.memmove(y.ctypes.data + 8 * o, v.y_start, 8 * m)
            ctypes.memmove(ln.ctypes.data + 8 * o, v.length, 8 * m)
            ctypes.memmove(st.ctypes.data + o, v.strand, m)
    gid, order = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
    rep = np.zeros(n, np.uint8)
    n_out, n_groups = np.zeros(ns, np.uint64), np.zeros(ns, np.uint64)
    soa = rk.FragsSoA(x.ctypes.data, y.ctypes.data, ln.ctypes.data, st.ctypes.data, n)
    prm = rk.BatchParams(ns, off.ctypes.data, lx.ctypes.data, ly.ctypes.data, 0.3, 0.3)
    res = rk.BatchResult(order.ctypes.data, gid.ctypes.data, rep.ctypes.data,
                         n_out.ctypes.data, n_groups.ctypes.data)
    rc = lib.rk_classify_batch(ctx._h, ctypes.byref(soa), ctypes.byref(prm), ctypes.byref(res))
    if rc:
        raise rk.RkError(rc, ctx.last_error())
    t2 = time.perf_counter()
    for k, h in enumerate(dbs):
        o = int(off[k])
        r = rk.Result(order.ctypes.data + 4 * o, gid.ctypes.data + 4 * o, rep.ctypes.data + o,
                      int(n_out[k]), int(n_groups[k]))
        rk._check(lib.rk_db_write_csv(h, outs[k].encode(), ctypes.byref(r)))
    t3 = time.perf_counter()
    for h in dbs:
        lib.rk_db_free(h)
    return {"load_s": t1 - t0, "classify_s": t2 - t1, "save_s": t3 - t2, "total_s": t3 - t0,
            "batch": ctx.batch_stats()}


def route_device(ctx, ins, outs, save):
    t0 = time.perf_counter()
    dbs = rk.FragmentsDatabaseSet(ins, ctx, keep_device=True, keep_rows=save)
    t1 = time.perf_counter()
    leg = {"load_s": t1 - t0, "ingress": ctx.ingress_stats()}
    if save:
        ctx.classify_dbset_to_csv(dbs, outs, 0.3, 0.3)
        t3 = time.perf_counter()
        leg.update(classify_save_s=t3 - t1, egress=ctx.egress_stats())
    else:
        res = ctx.classify_dbset(dbs, 0.3, 0.3)
        t2 = time.perf_counter()
        for k, r in enumerate(res):
            dbs.save_set(k, outs[k], r)
        t3 = time.perf_counter()
        leg.update(classify_s=t2 - t1, save_s=t3 - t2)
    leg.update(total_s=t3 - t0, batch=ctx.batch_stats())
    dbs.close()
    return leg


def summary(legs):
    """{field: {median, min, max}} over the runs, nested dicts alike."""
    out = {}
    for key, v in legs[0].items():
        vals = [leg[key] for leg in legs]
        if isinstance(v, dict):
            out[key] = summary(vals)
        elif isinstance(v, float):
            out[key] = {"median": round(statistics.median(vals), 4),
                        "min": round(min(vals), 4), "max": round(max(vals), 4)}
        else:
            out[key] = vals[0] if len(set(vals)) == 1 else vals
    return out


def bench_split(ctx, pool, tmp, total, nsets, runs):
    d = tempfile.mkdtemp(prefix=f"rk_bio_{nsets}_", dir=tmp)
    try:
        t0 = time.perf_counter()
        ins, rows, genome = write_inputs(pool, d, total, nsets)
        in_bytes = sum(os.path.getsize(p) for p in ins)
        print(f"[batch_io_bench] {nsets} sets x {rows} rows written, "
              f"{in_bytes / 1e9:.2f} GB in {time.perf_counter() - t0:.0f} s", file=sys.stderr,
              flush=True)
        routes = ("host", "device", "device_save")
        outs = {r: [os.path.join(d, f"{r}{k:05d}.csv") for k in range(nsets)] for r in routes}
        run = {"host": lambda: route_host(ctx, pool, ins, outs["host"]),
               "device": lambda: route_device(ctx, ins, outs["device"], False),
               "device_save": lambda: route_device(ctx, ins, outs["device_save"], True)}
        # warm-up: one run of every route (page cache, workspaces, staging ring)
        want = None
        for r in routes:
            run[r]()
            got = hash_all(pool, outs[r])
            want = want or got
            if got != want:
                raise SystemExit(f"{r}: outputs differ from the host route's")
        legs = {r: [] for r in routes}
        same = {r: True for r in routes}
        for i in range(runs):
            for r in routes:
                for p in outs[r]:
                    os.remove(p)
                legs[r].append(run[r]())
                same[r] &= hash_all(pool, outs[r]) == want
                print(f"[batch_io_bench] {nsets} sets, run {i}, {r}: "
                      f"{legs[r][-1]['total_s']:.3f} s", file=sys.stderr, flush=True)
        res = {"nsets": nsets, "rows_per_set": rows, "genome_len": genome, "runs": runs,
               "input_bytes": in_bytes, "output_bytes": want[1], "outputs_sha256": want[0]}
        for r in routes:
            res[r] = summary(legs[r])
            res[r]["same_outputs_as_host_route"] = same[r]
        ha = res["host"]["total_s"]
        for r in ("device", "device_save"):
            res[r]["speedup_vs_host_route"] = round(ha["median"] / res[r]["total_s"]["median"], 3)
        return res
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=CFG3_ROWS)
    ap.add_argument("--splits", default="16384,1024,64")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    ctx = rk.Context(0)
    doc = {}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            doc = json.load(f)
    doc.update({"tool": "tools/batch_io_bench.py", "total_rows": args.total,
                "device": torch.cuda.get_device_name(0), "host_threads": THREADS,
                "figures": "seconds (ms inside ingress / egress / batch): median, min, max "
                           "over the runs; routes alternate, one warm-up run each"})
    doc.setdefault("shapes", {})
    with ThreadPoolExecutor(THREADS) as pool:
        for nsets in [int(s) for s in args.splits.split(",") if s]:
            res = bench_split(ctx, pool, args.tmp, args.total, nsets, args.runs)
            doc["shapes"][str(nsets)] = res
            print(json.dumps({k: res[k] if not isinstance(res[k], dict) else
                              {"total_s": res[k]["total_s"],
                               "same": res[k]["same_outputs_as_host_route"]}
                              for k in res}), flush=True)
            if args.out:
                with open(args.out, "w") as f:
                    json.dump(doc, f, indent=1, sort_keys=True)
                    f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
