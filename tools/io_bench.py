#!/usr/bin/env python3
"""End-to-end file path: CSV ingress -> GPU classification -> CSV egress.

SURVEY.md §8(f) rows 1-2: the reference spends most of its wall time parsing
the fragment CSV (FragmentsDatabase.cpp:17-100) and formatting the output
(commonFunctions.cpp:101-146).  This times the repo's host ingress
(rk_db_load_csv: mmap + parallel parse with the reference's acceptance rules)
and egress (rk_db_write_csv: parallel formatting) around the device path on
one synthetic file, next to the reference itself (oracle/_ref/ref_driver,
1 core) on the same file, and checks that both outputs are byte-identical.

  python tools/io_bench.py [--n 50000000] [--genome 3000000000] [--tmp DIR]
                           [--device-parse-reps K [--egress-rows R1,R2,...]]

--device-parse-reps K alternates three routes K times each on the same file:
host (parse, classify, format on the host side of PCIe), device (parsed on the
GPU, formatted by the host) and device_save (parsed, classified and formatted
on the GPU); every output's SHA-256 is compared with the host route's.

(default: cfg3, the headline config: 50M fragments over 3 Gbp)

Prints one JSON line.  Test/benchmark infrastructure: the reference binary is
only timed and compared against, never used to produce results.
"""
from __future__ import annotations

import argparse
import filecmp
import hashlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (one shared HIP runtime)

import repkiller_amd as rk  # noqa: E402


def heartbeat(stop, t0):
    """A progress line every 30 s on stderr (the reference's run is minutes of silence)."""
    while not stop.wait(30):
        print(f"[io_bench] {time.perf_counter() - t0:.0f} s", file=sys.stderr, flush=True)


def sha256_file(path):
    h = hashlib.sha256()
    with open(path, "rb") as fh:
        for blk in iter(lambda: fh.read(1 << 24), b""):
            h.update(blk)
    return h.hexdigest()


def rounded(st):
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()}


def device_parse_leg(ctx, inp, d, host_csv, reps, egress_rows=()):
    """The host route (rk_db_load_csv -> rk_classify -> rk_db_write_csv), the
    device-parse route (rk_db_load_csv_device with the columns kept resident ->
    rk_classify_db_pairs -> rk_db_write_csv) and the device-save route (all nine
    columns resident -> rk_classify_db_pairs_to_csv: classified and formatted on
    the device, no separate save) on the same file, alternating, page cache
    warm for all.  The host route is the yardstick of the parse, the device
    route of the save: both are timed here, in the same job on the same box.
    egress_rows: RK_CSV_OUT_ROWS candidates, each timed once more per rep on the
    device-save route's database (the environment is restored afterwards)."""
    want = sha256_file(host_csv)
    legs = {"host": [], "device": [], "device_save": []}
    sweep = {str(r): [] for r in egress_rows}
    for _ in range(reps):
        for route in ("host", "device", "device_save"):
            out_csv = os.path.join(d, f"leg_{route}.csv")
            t0 = time.perf_counter()
            if route == "host":
                db = rk.FragmentsDatabase(inp)
            else:
                db = rk.FragmentsDatabase(inp, ctx=ctx, keep_device=True,
                                          keep_rows=route == "device_save")
            t1 = time.perf_counter()
            if route == "device_save":
                ctx.classify_db_to_csv(db, [(0.3, 0.3)], [out_csv])
                t3 = time.perf_counter()
                leg = {"load_s": round(t1 - t0, 3), "classify_save_s": round(t3 - t1, 3),
                       "total_s": round(t3 - t0, 3), "egress": rounded(ctx.egress_stats()),
                       "classify_device_ms": round(ctx.stats()["device_ms"], 3)}
                leg["ingress"] = rounded(ctx.ingress_stats())
                leg["same_csv_as_host_route"] = sha256_file(out_csv) == want
                os.remove(out_csv)
                saved = os.environ.get("RK_CSV_OUT_ROWS")
                for r in egress_rows:
                    os.environ["RK_CSV_OUT_ROWS"] = str(r)
                    t4 = time.perf_counter()
                    ctx.classify_db_to_csv(db, [(0.3, 0.3)], [out_csv])
                    t5 = time.perf_counter()
                    sweep[str(r)].append({"classify_save_s": round(t5 - t4, 3),
                                          "egress": rounded(ctx.egress_stats()),
                                          "same_csv_as_host_route": sha256_file(out_csv) == want})
                    os.remove(out_csv)
                if saved is None:
                    os.environ.pop("RK_CSV_OUT_ROWS", None)
                else:
                    os.environ["RK_CSV_OUT_ROWS"] = saved
                db.close()
                del db
                legs[route].append(leg)
                continue
            if route == "host":
                res = ctx.classify(db.frags, db.len_x_hdr, db.len_y_hdr, 0.3, 0.3)
            else:
                res = ctx.classify_db(db, 0.3, 0.3)
            t2 = time.perf_counter()
            db.save_all_frag_pairs(out_csv, res)
            t3 = time.perf_counter()
            leg = {"load_s": round(t1 - t0, 3), "classify_s": round(t2 - t1, 3),
                   "save_s": round(t3 - t2, 3), "total_s": round(t3 - t0, 3)}
            if route == "device":
                st = ctx.ingress_stats()
                leg["ingress"] = {k: (round(v, 3) if isinstance(v, float) else v)
                                  for k, v in st.items()}
                # the load is synchronous; the resident columns were complete
                # before the download of the host columns began
                leg["resident_columns_s"] = round(
                    (st["h2d_ms"] + st["device_ms"] + st["host_fix_ms"]) / 1e3, 3)
            leg["same_csv_as_host_route"] = sha256_file(out_csv) == want
            os.remove(out_csv)
            db.close()
            del db, res
            legs[route].append(leg)
    summary = {}
    for route, runs in legs.items():
        tot = sorted(r["total_s"] for r in runs)
        summary[route] = {"total_s_median": tot[len(tot) // 2], "total_s_min": tot[0],
                          "total_s_max": tot[-1],
                          "load_s_median": sorted(r["load_s"] for r in runs)[len(runs) // 2]}
    # the device-save route counts as faster than the device route only when its
    # median total is below that route's median by more than that route's spread
    dv, ds = summary["device"], summary["device_save"]
    summary["device_save_faster_than_device"] = bool(
        dv["total_s_median"] - ds["total_s_median"] > dv["total_s_max"] - dv["total_s_min"])
    cs = sorted(r["classify_s"] + r["save_s"] for r in legs["device"])
    dv["classify_plus_save_s_median"] = round(cs[len(cs) // 2], 3)
    cs = sorted(r["classify_save_s"] for r in legs["device_save"])
    ds["classify_save_s_median"] = cs[len(cs) // 2]
    out = {"reps": reps, "legs": legs, "summary": summary, "host_csv_sha256": want}
    if sweep:
        out["egress_rows_sweep"] = sweep
    return out


def main():
    import threading
    stop = threading.Event()
    threading.Thread(target=heartbeat, args=(stop, time.perf_counter()), daemon=True).start()
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--genome", type=int, default=3_000_000_000)  # cfg3
    ap.add_argument("--no-ref", action="store_true")
    ap.add_argument("--device-parse-reps", type=int, default=0,
                    help="alternate the host route and the device-parse route this many times "
                         "each on the same file (warm page cache) and record both")
    ap.add_argument("--egress-rows", default="",
                    help="comma-separated RK_CSV_OUT_ROWS candidates, each timed on the "
                         "device-save route in every rep")
    ap.add_argument("--device-save-only", type=int, default=0,
                    help="load once with every column resident, classify and save on the "
                         "device this many times, and stop (a run for a kernel trace)")
    ap.add_argument("--tmp", default=os.environ.get("TMPDIR", "/tmp"))
    args = ap.parse_args()
    n, L = args.n, args.genome
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = None
    cpu = "unknown"
    with open("/proc/cpuinfo") as fh:
        for line in fh:
            if line.startswith("model name"):
                cpu = line.split(":", 1)[1].strip()
                break
    out = {"fragments": n, "genome_bp": L, "seed": 3,
           "host": {"nproc": os.cpu_count(), "affinity_cpus": aff, "cpu_model": cpu},
           "note": "ours: rk_db_load_csv (mmap + parallel parse) -> rk_classify (host buffers, "
                   "PCIe included) -> rk_db_write_csv (parallel formatting); reference: "
                   "oracle/_ref/ref_driver (the reference's own code, one core) on the same file"}
    with tempfile.TemporaryDirectory(dir=args.tmp) as d:
        inp = os.path.join(d, "in.csv")
        f = rk.synth(n, L, seed=3)
        rk.write_input_csv(inp, f, L, L)
        del f
        out["csv_bytes"] = os.path.getsize(inp)
        ctx = rk.Context(0)
        if args.device_save_only > 0:
            db = rk.FragmentsDatabase(inp, ctx=ctx, keep_rows=True)
            runs = []
            for _ in range(args.device_save_only):
                ctx.classify_db_to_csv(db, [(0.3, 0.3)], [os.path.join(d, "save.csv")])
                runs.append(rounded(ctx.egress_stats()))
            db.close()
            stop.set()
            print(json.dumps({"fragments": n, "device_save_only": runs}), flush=True)
            return
        t0 = time.perf_counter()
        db = rk.FragmentsDatabase(inp)
        t1 = time.perf_counter()
        res = ctx.classify(db.frags, db.len_x_hdr, db.len_y_hdr, 0.3, 0.3)
        t2 = time.perf_counter()
        ours = os.path.join(d, "ours.csv")
        db.save_all_frag_pairs(ours, res)
        t3 = time.perf_counter()
        out.update(load_s=round(t1 - t0, 3), classify_s=round(t2 - t1, 3),
                   save_s=round(t3 - t2, 3), total_s=round(t3 - t0, 3),
                   host_threads=os.cpu_count())
        # the binary SoA cache: written once, then a load
        # with no parse; the classification from it must write the same bytes
        cache = os.path.join(d, "db.soa")
        t4 = time.perf_counter()
        db.save_soa(cache)
        t5 = time.perf_counter()
        db2 = rk.FragmentsDatabase.load_soa(cache)
        t6 = time.perf_counter()
        res2 = ctx.classify(db2.frags, db2.len_x_hdr, db2.len_y_hdr, 0.3, 0.3)
        t7 = time.perf_counter()
        ours2 = os.path.join(d, "ours_soa.csv")
        db2.save_all_frag_pairs(ours2, res2)
        t8 = time.perf_counter()
        out["soa_cache"] = {"bytes": os.path.getsize(cache), "save_s": round(t5 - t4, 3),
                            "load_s": round(t6 - t5, 3), "classify_s": round(t7 - t6, 3),
                            "save_csv_s": round(t8 - t7, 3), "total_s": round(t8 - t5, 3),
                            "same_csv_as_csv_route": filecmp.cmp(ours, ours2, shallow=False)}
        os.remove(ours2)
        os.remove(cache)
        del db2, res2
        if args.device_parse_reps > 0:
            del db, res
            rows = [int(r) for r in args.egress_rows.split(",") if r]
            out["device_parse"] = device_parse_leg(ctx, inp, d, ours, args.device_parse_reps, rows)
        ref = os.path.join(ROOT, "oracle", "_ref", "ref_driver")
        if not args.no_ref and os.path.exists(ref):
            theirs = os.path.join(d, "ref.csv")
            t0 = time.perf_counter()
            p = subprocess.run([ref, inp, theirs, "0.3", "0.3"], capture_output=True, text=True)
            out["reference_wall_s"] = round(time.perf_counter() - t0, 3)
            t = json.loads(p.stderr.strip().splitlines()[-1])
            out["reference"] = {k: round(t[k], 3) for k in ("load_s", "group_s", "diag_sort_s",
                                                             "save_s")}
            out["reference"]["total_s"] = round(sum(out["reference"].values()), 3)
            out["byte_identical"] = filecmp.cmp(ours, theirs, shallow=False)
            out["output_bytes"] = os.path.getsize(ours)
            out["speedup_total"] = round(out["reference"]["total_s"] / out["total_s"], 1)
    stop.set()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
