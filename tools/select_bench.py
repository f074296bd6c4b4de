#!/usr/bin/env python3
"""Selection by repeat flag, measured (DESIGN.md "Selection by repeat flag").

  device  rk_result_select (RK_RES_DEVICE) on cfg3's 50M-row result, masks 3, 4
          and 7: HIP-event time over >= 20 calls after warm-up, the algorithmic
          bytes 9 n + 9 kept (flag + order + gid read, the kept triples
          written), their share of the HBM peak, the launches per call; and,
          alternated in the same process, what a user could do without it:
          download the three arrays, filter with numpy, upload.
  file    cfg3 file to file through the CLI: --device-parse --device-save with
          --keep unique against the same command without --keep (the unchanged
          route, the yardstick), alternated, spread over the repeats.
  batch   the same for the rows as 1024 files through --batch.

  python tools/select_bench.py [--parts device,file,batch] [--n 50000000]
                               [--genome 3000000000] [--reps 3] [--tmp DIR]
                               [--out profiles/select_bench.json]

Results of the parts given are merged into --out.  Reports, not gates.
"""
from __future__ import annotations

import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import repkiller_amd as rk  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s (MI355X spec)
CALLS, WARM = 24, 3


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4),
            "max": round(max(v), 4), "n": len(v)}


def part_device(n, genome, reps):
    ctx = rk.Context(0)
    t0 = time.perf_counter()
    f = rk.synth(n, genome, seed=3, with_ident=False)
    x, y, ln = (torch.from_numpy(a.view(np.int64)).cuda() for a in (f.x_start, f.y_start, f.length))
    strand = torch.from_numpy(f.strand).cuda()
    gid, order = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    rep = torch.zeros(n, dtype=torch.uint8, device="cuda")
    n_out, n_groups = ctx.classify_device(x, y, ln, strand, gid, rep, order, genome, genome,
                                          0.3, 0.3)
    del x, y, ln, strand, f
    so, sg = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(2))
    sr = torch.empty(n, dtype=torch.uint8, device="cuda")
    out = {"rows": n_out, "groups": n_groups, "setup_s": round(time.perf_counter() - t0, 1),
           "launches_per_call": {"kernels": 4, "copies": 2,
                                 "what": "count, tile scan, set bases, scatter; the set table "
                                         "up, the bases and counts down"},
           "masks": {}}
    for keep in (3, 4, 7):
        ev, wall, alt = [], [], []
        kept = 0
        for r in range(reps):
            for c in range(WARM if r == 0 else 0):
                ctx.select_device(order, gid, rep, n_out, keep, so, sg, sr)
            for c in range((CALLS + reps - 1) // reps):
                t = time.perf_counter()
                kept = ctx.select_device(order, gid, rep, n_out, keep, so, sg, sr)
                wall.append((time.perf_counter() - t) * 1e3)
                ev.append(ctx.select_stats()["device_ms"])
            # without the feature: down, numpy, up
            torch.cuda.synchronize()
            t = time.perf_counter()
            ho, hg, hr = order[:n_out].cpu().numpy(), gid[:n_out].cpu().numpy(), \
                rep[:n_out].cpu().numpy()
            t1 = time.perf_counter()
            k = (hr <= 2) & (((keep >> np.minimum(hr, 7)) & 1) == 1)
            fo, fg, fr = ho[k], hg[k], hr[k]
            t2 = time.perf_counter()
            uo, ug, ur = torch.from_numpy(fo).cuda(), torch.from_numpy(fg).cuda(), \
                torch.from_numpy(fr).cuda()
            torch.cuda.synchronize()
            t3 = time.perf_counter()
            alt.append({"download_ms": (t1 - t) * 1e3, "numpy_ms": (t2 - t1) * 1e3,
                        "upload_ms": (t3 - t2) * 1e3, "total_ms": (t3 - t) * 1e3})
            if r == 0:
                same = (fo.shape[0] == kept and torch.equal(uo, so[:kept])
                        and torch.equal(ug, sg[:kept]) and torch.equal(ur, sr[:kept]))
            del uo, ug, ur
        st = ctx.select_stats()
        algo = 9 * n_out + 9 * kept
        med = statistics.median(ev)
        out["masks"][str(keep)] = {
            "kept": kept, "by_flag": st["by_flag"], "device_ms": spread(ev),
            "call_wall_ms": spread(wall), "algo_bytes": algo,
            "algo_gb_s": round(algo / med / 1e6, 1),
            "share_of_hbm_peak": round(algo / (med * 1e-3) / HBM_PEAK, 4),
            "numpy_route_ms": {k: spread([a[k] for a in alt]) for k in alt[0]},
            "same_as_numpy_route": bool(same)}
    ctx.close()
    return out


def cli(args):
    t = time.perf_counter()
    p = subprocess.run([rk.CLI_PATH] + args, capture_output=True, text=True)
    wall = time.perf_counter() - t
    if p.returncode:
        raise RuntimeError(p.stdout + p.stderr)
    info = {}
    for line in p.stderr.splitlines():
        if line.startswith("{"):
            info.update(json.loads(line))
    return wall, info


def alternate(reps, base_args, outs_note, outs):
    """[--keep unique] + base_args against base_args, alternated.  The outputs of
    the run before are removed first, outside the timed region: a run does not
    pay for truncating the other route's files."""
    legs = {"all": [], "unique": []}
    last = {}
    for _ in range(reps):
        for name, extra in (("all", []), ("unique", ["--keep", "unique"])):
            for p in outs:
                if os.path.exists(p):
                    os.remove(p)
            wall, info = cli(extra + base_args)
            legs[name].append(wall)
            last[name] = info
    res = {name: {"wall_s": spread(v)} for name, v in legs.items()}
    for name, info in last.items():
        for k in ("egress", "select", "classify_save_s", "load_s", "batch"):
            if k in info:
                res[name][k] = info[k]
    res["note"] = outs_note
    return res


def part_file(n, genome, reps, d):
    inp, out = os.path.join(d, "cfg3.csv"), os.path.join(d, "cfg3.out.csv")
    t0 = time.perf_counter()
    rk.write_input_csv(inp, rk.synth(n, genome, seed=3), genome, genome)
    gen = time.perf_counter() - t0
    res = alternate(reps, ["--timing", "--device-parse", "--device-save", inp, out, "0.3", "0.3"],
                    "whole process wall: HIP start-up, device parse, classification, "
                    "[selection,] device save", [out])
    res.update(rows=n, input_bytes=os.path.getsize(inp), gen_s=round(gen, 1))
    os.remove(inp)
    os.remove(out)
    return res


def part_batch(n, genome, reps, d, nsets=1024):
    rows = n // nsets
    g = max(1000, genome * rows // n)

    def one(k):
        p = os.path.join(d, f"in{k:05d}.csv")
        rk.write_input_csv(p, rk.synth(rows, g, seed=1000 + k), g, g)
        return p

    t0 = time.perf_counter()
    with ThreadPoolExecutor(16) as pool:
        ins = list(pool.map(one, range(nsets)))
    gen = time.perf_counter() - t0
    lst = os.path.join(d, "list.txt")
    outs = [os.path.join(d, f"out{k:05d}.csv") for k in range(nsets)]
    with open(lst, "w") as fh:
        for p, o in zip(ins, outs):
            fh.write(f"{p}\t{o}\n")
    res = alternate(reps, ["--timing", "--batch", lst, "--device-parse", "--device-save", "0.3",
                           "0.3"], "whole process wall, 1024 files in, 1024 files out", outs)
    res.update(sets=nsets, rows_per_set=rows, gen_s=round(gen, 1))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="device,file,batch")
    ap.add_argument("--n", type=int, default=50_000_000)
    ap.add_argument("--genome", type=int, default=3_000_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tmp", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "select_bench.json"))
    a = ap.parse_args()
    result = {}
    if os.path.exists(a.out):
        with open(a.out) as fh:
            result = json.load(fh)
    result.update(tool="tools/select_bench.py", gpu=torch.cuda.get_device_name(0),
                  tile=rk.select_tile())
    d = tempfile.mkdtemp(prefix="select_bench_", dir=a.tmp)
    try:
        for part in a.parts.split(","):
            t0 = time.perf_counter()
            if part == "device":
                result["device_select"] = part_device(a.n, a.genome, a.reps)
            elif part == "file":
                result["file"] = part_file(a.n, a.genome, a.reps, d)
            elif part == "batch":
                result["batch"] = part_batch(a.n, a.genome, a.reps, d)
            else:
                raise SystemExit(f"unknown part {part}")
            print(f"[select_bench] {part}: {time.perf_counter() - t0:.0f} s", file=sys.stderr,
                  flush=True)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as fh:
                json.dump(result, fh, indent=1)
                fh.write("\n")
    finally:
        shutil.rmtree(d, ignore_errors=True)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
