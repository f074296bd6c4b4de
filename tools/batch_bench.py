#!/usr/bin/env python3
"""Many fragment sets: a loop of rk_classify_device calls on one context
against ONE rk_classify_device_batch call over the same sets (DESIGN.md
"Batched sets").  ~50M rows in all, split into 16384, 1024, 64 and 8 sets of
cfg3's density (a set's genome length is 3 Gbp x rows / 50M; every set has its
own seed), device-resident inputs from rk_synth_generate, plus the plain 50M
cfg3 step for scale.

Each shape is warmed up (both variants), then the variants alternate in this
process; a timed window repeats its variant until at least one second has
passed and reports host wall time per pass.  The loop's entry point is the
one every earlier build has, unchanged by the batch work, so the yardstick is
timed on this same build.  The outputs of the two variants are compared set
by set.

  python tools/batch_bench.py [--total 50000000] [--splits 16384,1024,64,8]
                              [--out profiles/batch_bench.json]
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import repkiller_amd as rk  # noqa: E402

CFG3_ROWS, CFG3_GENOME = 50_000_000, 3_000_000_000


def make_sets(total: int, nsets: int):
    """Host columns of `nsets` sets of total // nsets rows, offsets, genome lengths."""
    rows = total // nsets
    genome = max(1000, CFG3_GENOME * rows // CFG3_ROWS)
    cols = [[], [], [], []]
    for k in range(nsets):
        f = rk.synth(rows, genome, seed=1000 + k, with_ident=False)
        for c, a in zip(cols, (f.x_start, f.y_start, f.length, f.strand)):
            c.append(a)
    off = np.arange(nsets + 1, dtype=np.uint64) * np.uint64(rows)
    return [np.concatenate(c) for c in cols], off, genome


def timed(fn, min_s: float):
    """Repeat fn until min_s have passed: (host wall ms per pass, passes)."""
    passes, t0 = 0, time.perf_counter()
    while True:
        fn()
        passes += 1
        dt = time.perf_counter() - t0
        if dt >= min_s:
            return dt * 1e3 / passes, passes


def bench_split(ctx, lib, dev, total, nsets, rounds, min_s, lr, pr):
    cols, off, genome = make_sets(total, nsets)
    n = int(off[-1])
    t = lambda v: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)
    x, y, ln, s = (t(c) for c in cols)
    del cols
    out = {v: (torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.int32, device=dev),
               torch.zeros(n, dtype=torch.uint8, device=dev)) for v in ("loop", "batch")}
    hdr = np.full(nsets, genome, np.uint64)
    n_out = {v: np.zeros(nsets, np.uint64) for v in out}
    n_groups = {v: np.zeros(nsets, np.uint64) for v in out}

    # the loop's per-set arguments, built once
    o, g, r = out["loop"]
    soas = (rk.FragsSoA * nsets)()
    ress = (rk.Result * nsets)()
    prm = rk.Params(genome, genome, lr, pr)
    for k in range(nsets):
        a, b = int(off[k]), int(off[k + 1])
        soas[k] = rk.FragsSoA(x.data_ptr() + 8 * a, y.data_ptr() + 8 * a, ln.data_ptr() + 8 * a,
                              s.data_ptr() + a, b - a)
        ress[k] = rk.Result(o.data_ptr() + 4 * a, g.data_ptr() + 4 * a, r.data_ptr() + a, 0, 0)
    fn, h, pp = lib.rk_classify_device, ctx._h, ctypes.byref(prm)

    def loop():
        for k in range(nsets):
            rc = fn(h, ctypes.byref(soas[k]), pp, ctypes.byref(ress[k]))
            if rc:
                raise rk.RkError(rc, ctx.last_error())

    o, g, r = out["batch"]
    bsoa = rk.FragsSoA(x.data_ptr(), y.data_ptr(), ln.data_ptr(), s.data_ptr(), n)
    bprm = rk.BatchParams(nsets, off.ctypes.data, hdr.ctypes.data, hdr.ctypes.data, lr, pr)
    bres = rk.BatchResult(o.data_ptr(), g.data_ptr(), r.data_ptr(),
                          n_out["batch"].ctypes.data, n_groups["batch"].ctypes.data)

    def batch():
        rc = lib.rk_classify_device_batch(h, ctypes.byref(bsoa), ctypes.byref(bprm),
                                          ctypes.byref(bres))
        if rc:
            raise rk.RkError(rc, ctx.last_error())

    torch.cuda.synchronize()
    loop()   # warm-up: workspaces sized for this shape
    batch()
    for k in range(nsets):
        n_out["loop"][k], n_groups["loop"][k] = ress[k].n_out, ress[k].n_groups
    # equal outputs: counts, then the first n_out entries of every set
    sizes = torch.from_numpy(np.diff(off).astype(np.int64)).to(dev)
    kept = torch.from_numpy(n_out["loop"].astype(np.int64)).to(dev)
    pos = torch.arange(n, device=dev) - torch.repeat_interleave(
        torch.from_numpy(off[:-1].astype(np.int64)).to(dev), sizes)
    valid = pos < torch.repeat_interleave(kept, sizes)
    equal = (np.array_equal(n_out["loop"], n_out["batch"])
             and np.array_equal(n_groups["loop"], n_groups["batch"])
             and all(bool(torch.equal(a[valid], b[valid]))
                     for a, b in zip(out["loop"], out["batch"])))
    assert equal, f"{nsets} sets: the loop and the batch disagree"
    del pos, valid
    loop_ms, batch_ms = [], []
    for _ in range(rounds):
        loop_ms.append(timed(loop, min_s))
        batch_ms.append(timed(batch, min_s))
    stats = ctx.batch_stats()  # (of the last timed batch call)
    best_l, best_b = min(m for m, _ in loop_ms), min(m for m, _ in batch_ms)
    return {"sets": nsets, "rows_per_set": n // nsets, "rows": n, "genome_bp_per_set": genome,
            "groups": int(n_groups["loop"].sum()),
            "loop_ms": round(best_l, 3), "batch_ms": round(best_b, 3),
            "loop_ms_rounds": [round(m, 3) for m, _ in loop_ms],
            "batch_ms_rounds": [round(m, 3) for m, _ in batch_ms],
            "passes_per_window": [loop_ms[0][1], batch_ms[0][1]],
            "loop_us_per_set": round(best_l * 1e3 / nsets, 2),
            "batch_us_per_set": round(best_b * 1e3 / nsets, 2),
            "speedup": round(best_l / best_b, 3),
            "sub_batches": stats["sub_batches"], "looped_sets": stats["looped_sets"],
            "batch_device_ms": round(stats["device_ms"], 3), "equal_outputs": equal}


def bench_plain(ctx, lib, dev, total, rounds, min_s, lr, pr):
    genome = CFG3_GENOME * total // CFG3_ROWS
    f = rk.synth(total, genome, seed=3, with_ident=False)
    t = lambda v: torch.from_numpy(v.view(np.int64) if v.dtype == np.uint64 else v).to(dev)
    x, y, ln, s = t(f.x_start), t(f.y_start), t(f.length), t(f.strand)
    n = f.n
    del f
    gid = torch.zeros(n, dtype=torch.int32, device=dev)
    order = torch.zeros(n, dtype=torch.int32, device=dev)
    rep = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    step = lambda: ctx.classify_device(x, y, ln, s, gid, rep, order, genome, genome, lr, pr)
    step()
    ms = [timed(step, min_s)[0] for _ in range(rounds)]
    return {"rows": n, "genome_bp": genome, "step_ms": round(min(ms), 3),
            "step_ms_rounds": [round(m, 3) for m in ms]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--total", type=int, default=CFG3_ROWS)
    ap.add_argument("--splits", default="16384,1024,64,8")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--min-seconds", type=float, default=1.0)
    ap.add_argument("--len-ratio", type=float, default=0.3)
    ap.add_argument("--pos-ratio", type=float, default=0.3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    ctx = rk.Context(0)
    lib = rk.load_library()
    res = {"what": "loop of rk_classify_device over the sets vs one rk_classify_device_batch, "
                   "host wall ms per pass (best of the rounds), device-resident inputs",
           "yardstick": "the loop, timed on this same build: rk_classify_device is unchanged "
                        "by the batch entry points",
           "device": torch.cuda.get_device_name(0), "len_ratio": a.len_ratio,
           "pos_ratio": a.pos_ratio, "min_window_s": a.min_seconds, "splits": []}
    for nsets in (int(v) for v in a.splits.split(",")):
        r = bench_split(ctx, lib, dev, a.total, nsets, a.rounds, a.min_seconds, a.len_ratio,
                        a.pos_ratio)
        res["splits"].append(r)
        print(json.dumps(r), flush=True)
        if a.out:  # (kept after every shape: a later shape may run out of time)
            with open(a.out, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
        torch.cuda.empty_cache()
    res["plain_cfg3_step"] = bench_plain(ctx, lib, dev, a.total, a.rounds, a.min_seconds,
                                         a.len_ratio, a.pos_ratio)
    print(json.dumps(res["plain_cfg3_step"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    ctx.close()


if __name__ == "__main__":
    main()
