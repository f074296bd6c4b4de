"""Shared by tests/test_select_host.py and tests/test_select_device.py: the
numpy selection every route is compared against, flag patterns, batch layouts
and the golden files filtered by the last field of their Frag lines."""
import gzip
import json
import os
import shutil

import numpy as np

from conftest import EDGE, GOLDEN

SENT32 = 0xDEADBEEF  # the untouched entries of an output array
SENT8 = 0xA5


def kept_flags(rep, keep):
    """The predicate on its own: flag f <= 2 and bit f of keep."""
    f = np.asarray(rep, np.uint8).astype(np.uint32)
    return (f <= 2) & (((keep >> np.minimum(f, 31)) & 1) == 1)


def np_select(off, n_out, order, gid, rep, keep):
    """(out_order, out_gid, out_rep, kept): arrays of off[-1] entries, sentinels
    where the selection writes nothing; set k's kept rows from off[k] on."""
    n = int(off[-1])
    oo, og = np.full(n, SENT32, np.uint32), np.full(n, SENT32, np.uint32)
    orp = np.full(n, SENT8, np.uint8)
    kept = np.zeros(len(off) - 1, np.uint64)
    for k in range(len(off) - 1):
        a, u = int(off[k]), int(n_out[k])
        idx = a + np.flatnonzero(kept_flags(rep[a:a + u], keep))
        m = idx.shape[0]
        oo[a:a + m], og[a:a + m], orp[a:a + m] = order[idx], gid[idx], rep[idx]
        kept[k] = m
    return oo, og, orp, kept


def by_flag(off, n_out, rep):
    """Used slots by flag: 0, 1, 2, anything else."""
    c = [0, 0, 0, 0]
    for k in range(len(off) - 1):
        f = rep[int(off[k]):int(off[k]) + int(n_out[k])]
        for v in range(3):
            c[v] += int((f == v).sum())
        c[3] += int((f > 2).sum())
    return c


def flags_for(pattern, n, keep, rnd):
    """n flags of which `pattern` says which rows are kept under `keep`: kept rows
    draw from the flags in keep, the others from the flags outside it, 3 and 255
    among them."""
    inside = [f for f in range(3) if (keep >> f) & 1]
    outside = [f for f in range(3) if not (keep >> f) & 1] + [3, 255]
    if pattern == "all":
        k = np.ones(n, bool)
    elif pattern == "none":
        k = np.zeros(n, bool)
    elif pattern == "alternating":
        k = np.arange(n) % 2 == 0
    elif pattern == "first":
        k = np.arange(n) == 0
    elif pattern == "last":
        k = np.arange(n) == n - 1
    elif pattern == "p02":
        k = rnd.rand(n) < 0.02
    elif pattern == "p98":
        k = rnd.rand(n) < 0.98
    else:
        raise ValueError(pattern)
    rep = np.asarray(outside, np.uint8)[rnd.randint(0, len(outside), n)]
    rep[k] = np.asarray(inside, np.uint8)[rnd.randint(0, len(inside), n)][k]
    return rep


PATTERNS = ("all", "none", "alternating", "first", "last", "p02", "p98")


def random_result(n, rnd):
    """order, gid of n rows (any values: the selection copies them)."""
    return (rnd.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32),
            rnd.randint(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32))


def poison_unused(off, n_out, order, rep):
    """The unused slots of every window read as kept rows if they are read at all."""
    for k in range(len(off) - 1):
        a, b = int(off[k]) + int(n_out[k]), int(off[k + 1])
        rep[a:b] = 1
        order[a:b] = 0xFFFFFFFF


def batch_layouts(tile):
    """name -> window sizes; every layout with empty sets where the issue asks."""
    rnd = np.random.RandomState(11)
    return {
        "one": [37],
        "two": [tile - 1, 2],
        "three_tile_edges": [tile - 1, 2, tile + 1],
        "wave_edges": [1, 63, 64, 65, 1, 63, 64, 65],
        "empties": [0, 0, 5, 0, 70, 0, 0, 9, 0],
        "seeded_5000": [0, 0] + list(rnd.randint(0, 41, 4996)) + [0, 0],
    }


def layout_arrays(sizes, rnd, short=True, first=0):
    """off, n_out (some below their window when short), order, gid, rep with the
    unused slots poisoned; the first set starts at slot `first`, and the slots
    before it, which belong to no set, are poisoned too."""
    sizes = np.asarray(sizes, np.uint64)
    off = (np.concatenate([[0], np.cumsum(sizes)]) + first).astype(np.uint64)
    n_out = sizes.copy()
    if short:
        cut = rnd.rand(len(sizes)) < 0.5
        n_out[cut] = (sizes[cut] * rnd.rand(int(cut.sum()))).astype(np.uint64)
    n = int(off[-1])
    order, gid = random_result(n, rnd)
    rep = np.asarray([0, 1, 2, 2, 2, 3, 255], np.uint8)[rnd.randint(0, 7, n)]
    poison_unused(off, n_out, order, rep)
    rep[:first] = 1
    order[:first] = 0xFFFFFFFF
    return off, n_out, order, gid, rep


def filtered(golden, keep):
    """The golden file with the Frag lines whose last field is not a kept flag
    deleted; everything else byte for byte."""
    out = []
    for line in golden.splitlines(keepends=True):
        if line.startswith(b"Frag,"):
            f = int(line.rstrip(b"\r\n").rsplit(b",", 1)[1])
            if not (f <= 2 and (keep >> f) & 1):
                continue
        out.append(line)
    return b"".join(out)


def golden_rows(golden):
    return sum(1 for line in golden.splitlines() if line.startswith(b"Frag,"))


def ref_fixtures():
    """(name, case) of every `expect: ref` edge fixture."""
    with open(os.path.join(EDGE, "manifest.json")) as f:
        man = json.load(f)
    return sorted((n, c) for n, c in man.items() if c["expect"] == "ref")


def edge_in(name):
    return os.path.join(EDGE, name + ".in.csv")


def edge_golden(name):
    with open(os.path.join(EDGE, name + ".out.csv"), "rb") as f:
        return f.read()


def unpack_corpus(d):
    """The 10k corpus as (input path, golden bytes)."""
    p = d / "corpus10k.in.csv"
    with gzip.open(os.path.join(GOLDEN, "corpus10k.in.csv.gz"), "rb") as f, open(p, "wb") as o:
        shutil.copyfileobj(f, o)
    with gzip.open(os.path.join(GOLDEN, "corpus10k.out.csv.gz"), "rb") as f:
        return str(p), f.read()
