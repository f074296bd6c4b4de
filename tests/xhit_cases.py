"""Inputs of tests/test_xhit_from_parents.py and their oracle results.

Every set is a synthetic one dense enough that fragments join groups (on X or
on Y) and others open groups of their own, on both strands; no set has more
than 64,000 rows.  The oracle runs once per (set, ratio pair) and its arrays
are read-only.
"""
import hashlib

import numpy as np

from oracle import rk_oracle as ro

import repkiller_amd as rk

# kept rows at the bitmask's word edges (a word is 32 rows, a wave's ballot 64,
# a load row of the bitmask kernel 1024, its tile 4096)
WORD_EDGES = [1, 31, 32, 33, 63, 64, 65, 1023, 1025, 4096, 4097]

BIG = dict(kind="synth", n=64_000, L=3_840_000, seed=7)      # cfg3's density
SMALL = dict(kind="synth", n=5_000, L=300_000, seed=8)
DENSE = dict(kind="synth", n=20_000, L=60_000, seed=24, lead_in=0)  # halo disagreements


def edge_case(m):
    return dict(kind="synth", n=m, L=max(2000, 40 * m), seed=100 + m, copies=(2, 6))


def frags(case):
    f = rk.synth(case["n"], case["L"], seed=case["seed"], family_frac=case.get("ff", 0.8),
                 copies=tuple(case.get("copies", (2, 30))))
    return f, case["L"], case["L"]


_ORACLE = {}


def oracle(case, lr=0.3, pr=0.3):
    """(gid, repval, out_order, n_groups) of the oracle, computed once."""
    key = (case["n"], case["L"], case["seed"], lr, pr)
    if key not in _ORACLE:
        f, lx, ly = frags(case)
        rc, gid, rep, order, ng = ro.classify(f.x_start, f.y_start, f.length, f.strand, lx, ly,
                                              lr, pr)
        assert rc == 0
        for a in (gid, rep, order):
            a.setflags(write=False)
        _ORACLE[key] = (gid, rep, order, ng)
    return _ORACLE[key]


def same(got, want):
    gid, rep, order, ng = want
    assert got.n_groups == ng
    assert np.array_equal(got.out_order, order)
    assert np.array_equal(got.gid, gid)
    assert np.array_equal(got.repval, rep)


def digest_arrays(order, gid, rep):
    h = hashlib.sha256()
    for a in (order, gid, rep):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def joiners_and_singletons(case, lr=0.3, pr=0.3):
    """Per strand: rows in groups of more than one member, rows alone."""
    f, _, _ = frags(case)
    gid, _, order, _ = oracle(case, lr, pr)
    multi = np.bincount(gid)[gid] > 1
    strand = f.strand[order]
    return {chr(c): (int((multi & (strand == c)).sum()), int((~multi & (strand == c)).sum()))
            for c in (ord("f"), ord("r"))}
