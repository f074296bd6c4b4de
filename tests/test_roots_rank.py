"""The record pipeline's roots pass with each root's group rank in its own
parent word: the rank scan flags the roots' words (4096-position tiles, a
4-word tail), a member's chase ends at the first flagged word it loads, and
every pair, repeat, restart and later call rebuilds the parents before it reads
them.  Every result is compared with the oracle bit for bit.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import batch_cases as bc
import direct_emit_cases as dc
from conftest import ROOT
from oracle import rk_oracle as ro

import repkiller_amd as rk

pytestmark = pytest.mark.gpu

_ORACLE = {}


def oracle(name, f, lx, ly, lr=0.3, pr=0.3):
    """The oracle's result, computed once per named input and left unchanged."""
    key = (name, lr, pr)
    if key not in _ORACLE:
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
    assert np.array_equal(got.gid, gid)
    assert np.array_equal(got.repval, rep)
    assert np.array_equal(got.out_order, order)


def digest(r):
    h = hashlib.sha256()
    for a in (r.out_order, r.gid, r.repval):
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def singletons(n):
    """n fragments 1000 apart on both axes: every one a group of its own."""
    i = np.arange(n, dtype=np.uint64)
    f = rk.Frags(5000 + 1000 * i, 7000 + 1000 * i, np.full(n, 200, np.uint64),
                 np.full(n, ord("f"), np.uint8))
    return f, 1000 * (n + 20), 1000 * (n + 20)


def two_tile_groups():
    """4095 copies + a singleton, then 4096 copies + a singleton: roots at the
    processing indices 0, 4095, 4096 and 8192 (the last)."""
    return dc.crafted(dc.group_keys([4095, 4096]))


@pytest.mark.parametrize("n", [1, 2, 3, 5, 4095, 4096, 4097, 8193])
def test_all_singletons(gpu_ctx, n):
    """Every word a root: the scan's tiles of 4096 positions (m + 1 of them) on
    both sides of one and two tiles, and the 4-word tail."""
    f, lx, ly = singletons(n)
    want = oracle(("singletons", n), f, lx, ly)
    assert want[3] == n
    same(gpu_ctx.classify(f, lx, ly), want)
    assert gpu_ctx.stats()["pipeline"] == 1


def test_one_group_holds_every_row(gpu_ctx):
    """A single root at index 0: every chain ends at word 0."""
    f, lx, ly = dc.crafted(dc.group_keys([5000]), tail=[False])
    want = oracle("one_group", f, lx, ly)
    assert f.n == 5000 and want[3] == 1
    same(gpu_ctx.classify(f, lx, ly), want)


def test_roots_on_both_sides_of_a_tile_bound(gpu_ctx):
    f, lx, ly = two_tile_groups()
    want = oracle("two_tiles", f, lx, ly)
    assert f.n == 8193 and want[3] == 4
    assert list(dc.group_sizes(want[0])) == [4095, 1, 4096, 1]
    # rows are in processing order and groups in creation order: the groups
    # are the rows [0, 4095), 4095, [4096, 8192) and 8192, each opened by its first
    order = want[2]
    assert order[4095] == 4095 and order[8192] == 8192
    assert order[:4095].min() == 0 and order[4096:8192].min() == 4096
    same(gpu_ctx.classify(f, lx, ly), want)


def test_crafted_sizes_default(gpu_ctx):
    f, lx, ly = dc.crafted_sizes()
    want = oracle("sizes", f, lx, ly)
    assert f.n == 14_236 and want[3] == 62
    same(gpu_ctx.classify(f, lx, ly), want)
    assert gpu_ctx.stats()["sweep_repeats"] == 0


_SWITCH_SCRIPT = r"""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import repkiller_amd as rk
import direct_emit_cases as dc
ctx = rk.Context(0)
f, lx, ly = dc.crafted_sizes()
g = rk.synth(300_000, 18_000_000, seed=41)
for r in (ctx.classify(f, lx, ly), ctx.classify(g, 18_000_000, 18_000_000)):
    h = hashlib.sha256()
    for a in (r.out_order, r.gid, r.repval):
        h.update(np.ascontiguousarray(a).tobytes())
    s = ctx.stats()
    print(h.hexdigest(), r.n_groups, s["sweep_repeats"], s["jump_rounds"])
"""

_DEFAULT = {}


def default_runs(ctx):
    """The crafted set and a 300k-row synthetic one (cfg3's density) in the
    default environment, each checked against the oracle, once."""
    if not _DEFAULT:
        f, lx, ly = dc.crafted_sizes()
        g, L = rk.synth(300_000, 18_000_000, seed=41), 18_000_000
        for name, (h, hx, hy) in (("sizes", (f, lx, ly)), ("synth300k", (g, L, L))):
            r = ctx.classify(h, hx, hy)
            same(r, oracle(name, h, hx, hy))
            assert ctx.stats()["sweep_repeats"] == 0
            _DEFAULT[name] = (digest(r), r.n_groups)
    return [_DEFAULT["sizes"], _DEFAULT["synth300k"]]


@pytest.mark.parametrize("env", ["RK_ROOTS_STEPS=1", "RK_ROOTS_STEPS=1 RK_ROOTS_REST_STEPS=1",
                                 "RK_SWEEP_BLIND=1", "RK_ROOTS_FUSED=0"])
def test_crafted_sizes_switches(gpu_ctx, env):
    """Listed chains; an open chain and the round-by-round restart; the repeat
    of a pair whose parents the scan has already flagged; the round-by-round
    form.  A switch is read once per process, so each runs in a child process,
    with the default environment's digest.

    The crafted set's chains are one link long and one queued sweep an axis
    resolves it (sweep_repeats measured 0 under RK_SWEEP_BLIND=1: its groups
    are copies inside one window or one long run, which a sweep settles in its
    own ballot rounds), so on its own it reaches neither the listed chains nor
    the repeat.  The child therefore also classifies the 300k-row synthetic set
    of test_schedule_switches_bit_identical, whose axes one queued sweep leaves
    open: the repeat (sweep_repeats == 1) is asserted on that set, and both
    sets' digests are the default environment's, which match the oracle."""
    want = default_runs(gpu_ctx)
    extra = dict(kv.split("=") for kv in env.split())
    out = subprocess.run(["python", "-c", _SWITCH_SCRIPT, str(ROOT)], capture_output=True,
                         text=True, timeout=120, env={**os.environ, **extra})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [ln.split() for ln in out.stdout.strip().split("\n")]
    assert len(lines) == 2
    for (d, ng, repeats, rounds), (wd, wng) in zip(lines, want):
        print(env, "sweep_repeats", repeats, "jump_rounds", rounds)
        assert d == wd and int(ng) == wng
    if env == "RK_SWEEP_BLIND=1":
        assert int(lines[1][2]) == 1


def test_one_context_three_calls(gpu_ctx):
    """A large set, a smaller one, the large one again: the parents of the
    later calls start out as the earlier call's flagged words."""
    f, lx, ly = dc.crafted_sizes()
    g, gx, gy = dc.crafted_sizes(dc.SIZES[:26])
    assert g.n < f.n
    same(gpu_ctx.classify(f, lx, ly), oracle("sizes", f, lx, ly))
    same(gpu_ctx.classify(g, gx, gy), oracle("sizes26", g, gx, gy))
    same(gpu_ctx.classify(f, lx, ly), oracle("sizes", f, lx, ly))


def test_three_ratio_pairs(gpu_ctx):
    """The second and third pairs sweep over the first pair's flagged words."""
    g = rk.synth(30_000, 1_000_000, seed=12)
    pairs = [(0.3, 0.3), (0.05, 0.05), (0.6, 0.2)]
    want = [oracle("synth30k", g, 1_000_000, 1_000_000, lr, pr) for lr, pr in pairs]
    assert len({w[3] for w in want}) == 3  # three different results
    for r, w in zip(gpu_ctx.classify_pairs(g, 1_000_000, 1_000_000, pairs), want):
        same(r, w)


def test_batch_of_three_sets(gpu_ctx):
    sets = [singletons(5), dc.crafted_sizes(dc.SIZES[:12]), dc.crafted(dc.group_keys([300, 7]))]
    want = bc.oracle_sets(sets)
    assert [w[4] for w in want] == [5, 24, 4]
    bc.assert_matches(gpu_ctx.classify_batch(sets), want)
