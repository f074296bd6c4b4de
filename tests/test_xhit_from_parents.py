"""The X-hit bits come from the parent words: after a closed X axis fragment k
hit on X exactly when par[k] != k, so the Y sort's bitmask (k_nw_x_bits) and
the sharded drivers' own X results (k_sh_x_own, k_sh_x_own_fast) read the
parents and the fragments' X positions are no longer kept.  Every result is
compared with the oracle bit for bit (out_order, gid, repval, group count).
"""
import os
import subprocess

import numpy as np
import pytest

import xhit_cases as xc
from conftest import ROOT

import repkiller_amd as rk


# ---- CPU: the inputs hold joiners and singletons on both strands ---------------
@pytest.mark.parametrize("case", [xc.edge_case(m) for m in xc.WORD_EDGES if m >= 31]
                         + [xc.BIG, xc.SMALL, xc.DENSE], ids=lambda c: f"n{c['n']}")
def test_inputs_have_hits_and_misses(case):
    gid, _, order, ng = xc.oracle(case)
    assert len(gid) == case["n"] == len(order)  # every row is kept
    sizes = np.bincount(gid)
    assert len(sizes) == ng
    assert (sizes > 1).any() and (sizes == 1).any()
    for strand, (joined, alone) in xc.joiners_and_singletons(case).items():
        assert joined > 0 and alone > 0, strand


def test_ratio_pairs_differ():
    tight, loose = xc.oracle(xc.BIG, 0.05, 0.05), xc.oracle(xc.BIG, 0.3, 0.3)
    assert tight[3] != loose[3]
    assert not np.array_equal(tight[0], loose[0])


# ---- GPU ------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("m", xc.WORD_EDGES)
def test_bitmask_word_edges(gpu_ctx, m):
    """The partial last word, the wave whose lanes 32..63 hold no row, the
    16-byte loads' tail, one load row and one tile of the bitmask kernel on
    both sides."""
    case = xc.edge_case(m)
    f, lx, ly = xc.frags(case)
    xc.same(gpu_ctx.classify(f, lx, ly), xc.oracle(case))
    s = gpu_ctx.stats()
    assert s["pipeline"] == 1 and s["n_proc"] == m


@pytest.mark.gpu
def test_stale_parent_words():
    """One context: the 64,000-row call leaves its roots' flagged ranks in the
    parent words, the smaller and different set after it must not see them."""
    ctx = rk.Context(0)
    try:
        for case in (xc.BIG, xc.SMALL, xc.edge_case(65), xc.BIG):
            f, lx, ly = xc.frags(case)
            xc.same(ctx.classify(f, lx, ly), xc.oracle(case))
            assert ctx.stats()["pipeline"] == 1
    finally:
        ctx.close()


@pytest.mark.gpu
def test_several_ratio_pairs(gpu_ctx):
    """Later pairs keep the Y CSR and take their Y states from the new bits
    (k_nw_fill_y), over the parent words the pair before left behind."""
    pairs = [(0.05, 0.05), (0.3, 0.3), (0.05, 0.05), (0.6, 0.2)]
    f, lx, ly = xc.frags(xc.BIG)
    got = gpu_ctx.classify_pairs(f, lx, ly, pairs)
    assert len(got) == len(pairs)
    for r, (lr, pr) in zip(got, pairs):
        xc.same(r, xc.oracle(xc.BIG, lr, pr))


_CHILD = r"""
import os, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import repkiller_amd as rk
import xhit_cases as xc
ctx = rk.Context(0)
f, lx, ly = xc.frags(xc.BIG)
r = ctx.classify(f, lx, ly)
s = ctx.stats()
print(xc.digest_arrays(r.out_order, r.gid, r.repval), r.n_groups, s["sweep_repeats"], s["pipeline"])
"""

_DEFAULT = {}


def default_digest(ctx):
    """The default schedule's result on the 64,000-row set: equal to the
    oracle, then kept as a digest."""
    if not _DEFAULT:
        f, lx, ly = xc.frags(xc.BIG)
        r = ctx.classify(f, lx, ly)
        xc.same(r, xc.oracle(xc.BIG))
        assert ctx.stats()["sweep_repeats"] == 0
        _DEFAULT["d"] = (xc.digest_arrays(r.out_order, r.gid, r.repval), r.n_groups)
    return _DEFAULT["d"]


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["RK_Y_OVERLAP=1", "RK_NW_YSPLIT=0", "RK_SWEEP_QUEUED=0",
                                 "RK_ROOTS_FUSED=0", "RK_SWEEP_BLIND=1"])
def test_schedules_that_consume_the_bits(gpu_ctx, env):
    """The Y sort's last pass looking the bits up, the one-stage Y sort, the
    sweeps with readbacks, the round-by-round roots (parent words left
    unflagged), and an attempt that ends with an open axis -- stale parent
    words, arbitrary bits -- and is repeated.  A switch is read once per
    process, so each runs in a child process."""
    want, wng = default_digest(gpu_ctx)
    k, v = env.split("=")
    out = subprocess.run(["python", "-c", _CHILD, str(ROOT)], capture_output=True, text=True,
                         timeout=120, env={**os.environ, k: v})
    assert out.returncode == 0, out.stderr[-2000:]
    d, ng, repeats, pipeline = out.stdout.strip().split()
    print(env, "sweep_repeats", repeats)
    assert d == want and int(ng) == wng and int(pipeline) == 1
    # one queued sweep an axis leaves this set open: the attempt is repeated
    assert int(repeats) == (1 if env == "RK_SWEEP_BLIND=1" else 0)


@pytest.mark.gpu
@pytest.mark.parametrize("driver", ["fast", "careful"])
@pytest.mark.parametrize("world", [1, 2, 3])
def test_sharded(world, driver):
    """The sharded record drivers on one device: the fast path (at one rank the
    bitmask kernel over the shared parent words, else k_sh_x_own_fast) and the
    careful driver (k_sh_x_own; the dense set without lead-in makes it resolve
    X again over a selected halo), halo entries included."""
    import test_sharded as ts
    cases = [dict(xc.BIG, repeat=2), xc.DENSE, xc.edge_case(65)]
    got = ts.run_ranks(world, cases, env={"RK_SH_FAST": "0"} if driver == "careful" else None)
    for ci, case in enumerate(cases):
        order, gid, rep, ng, stats = ts.assemble(got, ci, world)
        wgid, wrep, worder, wng = xc.oracle(case)
        assert ng == wng, case
        assert np.array_equal(order, worder), case
        assert np.array_equal(gid, wgid) and np.array_equal(rep, wrep), case
        for st in stats:
            assert all(c["generic_driver"] == 0 for c in st["calls"]), st
            if driver == "careful":
                assert all(c["fast_path"] == 0 for c in st["calls"]), st
    if driver == "fast":
        big = ts.assemble(got, 0, world)[4]
        assert all(c["fast_path"] == 1 and c["fast_retry"] == 0 for st in big
                   for c in st["calls"]), big
