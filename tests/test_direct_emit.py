"""The record pipeline's direct emit: the group ids go straight to the caller's
array, the pass that finds the group starts writes the repeat flags and the
singletons' rows, the group-sort tiers up to 2048 members store file rows, and
only larger groups' rows follow from the sorted tags.  Crafted sets put a group
on every side of every tier bound (direct_emit_cases.py); every result is
compared with the oracle bit for bit.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

import direct_emit_cases as dc
from conftest import ROOT
from oracle import rk_oracle as ro
from sort_cases import heap_fallbacks, killer_with_keys

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


@pytest.mark.parametrize("interleave", [None, 9], ids=["as_built", "interleaved"])
def test_every_tier_bound(pctx, interleave):
    """Groups of 1 .. 5000 members around every tier bound, each followed by a
    singleton: 62 groups over 14,236 rows."""
    f, lx, ly = dc.crafted_sizes(interleave_seed=interleave)
    want = oracle(("sizes", interleave), f, lx, ly)
    assert f.n == 14_236 and want[3] == 62
    assert sorted(dc.group_sizes(want[0])) == sorted(dc.SIZES + [1] * len(dc.SIZES))
    same(pctx.classify(f, lx, ly), want)


@pytest.mark.parametrize("ngroups,rem", [(31, 0), (30, 1), (26, 2), (29, 3)])
def test_totals_mod_four(gpu_ctx, ngroups, rem):
    """The four-positions-per-thread pass with every remainder of m."""
    f, lx, ly = dc.crafted_sizes(dc.SIZES[:ngroups])
    assert f.n % 4 == rem
    same(gpu_ctx.classify(f, lx, ly), oracle(("mod4", ngroups), f, lx, ly))


def test_first_and_last_groups_with_several_members(gpu_ctx):
    f, lx, ly = dc.crafted(dc.group_keys([5, 1, 17, 40]), tail=[True, True, True, False])
    want = oracle("several", f, lx, ly)
    sizes = dc.group_sizes(want[0])
    assert sizes[0] == 5 and sizes[-1] == 40
    same(gpu_ctx.classify(f, lx, ly), want)


def test_first_and_last_groups_singletons(gpu_ctx):
    f, lx, ly = dc.crafted(dc.group_keys([1, 5, 40, 1]))
    want = oracle("singles", f, lx, ly)
    sizes = dc.group_sizes(want[0])
    assert sizes[0] == 1 and sizes[-1] == 1
    same(gpu_ctx.classify(f, lx, ly), want)


@pytest.mark.parametrize("sizes,tail,m", [([1], False, 1), ([1], True, 2), ([2], False, 2)],
                         ids=["m1", "m2_two_groups", "m2_one_group"])
def test_one_and_two_members(pctx, sizes, tail, m):
    f, lx, ly = dc.crafted(dc.group_keys(sizes), tail=[tail])
    assert f.n == m
    same(pctx.classify(f, lx, ly), oracle(("tiny", tuple(sizes), tail), f, lx, ly))


def test_outputs_off_alignment(gpu_ctx):
    """classify_device with the three outputs one element into their buffers:
    the gid and order arrays 4 B off a 16-B boundary, the flags 1 B off."""
    import torch
    f, lx, ly = dc.crafted_sizes()
    gid_w, rep_w, order_w, ng_w = oracle(("sizes", None), f, lx, ly)
    dev = torch.device("cuda", 0)
    cols = [torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).to(dev)
            for a in (f.x_start, f.y_start, f.length, f.strand)]
    n = f.n
    gid = torch.empty(n + 1, dtype=torch.int32, device=dev)[1:]
    rep = torch.empty(n + 1, dtype=torch.uint8, device=dev)[1:]
    order = torch.empty(n + 1, dtype=torch.int32, device=dev)[1:]
    assert gid.data_ptr() % 16 == 4 and order.data_ptr() % 16 == 4 and rep.data_ptr() % 4 == 1
    n_out, ng = gpu_ctx.classify_device(*cols, gid, rep, order, lx, ly)
    assert (n_out, ng) == (gid_w.size, ng_w)
    assert np.array_equal(gid.cpu().numpy().view(np.uint32), gid_w)
    assert np.array_equal(rep.cpu().numpy(), rep_w)
    assert np.array_equal(order.cpu().numpy().view(np.uint32), order_w)


def test_two_ratio_pairs_keep_their_own_arrays(gpu_ctx):
    """Two different ratio pairs in one call, each against the oracle: on the
    crafted set, and on a synthetic one where the two results differ."""
    f, lx, ly = dc.crafted_sizes()
    pairs = [(0.3, 0.3), (0.05, 0.05)]
    for r, (lr, pr) in zip(gpu_ctx.classify_pairs(f, lx, ly, pairs), pairs):
        same(r, oracle(("sizes", None), f, lx, ly, lr, pr))
    g = rk.synth(30_000, 1_000_000, seed=12)
    res = gpu_ctx.classify_pairs(g, 1_000_000, 1_000_000, pairs)
    want = [oracle("synth30k", g, 1_000_000, 1_000_000, lr, pr) for lr, pr in pairs]
    assert not np.array_equal(want[0][0], want[1][0])
    for r, w in zip(res, want):
        same(r, w)


def _with_killer():
    k = killer_with_keys(20000, 3, 31)
    assert heap_fallbacks(k) > 0
    return dc.crafted(dc.group_keys(dc.SIZES) + [k])


def test_small_groups_direct_large_group_through_tags():
    """The crafted set and a 20,000-member median-of-three killer group in one
    call: the small groups' rows come from the tiers, the killer group's from
    its sorted tags -- after the heap segments, which a single pair sorts once
    its final status word is back, and two pairs inside each pair's sort."""
    f, lx, ly = _with_killer()
    want = oracle("killer", f, lx, ly)
    assert dc.group_sizes(want[0]).max() == 20000
    ctx = rk.Context(0)  # (its own: the larger workspace is freed with it)
    try:
        same(ctx.classify(f, lx, ly), want)
        for r in ctx.classify_pairs(f, lx, ly, [(0.3, 0.3), (0.3, 0.3)]):
            same(r, want)
    finally:
        ctx.close()


def test_context_reused_with_a_smaller_set(gpu_ctx):
    f, lx, ly = dc.crafted_sizes()
    same(gpu_ctx.classify(f, lx, ly), oracle(("sizes", None), f, lx, ly))
    g, gx, gy = dc.crafted_sizes(dc.SIZES[:26])
    same(gpu_ctx.classify(g, gx, gy), oracle(("mod4", 26), g, gx, gy))


_SWITCH_SCRIPT = r"""
import hashlib, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import repkiller_amd as rk
import direct_emit_cases as dc
ctx = rk.Context(0)
f, lx, ly = dc.crafted_sizes()
g = rk.synth(400_000, 40_000_000, seed=47, family_frac=0.95, copies=(100, 600))
for r in (ctx.classify(f, lx, ly), ctx.classify(g, 40_000_000, 40_000_000)):
    h = hashlib.sha256()
    for a in (r.out_order, r.gid, r.repval):
        h.update(np.ascontiguousarray(a).tobytes())
    print(h.hexdigest(), r.n_groups)
"""


def test_switch_restores_the_emit_pass(gpu_ctx):
    """RK_EMIT_DIRECT=0 (tags in every tier, then the emit pass over all
    members) gives the default's result; the switch is read once per process,
    so the variant runs in a child process."""
    f, lx, ly = dc.crafted_sizes()
    g = rk.synth(400_000, 40_000_000, seed=47, family_frac=0.95, copies=(100, 600))
    want = [gpu_ctx.classify(f, lx, ly), gpu_ctx.classify(g, 40_000_000, 40_000_000)]
    same(want[0], oracle(("sizes", None), f, lx, ly))
    out = subprocess.run(["python", "-c", _SWITCH_SCRIPT, str(ROOT)], capture_output=True,
                         text=True, timeout=120, env={**os.environ, "RK_EMIT_DIRECT": "0"})
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.split("\n")
    for r, line in zip(want, lines):
        d, ng = line.split()
        assert d == digest(r) and int(ng) == r.n_groups
