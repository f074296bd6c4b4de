"""The segment kernels (k_seg_fine / k_seg_big) on crafted segment shapes.

A split sort hands every coarse key's records (a segment) to one block, which
splits them evenly over its waves: nit = ceil(size / T) items per lane, T the
block's threads, up to cap = 8 T records in LDS; larger segments go through
global memory (k_seg_big).  The inputs here place an exact number of rows in
chosen coarse keys of the processing order (xStart / 10) and, independently,
of the Y axis (strand * nby + centre / 100):

  sizes   1, 63, 64, 65; k T - 1, k T, k T + 1 for k = 1..7 (every nit
          boundary; spread over the three cases); cap - 1, cap, cap + 1 (the
          last one is k_seg_big's); empty segments between the groups; the
          remaining rows fill the segments left over (whatever size results,
          above cap where few are left)
  equal   a segment whose fine keys are all equal, below cap (700 rows) and
          above it (cap + 500 rows: k_seg_big's already-sorted shortcut); the
          file order is shuffled, so stability shows
  F       nw_order_split picks the largest F with n 2^F <= target nkeys,
          target = 3/4 cap.  With nkeys = nseg 2^F key values and n = 64,000
          rows over nseg = 32 * 4096 / cap segments, n <= target nseg = 98,304
          and 2 n > 98,304, so that F is the plan's for either capacity
          (checked by `plan_f`, the rule restated): F = 8 (one fine round),
          F = 9 (the second round a single bit), F = 15 (two full-width
          rounds: 8 + 7 bits), each on both axes.

Both strands occur on both axes (the Y key's upper half is the reverse
strand).  Everything is compared bit for bit with the oracle.
"""
import functools

import numpy as np
import pytest

from oracle import rk_oracle as ro

import repkiller_amd as rk

# the kernels' LDS capacities (rk_internal.h: NW_SEG_CAP_ORDER, NW_SEG_CAP_Y)
CAP_ORDER = 4096
CAP_Y = 2048
N_ROWS = 64_000
# (Fx, Fy) of the three cases
CASES = {"f8_f9": (8, 9), "f9_f15": (9, 15), "f15_f8": (15, 8)}


def plan_f(n, nkeys, cap):
    """nw_order_split's rule: (F, C), or None where it declines the split."""
    target = cap * 3 // 4
    b = (nkeys - 1).bit_length()
    f = 0
    while f < b and n * (2 << f) <= target * nkeys:
        f += 1
    c = b - f
    if f < 1 or c < 1 or c > 24 or (1 << c) + 1 > n // 256 + 64:  # nw_seg_words(n)
        return None
    return f, c


def segment_sizes(cap, case_no, nseg, n):
    """(size, equal-keys?) per coarse key 0..nseg-1, summing to n."""
    t = cap // 8
    groups = [[1, 63, 64, 65]]
    groups += [[k * t - 1, k * t, k * t + 1] for k in range(1, 8) if k % 3 == case_no]
    groups += [[cap - 1, cap, cap + 1]]
    segs = []
    for g in groups:
        segs += [(s, False) for s in g] + [(0, False)]  # an empty segment after each group
    segs += [(700, True), (0, False), (cap + 500, True)]
    free = nseg - len(segs)
    fill = n - sum(s for s, _ in segs)
    assert free >= 2 and fill > 0, (free, fill)
    per = -(-fill // free)
    while fill > 0:
        segs.append((min(per, fill), False))
        fill -= min(per, fill)
    segs += [(0, False)] * (nseg - len(segs))
    assert len(segs) == nseg and sum(s for s, _ in segs) == n
    return segs


def axis_keys(rng, segs, f, margin):
    """One key per row, segment by segment: coarse key j, fine keys random in
    [2, 2^F - margin) (clear of the axis' ends), or all 5 for an equal segment."""
    out = []
    for j, (size, equal) in enumerate(segs):
        fine = (np.full(size, 5) if equal else rng.integers(2, (1 << f) - margin, size))
        out.append((j << f) + fine)
    return np.concatenate(out).astype(np.int64)


@functools.lru_cache(maxsize=None)
def case_input(name):
    """(frags, lx, ly, sizes of the order segments, sizes of the Y segments)"""
    fx, fy = CASES[name]
    no = sorted(CASES).index(name)
    rng = np.random.default_rng(7100 + no)
    n = N_ROWS
    nsx, nsy = 32 * 4096 // CAP_ORDER, 32 * 4096 // CAP_Y
    nkx, nky = nsx << fx, nsy << fy
    assert plan_f(n, nkx, CAP_ORDER) == (fx, nsx.bit_length() - 1)
    assert plan_f(n, nky, CAP_Y) == (fy, nsy.bit_length() - 1)
    # vsize = 1 + (lx + 1) / 10 = nkx; 2 nby = 2 ((ly + 1) / 100 + 1) = nky
    lx, ly = 10 * (nkx - 1) - 1, 100 * (nky // 2 - 1) - 1
    nby = nky // 2
    length = rng.integers(20, 200, n)
    xkey = axis_keys(rng, segment_sizes(CAP_ORDER, no, nsx, n), fx, 42)
    ykey = axis_keys(rng, segment_sizes(CAP_Y, no, nsy, n), fy, 3)
    rng.shuffle(ykey)  # the Y segments are independent of the order segments
    rev = ykey >= nby
    centre = (ykey - rev * nby) * 100 + rng.integers(0, 100, n)
    x = xkey * 10 + rng.integers(0, 10, n)
    y = centre - length // 2
    assert y.min() >= 0 and (y + length).max() <= ly and (x + length).max() <= lx
    rows = rng.permutation(n)  # file order: shuffled
    f = rk.Frags(x[rows].astype(np.uint64), y[rows].astype(np.uint64),
                 length[rows].astype(np.uint64),
                 np.where(rev[rows], ord("r"), ord("f")).astype(np.uint8))
    sx = np.bincount(f.x_start.astype(np.int64) // 10 >> fx, minlength=nsx)
    yk = (f.y_start.astype(np.int64) + f.length.astype(np.int64) // 2) // 100 + rev[rows] * nby
    sy = np.bincount(yk >> fy, minlength=nsy)
    return f, lx, ly, sx, sy


@functools.lru_cache(maxsize=None)
def case_oracle(name):
    f, lx, ly, _, _ = case_input(name)
    return ro.classify(f.x_start, f.y_start, f.length, f.strand, lx, ly, 0.3, 0.3)


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_hold_the_shapes_and_the_oracle_takes_them(name):
    """No GPU: the crafted inputs hold the segment sizes they are meant to on
    both axes, both strands, and the oracle classifies them."""
    f, _, _, sx, sy = case_input(name)
    no = sorted(CASES).index(name)
    for cap, got in ((CAP_ORDER, sx), (CAP_Y, sy)):
        t = cap // 8
        want = {1, 63, 64, 65, cap - 1, cap, cap + 1, 700, cap + 500, 0}
        want |= {k * t + d for k in range(1, 8) if k % 3 == no for d in (-1, 0, 1)}
        assert want <= set(got.tolist()), sorted(want - set(got.tolist()))
    assert {ord("f"), ord("r")} == set(f.strand.tolist())
    rc, gid, rep, order, ng = case_oracle(name)
    assert rc == 0 and ng > 0 and len(order) == len(gid) == len(rep)


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(CASES))
def test_segment_shapes_vs_oracle(gpu_ctx, name):
    f, lx, ly, _, _ = case_input(name)
    got = gpu_ctx.classify(f, lx, ly, 0.3, 0.3)
    st = gpu_ctx.stats()
    assert st["pipeline"] == 1 and st["record_fallback"] == 0
    rc, gid, rep, order, ng = case_oracle(name)
    assert rc == 0 and got.n_groups == ng
    assert np.array_equal(got.out_order, order)
    assert np.array_equal(got.gid, gid)
    assert np.array_equal(got.repval, rep)
