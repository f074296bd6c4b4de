"""Crafted fragment sets with chosen group sizes (tests/test_direct_emit.py).

Group j is n_j copies of one fragment (xStart 5000 + 100000 j, length 200,
strand f) at yStart Y_j + key: every copy hits the first on X, so they form
one group whose in-group sort keys are the given ones.  One more fragment of
the same xStart with length 5000 at Y_j follows: a group of its own, which
sets the bucket's diagonal to Y_j (the recipe of
test_killer_group_heap_segment_vs_oracle, once per group).
"""
import numpy as np

import repkiller_amd as rk

SIZES = [1, 2, 3, 4, 5, 15, 16, 17, 18, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511,
         512, 513, 2047, 2048, 2049, 5000, 1, 1, 2]
Y_STEP = 4_000_000  # above every key (20-bit random, or a killer's n + span)


def group_keys(sizes, seed=5):
    """Keys alternate between heavy ties (0..3) and 20-bit random."""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 4 if j % 2 == 0 else 1 << 20, n).astype(np.uint64)
            for j, n in enumerate(sizes)]


def crafted(keys, tail=None, interleave_seed=None):
    """keys: one array per group.  tail[j] False: no length-5000 fragment after
    group j.  interleave_seed: the rows of different buckets interleaved, the
    order inside a bucket kept.  Returns (Frags, len_x, len_y)."""
    xs, ys, ls, gs = [], [], [], []
    for j, k in enumerate(keys):
        t = 1 if tail is None or tail[j] else 0
        x0, y0 = 5000 + 100_000 * j, 1_000_000 + Y_STEP * j
        xs.append(np.full(k.size + t, x0, np.uint64))
        ys.append(np.r_[y0 + k, np.full(t, y0)].astype(np.uint64))
        ls.append(np.r_[np.full(k.size, 200), np.full(t, 5000)].astype(np.uint64))
        gs.append(np.full(k.size + t, j))
    x, y, ln, g = (np.concatenate(a) for a in (xs, ys, ls, gs))
    if interleave_seed is not None:
        lab = np.random.default_rng(interleave_seed).permutation(g)
        idx = np.empty(g.size, np.int64)
        for j in range(len(keys)):
            idx[lab == j] = np.flatnonzero(g == j)
        x, y, ln = x[idx], y[idx], ln[idx]
    f = rk.Frags(x, y, ln, np.full(x.size, ord("f"), np.uint8))
    return f, 100_000 * (len(keys) + 1), Y_STEP * (len(keys) + 1)


def crafted_sizes(sizes=SIZES, **kw):
    return crafted(group_keys(sizes), **kw)


def group_sizes(gid):
    """Sizes of the groups in output order (gid is group-major)."""
    cut = np.flatnonzero(np.r_[True, gid[1:] != gid[:-1], True])
    return np.diff(cut)
