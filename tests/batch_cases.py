"""Fragment sets for the batched-classification tests and the translation model
(shared by tests/test_batch_layout.py and tests/test_batch.py).  Every expected
value comes from oracle.rk_oracle.classify, one set at a time."""
import numpy as np

from oracle import rk_oracle as ro

import repkiller_amd as rk


def geom(hdr):
    """(vsize, max_index) of a raw header length (FragmentsDatabase.cpp:62,84)."""
    ln = hdr + 1
    return 1 + ln // 10, ln // 100


def random_set(rng, n, hx, hy, last_bucket=0, avoid_edges=False, all_dropped=False):
    """n valid rows (both strands, lengths 10-59) + `last_bucket` rows of the
    never-iterated last xStart/10 bucket, shuffled.  avoid_edges: no centre of
    remainder 98 / 99 on either axis (the only rows translation cannot place)."""
    ln = rng.integers(10, 60, n)
    x = rng.integers(0, hx + 1 - 64, n)
    y = rng.integers(0, hy + 1 - 64, n)
    if avoid_edges:
        x += np.where((x + ln // 2) % 100 >= 98, 2, 0)
        y += np.where((y + ln // 2) % 100 >= 98, 2, 0)
    vsize, _ = geom(hx)
    if all_dropped:
        last_bucket, n = max(last_bucket, 3), 0
        x, y, ln = x[:0], y[:0], ln[:0]
    xl = 10 * (vsize - 1) + rng.integers(0, 10, last_bucket)
    x = np.concatenate([x, xl])
    y = np.concatenate([y, rng.integers(0, 10 * hy + 1000, last_bucket)])  # never validated
    ln = np.concatenate([ln, rng.integers(10, 5000, last_bucket)])
    s = np.where(rng.random(x.shape[0]) < 0.5, ord("f"), ord("r")).astype(np.uint8)
    p = rng.permutation(x.shape[0])
    return rk.Frags(x[p].astype(np.uint64), y[p].astype(np.uint64), ln[p].astype(np.uint64), s[p])


def random_sets(seed, nsets, max_rows=600, avoid_edges=False, hdr=(300, 9000)):
    """[(Frags, len_x_hdr, len_y_hdr)]: some sets empty, some with last-bucket
    rows, one dropped entirely."""
    rng = np.random.default_rng(seed)
    sets = []
    gone = int(rng.integers(0, nsets)) if nsets > 2 else -1
    for k in range(nsets):
        hx, hy = (int(v) for v in rng.integers(hdr[0], hdr[1] + 1, 2))
        n = 0 if rng.random() < 0.1 else int(rng.integers(0, max_rows + 1))
        lb = int(rng.integers(1, 6)) if rng.random() < 0.4 else 0
        sets.append((random_set(rng, n, hx, hy, lb, avoid_edges, all_dropped=k == gone), hx, hy))
    return sets


def frags(rows, strand):
    a = np.array(rows, np.uint64).reshape(-1, 3)
    return rk.Frags(a[:, 0].copy(), a[:, 1].copy(), a[:, 2].copy(),
                    np.full(a.shape[0], ord(strand), np.uint8))


# the upward-probe guards (SequenceOcupationList.cpp:58,80): the second row
# joins the first's group only when its centre (99 or 98) is below max_index
# (max_index - 1) -- header 9999 (max_index 100), not 9998 (max_index 99)
BIG = 20000


def guard_pairs():
    """{name: (rows, strand, axis the threshold header is on)}"""
    return {
        "x99": (frags([(90, 1000, 20), (91, 5000, 16)], "f"), "x"),
        "x98": (frags([(90, 1000, 20), (90, 5000, 16)], "f"), "x"),
        "y99": (frags([(1000, 90, 20), (5000, 91, 16)], "r"), "y"),
    }


def guard_set(name, hdr):
    f, axis = guard_pairs()[name]
    return (f, hdr, BIG) if axis == "x" else (f, BIG, hdr)


def oracle_set(f, hx, hy, lr=0.3, pr=0.3):
    """(rc, gid, repval, out_order, n_groups) of one set alone."""
    return ro.classify(f.x_start, f.y_start, f.length, f.strand, hx, hy, lr, pr)


def oracle_sets(sets, lr=0.3, pr=0.3):
    return [oracle_set(f, hx, hy, lr, pr) for f, hx, hy in sets]


def assert_matches(results, expected):
    assert len(results) == len(expected)
    for k, (got, (rc, gid, rep, order, ng)) in enumerate(zip(results, expected)):
        assert rc == 0, k
        assert got.n_groups == ng, (k, got.n_groups, ng)
        assert np.array_equal(got.out_order, order), k
        assert np.array_equal(got.gid, gid), k
        assert np.array_equal(got.repval, rep), k


def translation_model(sets, base_x, base_y, lr=0.3, pr=0.3):
    """The batch as the library lays it out, classified by the oracle WITHOUT the
    per-set probe guards: translate every set by its bases, send the rows of its
    dropped last bucket to the combined set's own last bucket, classify, split.
    Returns [(gid, repval, out_order, n_groups)] per set."""
    xs, ys, ls, ss, owner = [], [], [], [], []
    for k, (f, hx, hy) in enumerate(sets):
        vsize, _ = geom(hx)
        drop = f.x_start // np.uint64(10) >= np.uint64(vsize - 1)
        xs.append(np.where(drop, base_x[-1], f.x_start + base_x[k]))
        ys.append(np.where(drop, 0, f.y_start + base_y[k]))
        ls.append(np.where(drop, 0, f.length))
        ss.append(f.strand)
        owner.append(np.full(f.n, k))
    x, y, ln, s, owner = (np.concatenate(a) for a in (xs, ys, ls, ss, owner))
    off = np.concatenate([[0], np.cumsum([f.n for f, _, _ in sets])])
    rc, gid, rep, order, ng = ro.classify(x.astype(np.uint64), y.astype(np.uint64),
                                          ln.astype(np.uint64), s, int(base_x[-1]) - 1,
                                          int(base_y[-1]) - 1, lr, pr)
    assert rc == 0
    own = owner[order]
    assert np.all(np.diff(own) >= 0), "a set's output rows are not one contiguous range"
    out = []
    for k in range(len(sets)):
        sel = own == k
        g = gid[sel]
        if g.size:
            assert np.all(np.diff(g.astype(np.int64)) >= 0)
        out.append(((g - g[0]) if g.size else g, rep[sel], order[sel] - np.uint32(off[k]),
                    int(g[-1] - g[0] + 1) if g.size else 0))
    return out
