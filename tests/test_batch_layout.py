"""rk_batch_layout and the translation it stands for, on the CPU: a batch laid
out by the library's bases and classified as ONE set by the oracle restatement
splits into exactly the per-set oracle results -- except for the upward-probe
guards, which the device corrects per set (tests/test_batch.py)."""
import numpy as np
import pytest

import batch_cases as bc

import repkiller_amd as rk


def test_layout_properties():
    rng = np.random.default_rng(5)
    lx = rng.integers(0, 200_000, 300).astype(np.uint64)
    ly = rng.integers(0, 200_000, 300).astype(np.uint64)
    lx[:6] = [0, 8, 9, 98, 99, 100]
    ly[:6] = [100, 99, 98, 9, 8, 0]
    bx, by = rk.batch_layout(lx, ly)
    assert bx.shape == by.shape == (301,)
    assert bx[0] == 0 and by[0] == 0
    assert np.all(bx % 100 == 0) and np.all(by % 100 == 0)
    for k in range(300):
        vsize, mi_x = bc.geom(int(lx[k]))
        _, mi_y = bc.geom(int(ly[k]))
        wx, wy = int(bx[k + 1] - bx[k]), int(by[k + 1] - by[k])
        # disjoint windows that hold every admissible xStart and centre bucket
        # 0..max_index, with an empty 100-bucket above them
        assert wx > 0 and wy > 0
        assert 10 * vsize - 1 < wx - 100
        assert 100 * mi_x + 99 < wx - 100
        assert 100 * mi_y + 99 < wy - 100
    # the combined headers make the combined last xStart/10 bucket the trash bucket
    vsize_all, _ = bc.geom(int(bx[-1]) - 1)
    assert vsize_all - 1 == int(bx[-1]) // 10


def test_layout_rejects_overflow():
    with pytest.raises(rk.RkError) as e:
        rk.batch_layout([2**64 - 2] * 4, [10] * 4)
    assert e.value.code == -1


@pytest.mark.parametrize("trial", range(8))
def test_translation_model_matches_per_set_oracle(trial):
    rng = np.random.default_rng(100 + trial)
    sets = bc.random_sets(1000 + trial, int(rng.integers(1, 9)), avoid_edges=True)
    bx, by = rk.batch_layout([s[1] for s in sets], [s[2] for s in sets])
    got = bc.translation_model(sets, bx, by)
    for (gid, rep, order, ng), (rc, egid, erep, eorder, eng) in zip(got, bc.oracle_sets(sets)):
        assert rc == 0
        assert ng == eng
        assert np.array_equal(order, eorder)
        assert np.array_equal(gid, egid)
        assert np.array_equal(rep, erep)


@pytest.mark.parametrize("name", sorted(bc.guard_pairs()))
def test_guard_pairs_depend_on_their_own_header(name):
    """What keeps the GPU probe-guard test meaningful: the pairs flip between 2
    groups and 1 with their own header, and the translation model WITHOUT the
    per-set guards gets the mixed batch wrong."""
    hdrs = [9998, 9999, 9998, 9999]
    sets = [bc.guard_set(name, h) for h in hdrs]
    want = [bc.oracle_set(*s)[4] for s in sets]
    assert want == [2, 1, 2, 1]
    bx, by = rk.batch_layout([s[1] for s in sets], [s[2] for s in sets])
    naive = [r[3] for r in bc.translation_model(sets, bx, by)]
    assert naive != want
