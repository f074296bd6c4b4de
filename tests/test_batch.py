"""rk_classify_batch / rk_classify_device_batch on the GPU: every set's result
equals oracle.rk_oracle.classify of that set alone (or the reference's golden
CSV bytes)."""
import json
import os
import subprocess

import numpy as np
import pytest

import batch_cases as bc
from conftest import EDGE
from long_runs import long_run_set

import repkiller_amd as rk

pytestmark = pytest.mark.gpu

RATIOS = [(0.3, 0.3), (0.05, 0.05), (1.5, 0.7)]


@pytest.fixture(scope="module")
def mix():
    """40 random sets and their per-set oracle results for every ratio pair."""
    sets = bc.random_sets(7, 40)
    assert any(f.n == 0 for f, _, _ in sets)
    return sets, {r: bc.oracle_sets(sets, *r) for r in RATIOS}


@pytest.mark.parametrize("lr,pr", RATIOS)
def test_random_mix(gpu_ctx, mix, lr, pr):
    sets, want = mix
    bc.assert_matches(gpu_ctx.classify_batch(sets, lr, pr), want[(lr, pr)])
    st = gpu_ctx.batch_stats()
    assert st["sub_batches"] == 1 and st["batched_sets"] == 40 and st["looped_sets"] == 0


def guard_arrangements(name):
    four = [bc.guard_set(name, h) for h in (9998, 9999, 9998, 9999)]
    rng = np.random.default_rng(3)
    big = (bc.random_set(rng, 5000, 9000, 9000), 9000, 9000)
    return {"mixed": four, "reversed": four[::-1], "behind": [big] + four, "before": four + [big]}


@pytest.mark.parametrize("arr", ["mixed", "reversed", "behind", "before"])
@pytest.mark.parametrize("name", sorted(bc.guard_pairs()))
def test_probe_guards(gpu_ctx, name, arr):
    sets = guard_arrangements(name)[arr]
    want = bc.oracle_sets(sets)
    groups = [w[4] for w in want if w[1].shape[0] == 2]
    assert sorted(groups) == [1, 1, 2, 2]  # (the pairs do flip with their own header)
    bc.assert_matches(gpu_ctx.classify_batch(sets), want)
    assert gpu_ctx.batch_stats()["batched_sets"] == len(sets)


@pytest.mark.parametrize("c_low", [0, 1])
@pytest.mark.parametrize("strand", ["f", "r"])
def test_window_isolation(gpu_ctx, c_low, strand):
    """A centre in a set's top bucket and a centre at 0 / 1 of the next set are
    neighbours only in the combined space: they must not be grouped."""
    hdr = 999  # max_index 10: centre bucket 10 is the top one
    top = bc.frags([(999, 999, 2)], strand)       # centre 1000 on both axes
    low = bc.frags([(0, 0, 1 + c_low)], strand)   # centre 0 (length 1) or 1 (length 2)
    sets = [(top, hdr, hdr), (low, hdr, hdr)]
    want = bc.oracle_sets(sets, 1.5, 1.5)
    assert [w[4] for w in want] == [1, 1]
    bc.assert_matches(gpu_ctx.classify_batch(sets, 1.5, 1.5), want)
    assert gpu_ctx.batch_stats()["batched_sets"] == 2


def test_many_tiny_sets(gpu_ctx):
    sets = bc.random_sets(11, 3000, max_rows=8, hdr=(199, 400))
    bc.assert_matches(gpu_ctx.classify_batch(sets), bc.oracle_sets(sets))
    assert gpu_ctx.batch_stats()["batched_sets"] == 3000


def test_forced_sub_batches(gpu_ctx, mix, monkeypatch):
    sets, want = mix
    monkeypatch.setenv("RK_BATCH_MAX_ROWS", "1000")
    bc.assert_matches(gpu_ctx.classify_batch(sets), want[(0.3, 0.3)])
    st = gpu_ctx.batch_stats()
    assert st["sub_batches"] > 1 and st["batched_sets"] + st["looped_sets"] == 40
    monkeypatch.delenv("RK_BATCH_MAX_ROWS")
    monkeypatch.setenv("RK_BATCH_MAX_SPAN", "30000")
    bc.assert_matches(gpu_ctx.classify_batch(sets), want[(0.3, 0.3)])
    st = gpu_ctx.batch_stats()
    assert st["sub_batches"] > 1 and st["batched_sets"] + st["looped_sets"] == 40


def test_fallback_row_that_does_not_pack(gpu_ctx):
    sets = bc.random_sets(13, 6, max_rows=200)
    hx = 1 << 26
    wide = rk.Frags(np.array([1 << 25, 5000], np.uint64), np.array([7000, 5000], np.uint64),
                    np.array([(1 << 24) + 10, 30], np.uint64), np.array([102, 102], np.uint8))
    sets.insert(3, (wide, hx, hx))
    bc.assert_matches(gpu_ctx.classify_batch(sets), bc.oracle_sets(sets))
    assert gpu_ctx.batch_stats()["looped_sets"] > 0


def test_fallback_generic_context(generic_ctx, mix):
    sets, want = mix
    bc.assert_matches(generic_ctx.classify_batch(sets[:12]), want[(0.3, 0.3)][:12])
    st = generic_ctx.batch_stats()
    assert st["looped_sets"] == 12 and st["batched_sets"] == 0


def test_large_group_between_random_sets(gpu_ctx):
    f = long_run_set(2500, 4)
    hdr = 6_000_000
    sets = bc.random_sets(17, 3, max_rows=300)
    sets.insert(2, (f, hdr, hdr))
    for lr, pr in ((0.05, 0.05), (1.5, 0.7)):
        bc.assert_matches(gpu_ctx.classify_batch(sets, lr, pr), bc.oracle_sets(sets, lr, pr))
    assert gpu_ctx.batch_stats()["batched_sets"] == 4


# header 1000: vsize 101 (last bucket xStart 1000..1009), max_index 10
UB_ROWS = {
    -4: (1015, 500, 20),    # xStart/10 = 101 >= vsize
    -5: (990, 500, 240),    # X centre 1110: bucket 11 past the occupancy array
}


@pytest.mark.parametrize("code", [-4, -5])
def test_error_names_the_set(gpu_ctx, code):
    sets = bc.random_sets(19, 5, max_rows=100)
    rng = np.random.default_rng(1)
    good = bc.random_set(rng, 50, 1000, 1000)
    bad = rk.Frags(*(np.append(a, np.uint64(v)) for a, v in
                     zip((good.x_start, good.y_start, good.length), UB_ROWS[code])),
                   np.append(good.strand, np.uint8(102)))
    sets[2] = (bad, 1000, 1000)
    # (the oracle's own codes: RKO_E_UB_BUCKET -3, RKO_E_UB_CENTER -4)
    assert bc.oracle_set(*sets[2])[0] == {-4: -3, -5: -4}[code]
    # a later set that fails too: the lowest-numbered one is reported
    sets[4] = (bad, 1000, 1000)
    with pytest.raises(rk.RkError) as e:
        gpu_ctx.classify_batch(sets)
    assert e.value.code == code
    assert "set 2" in str(e.value)


def test_offending_rows_in_the_dropped_bucket_pass(gpu_ctx):
    sets = bc.random_sets(23, 5, max_rows=100)
    rng = np.random.default_rng(2)
    good = bc.random_set(rng, 50, 1000, 1000)
    # X and Y centres far past the arrays, but in the never-iterated last bucket
    extra = [(1005, 500, 4000), (1009, 900_000, 20)]
    f = rk.Frags(*(np.concatenate([a, np.array([r[i] for r in extra], np.uint64)])
                   for i, a in enumerate((good.x_start, good.y_start, good.length))),
                 np.concatenate([good.strand, np.array([102, 114], np.uint8)]))
    sets[2] = (f, 1000, 1000)
    want = bc.oracle_sets(sets)
    assert want[2][0] == 0 and want[2][1].shape[0] == 50
    bc.assert_matches(gpu_ctx.classify_batch(sets), want)


def test_argument_errors(gpu_ctx):
    rng = np.random.default_rng(29)
    sets = [(bc.random_set(rng, 20, 1000, 1000), 1000, 1000) for _ in range(3)]
    for lr, pr in ((0.0, 0.3), (0.3, 0.0), (-1.0, 0.3)):
        with pytest.raises(rk.RkError) as e:
            gpu_ctx.classify_batch(sets, lr, pr)
        assert e.value.code == -1
    n = [f.n for f, _, _ in sets]
    with pytest.raises(rk.RkError) as e:
        gpu_ctx.classify_batch(sets, set_off=[0, n[0] + n[1], n[0], sum(n)])
    assert e.value.code == -1
    assert gpu_ctx.classify_batch([]) == []


def test_golden_csvs(gpu_ctx, tmp_path):
    with open(os.path.join(EDGE, "manifest.json")) as f:
        man = json.load(f)
    by_ratio = {}
    for name, case in sorted(man.items()):
        if case["expect"] == "ref":
            by_ratio.setdefault((case["len_ratio"], case["pos_ratio"]), []).append(name)
    assert max(len(v) for v in by_ratio.values()) > 10
    for (lr, pr), names in by_ratio.items():
        dbs = [rk.FragmentsDatabase(os.path.join(EDGE, n + ".in.csv")) for n in names]
        res = gpu_ctx.classify_batch([(d.frags, d.len_x_hdr, d.len_y_hdr) for d in dbs], lr, pr)
        for name, db, r in zip(names, dbs, res):
            out = tmp_path / (name + ".csv")
            db.save_all_frag_pairs(str(out), r)
            with open(os.path.join(EDGE, name + ".out.csv"), "rb") as f:
                assert out.read_bytes() == f.read(), name


def test_repeatable(gpu_ctx, mix):
    sets, want = mix
    other = bc.random_sets(31, 9, max_rows=900)
    first = gpu_ctx.classify_batch(sets)
    bc.assert_matches(gpu_ctx.classify_batch(other), bc.oracle_sets(other))
    second = gpu_ctx.classify_batch(sets)
    bc.assert_matches(first, want[(0.3, 0.3)])
    bc.assert_matches(second, want[(0.3, 0.3)])


def test_device_entry_point(gpu_ctx, mix):
    import torch
    sets, want = mix
    off = np.concatenate([[0], np.cumsum([f.n for f, _, _ in sets])]).astype(np.uint64)
    n = int(off[-1])
    dev = torch.device("cuda", gpu_ctx.device)

    def col(name, view):
        a = np.concatenate([getattr(f, name) for f, _, _ in sets])
        return torch.from_numpy(a.view(view)).to(dev)

    x, y, ln = (col(c, np.int64) for c in ("x_start", "y_start", "length"))
    s = col("strand", np.uint8)
    gid = torch.zeros(n, dtype=torch.int32, device=dev)
    order = torch.zeros(n, dtype=torch.int32, device=dev)
    rep = torch.zeros(n, dtype=torch.uint8, device=dev)
    torch.cuda.synchronize()
    n_out, n_groups = gpu_ctx.classify_device_batch(
        x, y, ln, s, gid, rep, order, off, [s_[1] for s_ in sets], [s_[2] for s_ in sets])
    gid, order, rep = gid.cpu().numpy().view(np.uint32), order.cpu().numpy().view(np.uint32), \
        rep.cpu().numpy()
    got = []
    for k in range(len(sets)):
        a, b = int(off[k]), int(off[k]) + int(n_out[k])
        got.append(rk.ClassifyResult(gid[a:b], rep[a:b], order[a:b], int(n_groups[k])))
    bc.assert_matches(got, want[(0.3, 0.3)])


def test_cli_batch(tmp_path):
    names = ["e02b_upward_probe_on", "e05b_big_group_ties", "e15_processing_order"]
    lst = tmp_path / "list.tsv"
    lst.write_text("".join(f"{os.path.join(EDGE, n + '.in.csv')}\t{tmp_path / (n + '.csv')}\n"
                           for n in names))
    p = subprocess.run([rk.CLI_PATH, "--batch", str(lst), "0.3", "0.3"], capture_output=True,
                       text=True)
    assert p.returncode == 0, p.stderr
    for n in names:
        with open(os.path.join(EDGE, n + ".out.csv"), "rb") as f:
            assert (tmp_path / (n + ".csv")).read_bytes() == f.read(), n
