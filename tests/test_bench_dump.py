"""bench.py --dump-outputs on CPU: which output rows are written and how."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_dump_rows_fixed_sample():
    n_out = 5 * bench.DUMP_ROWS
    for world in (1, 2, 8):
        for rank in range(world):
            rows = bench.dump_rows(n_out, rank, world)
            assert rows.dtype == np.int64 and 0 < rows.size <= bench.DUMP_ROWS // world
            assert rows[0] >= 0 and rows[-1] < n_out and bool((np.diff(rows) > 0).all())
            assert np.array_equal(rows, bench.dump_rows(n_out, rank, world))  # run to run
    # an output that fits is written whole
    assert np.array_equal(bench.dump_rows(1000, 0, 1), np.arange(1000))
    assert bench.dump_rows(0, 0, 1).size == 0


def test_dump_outputs_small_is_exact(tmp_path):
    """Device-side layout (int32 / uint8 torch tensors longer than n_out): every
    value comes back exactly, above 2^31 too."""
    n, n_out = 1000, 900
    rng = np.random.default_rng(1)
    order = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    gid = np.sort(rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32))
    rep = rng.integers(0, 3, n).astype(np.uint8)
    bench.dump_outputs(str(tmp_path), 0, 1, n_out, 77, torch.from_numpy(order.view(np.int32)),
                       torch.from_numpy(gid.view(np.int32)), torch.from_numpy(rep))
    got = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    assert sorted(got) == ["counts", "gid", "out_order", "repval", "rows"]
    assert got["counts"].tolist() == [n_out, 77]
    assert np.array_equal(got["rows"], np.arange(n_out))
    assert got["out_order"].dtype == np.float64 and got["repval"].dtype == np.float32
    assert np.array_equal(got["out_order"].astype(np.uint32), order[:n_out])
    assert np.array_equal(got["gid"].astype(np.uint32), gid[:n_out])
    assert np.array_equal(got["repval"].astype(np.uint8), rep[:n_out])


def test_dump_outputs_large_is_sampled_and_bounded(tmp_path):
    """A share's host arrays (numpy, rank 1 of 2): the seeded rows, under 64 MB."""
    n_out = 2 * bench.DUMP_ROWS
    order = np.arange(n_out, dtype=np.uint32)[::-1].copy()
    gid = np.arange(n_out, dtype=np.uint32) // 3
    rep = (np.arange(n_out) % 3).astype(np.uint8)
    bench.dump_outputs(str(tmp_path / "d"), 1, 2, n_out, 5, order, gid, rep)
    files = sorted(os.listdir(tmp_path / "d"))
    assert files == [f"{k}_rank1.npy" for k in ("counts", "gid", "out_order", "repval", "rows")]
    assert sum(os.path.getsize(tmp_path / "d" / f) for f in files) * 2 <= 64_000_000
    rows = np.load(tmp_path / "d" / "rows_rank1.npy").astype(np.int64)
    assert np.array_equal(rows, bench.dump_rows(n_out, 1, 2))
    assert np.array_equal(np.load(tmp_path / "d" / "out_order_rank1.npy"), order[rows])
    assert np.array_equal(np.load(tmp_path / "d" / "gid_rank1.npy"), gid[rows])
    assert np.array_equal(np.load(tmp_path / "d" / "repval_rank1.npy"), rep[rows])
