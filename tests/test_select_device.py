"""Selection of result rows by repeat flag on the GPU (rk_select.hip):
rk_result_select / rk_batch_result_select with RK_RES_DEVICE against numpy, the
classification followed by the device selection against the host selection, and
the *_to_csv_keep routes and the CLI's --keep against the reference's golden
files filtered by the last field of their Frag lines."""
import ctypes
import os
import subprocess

import numpy as np
import pytest
import torch

import select_cases as sc

import repkiller_amd as rk

pytestmark = pytest.mark.gpu

DEV_MASKS = (3, 4, 7)


def dev(a):
    """A numpy array as a device tensor of the same bytes."""
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).cuda()


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def device_select(ctx, order, gid, rep, n_out, keep, tail=5, shift=0):
    """rk_result_select with RK_RES_DEVICE: inputs of n_out + tail entries, outputs
    sentinel-filled; `shift` entries are cut off the front of every tensor, so the
    arrays start off a 16-B boundary.  Returns the outputs as numpy, the kept count."""
    n = order.shape[0]
    pad = lambda a, fill: np.concatenate([np.full(shift, fill, a.dtype), a])
    d_in = [dev(pad(order, 7))[shift:], dev(pad(gid, 7))[shift:], dev(pad(rep, 1))[shift:]]
    d_out = [dev(np.full(n + shift, sc.SENT32, np.uint32))[shift:],
             dev(np.full(n + shift, sc.SENT32, np.uint32))[shift:],
             dev(np.full(n + shift, sc.SENT8, np.uint8))[shift:]]
    kept = ctx.select_device(d_in[0], d_in[1], d_in[2], n_out, keep, *d_out)
    torch.cuda.synchronize()
    return host(d_out[0], np.uint32), host(d_out[1], np.uint32), host(d_out[2], np.uint8), kept


def check_single(ctx, n_out, pattern, keep, rnd, tail=5, shift=0):
    order, gid = sc.random_result(n_out + tail, rnd)
    rep = np.concatenate([sc.flags_for(pattern, n_out, keep, rnd), np.full(tail, 1, np.uint8)])
    oo, og, orp, kept = device_select(ctx, order, gid, rep, n_out, keep, tail, shift)
    off = np.array([0, n_out], np.uint64)
    wo, wg, wr, wk = sc.np_select(off, [n_out], order, gid, rep, keep)
    k = int(wk[0])
    tag = (n_out, pattern, keep, shift)
    assert kept == k, tag
    assert np.array_equal(oo[:k], wo[:k]) and np.array_equal(og[:k], wg[:k]), tag
    assert np.array_equal(orp[:k], wr[:k]), tag
    assert (oo[k:] == sc.SENT32).all() and (og[k:] == sc.SENT32).all(), tag
    assert (orp[k:] == sc.SENT8).all(), tag
    st = ctx.select_stats()
    assert (st["rows_in"], st["kept"], st["sets"]) == (n_out, k, 1), tag
    assert st["by_flag"] == sc.by_flag(off, [n_out], rep), tag
    if pattern == "all":
        assert k == n_out
    if pattern == "none":
        assert k == 0


# ---- 1: one result against numpy ----------------------------------------------------

@pytest.mark.parametrize("keep", DEV_MASKS)
def test_single_sizes_and_patterns(keep, gpu_ctx):
    T = rk.select_tile()
    rnd = np.random.RandomState(keep)
    for n_out in (0, 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 5):
        for pattern in sc.PATTERNS:
            check_single(gpu_ctx, n_out, pattern, keep, rnd)


@pytest.mark.parametrize("keep", DEV_MASKS)
def test_single_many_tiles(keep, gpu_ctx):
    """More than one tile per lane of the tile scan."""
    T = rk.select_tile()
    rnd = np.random.RandomState(40 + keep)
    for pattern in ("all", "none", "p02" if keep == 4 else "p98"):
        check_single(gpu_ctx, 1025 * T + 3, pattern, keep, rnd)


def test_single_unaligned_arrays(gpu_ctx):
    """Arrays that start off a 16-B boundary: the flags come byte by byte and
    the flag run is written from an unaligned first byte."""
    T = rk.select_tile()
    rnd = np.random.RandomState(9)
    for shift in (1, 2, 3, 5):
        for n_out in (1, 17, T + 1, 2 * T + 9):
            check_single(gpu_ctx, n_out, "p98", 3, rnd, shift=shift)
            check_single(gpu_ctx, n_out, "alternating", 4, rnd, shift=shift)


# ---- 2: batch layout --------------------------------------------------------------------

def check_batch(ctx, sizes, keep, rnd, short=True, first=0):
    off, n_out, order, gid, rep = sc.layout_arrays(sizes, rnd, short, first)
    n = int(off[-1])
    d_out = [dev(np.full(n, sc.SENT32, np.uint32)), dev(np.full(n, sc.SENT32, np.uint32)),
             dev(np.full(n, sc.SENT8, np.uint8))]
    kept = ctx.select_batch(off, n_out, dev(order), dev(gid), dev(rep), keep, *d_out)
    torch.cuda.synchronize()
    wo, wg, wr, wk = sc.np_select(off, n_out, order, gid, rep, keep)
    assert np.array_equal(kept, wk)
    oo, og, orp = host(d_out[0], np.uint32), host(d_out[1], np.uint32), host(d_out[2], np.uint8)
    assert np.array_equal(oo, wo) and np.array_equal(og, wg) and np.array_equal(orp, wr)
    assert not (oo == 0xFFFFFFFF).any(), "an unused slot was read as a row"
    assert (oo[:first] == sc.SENT32).all() and (orp[:first] == sc.SENT8).all()
    st = ctx.select_stats()
    assert (st["rows_in"], st["kept"], st["sets"]) == (int(n_out.sum()), int(wk.sum()),
                                                       len(sizes))
    assert st["by_flag"] == sc.by_flag(off, n_out, rep)


@pytest.mark.parametrize("layout", sorted(sc.batch_layouts(4096)))
def test_batch_layouts(layout, gpu_ctx):
    T = rk.select_tile()
    sizes = sc.batch_layouts(T)[layout]
    assert len(sizes) in (1, 2, 3, 8, 9, 5000)
    rnd = np.random.RandomState(21)
    for keep in DEV_MASKS:
        check_batch(gpu_ctx, sizes, keep, rnd)
    check_batch(gpu_ctx, sizes, 3, rnd, short=False)


@pytest.mark.parametrize("first", [1, 5, 16, 4099])
def test_batch_first_offset(first, gpu_ctx):
    """set_off[0] above zero: the slots before it belong to no set, are not read
    as rows, not counted and not written."""
    T = rk.select_tile()
    rnd = np.random.RandomState(first)
    for layout in ("one", "empties", "three_tile_edges"):
        for keep in DEV_MASKS:
            check_batch(gpu_ctx, sc.batch_layouts(T)[layout], keep, rnd, first=first)


def test_batch_matches_host_batch(gpu_ctx):
    """The same call with host arrays and with device tensors."""
    rnd = np.random.RandomState(3)
    off, n_out, order, gid, rep = sc.layout_arrays(sc.batch_layouts(rk.select_tile())["empties"],
                                                   rnd)
    n = int(off[-1])
    ho = [np.full(n, sc.SENT32, np.uint32), np.full(n, sc.SENT32, np.uint32),
          np.full(n, sc.SENT8, np.uint8)]
    hk = gpu_ctx.select_batch(off, n_out, order, gid, rep, 5, *ho)
    do = [dev(np.full(n, sc.SENT32, np.uint32)), dev(np.full(n, sc.SENT32, np.uint32)),
          dev(np.full(n, sc.SENT8, np.uint8))]
    dk = gpu_ctx.select_batch(off, n_out, dev(order), dev(gid), dev(rep), 5, *do)
    torch.cuda.synchronize()
    assert np.array_equal(hk, dk)
    for h, d, t in zip(ho, do, (np.uint32, np.uint32, np.uint8)):
        assert np.array_equal(h, host(d, t))


def test_device_argument_errors(gpu_ctx):
    n = 64
    a, b = dev(np.zeros(n, np.uint32)), dev(np.zeros(n, np.uint32))
    r, o = dev(np.zeros(n, np.uint8)), dev(np.zeros(n, np.uint8))
    for keep in (0, 8):
        with pytest.raises(rk.RkError) as e:
            gpu_ctx.select_device(a, a, r, n, keep, b, b, o)
        assert e.value.code == -1
    with pytest.raises(rk.RkError) as e:  # in place
        gpu_ctx.select_device(a, b, r, n, 3, a, a, o)
    assert e.value.code == -1


# ---- 3: classification, then the selection --------------------------------------------------

@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    return sc.unpack_corpus(tmp_path_factory.mktemp("select"))


def test_corpus_end_to_end(corpus, gpu_ctx):
    db = rk.FragmentsDatabase(corpus[0])
    f = db.frags
    want = gpu_ctx.classify(f, db.len_x_hdr, db.len_y_hdr, 0.3, 0.3)
    n = f.n
    x, y, ln = (torch.from_numpy(a.view(np.int64).copy()).cuda()
                for a in (f.x_start, f.y_start, f.length))
    strand = torch.from_numpy(f.strand.copy()).cuda()
    gid, order = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(2))
    rep = torch.zeros(n, dtype=torch.uint8, device="cuda")
    n_out, n_groups = gpu_ctx.classify_device(x, y, ln, strand, gid, rep, order, db.len_x_hdr,
                                              db.len_y_hdr, 0.3, 0.3)
    assert (n_out, n_groups) == (want.out_order.shape[0], want.n_groups)
    for keep in range(1, 8):
        so, sg = (torch.full((n,), -1, dtype=torch.int32, device="cuda") for _ in range(2))
        sr = torch.full((n,), sc.SENT8, dtype=torch.uint8, device="cuda")
        kept = gpu_ctx.select_device(order, gid, rep, n_out, keep, so, sg, sr)
        torch.cuda.synchronize()
        h = rk.select(want, keep)
        assert kept == h.out_order.shape[0]
        assert np.array_equal(host(so, np.uint32)[:kept], h.out_order)
        assert np.array_equal(host(sg, np.uint32)[:kept], h.gid)
        assert np.array_equal(host(sr, np.uint8)[:kept], h.repval)
        if keep == rk.KEEP_UNIQUE:
            assert kept == n_groups
            assert np.array_equal(host(sg, np.uint32)[:kept], np.arange(n_groups, dtype=np.uint32))
    assert gpu_ctx.select_stats()["by_flag"] == [1858, 209, 7933, 0]
    db.close()


# ---- 4: files ------------------------------------------------------------------------------

def read(p):
    with open(p, "rb") as f:
        return f.read()


def kept_rows(golden, keep):
    return sc.golden_rows(sc.filtered(golden, keep))


@pytest.mark.parametrize("rows_env", [None, "small"])
@pytest.mark.parametrize("keep", [3, 4])
def test_file_corpus(keep, rows_env, corpus, gpu_ctx, tmp_path, monkeypatch):
    if rows_env:
        monkeypatch.setenv("RK_CSV_OUT_ROWS", "100")  # kept rows cross chunk edges
    db = rk.FragmentsDatabase(corpus[0], ctx=gpu_ctx, keep_rows=True)
    out = tmp_path / "out.csv"
    (n_out, n_groups, n_kept), = gpu_ctx.classify_db_to_csv(db, [(0.3, 0.3)], [str(out)],
                                                            keep=keep, with_kept=True)
    assert read(out) == sc.filtered(corpus[1], keep)
    assert n_out == sc.golden_rows(corpus[1])
    want = kept_rows(corpus[1], keep)
    assert gpu_ctx.egress_stats()["rows"] == want and n_kept == want
    if keep == rk.KEEP_UNIQUE:
        assert want == n_groups
    db.close()


@pytest.mark.parametrize("rows_env", [None, "one"])
@pytest.mark.parametrize("keep", [3, 4])
def test_file_e06(keep, rows_env, gpu_ctx, tmp_path, monkeypatch):
    if rows_env:
        monkeypatch.setenv("RK_CSV_OUT_ROWS", "1")
    golden = sc.edge_golden("e06_parse_rules")
    db = rk.FragmentsDatabase(sc.edge_in("e06_parse_rules"), ctx=gpu_ctx, keep_rows=True)
    out = tmp_path / "out.csv"
    gpu_ctx.classify_db_to_csv(db, [(0.3, 0.3)], [str(out)], keep=keep)
    assert read(out) == sc.filtered(golden, keep)
    assert gpu_ctx.egress_stats()["rows"] == kept_rows(golden, keep)
    db.close()


def test_file_two_pairs(corpus, gpu_ctx, tmp_path):
    """Every pair of one call is selected on its own."""
    db = rk.FragmentsDatabase(corpus[0], ctx=gpu_ctx, keep_rows=True)
    outs = [str(tmp_path / "a.csv"), str(tmp_path / "b.csv")]
    gpu_ctx.classify_db_to_csv(db, [(0.3, 0.3), (0.3, 0.3)], outs, keep=rk.KEEP_UNIQUE)
    want = sc.filtered(corpus[1], rk.KEEP_UNIQUE)
    assert read(outs[0]) == want and read(outs[1]) == want
    db.close()


@pytest.mark.parametrize("keep", [3, 4])
def test_files_batched(keep, corpus, gpu_ctx, tmp_path):
    fixtures = sc.ref_fixtures()
    by_ratio = {}
    for name, case in fixtures:
        by_ratio.setdefault((case["len_ratio"], case["pos_ratio"]), []).append(name)
    assert sum(len(v) for v in by_ratio.values()) == len(fixtures) == 15
    seen = 0
    for (lr, pr), names in sorted(by_ratio.items()):
        ins = [sc.edge_in(n) for n in names]
        goldens = [sc.edge_golden(n) for n in names]
        if (lr, pr) == (0.3, 0.3):
            assert "e13_no_fragments" in names
            ins += [sc.edge_in("e06_parse_rules"), corpus[0]]
            goldens += [sc.edge_golden("e06_parse_rules"), corpus[1]]
        outs = [str(tmp_path / f"{lr}_{k}.csv") for k in range(len(ins))]
        dbs = rk.FragmentsDatabaseSet(ins, gpu_ctx, keep_rows=True)
        n_out, n_groups, n_kept = gpu_ctx.classify_dbset_to_csv(dbs, outs, lr, pr, keep=keep,
                                                                with_kept=True)
        dbs.close()
        for k, g in enumerate(goldens):
            assert read(outs[k]) == sc.filtered(g, keep), (ins[k], keep)
            assert int(n_out[k]) == sc.golden_rows(g)
            assert int(n_kept[k]) == kept_rows(g, keep)
            if keep == rk.KEEP_UNIQUE:
                assert int(n_kept[k]) == int(n_groups[k])
        assert gpu_ctx.egress_stats()["rows"] == sum(kept_rows(g, keep) for g in goldens)
        seen += len(names)
    assert seen == 15


def test_keep_all_is_the_existing_route(corpus, gpu_ctx, tmp_path):
    lib = rk.load_library()
    db = rk.FragmentsDatabase(corpus[0], ctx=gpu_ctx, keep_rows=True)
    a, b = tmp_path / "a.csv", tmp_path / "b.csv"
    lr, pr = ctypes.c_double(0.3), ctypes.c_double(0.3)
    pa = (ctypes.c_char_p * 1)(str(a).encode())
    assert lib.rk_classify_db_pairs_to_csv(gpu_ctx._h, db._h, ctypes.byref(lr), ctypes.byref(pr),
                                           1, pa, None, None) == 0
    (_, _, n_kept), = gpu_ctx.classify_db_to_csv(db, [(0.3, 0.3)], [str(b)], keep=rk.KEEP_ALL,
                                                 with_kept=True)
    assert read(a) == read(b) == corpus[1]
    assert n_kept == sc.golden_rows(corpus[1])
    db.close()

    ins = [sc.edge_in("e06_parse_rules"), corpus[0], sc.edge_in("e13_no_fragments")]
    dbs = rk.FragmentsDatabaseSet(ins, gpu_ctx, keep_rows=True)
    oa = [str(tmp_path / f"sa{k}.csv") for k in range(3)]
    ob = [str(tmp_path / f"sb{k}.csv") for k in range(3)]
    arr = (ctypes.c_char_p * 3)(*[p.encode() for p in oa])
    assert lib.rk_classify_dbset_to_csv(gpu_ctx._h, dbs._h, 0.3, 0.3, arr, None, None) == 0
    gpu_ctx.classify_dbset_to_csv(dbs, ob, 0.3, 0.3, keep=rk.KEEP_ALL)
    dbs.close()
    for x, y in zip(oa, ob):
        assert read(x) == read(y)
    assert read(ob[1]) == corpus[1]


# ---- 5: the CLI ------------------------------------------------------------------------------

def run_cli(args):
    p = subprocess.run([rk.CLI_PATH] + args, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    return p


def test_cli_keep_unique(corpus, tmp_path):
    want = sc.filtered(corpus[1], rk.KEEP_UNIQUE)
    a, b, c = (str(tmp_path / f"{x}.csv") for x in "abc")
    run_cli(["--keep", "unique", corpus[0], a, "0.3", "0.3"])
    assert read(a) == want
    p = run_cli(["--keep", "unique", "--timing", "--device-parse", "--device-save", corpus[0], b,
                 "0.3", "0.3"])
    assert read(b) == want
    assert '"select": {"rows_in": 10000, "by_flag": [1858, 209, 7933, 0], "kept": 2067' in p.stderr
    lst = tmp_path / "list.txt"
    lst.write_text(f"{corpus[0]}\t{c}\n{sc.edge_in('e06_parse_rules')}\t{tmp_path / 'e06.csv'}\n")
    run_cli(["--keep", "unique", "--batch", str(lst), "--device-parse", "--device-save", "0.3",
             "0.3"])
    assert read(c) == want
    assert read(tmp_path / "e06.csv") == sc.filtered(sc.edge_golden("e06_parse_rules"), 3)


def test_cli_keep_batch_host_save(corpus, tmp_path):
    """--keep by number and by name on the two batch routes that save on the host."""
    a = str(tmp_path / "a.csv")
    lst = tmp_path / "list.txt"
    lst.write_text(f"{corpus[0]}\t{a}\n")
    run_cli(["--keep", "4", "--batch", str(lst), "0.3", "0.3"])
    assert read(a) == sc.filtered(corpus[1], rk.KEEP_REPEATED)
    run_cli(["--keep", "groups", "--batch", str(lst), "--device-parse", "0.3", "0.3"])
    assert read(a) == sc.filtered(corpus[1], 6)


def test_cli_keep_sharded(corpus, tmp_path):
    """The sharded driver (two ranks on the one GPU) selects on the host after
    its gather."""
    c = str(tmp_path / "c.csv")
    p = run_cli(["--keep", "repeated", "--timing", "--gpus", "2", "--same-device", corpus[0], c,
                 "0.3", "0.3"])
    assert read(c) == sc.filtered(corpus[1], rk.KEEP_REPEATED)
    # (no context on this route: the rows by flag are counted from the result itself)
    assert '"select": {"rows_in": 10000, "by_flag": [1858, 209, 7933, 0], "kept": 7933' in p.stderr
