"""Selection of result rows by repeat flag on the host (rk_result_select,
rk_batch_result_select without RK_RES_DEVICE; CPU only): against numpy, against
the reference's golden files filtered by the last field of their Frag lines,
the argument errors, the CLI's --keep parsing, and the predicate and
destination arithmetic of rk_select.h in a stand-alone program under the
address and undefined-behaviour sanitizers (tests/cpp/select_check.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from oracle import rk_oracle as ro
import select_cases as sc

import repkiller_amd as rk

CSRC = os.path.join(ROOT, "repkiller_amd", "csrc")
MASKS = range(1, 8)


def oracle_result(db, lr, pr):
    f = db.frags
    rc, gid, rep, order, ng = ro.classify(f.x_start, f.y_start, f.length, f.strand,
                                          db.len_x_hdr, db.len_y_hdr, lr, pr)
    assert rc == 0
    return rk.ClassifyResult(gid, rep, order, ng)


# ---- 1: against numpy -----------------------------------------------------------

def raw_select(order, gid, rep, n_out, keep, tail=9):
    """rk_result_select on the host into sentinel-filled arrays of n_out + tail
    entries; returns them and the struct."""
    n = order.shape[0]
    oo, og = np.full(n + tail, sc.SENT32, np.uint32), np.full(n + tail, sc.SENT32, np.uint32)
    orp = np.full(n + tail, sc.SENT8, np.uint8)
    res = rk.Result(order.ctypes.data, gid.ctypes.data, rep.ctypes.data, n_out, 77)
    out = rk.Result(oo.ctypes.data, og.ctypes.data, orp.ctypes.data, 0, 0)
    rc = rk.load_library().rk_result_select(None, ctypes.byref(res), keep, 0, ctypes.byref(out))
    assert rc == 0
    return oo, og, orp, out


@pytest.mark.parametrize("keep", MASKS)
def test_host_select_numpy(keep):
    rnd = np.random.RandomState(100 + keep)
    for n in (1, 2, 15, 16, 17, 31, 32, 33, 1000, 4097):
        order, gid = sc.random_result(n + 5, rnd)
        rep = np.asarray([0, 1, 2, 2, 3, 255], np.uint8)[rnd.randint(0, 6, n + 5)]
        rep[n:] = 1  # past n_out: never read as rows
        oo, og, orp, out = raw_select(order, gid, rep, n, keep)
        off = np.array([0, n], np.uint64)
        wo, wg, wr, kept = sc.np_select(off, [n], order, gid, rep, keep)
        k = int(kept[0])
        assert out.n_out == k and out.n_groups == 77
        assert np.array_equal(oo[:k], wo[:k]) and np.array_equal(og[:k], wg[:k])
        assert np.array_equal(orp[:k], wr[:k])
        assert not np.isin(orp[:k], (3, 255)).any()
        # entries from n_out on are untouched
        assert (oo[k:] == sc.SENT32).all() and (og[k:] == sc.SENT32).all()
        assert (orp[k:] == sc.SENT8).all()


def test_python_select_matches_numpy():
    rnd = np.random.RandomState(5)
    order, gid = sc.random_result(300, rnd)
    rep = rnd.randint(0, 3, 300).astype(np.uint8)
    res = rk.ClassifyResult(gid, rep, order, 123)
    for keep in MASKS:
        got = rk.select(res, keep)
        k = sc.kept_flags(rep, keep)
        assert np.array_equal(got.out_order, order[k]) and np.array_equal(got.gid, gid[k])
        assert np.array_equal(got.repval, rep[k]) and got.n_groups == 123
    assert (rk.KEEP_SINGLETON, rk.KEEP_REPRESENTATIVE, rk.KEEP_REPEATED, rk.KEEP_UNIQUE,
            rk.KEEP_ALL) == (1, 2, 4, 3, 7)


# ---- 2: golden files --------------------------------------------------------------

def check_unique(res):
    u = rk.select(res, rk.KEEP_UNIQUE)
    assert u.out_order.shape[0] == res.n_groups
    assert np.array_equal(u.gid, np.arange(res.n_groups, dtype=np.uint32))


@pytest.mark.parametrize("name,case", sc.ref_fixtures(), ids=[n for n, _ in sc.ref_fixtures()])
def test_edge_fixture_filtered(name, case, tmp_path):
    db = rk.FragmentsDatabase(sc.edge_in(name))
    res = oracle_result(db, case["len_ratio"], case["pos_ratio"])
    golden = sc.edge_golden(name)
    for keep in (3, 4):
        out = tmp_path / f"k{keep}.csv"
        db.save_all_frag_pairs(str(out), rk.select(res, keep))
        assert out.read_bytes() == sc.filtered(golden, keep), (name, keep)
    check_unique(res)
    if name.startswith(("e06", "e14")):
        assert set(np.unique(res.repval)) == {0, 1, 2}
    if name.startswith(("e12", "e13")):
        assert res.out_order.shape[0] == 0
    db.close()


def test_corpus_filtered(tmp_path):
    path, golden = sc.unpack_corpus(tmp_path)
    db = rk.FragmentsDatabase(path)
    res = oracle_result(db, 0.3, 0.3)
    assert [int((res.repval == f).sum()) for f in range(3)] == [1858, 209, 7933]
    for keep in MASKS:
        out = tmp_path / f"k{keep}.csv"
        db.save_all_frag_pairs(str(out), rk.select(res, keep))
        assert out.read_bytes() == sc.filtered(golden, keep), keep
    assert sc.filtered(golden, rk.KEEP_ALL) == golden
    check_unique(res)
    db.close()


# ---- 3: batch layout -----------------------------------------------------------------

def batch_select(off, n_out, order, gid, rep, keep, n_groups=None):
    n = int(off[-1])
    oo, og = np.full(n, sc.SENT32, np.uint32), np.full(n, sc.SENT32, np.uint32)
    orp = np.full(n, sc.SENT8, np.uint8)
    ns = len(off) - 1
    kept = np.full(max(ns, 1), 99, np.uint64)
    no = np.ascontiguousarray(n_out, np.uint64)
    ng_out = np.zeros(max(ns, 1), np.uint64)
    res = rk.BatchResult(rk._ptr(order), rk._ptr(gid), rk._ptr(rep), rk._ptr(no),
                         rk._ptr(n_groups) if n_groups is not None else 0)
    out = rk.BatchResult(rk._ptr(oo), rk._ptr(og), rk._ptr(orp), kept.ctypes.data,
                         ng_out.ctypes.data)
    rc = rk.load_library().rk_batch_result_select(None, ns, off.ctypes.data, ctypes.byref(res),
                                                  keep, 0, ctypes.byref(out))
    assert rc == 0
    return oo, og, orp, kept[:ns], ng_out[:ns]


@pytest.mark.parametrize("layout", sorted(sc.batch_layouts(4096)))
def test_host_batch_select(layout):
    rnd = np.random.RandomState(7)
    off, n_out, order, gid, rep = sc.layout_arrays(sc.batch_layouts(4096)[layout], rnd)
    ns = len(off) - 1
    ng = np.arange(ns, dtype=np.uint64) + 3
    for keep in MASKS:
        oo, og, orp, kept, ng_out = batch_select(off, n_out, order, gid, rep, keep, ng)
        wo, wg, wr, wk = sc.np_select(off, n_out, order, gid, rep, keep)
        assert np.array_equal(kept, wk)
        assert np.array_equal(oo, wo) and np.array_equal(og, wg) and np.array_equal(orp, wr)
        assert np.array_equal(ng_out, ng)
        assert not (oo == 0xFFFFFFFF).any(), "an unused slot was read as a row"
    # every set equals the single select of that set alone
    for k in list(range(min(ns, 12))) + list(range(max(ns - 12, 0), ns)):
        a, u = int(off[k]), int(n_out[k])
        one = rk.select(rk.ClassifyResult(gid[a:a + u], rep[a:a + u], order[a:a + u], 0), 5)
        oo, og, orp, kept, _ = batch_select(off, n_out, order, gid, rep, 5)
        m = int(kept[k])
        assert m == one.out_order.shape[0]
        assert np.array_equal(oo[a:a + m], one.out_order) and np.array_equal(og[a:a + m], one.gid)
        assert np.array_equal(orp[a:a + m], one.repval)


@pytest.mark.parametrize("first", [1, 5, 16, 4099])
def test_host_batch_first_offset(first):
    """set_off[0] above zero: the slots before it belong to no set, are not read
    as rows and are not written."""
    rnd = np.random.RandomState(first)
    for layout in ("one", "empties", "wave_edges"):
        off, n_out, order, gid, rep = sc.layout_arrays(sc.batch_layouts(4096)[layout], rnd,
                                                       first=first)
        for keep in MASKS:
            oo, og, orp, kept, _ = batch_select(off, n_out, order, gid, rep, keep)
            wo, wg, wr, wk = sc.np_select(off, n_out, order, gid, rep, keep)
            assert np.array_equal(kept, wk)
            assert np.array_equal(oo, wo) and np.array_equal(og, wg) and np.array_equal(orp, wr)
            assert (oo[:first] == sc.SENT32).all() and (orp[:first] == sc.SENT8).all()
            assert not (oo == 0xFFFFFFFF).any()


# ---- 4: argument errors -----------------------------------------------------------------

def test_argument_errors():
    lib = rk.load_library()
    n = 8
    order, gid = np.arange(n, dtype=np.uint32), np.arange(n, dtype=np.uint32)
    rep = np.zeros(n, np.uint8)
    oo, og, orp = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)

    def single(keep=3, flags=0, res=None, out=None):
        res = res or rk.Result(order.ctypes.data, gid.ctypes.data, rep.ctypes.data, n, 0)
        out = out or rk.Result(oo.ctypes.data, og.ctypes.data, orp.ctypes.data, 0, 0)
        return lib.rk_result_select(None, ctypes.byref(res), keep, flags, ctypes.byref(out))

    assert single() == 0
    assert single(keep=0) == -1 and single(keep=8) == -1
    assert single(flags=2) == -1 and single(flags=3) == -1
    assert single(flags=rk.RK_RES_DEVICE) == -1  # device arrays need a context
    assert single(res=rk.Result(0, gid.ctypes.data, rep.ctypes.data, n, 0)) == -1
    assert single(out=rk.Result(oo.ctypes.data, og.ctypes.data, 0, 0, 0)) == -1
    # no in-place selection, array by array
    assert single(out=rk.Result(order.ctypes.data, og.ctypes.data, orp.ctypes.data, 0, 0)) == -1
    assert single(out=rk.Result(oo.ctypes.data, gid.ctypes.data, orp.ctypes.data, 0, 0)) == -1
    assert single(out=rk.Result(oo.ctypes.data, og.ctypes.data, rep.ctypes.data, 0, 0)) == -1
    # n_out == 0 is RK_OK, null arrays and all
    out = rk.Result(0, 0, 0, 5, 0)
    assert single(res=rk.Result(0, 0, 0, 0, 9), out=out) == 0
    assert (out.n_out, out.n_groups) == (0, 9)

    off = np.array([0, 3, 8], np.uint64)
    no = np.array([3, 5], np.uint64)
    kept = np.zeros(2, np.uint64)

    def batch(ns=2, off=off, no=no, keep=3, flags=0, res=None, out=None):
        res = res or rk.BatchResult(order.ctypes.data, gid.ctypes.data, rep.ctypes.data,
                                    no.ctypes.data, 0)
        out = out or rk.BatchResult(oo.ctypes.data, og.ctypes.data, orp.ctypes.data,
                                    kept.ctypes.data, 0)
        return lib.rk_batch_result_select(None, ns, off.ctypes.data if off is not None else 0,
                                          ctypes.byref(res), keep, flags, ctypes.byref(out))

    assert batch() == 0
    assert batch(keep=0) == -1 and batch(keep=8) == -1
    assert batch(flags=4) == -1
    assert batch(flags=rk.RK_RES_DEVICE) == -1
    assert batch(off=np.array([0, 5, 3], np.uint64)) == -1           # decreasing
    assert batch(no=np.array([4, 5], np.uint64)) == -1               # n_out beyond its window
    assert batch(off=None) == -1
    assert batch(res=rk.BatchResult(order.ctypes.data, 0, rep.ctypes.data, no.ctypes.data, 0)) == -1
    assert batch(res=rk.BatchResult(order.ctypes.data, gid.ctypes.data, rep.ctypes.data, 0, 0)) == -1
    assert batch(out=rk.BatchResult(oo.ctypes.data, og.ctypes.data, orp.ctypes.data, 0, 0)) == -1
    assert batch(out=rk.BatchResult(order.ctypes.data, og.ctypes.data, orp.ctypes.data,
                                    kept.ctypes.data, 0)) == -1
    assert batch(ns=0) == 0
    # no rows at all: null arrays are fine
    zero = np.zeros(2, np.uint64)
    assert batch(res=rk.BatchResult(0, 0, 0, zero.ctypes.data, 0),
                 out=rk.BatchResult(0, 0, 0, kept.ctypes.data, 0)) == 0


def test_select_tile_exported():
    t = rk.select_tile()
    assert t >= 64 and t % 64 == 0


# ---- 5: the CLI's --keep ---------------------------------------------------------------------

@pytest.mark.parametrize("value", ["0", "8", "x", "", "3x", "-1"])
def test_cli_bad_keep(value, tmp_path):
    p = subprocess.run([rk.CLI_PATH, "--keep", value, str(tmp_path / "missing.csv"),
                        str(tmp_path / "out.csv"), "0.3", "0.3"], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 1
    assert "Usage:" in p.stdout and "--keep" in p.stdout
    assert "Invalid --keep" in p.stderr
    assert not (tmp_path / "out.csv").exists()


# ---- 6: rk_select.h under the sanitizers --------------------------------------------------------

def test_select_header_sanitized(tmp_path):
    exe = tmp_path / "select_check_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "cpp", "select_check.cpp"), "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe), "1500"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches 0" in p.stdout
