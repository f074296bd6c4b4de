"""Device CSV egress (rk_db_write_csv_device) against the host writer
(rk_db_write_csv): the same database and the same result through both routes,
and the two files byte-identical; where a golden output exists, identical to
that too.

The output format bounds a row: the integer columns come from atoll (at most
20 digits, a negative spelling wrapped to u64), ident is (uint64_t)similarity,
so the longest row the two routes can be given is about 190 bytes (a host row)
and about 165 bytes for a row the device formats; the shortest is 31.  (A
denormal similarity cannot come in through a CSV: strtof reports ERANGE and the
line is dropped; tests/test_csv_row.py covers those.)"""
import glob
import gzip
import json
import os
import random
import shutil
import struct
import subprocess

import numpy as np
import pytest

from conftest import EDGE, GOLDEN

import repkiller_amd as rk

pytestmark = pytest.mark.gpu


def header(total):
    out = []
    for k in range(1, 17):
        if k == 7:
            out.append("SeqX length : 1000000000")
        elif k == 8:
            out.append("SeqY length : 1000000000")
        elif k == 13:
            out.append(f"Total fragments : {total}")
        else:
            out.append(f"header line {k}")
    return ("\n".join(out) + "\n").encode()


def write_input(path, rows):
    """rows: (xs, ys, xe, ye, strand, length, score, similarity spelling)."""
    with open(path, "wb") as f:
        f.write(header(len(rows)))
        f.write("".join(f"Frag,{a},{b},{c},{d},{s},0,{ln},{sc},0,{sim},0,0,0\n"
                        for a, b, c, d, s, ln, sc, sim in rows).encode())
    return str(path)


def columns(db, tmp):
    """ident, length (uint64) and similarity (float32) of a database, from its
    SoA cache: magic, n + 3 header numbers + header bytes, the header text, then
    each column on a 4-KB boundary."""
    p = str(tmp) + ".cols.soa"
    db.save_soa(p)
    with open(p, "rb") as f:
        blob = f.read()
    os.remove(p)
    n, _, _, _, hb = struct.unpack_from("<5Q", blob, 8)
    up = lambda v: (v + 4095) & ~4095
    off, o = [], up(48 + hb)
    for w in (8, 8, 8, 8, 8, 8, 8, 4, 1):
        off.append(o)
        o = up(o + n * w)
    length = np.frombuffer(blob, np.uint64, n, off[4])
    ident = np.frombuffer(blob, np.uint64, n, off[6])
    sim = np.frombuffer(blob, np.float32, n, off[7])
    return ident, length, sim


def device_prints(f):
    """The floats the device formats: +0, and [1e-3, 1e6) unless "%.6g" rounds
    them up to 1e+06 (rk_csv_row.h)."""
    f = np.asarray(f, np.float32)
    bits = f.view(np.uint32)
    with np.errstate(invalid="ignore"):
        inside = (f >= np.float32(1e-3)) & (f < np.float32(1e6))
    near = inside & (f > np.float32(999990.0))
    for i in np.flatnonzero(near):
        if "%.6g" % float(f[i]) == "1e+06":
            inside[i] = False
    return (bits == 0) | inside


def expected_host_rows(db, res, tmp):
    ident, length, sim = columns(db, tmp)
    o = res.out_order.astype(np.int64)
    with np.errstate(all="ignore"):
        identity = ident[o].astype(np.float32) * np.float32(100) / length[o].astype(np.float32)
    return int((~(device_prints(sim[o]) & device_prints(identity))).sum())


def both_routes(db, ctx, res, tmp_path, tag="x"):
    """The file of both routes for `res`; asserts they are equal, returns it and
    the egress stats."""
    hp, dp = str(tmp_path / f"{tag}.host.csv"), str(tmp_path / f"{tag}.dev.csv")
    db.save_all_frag_pairs(hp, res)
    db.save_all_frag_pairs_device(ctx, dp, res)
    st = ctx.egress_stats()
    with open(hp, "rb") as f:
        host = f.read()
    with open(dp, "rb") as f:
        dev = f.read()
    assert len(dev) == len(host)
    assert dev == host, "the device route's file differs from the host route's"
    return dev, st


def synthetic_result(n, n_out, seed):
    rnd = np.random.RandomState(seed)
    order = rnd.permutation(n)[:n_out].astype(np.uint32)
    gid = rnd.randint(0, 1 << 20, n_out).astype(np.uint32)
    gid[rnd.rand(n_out) < 0.1] = 0xFFFFFFFF
    gid[rnd.rand(n_out) < 0.1] = 0
    rep = rnd.randint(0, 3, n_out).astype(np.uint8)
    return rk.ClassifyResult(gid, rep, order, int(n_out))


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("csvout")
    p = d / "corpus10k.in.csv"
    with gzip.open(os.path.join(GOLDEN, "corpus10k.in.csv.gz"), "rb") as f, open(p, "wb") as o:
        shutil.copyfileobj(f, o)
    with gzip.open(os.path.join(GOLDEN, "corpus10k.out.csv.gz"), "rb") as f:
        golden = f.read()
    return str(p), golden


@pytest.fixture(scope="module")
def corpus_db(corpus, gpu_ctx):
    """The corpus loaded once with all nine columns resident, and its result."""
    db = rk.FragmentsDatabase(corpus[0], ctx=gpu_ctx, keep_rows=True)
    res = gpu_ctx.classify_db(db, 0.3, 0.3)
    yield db, res
    db.close()


# ---- 1: fixtures ------------------------------------------------------------

with open(os.path.join(EDGE, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
WITH_OUT = sorted(os.path.basename(p)[:-8] for p in glob.glob(os.path.join(EDGE, "*.out.csv")))


@pytest.mark.parametrize("name", WITH_OUT)
def test_edge_fixture(name, gpu_ctx, tmp_path):
    case = MANIFEST[name]
    db = rk.FragmentsDatabase(os.path.join(EDGE, name + ".in.csv"), ctx=gpu_ctx, keep_rows=True)
    res = gpu_ctx.classify_db(db, case["len_ratio"], case["pos_ratio"])
    dev, st = both_routes(db, gpu_ctx, res, tmp_path)
    with open(os.path.join(EDGE, name + ".out.csv"), "rb") as f:
        assert dev == f.read()
    want = expected_host_rows(db, res, tmp_path / "c")
    assert st["host_rows"] == want
    assert st["rows"] == res.out_order.shape[0]
    if name.startswith(("e06", "e07")):
        assert want > 0
    db.close()


# ---- 2: corpus ----------------------------------------------------------------

def test_corpus(corpus, corpus_db, gpu_ctx, tmp_path):
    db, res = corpus_db
    dev, st = both_routes(db, gpu_ctx, res, tmp_path)
    assert dev == corpus[1]
    with open(corpus[0], "rb") as f:
        head = b"".join(f.readlines()[:16])
    assert dev.startswith(head)
    assert st["host_rows"] == 0 and st["chunks"] == 1 and st["rows"] == 10000
    assert st["bytes"] == len(dev) - len(head)
    assert expected_host_rows(db, res, tmp_path / "c") == 0


# ---- 3: chunks ------------------------------------------------------------------

@pytest.mark.parametrize("rows", ["1", "255", "256", "257", "n-1", "n", "n+1"])
def test_chunks(rows, corpus, corpus_db, gpu_ctx, tmp_path, monkeypatch):
    db, res = corpus_db
    if rows == "1":  # one row per chunk: the first 700 rows of the result only
        res = rk.ClassifyResult(res.gid[:700].copy(), res.repval[:700].copy(),
                                res.out_order[:700].copy(), res.n_groups)
    n_out = res.out_order.shape[0]
    R = {"n-1": n_out - 1, "n": n_out, "n+1": n_out + 1}.get(rows) or int(rows)
    hp = str(tmp_path / "host.csv")
    db.save_all_frag_pairs(hp, res)
    monkeypatch.setenv("RK_CSV_OUT_ROWS", str(R))
    dp = str(tmp_path / "dev.csv")
    db.save_all_frag_pairs_device(gpu_ctx, dp, res)
    st = gpu_ctx.egress_stats()
    with open(hp, "rb") as f, open(dp, "rb") as g:
        host, dev = f.read(), g.read()
    assert dev == host
    if rows != "1":
        assert dev == corpus[1]
    assert st["chunks"] == -(-n_out // R) and st["rows"] == n_out


# ---- 4: the primitive with a synthetic result ---------------------------------------

# similarity spellings inside the device's range, on its edges, and outside;
# ident = (uint64_t)similarity gets every digit count from 1 to 19 from them
SIMS_INSIDE = ["93.45", "0", "100", "7.", ".5", "0.001", "0.0010001", "999999", "999999.4",
               "12345.67", "0.0123456", "1", "99.99995", "0.5", "50", "1.5", "15", "150", "1500",
               "15000", "150000"]
SIMS_OUTSIDE = ["1e6", "1000000", "999999.5", "999999.97", "0.00099999", "0.0009", "-3.25", "-0",
                "1.2e-38", "nan", "inf", "-inf", "3e19", "1234567", "-1"] + \
               [f"1.5e{d - 1}" for d in range(7, 20)]


def wide_rows(n, seed):
    rnd = random.Random(seed)

    def u64():
        d = rnd.randrange(1, 20)  # 1..19 digits
        return str(rnd.randrange(10 ** (d - 1) if d > 1 else 0, min(10 ** d, 2 ** 63)))

    rows = []
    for i in range(n):
        sim = rnd.choice(SIMS_INSIDE if rnd.random() < 0.7 else SIMS_OUTSIDE)
        # a length near ident keeps the identity inside the device's range often
        if rnd.random() < 0.6:
            ln = str(rnd.randrange(1, 1000))
        else:
            ln = u64()
        rows.append((u64(), u64(), u64(), u64(), rnd.choice("fr"), ln, u64(), sim))
    return rows


@pytest.fixture(scope="module")
def wide_db(tmp_path_factory, gpu_ctx):
    p = write_input(tmp_path_factory.mktemp("wide") / "wide.csv", wide_rows(20_000, 11))
    db = rk.FragmentsDatabase(p, ctx=gpu_ctx, keep_rows=True)
    assert db.frags.n == 20_000
    yield db
    db.close()


def test_primitive_host_arrays(wide_db, gpu_ctx, tmp_path):
    res = synthetic_result(20_000, 20_000, 3)
    dev, st = both_routes(wide_db, gpu_ctx, res, tmp_path)
    want = expected_host_rows(wide_db, res, tmp_path / "c")
    assert st["host_rows"] == want and 1000 < want < 19_000
    assert st["rows"] == 20_000 and st["upload_ms"] > 0
    # every digit count of a u64 column is present
    body = dev.split(b"\n")[16:-1]
    assert {len(l.split(b",")[1]) for l in body} == set(range(1, 20))
    assert {len(l.split(b",")[9]) for l in body} >= set(range(1, 20))


def test_primitive_device_tensors(wide_db, gpu_ctx, tmp_path):
    import torch
    res = synthetic_result(20_000, 17_001, 4)
    hp, dp = str(tmp_path / "host.csv"), str(tmp_path / "dev.csv")
    wide_db.save_all_frag_pairs(hp, res)
    dev = torch.device("cuda", gpu_ctx.device)
    t = [torch.from_numpy(a.view(v)).to(dev) for a, v in
         ((res.out_order, np.int32), (res.gid, np.int32), (res.repval, np.uint8))]
    torch.cuda.synchronize()
    wide_db.save_all_frag_pairs_device(gpu_ctx, dp, tuple(t))
    st = gpu_ctx.egress_stats()
    with open(hp, "rb") as f, open(dp, "rb") as g:
        assert g.read() == f.read()
    assert st["rows"] == 17_001 and st["upload_ms"] == 0


# ---- 5: block boundaries --------------------------------------------------------------

BIG = "9223372036854775807"
NEG = "-1"  # atoll gives -1: 18446744073709551615 as u64, 20 digits


def boundary_rows(n):
    rows = []
    for i in range(n):
        if i % 2 == 0:    # the shortest row: 31 bytes
            rows.append(("0", "0", "0", "0", "f", "1", "0", "0"))
        elif i % 4 == 1:  # the longest rows the device formats; the width varies with i
            rows.append((NEG, NEG, "1" * (1 + i % 19), NEG, "r", NEG, NEG, "0.00123457"))
        else:             # the longest row: a host row
            rows.append((NEG, NEG, NEG, NEG, "r", NEG, NEG, "-1.23457e18"))
    return rows


@pytest.fixture(scope="module")
def boundary_db(tmp_path_factory, gpu_ctx):
    p = write_input(tmp_path_factory.mktemp("bound") / "b.csv", boundary_rows(513))
    db = rk.FragmentsDatabase(p, ctx=gpu_ctx, keep_rows=True)
    assert db.frags.n == 513
    yield db
    db.close()


@pytest.mark.parametrize("n_out", [0, 1, 255, 256, 257, 513])
def test_block_boundaries(n_out, boundary_db, gpu_ctx, tmp_path):
    k = np.arange(n_out, dtype=np.uint32)
    res = rk.ClassifyResult((k * 7919).astype(np.uint32), (k % 3).astype(np.uint8), k, n_out)
    dev, st = both_routes(boundary_db, gpu_ctx, res, tmp_path)
    lines = dev.split(b"\n")[16:-1]
    assert len(lines) == n_out and st["rows"] == n_out
    assert st["host_rows"] == sum(1 for i in range(n_out) if i % 4 == 3)
    if n_out:
        assert min(map(len, lines)) == 30 and st["chunks"] == 1
    else:
        assert dev == header(513) and st["chunks"] == 0
    if n_out >= 4:
        assert max(map(len, lines)) > 180
    if n_out == 513:
        # the 128-row blocks' byte ranges start at several alignments
        starts = np.cumsum([0] + [len(l) + 1 for l in lines])[::128]
        assert len({int(s) % 16 for s in starts}) >= 3


# ---- 6: every row a host row ---------------------------------------------------------------

def test_every_row_a_host_row(gpu_ctx, tmp_path):
    """length == 0: the identity is NaN or inf, every row goes through the host
    fix-up (its threaded form, above 16k rows)."""
    rows = [(str(1000 + i), str(2000 + i), "5", "6", "fr"[i & 1], "0", str(i % 97),
             ["0", "93.45", "7"][i % 3]) for i in range(40_000)]
    db = rk.FragmentsDatabase(write_input(tmp_path / "z.csv", rows), ctx=gpu_ctx, keep_rows=True)
    res = synthetic_result(40_000, 40_000, 6)
    dev, st = both_routes(db, gpu_ctx, res, tmp_path)
    assert st["host_rows"] == 40_000 and st["rows"] == 40_000 and st["host_fix_ms"] > 0
    db.close()


def test_one_host_row_at_the_block_edges(gpu_ctx, tmp_path):
    """One host row per 256 output rows, at lane 0 and at lane 255."""
    n = 256 * 12
    rows = []
    for i in range(n):
        edge = (i % 512 == 0) or (i % 512 == 511)
        rows.append((str(i), str(i * 3), str(i + 9), "4", "f", "0" if edge else "100", "1",
                     "93.45"))
    db = rk.FragmentsDatabase(write_input(tmp_path / "e.csv", rows), ctx=gpu_ctx, keep_rows=True)
    k = np.arange(n, dtype=np.uint32)
    res = rk.ClassifyResult(k.copy(), (k % 3).astype(np.uint8), k, n)
    dev, st = both_routes(db, gpu_ctx, res, tmp_path)
    assert st["host_rows"] == 12
    db.close()


# ---- 7: errors ----------------------------------------------------------------------------------

def test_errors(corpus, corpus_db, gpu_ctx, tmp_path):
    db, res = corpus_db
    missing = tmp_path / "no-such-dir" / "out.csv"
    with pytest.raises(rk.RkError) as e:
        db.save_all_frag_pairs_device(gpu_ctx, str(missing), res)
    assert e.value.code == -2 and not missing.parent.exists()
    bad = rk.ClassifyResult(res.gid.copy(), res.repval.copy(), res.out_order.copy(), res.n_groups)
    bad.out_order[5000] = db.frags.n
    with pytest.raises(rk.RkError) as e:
        db.save_all_frag_pairs_device(gpu_ctx, str(tmp_path / "bad.csv"), bad)
    assert e.value.code == -1
    r = res.as_struct()
    lib = rk.load_library()
    assert lib.rk_db_write_csv_device(gpu_ctx._h, db._h, str(tmp_path / "f.csv").encode(), r,
                                      2) == -1  # an unknown flag bit
    only4 = rk.FragmentsDatabase(corpus[0], ctx=gpu_ctx, keep_device=True)
    with pytest.raises(rk.RkError) as e:
        only4.save_all_frag_pairs_device(gpu_ctx, str(tmp_path / "k.csv"), res)
    assert e.value.code == -1 and "RK_DB_KEEP_ROWS" in str(e.value)
    assert not (tmp_path / "k.csv").exists()
    only4.close()
    # a clean call on the same context afterwards
    dev, st = both_routes(db, gpu_ctx, res, tmp_path)
    assert dev == corpus[1]


# ---- 8: classify_db_to_csv ---------------------------------------------------------------------------

def test_classify_db_to_csv(corpus_db, gpu_ctx, tmp_path):
    db, _ = corpus_db
    pairs = [(0.3, 0.3), (0.05, 0.05)]
    paths = [str(tmp_path / "a.csv"), str(tmp_path / "b.csv")]
    got = gpu_ctx.classify_db_to_csv(db, pairs, paths)
    st = gpu_ctx.egress_stats()
    files = []
    for (lr, pr), path, (n_out, n_groups) in zip(pairs, paths, got):
        res = gpu_ctx.classify_db(db, lr, pr)
        assert (n_out, n_groups) == (res.out_order.shape[0], res.n_groups)
        hp = path + ".host"
        db.save_all_frag_pairs(hp, res)
        with open(hp, "rb") as f, open(path, "rb") as g:
            files.append(g.read())
            assert files[-1] == f.read()
    assert files[0] != files[1]
    assert st["rows"] == got[1][0] and st["upload_ms"] == 0  # the last pair's


# ---- 9: CLI ---------------------------------------------------------------------------------------------

def test_cli_device_save(corpus, tmp_path):
    out = tmp_path / "out.csv"
    p = subprocess.run([rk.CLI_PATH, "--device-parse", "--device-save", "--timing", corpus[0],
                        str(out), "0.3", "0.3"], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert '"egress"' in p.stderr
    assert out.read_bytes() == corpus[1]


def test_cli_device_save_usage(corpus, tmp_path):
    p = subprocess.run([rk.CLI_PATH, "--device-save", corpus[0], str(tmp_path / "o.csv"), "0.3",
                        "0.3"], capture_output=True, text=True, timeout=60)
    assert p.returncode == 1 and "--device-save" in p.stderr
    assert not (tmp_path / "o.csv").exists()


def test_cli_device_save_fallback(corpus, tmp_path):
    """An output path that cannot be opened: the pair goes to represults-1.csv in
    the working directory, with the saver thread's message (SaverQueue.cpp:16-20)."""
    out = tmp_path / "no-such-dir" / "out.csv"
    p = subprocess.run([rk.CLI_PATH, "--device-parse", "--device-save", corpus[0], str(out),
                        "0.3", "0.3"], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert p.returncode == 0, p.stdout + p.stderr
    assert f"Couldn't access {out}, saving into represults-1.csv" in p.stderr
    assert (tmp_path / "represults-1.csv").read_bytes() == corpus[1]
    assert not out.parent.exists()
