"""Batched sets as files (rk_dbset_*): many CSVs parsed on the GPU as one byte
stream, classified by the batched pipeline and formatted on the GPU, every
set's text going to its own file.

The expected bytes are the reference's fixtures under tests/golden/ where one
exists; elsewhere they come from the unchanged host route of the same build,
per file: rk_db_load_csv, classify_batch, rk_db_write_csv."""
import gzip
import json
import os
import random
import resource
import shutil
import subprocess

import numpy as np
import pytest

from conftest import EDGE, GOLDEN

import repkiller_amd as rk

pytestmark = pytest.mark.gpu

SEQ = 1_000_000


def header(total, seq=SEQ):
    out = []
    for k in range(1, 17):
        if k == 7:
            out.append(f"SeqX length : {seq}")
        elif k == 8:
            out.append(f"SeqY length : {seq}")
        elif k == 13:
            out.append(f"Total fragments : {total}")
        else:
            out.append(f"header line {k}")
    return ("\n".join(out) + "\n").encode()


def row(rnd, sim=None, length=None, seq=SEQ, pad=0):
    """One body line (no newline); pad: blanks before an integer field, which
    atoll skips."""
    ln = rnd.randrange(50, 500) if length is None else length
    xs, ys = rnd.randrange(100, seq - 2000), rnd.randrange(100, seq - 2000)
    sim = f"{rnd.randrange(5000, 10000) / 100:.2f}" if sim is None else sim
    return (f"Frag,{xs},{ys},{' ' * pad}{xs + ln},{ys + ln},{rnd.choice('fr')},0,{ln},"
            f"{4 * ln},{rnd.randrange(0, ln + 1)},{sim},90.00,0,1")


def write_set(path, lines, final_newline=True, total=None, seq=SEQ):
    body = "\n".join(lines) + ("\n" if lines and final_newline else "")
    with open(path, "wb") as f:
        f.write(header(len(lines) if total is None else total, seq))
        f.write(body.encode())
    return str(path)


def host_route(ctx, ins, outs, lr=0.3, pr=0.3):
    """The yardstick: every file through the host parser, one classify_batch,
    the host writer per file."""
    dbs = [rk.FragmentsDatabase(p) for p in ins]
    res = ctx.classify_batch([(d.frags, d.len_x_hdr, d.len_y_hdr) for d in dbs], lr, pr)
    for d, r, o in zip(dbs, res, outs):
        d.save_all_frag_pairs(str(o), r)
    for d in dbs:
        d.close()
    return res


def device_route(ctx, ins, outs, lr=0.3, pr=0.3):
    dbs = rk.FragmentsDatabaseSet(ins, ctx, keep_rows=True)
    try:
        n_out, n_groups = ctx.classify_dbset_to_csv(dbs, [str(o) for o in outs], lr, pr)
        return n_out, n_groups, dbs.set_off.copy()
    finally:
        dbs.close()


def read(p):
    with open(p, "rb") as f:
        return f.read()


def same_as_host(ctx, ins, d, tag="x"):
    """Both routes over the list; every file of the device route equals the host
    route's.  Returns the device route's (n_out, n_groups, set_off)."""
    d = d / tag
    d.mkdir()
    ho = [d / f"{k}.host.csv" for k in range(len(ins))]
    do = [d / f"{k}.dev.csv" for k in range(len(ins))]
    host_route(ctx, ins, ho)
    n_out, n_groups, set_off = device_route(ctx, ins, do)
    for k in range(len(ins)):
        assert read(do[k]) == read(ho[k]), f"set {k} ({ins[k]}) differs from the host route"
    return n_out, n_groups, set_off, do


def edge_in(name):
    return os.path.join(EDGE, name + ".in.csv")


def golden_names():
    with open(os.path.join(EDGE, "manifest.json")) as f:
        man = json.load(f)
    return sorted(n for n, m in man.items()
                  if m["expect"] == "ref" and (m["len_ratio"], m["pos_ratio"]) == (0.3, 0.3))


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    d = tmp_path_factory.mktemp("csvbatch")
    p = d / "corpus10k.in.csv"
    with gzip.open(os.path.join(GOLDEN, "corpus10k.in.csv.gz"), "rb") as f, open(p, "wb") as o:
        shutil.copyfileobj(f, o)
    with gzip.open(os.path.join(GOLDEN, "corpus10k.out.csv.gz"), "rb") as f:
        golden = f.read()
    return str(p), golden


# ---- 1: golden ---------------------------------------------------------------

def golden_lists():
    names = golden_names()
    assert len(names) == 14
    rest = [n for n in names if n not in ("e16_no_final_newline", "e13_no_fragments")]
    e16, e13 = "e16_no_final_newline", "e13_no_fragments"
    return {
        "sorted": names,
        "reversed": names[::-1],
        "e16_first": [e16] + rest + [e13],
        "e16_middle": rest[:5] + [e16] + rest[5:] + [e13],
        "e13_first": [e13] + rest + [e16],
        "e13_last": [e16] + rest + [e13],
        "e13_twice": rest[:4] + [e13, e13] + rest[4:] + [e16],
        "one_three_times": ["e05b_big_group_ties"] * 3,
        # one set is a legal batch; its body still gets its newline in the stream
        "e16_alone": [e16],
        "e13_alone": [e13],
    }


@pytest.mark.parametrize("which", sorted(golden_lists()))
def test_golden(which, gpu_ctx, tmp_path):
    names = golden_lists()[which]
    ins = [edge_in(n) for n in names]
    outs = [tmp_path / f"{k}_{n}.csv" for k, n in enumerate(names)]
    device_route(gpu_ctx, ins, outs)
    for n, o in zip(names, outs):
        assert read(o) == read(os.path.join(EDGE, n + ".out.csv")), n


def test_golden_e14_own_ratios(gpu_ctx, tmp_path):
    out = tmp_path / "e14.csv"
    device_route(gpu_ctx, [edge_in("e14_tie_newest_wins")], [out], 0.5, 0.3)
    assert read(out) == read(os.path.join(EDGE, "e14_tie_newest_wins.out.csv"))


# ---- 2: ingress parity ---------------------------------------------------------

def download(view, n):
    """The four resident columns as host arrays."""
    lib = hip_runtime()
    out = []
    for name, dt in (("x_start", np.uint64), ("y_start", np.uint64), ("length", np.uint64),
                     ("strand", np.uint8)):
        a = np.empty(n, dt)
        if n:
            assert lib.hipMemcpy(a.ctypes.data, view[name], a.nbytes, 2) == 0
        out.append(a)
    return out


def hip_runtime():
    """hipMemcpy of the HIP runtime the library itself is linked against (a
    symbol lookup on the library's handle searches its dependencies)."""
    import ctypes
    lib = rk.load_library()
    lib.hipMemcpy.restype = ctypes.c_int
    lib.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    return lib


@pytest.mark.parametrize("which", sorted(golden_lists()))
def test_ingress_parity(which, gpu_ctx):
    names = golden_lists()[which]
    ins = [edge_in(n) for n in names]
    host = [rk.FragmentsDatabase(p) for p in ins]
    dbs = rk.FragmentsDatabaseSet(ins, gpu_ctx, keep_device=True)
    assert dbs.nsets == len(ins)
    want_off = np.concatenate([[0], np.cumsum([d.frags.n for d in host])]).astype(np.uint64)
    assert np.array_equal(dbs.set_off, want_off)
    for k, d in enumerate(host):
        assert (dbs.len_x_hdr[k], dbs.len_y_hdr[k], dbs.total_hdr[k]) == \
            (d.len_x_hdr, d.len_y_hdr, d.total_hdr), names[k]
        f = dbs.frags(k)
        for col in ("x_start", "y_start", "length", "strand"):
            assert np.array_equal(getattr(f, col), getattr(d.frags, col)), (names[k], col)
    view = dbs.device_view()
    assert view["n"] == int(want_off[-1])
    got = download(view, view["n"])
    h = dbs._host
    for a, b in zip(got, (h.x_start, h.y_start, h.length, h.strand)):
        assert np.array_equal(a, b)
    st = gpu_ctx.ingress_stats()
    assert st["accepted"] == int(dbs.set_off[-1])
    dbs.close()
    for d in host:
        d.close()


@pytest.mark.parametrize("page_multiple", [False, True])
def test_one_set_without_final_newline(page_multiple, gpu_ctx, tmp_path):
    """A one-file batch whose body does not end in a newline: the stream's last
    byte is the appended newline, which is not a byte of the file (with
    page_multiple the file ends exactly at the end of its mapping's last page)."""
    rnd = random.Random(16)
    lines = [row(rnd) for _ in range(40)]
    if page_multiple:
        size = len(header(len(lines))) + len("\n".join(lines))
        f = lines[-1].split(",")
        f[3] = " " * (-size % 4096) + f[3]
        lines[-1] = ",".join(f)
    p = write_set(tmp_path / "one.csv", lines, final_newline=False)
    assert not read(p).endswith(b"\n")
    assert (os.path.getsize(p) % 4096 == 0) == page_multiple
    host = rk.FragmentsDatabase(p)
    assert host.frags.n == len(lines)
    dbs = rk.FragmentsDatabaseSet([p], gpu_ctx, keep_device=True)
    assert list(dbs.set_off) == [0, len(lines)]
    f = dbs.frags(0)
    for col in ("x_start", "y_start", "length", "strand"):
        assert np.array_equal(getattr(f, col), getattr(host.frags, col)), col
    st = gpu_ctx.ingress_stats()
    assert st["lines"] == st["accepted"] == len(lines)
    assert st["body_bytes"] == os.path.getsize(p) - len(header(len(lines)))
    dbs.close()
    host.close()
    n_out, _, _, _ = same_as_host(gpu_ctx, [p], tmp_path)
    assert int(n_out[0]) == len(lines)


def test_empty_list(gpu_ctx):
    dbs = rk.FragmentsDatabaseSet([], gpu_ctx, keep_rows=True)
    assert dbs.nsets == 0 and list(dbs.set_off) == [0]
    assert gpu_ctx.classify_dbset(dbs) == []
    n_out, _ = gpu_ctx.classify_dbset_to_csv(dbs, [])
    assert len(n_out) == 0
    dbs.close()


def test_device_view_needs_keep_device(gpu_ctx):
    dbs = rk.FragmentsDatabaseSet([edge_in("e03_strands")], gpu_ctx)
    with pytest.raises(rk.RkError):
        dbs.device_view()
    with pytest.raises(rk.RkError) as e:
        gpu_ctx.classify_dbset(dbs)
    assert e.value.code == -1
    dbs.close()


# ---- 3: block, tile and chunk seams --------------------------------------------------

PIECES = (1, 2, 127, 128, 129, 255, 256, 257, 511, 513)


@pytest.fixture(scope="module")
def corpus_pieces(corpus, gpu_ctx, tmp_path_factory):
    """The corpus body cut at line boundaries into consecutive pieces, each under
    the corpus header (its total of 10k leaves no count overflow)."""
    d = tmp_path_factory.mktemp("pieces")
    lines = read(corpus[0]).split(b"\n")
    head, body = lines[:16], [x for x in lines[16:] if x]
    ins, at = [], 0
    for k, cnt in enumerate(PIECES + (len(body),)):
        part = body[at:at + cnt]
        at += len(part)
        p = d / f"piece{k}.csv"
        p.write_bytes(b"\n".join(head) + b"\n" + b"".join(x + b"\n" for x in part))
        ins.append(str(p))
    assert at == len(body)
    ho = [d / f"{k}.host.csv" for k in range(len(ins))]
    host_route(gpu_ctx, ins, ho)
    return ins, [read(p) for p in ho]


@pytest.mark.parametrize("env", [None, ("RK_CSV_OUT_ROWS", "1"), ("RK_CSV_OUT_ROWS", "100"),
                                 ("RK_CSV_OUT_ROWS", "128"), ("RK_CSV_OUT_ROWS", "129"),
                                 ("RK_CSV_WINDOW", "100"), ("RK_CSV_WINDOW", "4096")])
def test_seams(env, corpus_pieces, gpu_ctx, tmp_path, monkeypatch):
    ins, want = corpus_pieces
    if env:
        monkeypatch.setenv(*env)
    outs = [tmp_path / f"{k}.csv" for k in range(len(ins))]
    n_out, _, set_off = device_route(gpu_ctx, ins, outs)
    for k in range(len(ins)):
        assert read(outs[k]) == want[k], f"piece {k}"
    ing, eg = gpu_ctx.ingress_stats(), gpu_ctx.egress_stats()
    assert ing["accepted"] == int(set_off[-1])
    if env and env[0] == "RK_CSV_WINDOW":
        assert ing["windows"] > 1
    if env and env[0] == "RK_CSV_OUT_ROWS":
        assert eg["chunks"] == -(-int(set_off[-1]) // int(env[1]))


# ---- 4: byte seams ---------------------------------------------------------------------

def padded_body(rnd, size, final_newline):
    """Lines whose bytes (newlines included, the last only with final_newline)
    sum to exactly `size`."""
    lines, used = [], 0
    while True:
        ln = row(rnd)
        if size - used - len(ln) - 1 < 200:  # the last line takes the rest as blanks
            pad = size - used - len(ln) - (1 if final_newline else 0)
            assert 0 <= pad <= 400, (size, used, pad)
            f = ln.split(",")
            f[3] = " " * pad + f[3]
            lines.append(",".join(f))
            return lines
        lines.append(ln)
        used += len(ln) + 1


@pytest.mark.parametrize("final_newline", [True, False])
def test_byte_seams(final_newline, gpu_ctx, tmp_path):
    """Bodies that end at combined-stream offsets 2048 m - 1, 2048 m, 2048 m + 1
    (the line index's tile) and the same around multiples of 16 (its load)."""
    rnd = random.Random(7)
    targets = [16 * 65 - 1, 2048 - 1, 16 * 195, 2048 * 2, 16 * 323 + 1, 2048 * 3 + 1,
               2048 * 4 - 1, 16 * 600, 2048 * 5, 16 * 700 - 1, 16 * 770 + 1, 2048 * 7 + 1]
    ins, at = [], 0
    for k, t in enumerate(targets):
        # the stream holds one more byte per body without a final newline
        size = t - at
        lines = padded_body(rnd, size, final_newline)
        p = write_set(tmp_path / f"s{k}.csv", lines, final_newline)
        assert os.path.getsize(p) - len(header(len(lines))) == size
        at = t + (0 if final_newline else 1)
        ins.append(p)
    ins.append(write_set(tmp_path / "tail.csv", [row(rnd) for _ in range(5)], final_newline))
    same_as_host(gpu_ctx, ins, tmp_path)
    # the newlines the stream adds are not bytes of any body
    assert gpu_ctx.ingress_stats()["body_bytes"] == sum(
        len(read(p)) - len(b"".join(x + b"\n" for x in read(p).split(b"\n")[:16])) for p in ins)


# ---- 5: host lines and host rows at set edges ----------------------------------------

def test_host_lines_and_rows_at_set_edges(gpu_ctx, tmp_path):
    rnd = random.Random(11)
    cap = rk.load_library().rk_csv_max_line()
    exp = lambda: row(rnd, sim="9.345e+01")                 # CSV_HOST: strtof
    longl = lambda: row(rnd, pad=cap + 10)                  # CSV_HOST: longer than a lane parses
    zero = lambda: row(rnd, length=0)                       # ROW_HOST: identity is not finite
    big = lambda: row(rnd, sim="999999.9")                  # ROW_HOST: prints as 1e+06
    plain = lambda k: [row(rnd) for _ in range(k)]
    sets = [
        ([exp()] + plain(5), True),                # host line first
        (plain(5) + [longl()], True),              # host line last
        (plain(4) + [exp()], False),               # host line last, no newline
        ([longl()] + plain(3) + [exp()], False),
        ([exp(), longl(), exp(), exp()], True),    # only host lines
        ([zero()] + plain(6), True),               # host row first
        (plain(6) + [big()], True),                # host row last
        (plain(3) + [zero()], False),              # host row last, no newline
        ([zero(), big(), zero()], False),          # only host rows
        ([exp()], False),
        (plain(300), True),
    ]
    ins = [write_set(tmp_path / f"s{k}.csv", lines, nl) for k, (lines, nl) in enumerate(sets)]
    n_out, _, set_off, _ = same_as_host(gpu_ctx, ins, tmp_path)
    ing, eg = gpu_ctx.ingress_stats(), gpu_ctx.egress_stats()
    host_lines = sum(1 for lines, _ in sets for ln in lines
                     if "e+01" in ln or len(ln) > cap)
    assert ing["host_lines"] == host_lines
    assert ing["lines"] == sum(len(lines) for lines, _ in sets)
    assert ing["accepted"] == int(set_off[-1]) == ing["lines"]
    # every row is written here (no row sits in a last xStart/10 bucket), so the
    # host rows are the ones built above
    assert int(n_out.sum()) == ing["lines"]
    host_rows = sum(1 for lines, _ in sets for ln in lines
                    if ln.split(",")[7] == "0" or ln.split(",")[10] == "999999.9")
    assert eg["host_rows"] == host_rows and eg["rows"] == int(n_out.sum())


# ---- 6: many tiny sets ---------------------------------------------------------------

def test_many_tiny_sets(gpu_ctx, tmp_path):
    rnd = random.Random(2000)
    d = tmp_path / "in"
    d.mkdir()
    ins = []
    for k in range(2000):
        cnt = 0 if 700 <= k < 1000 else rnd.randrange(0, 6)
        lines = [row(rnd, seq=100_000) for _ in range(cnt)]
        ins.append(write_set(d / f"{k}.csv", lines, rnd.random() < 0.7, seq=100_000))
    n_out, _, set_off, outs = same_as_host(gpu_ctx, ins, tmp_path)
    assert int(set_off[-1]) > 2000 and set_off[700] == set_off[1000]
    # 9: the stats run over all sets
    ing, eg = gpu_ctx.ingress_stats(), gpu_ctx.egress_stats()
    assert ing["accepted"] == int(set_off[-1])
    assert eg["rows"] == int(n_out.sum())
    hdr = len(header(0, 100_000))
    assert eg["bytes"] == sum(os.path.getsize(o) - hdr for o in outs)


# ---- 7: errors -------------------------------------------------------------------------

def test_count_overflow_names_the_lowest_set(gpu_ctx):
    names = golden_names()[:9]
    ins = [edge_in(n) for n in names]
    ins[3] = ins[7] = edge_in("e08_count_overflow")
    with pytest.raises(rk.RkError) as e:
        rk.FragmentsDatabaseSet(ins, gpu_ctx, keep_rows=True)
    assert e.value.code == -3 and "set 3" in str(e.value)


def test_io_error_comes_before_the_count_check(gpu_ctx, tmp_path):
    ins = [edge_in(n) for n in golden_names()[:8]]
    ins[2] = edge_in("e08_count_overflow")
    ins[5] = str(tmp_path / "missing.csv")
    with pytest.raises(rk.RkError) as e:
        rk.FragmentsDatabaseSet(ins, gpu_ctx)
    assert e.value.code == -2 and "set 5" in str(e.value)


def test_classification_error_opens_no_output(gpu_ctx, tmp_path):
    names = golden_names()[:4] + ["e11a_ub_xstart_bucket"] + golden_names()[4:6]
    ins = [edge_in(n) for n in names]
    outs = [tmp_path / f"{k}.csv" for k in range(len(ins))]
    dbs = rk.FragmentsDatabaseSet(ins, gpu_ctx, keep_rows=True)
    with pytest.raises(rk.RkError) as e:
        gpu_ctx.classify_dbset_to_csv(dbs, outs)
    dbs.close()
    assert e.value.code == -4 and "set 4" in str(e.value)
    assert os.listdir(tmp_path) == []


def test_unopenable_output_names_the_set(gpu_ctx, tmp_path):
    names = golden_names()
    ins = [edge_in(n) for n in names]
    K = 6
    outs = [tmp_path / f"{k}.csv" for k in range(len(ins))]
    outs[K] = tmp_path / "no_such_dir" / "x.csv"
    dbs = rk.FragmentsDatabaseSet(ins, gpu_ctx, keep_rows=True)
    with pytest.raises(rk.RkError) as e:
        gpu_ctx.classify_dbset_to_csv(dbs, outs)
    dbs.close()
    assert e.value.code == -2 and f"set {K}" in str(e.value)
    for k in range(K):
        assert read(outs[k]) == read(os.path.join(EDGE, names[k] + ".out.csv")), names[k]


def test_out_order_past_its_set(gpu_ctx, tmp_path):
    ins = [edge_in(n) for n in ("e03_strands", "e05b_big_group_ties", "e15_processing_order")]
    outs = [tmp_path / f"{k}.csv" for k in range(3)]
    dbs = rk.FragmentsDatabaseSet(ins, gpu_ctx, keep_rows=True)
    res = gpu_ctx.classify_dbset(dbs)
    dbs.save_all_device(gpu_ctx, outs, res)  # the host-array form of the save
    for k, (n, o) in enumerate(zip(("e03_strands", "e05b_big_group_ties",
                                    "e15_processing_order"), outs)):
        assert read(o) == read(os.path.join(EDGE, n + ".out.csv")), n
        dbs.save_set(k, tmp_path / "host.csv", res[k])  # and the host save of one set
        assert read(tmp_path / "host.csv") == read(o), n
    # an entry that is a valid COMBINED row but not a row of its set
    rows1 = int(dbs.set_off[2] - dbs.set_off[1])
    bad = rk.ClassifyResult(res[1].gid.copy(), res[1].repval.copy(), res[1].out_order.copy(),
                            res[1].n_groups)
    bad.out_order[len(bad.out_order) // 2] = rows1
    with pytest.raises(rk.RkError) as e:
        dbs.save_all_device(gpu_ctx, outs, [res[0], bad, res[2]])
    assert e.value.code == -1
    dbs.close()


# ---- 8: context reuse --------------------------------------------------------------------

def test_context_reuse(corpus, gpu_ctx, tmp_path):
    names = golden_names()
    ins = [edge_in(n) for n in names]
    a = [tmp_path / f"a{k}.csv" for k in range(len(ins))]
    b = [tmp_path / f"b{k}.csv" for k in range(len(ins))]
    device_route(gpu_ctx, ins, a)
    db = rk.FragmentsDatabase(corpus[0], ctx=gpu_ctx, keep_rows=True)
    one = tmp_path / "corpus.csv"
    gpu_ctx.classify_db_to_csv(db, [(0.3, 0.3)], [str(one)])
    db.close()
    assert read(one) == corpus[1]
    device_route(gpu_ctx, ins, b)
    for k, n in enumerate(names):
        assert read(a[k]) == read(b[k]) == read(os.path.join(EDGE, n + ".out.csv")), n


# ---- 9: one chunk driver, two routes -------------------------------------------------------

ROUTE_ROWS, ROUTE_CHUNK = 300, 129


@pytest.fixture(scope="module")
def two_routes(gpu_ctx, tmp_path_factory):
    """The same 300 rows (the single route's boundary_rows: shortest rows, longest
    device rows, a host row in every fourth place) as an rk_db and as a one-set
    rk_dbset, one synthetic result over all of them, and the host writer's file."""
    import test_csv_egress_device as single
    d = tmp_path_factory.mktemp("routes")
    p = single.write_input(d / "b.csv", single.boundary_rows(ROUTE_ROWS))
    db = rk.FragmentsDatabase(p, ctx=gpu_ctx, keep_rows=True)
    dbs = rk.FragmentsDatabaseSet([p], gpu_ctx, keep_rows=True)
    assert db.frags.n == ROUTE_ROWS and list(dbs.set_off) == [0, ROUTE_ROWS]
    k = np.arange(ROUTE_ROWS, dtype=np.uint32)
    res = rk.ClassifyResult((k * 7919).astype(np.uint32), (k % 3).astype(np.uint8), k, ROUTE_ROWS)
    db.save_all_frag_pairs(str(d / "host.csv"), res)
    want = read(d / "host.csv")
    assert len(want.split(b"\n")) == 16 + ROUTE_ROWS + 1
    yield db, dbs, res, want
    dbs.close()
    db.close()


def with_order(res, k, value):
    bad = rk.ClassifyResult(res.gid.copy(), res.repval.copy(), res.out_order.copy(), res.n_groups)
    bad.out_order[k] = value
    return bad


def test_both_routes_same_bytes(two_routes, gpu_ctx, tmp_path, monkeypatch):
    """Three chunks of 129 rows: a 128-row block seam inside the first, host rows
    (every fourth) on both sides of the chunk edges."""
    db, dbs, res, want = two_routes
    monkeypatch.setenv("RK_CSV_OUT_ROWS", str(ROUTE_CHUNK))
    one, batch = tmp_path / "one.csv", tmp_path / "batch.csv"
    db.save_all_frag_pairs_device(gpu_ctx, str(one), res)
    st1 = gpu_ctx.egress_stats()
    dbs.save_all_device(gpu_ctx, [batch], [res])
    stb = gpu_ctx.egress_stats()
    assert read(one) == want, "the single route's file differs from the host writer's"
    assert read(batch) == want, "the batch route's file differs from the host writer's"
    for key in ("rows", "bytes", "host_rows"):
        assert st1[key] == stb[key], key
    assert st1["rows"] == ROUTE_ROWS and st1["host_rows"] == ROUTE_ROWS // 4
    assert st1["bytes"] == len(want) - len(header(ROUTE_ROWS, 1_000_000_000))
    n_out, slots = int(res.out_order.shape[0]), int(dbs.set_off[-1])
    assert st1["chunks"] == -(-n_out // ROUTE_CHUNK) == 3
    assert stb["chunks"] == -(-slots // ROUTE_CHUNK) == 3


def test_error_on_one_route_leaves_the_other_clean(two_routes, gpu_ctx, tmp_path, monkeypatch):
    """An out_order entry past the rows fails the length pass of the second chunk
    (RK_E_ARG, by flag) while the first chunk's patch buffer is live; the next
    write on the same context, through the other route, is whole."""
    db, dbs, res, want = two_routes
    monkeypatch.setenv("RK_CSV_OUT_ROWS", str(ROUTE_CHUNK))
    bad = with_order(res, 200, ROUTE_ROWS)  # (row 200 lies in the second chunk)
    one, batch = tmp_path / "one.csv", tmp_path / "batch.csv"
    with pytest.raises(rk.RkError) as e:
        dbs.save_all_device(gpu_ctx, [batch], [bad])
    assert e.value.code == -1
    db.save_all_frag_pairs_device(gpu_ctx, str(one), res)
    assert read(one) == want
    assert gpu_ctx.egress_stats()["chunks"] == 3
    os.remove(one)
    with pytest.raises(rk.RkError) as e:
        db.save_all_frag_pairs_device(gpu_ctx, str(one), bad)
    assert e.value.code == -1
    dbs.save_all_device(gpu_ctx, [batch], [res])
    assert read(batch) == want
    assert gpu_ctx.egress_stats()["chunks"] == 3


# ---- 10: CLI ---------------------------------------------------------------------------

CLI_NAMES = ["e01_last_bucket", "e13_no_fragments", "e16_no_final_newline"]


@pytest.mark.parametrize("save", [True, False])
def test_cli_batch_device(save, tmp_path):
    lst = tmp_path / "list.tsv"
    lst.write_text("".join(f"{edge_in(n)}\t{tmp_path / (n + '.csv')}\n" for n in CLI_NAMES))
    cmd = [rk.CLI_PATH, "--batch", str(lst), "--device-parse"]
    cmd += ["--device-save", "--timing"] if save else []
    p = subprocess.run(cmd + ["0.3", "0.3"], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    for n in CLI_NAMES:
        assert (tmp_path / (n + ".csv")).read_bytes() == read(os.path.join(EDGE, n + ".out.csv")), n
    if save:
        t = json.loads(p.stderr.strip().splitlines()[-1])
        assert t["sets"] == 3 and t["ingress"]["accepted"] == t["frags"]
        assert {"ingress", "batch", "egress"} <= set(t)


def test_cli_descriptor_bound(tmp_path):
    """600 one-row files under a soft RLIMIT_NOFILE of 256: the descriptors open
    at once are bounded by a constant, not by the sets."""
    rnd = random.Random(3)
    d = tmp_path / "in"
    d.mkdir()
    ins = [write_set(d / f"{k}.csv", [row(rnd, seq=100_000)], seq=100_000) for k in range(600)]

    def run(tag, extra):
        o = tmp_path / tag
        o.mkdir()
        lst = tmp_path / (tag + ".tsv")
        lst.write_text("".join(f"{p}\t{o / (str(k) + '.csv')}\n" for k, p in enumerate(ins)))

        def limit():
            hard = resource.getrlimit(resource.RLIMIT_NOFILE)[1]
            resource.setrlimit(resource.RLIMIT_NOFILE, (256, hard))

        p = subprocess.run([rk.CLI_PATH, "--batch", str(lst)] + extra + ["0.3", "0.3"],
                           capture_output=True, text=True, preexec_fn=limit)
        return p, [o / f"{k}.csv" for k in range(len(ins))]

    control, want = run("host", [])
    if control.returncode != 0:
        pytest.skip("the plain --batch route does not run under RLIMIT_NOFILE 256 here: the "
                    "descriptors the runtime itself needs have not been measured")
    got_p, got = run("dev", ["--device-parse", "--device-save"])
    assert got_p.returncode == 0, got_p.stderr
    for k in range(len(ins)):
        assert read(got[k]) == read(want[k]), k
