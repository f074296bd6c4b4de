"""Device CSV ingress (rk_db_load_csv_device) against the host parser
(rk_db_load_csv): the same file through both routes, both databases saved as SoA
caches, and the two cache files byte-identical -- header text, the three header
numbers, n and all nine columns."""
import glob
import gzip
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

from conftest import EDGE, GOLDEN

import repkiller_amd as rk

pytestmark = pytest.mark.gpu

BASE = "Frag,123456789,223456789,123456999,223456999,f,0,210,840,200,93.45,95.23,0,1"


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


def write_csv(path, body: bytes, total=1 << 40):
    with open(path, "wb") as f:
        f.write(header(total))
        f.write(body)
    return str(path)


def load(route, path, ctx):
    """(cache bytes, n) or the RkError code the route raises."""
    try:
        db = rk.FragmentsDatabase(path) if route == "host" else \
            rk.FragmentsDatabase(path, ctx=ctx, keep_device=True)
    except rk.RkError as e:
        return e.code, None
    tmp = path + "." + route + ".soa"
    db.save_soa(tmp)
    n = db.frags.n
    db.close()
    with open(tmp, "rb") as f:
        blob = f.read()
    os.remove(tmp)
    return blob, n


def same_database(path, ctx):
    """Both routes on `path`; returns (n, ingress stats) when both load."""
    host, n = load("host", path, ctx)
    dev, nd = load("device", path, ctx)
    if isinstance(host, int) or isinstance(dev, int):
        assert host == dev, (host, dev)
        return None, None
    st = ctx.ingress_stats()
    assert n == nd and st["accepted"] == n
    assert host == dev, "the SoA caches of the two routes differ"
    return n, st


@pytest.fixture(scope="module")
def corpus(tmp_path_factory):
    p = tmp_path_factory.mktemp("csvdev") / "corpus10k.in.csv"
    with gzip.open(os.path.join(GOLDEN, "corpus10k.in.csv.gz"), "rb") as f, open(p, "wb") as o:
        shutil.copyfileobj(f, o)
    return str(p)


# ---- 1: fixtures ------------------------------------------------------------

EDGE_FILES = sorted(glob.glob(os.path.join(EDGE, "*.in.csv")))


@pytest.mark.parametrize("name", [os.path.basename(p)[:-7] for p in EDGE_FILES])
def test_edge_fixture(name, gpu_ctx, tmp_path):
    p = str(tmp_path / "in.csv")
    shutil.copy(os.path.join(EDGE, name + ".in.csv"), p)
    n, st = same_database(p, gpu_ctx)
    if name.startswith("e08"):
        assert n is None
        assert load("device", p, gpu_ctx)[0] == -3  # RK_E_COUNT
    else:
        assert n is not None
    if name.startswith("e13"):
        assert n == 0


def test_corpus(corpus, gpu_ctx):
    n, st = same_database(corpus, gpu_ctx)
    assert n > 9000 and st["host_lines"] == 0 and st["windows"] == 1


def test_unopenable_path(gpu_ctx, tmp_path):
    assert load("device", str(tmp_path / "missing.csv"), gpu_ctx)[0] == -2  # RK_E_IO
    assert load("host", str(tmp_path / "missing.csv"), gpu_ctx)[0] == -2


# ---- 2: generated hostile file ------------------------------------------------

SLOW = ["1e3", "9.5E-2", "12345678", "0.123456789", "nan", "-nan", "inf", "0x1p3", "1e50",
        "1e-50", "93.4x", "93.45abc", " 1e2", "\t0x1p3", " nan", "abc", "1.2.3", "16777217"]
FAST = ["93.45", "0", "100", "7.", ".5", "-3.25", "+12.5", "0.0000001234", "0001.50", " 88.1",
        "1234567", "0.1234567", "00.0000000001", "99.99999"]


def hostile_lines(n, seed):
    """[(line bytes, tagged slow-float-with-valid-fields)]; every class of the
    issue's list, each line tagged as it is emitted."""
    rnd = random.Random(seed)
    out = []

    def fields():
        f = BASE.split(",")
        f[1] = str(rnd.randrange(10 ** 8, 10 ** 9))
        f[2] = str(rnd.randrange(10 ** 8, 10 ** 9))
        f[7] = str(rnd.randrange(1, 10 ** 5))
        f[5] = rnd.choice("fr")
        f[10] = rnd.choice(FAST)
        return f

    def big(sign):
        return sign + "".join(rnd.choice("123456789") for _ in range(rnd.randrange(19, 26)))

    for _ in range(n):
        f = fields()
        c = rnd.randrange(40)
        slow = False
        tail = b""
        if c == 0:
            tail = b"\r"
        elif c == 1 and rnd.random() < 0.3:
            out.append((b"", False))
            continue
        elif c == 2 and rnd.random() < 0.5:
            # fewer than 14 fields: the last one repeats, so it is field 10 for
            # k <= 10 -- a number there keeps the line fast; "Frag" alone has
            # valid fields and a field 10 ("Frag") that only strtof can refuse
            k = rnd.choice(list(range(1, 14)))
            f = f[:k]
            if 2 <= k <= 10:
                f[k - 1] = "42"
            slow = k == 1
        elif c == 3:
            f = f + [str(rnd.randrange(100)) for _ in range(rnd.randrange(1, 5))]
        elif c == 4:
            tail = b","
        elif c == 5:
            f[0] = rnd.choice(["frag", "Frag ", "Fra", "Fragx", " Frag"])
        elif c == 6:
            f[rnd.choice([1, 2, 3, 4, 7, 8])] = rnd.choice([" ", "\t ", "  "]) + rnd.choice("+-") + \
                str(rnd.randrange(10 ** 6))
        elif c == 7:
            f[rnd.choice([1, 2, 3, 4, 7, 8])] = big(rnd.choice(["", "-", "+"]))
        elif c == 8:
            f[rnd.choice([1, 2, 3, 4, 7, 8])] = "12a45"
        elif c == 9:
            f[rnd.choice([1, 2, 3, 4, 7, 8])] = "12\x0034"
        elif c in (10, 11, 12, 13):
            f[10] = rnd.choice(SLOW)
            slow = True
        elif c == 14:  # a slow float in a line the field rules reject
            f[10] = rnd.choice(SLOW)
            f[rnd.choice([0, 3, 12])] = "" if rnd.random() < 0.5 else f[0] + "x"
            if f[0] == "Frag" and "" not in f:
                f[0] = "Fraq"
        elif c == 15:
            f[rnd.randrange(1, 14)] = ""
        out.append((",".join(f).encode("latin-1") + tail, slow))
    return out


@pytest.fixture(scope="module")
def hostile_file(tmp_path_factory):
    lines = hostile_lines(20000, 20240607)
    p = tmp_path_factory.mktemp("hostile") / "hostile.csv"
    write_csv(p, b"".join(l + b"\n" for l, _ in lines))
    return str(p), lines


def test_hostile_file(hostile_file, gpu_ctx):
    path, lines = hostile_file
    n, st = same_database(path, gpu_ctx)
    assert st["lines"] == len(lines)
    assert st["host_lines"] == sum(1 for _, slow in lines if slow)
    assert st["host_lines"] > 1000 and 0 < n < len(lines)


def test_every_line_a_host_line(gpu_ctx, tmp_path):
    """A similarity column written with exponents: every line goes through the
    host fix-up (its threaded form, above 16k lines), kept and dropped alike."""
    rnd = random.Random(5)
    f = BASE.split(",")
    lines = []
    for i in range(40_000):
        f[1] = str(100_000_000 + i)
        f[10] = rnd.choice(["9.345e+01", "1.0e2", "7e-1", "1e50", "abc"])
        lines.append(",".join(f))
    p = write_csv(tmp_path / "h.csv", ("\n".join(lines) + "\n").encode())
    n, st = same_database(p, gpu_ctx)
    assert st["host_lines"] == len(lines) and 0 < n < len(lines)


# ---- 3: boundaries -------------------------------------------------------------

def padded_line(length):
    """A valid line of exactly `length` bytes: an integer field padded with
    leading blanks, which atoll skips."""
    f = BASE.split(",")
    pad = length - len(BASE)
    assert pad >= 0
    f[3] = " " * pad + f[3]
    line = ",".join(f)
    assert len(line) == length
    return line.encode()


def boundary_bodies():
    lib = rk.load_library()
    T, cap = lib.rk_csv_tile(), lib.rk_csv_max_line()
    more = (BASE + "\n").encode() * 3
    cases = {}
    for at in (T - 1, T, T + 1):
        cases[f"newline_at_{at - T:+d}"] = (padded_line(at) + b"\n" + more, 0)
    assert T + 30 <= cap, "a line within the cap must be able to span three tiles"
    first = padded_line(T - 10)
    cases["three_tiles"] = (first + b"\n" + padded_line(T + 30) + b"\n" + more, 0)
    cases["over_cap"] = (more + padded_line(cap + 1) + b"\n" + more, 1)
    cases["at_cap"] = (more + padded_line(cap) + b"\n" + more, 0)
    cases["no_newline"] = (BASE.encode(), 0)
    cases["no_newline_garbage"] = (b"xyz", 0)
    cases["only_newlines"] = (b"\n" * 5000, 0)
    cases["empty_body"] = (b"", 0)
    cases["no_final_newline"] = (more + BASE.encode(), 0)
    return cases


@pytest.mark.parametrize("case", ["newline_at_-1", "newline_at_+0", "newline_at_+1",
                                  "three_tiles", "over_cap", "at_cap", "no_newline",
                                  "no_newline_garbage", "only_newlines", "empty_body",
                                  "no_final_newline"])
def test_boundaries(case, gpu_ctx, tmp_path):
    body, host_lines = boundary_bodies()[case]
    p = write_csv(tmp_path / "b.csv", body)
    n, st = same_database(p, gpu_ctx)
    assert st["host_lines"] == host_lines
    assert st["body_bytes"] == len(body)
    want_lines = body.count(b"\n") + (1 if body and not body.endswith(b"\n") else 0)
    assert st["lines"] == want_lines
    if case in ("over_cap", "at_cap"):
        assert n == 7
    if case == "three_tiles":
        assert n == 5
    if case == "only_newlines":
        assert n == 0


# ---- 4: stable compaction across blocks -----------------------------------------

def test_stable_compaction(gpu_ctx, tmp_path):
    n_lines = 300_000
    x = np.arange(n_lines, dtype=np.int64) * 7 + 100_000_000
    good = np.char.add(np.char.add("Frag,", x.astype("U")),
                       ",223456789,123456999,223456999,f,0,210,840,200,93.45,95.23,0,1")
    bad = np.char.add("Frog,", x.astype("U"))
    idx = np.arange(n_lines)
    reject = (idx % 7 == 3) | ((idx >= 131_071) & (idx < 136_071))
    lines = np.where(reject, bad, good)
    p = write_csv(tmp_path / "c.csv", ("\n".join(lines.tolist()) + "\n").encode())
    n, st = same_database(p, gpu_ctx)
    assert n == int((~reject).sum()) and st["lines"] == n_lines and st["host_lines"] == 0


# ---- 5: windows -----------------------------------------------------------------

def test_windows_corpus(corpus, gpu_ctx, monkeypatch):
    monkeypatch.setenv("RK_CSV_WINDOW", "4096")
    n, st = same_database(corpus, gpu_ctx)
    assert st["windows"] > 1 and st["host_lines"] == 0


def test_windows_smaller_than_lines(hostile_file, gpu_ctx, monkeypatch):
    path, lines = hostile_file
    monkeypatch.setenv("RK_CSV_WINDOW", "64")
    n, st = same_database(path, gpu_ctx)
    assert st["lines"] == len(lines)
    assert st["host_lines"] > len(lines) // 2


# ---- 6: float rounding on the device ----------------------------------------------

def test_float_rounding(gpu_ctx, tmp_path):
    rnd = random.Random(77)
    seen = set()
    while len(seen) < 200_000:
        sig = rnd.randrange(1, 8)
        frac = rnd.randrange(0, 11)
        d = str(rnd.randrange(10 ** (sig - 1), 10 ** sig))
        if frac == 0:
            s = d
        elif frac >= sig:
            s = "0." + "0" * (frac - sig) + d
        else:
            s = d[:sig - frac] + "." + d[sig - frac:]
        s = "0" * rnd.randrange(0, 3) + s
        s = rnd.choice(["", "", "-", "+"]) + s
        seen.add(s)
    spell = sorted(seen)
    rnd.shuffle(spell)
    head = "Frag,123456789,223456789,123456999,223456999,f,0,210,840,200,"
    body = "".join(head + s + ",95.23,0,1\n" for s in spell).encode()
    p = write_csv(tmp_path / "f.csv", body)
    n, st = same_database(p, gpu_ctx)
    # every spelling is on the fast path: the device decided all of them
    assert n == len(spell) and st["host_lines"] == 0


# ---- 7: resident columns ------------------------------------------------------------

def results_equal(a, b):
    return (a.n_groups == b.n_groups and np.array_equal(a.gid, b.gid) and
            np.array_equal(a.repval, b.repval) and np.array_equal(a.out_order, b.out_order))


@pytest.mark.parametrize("which", ["corpus", "e01_last_bucket", "e03_strands"])
def test_classify_db(which, corpus, gpu_ctx):
    path = corpus if which == "corpus" else os.path.join(EDGE, which + ".in.csv")
    db = rk.FragmentsDatabase(path, ctx=gpu_ctx, keep_device=True)
    view = db.device_view()
    assert view["n"] == db.frags.n and (view["n"] == 0 or view["x_start"])
    want = gpu_ctx.classify(db.frags, db.len_x_hdr, db.len_y_hdr, 0.3, 0.3)
    got = gpu_ctx.classify_db(db, 0.3, 0.3)
    assert results_equal(got, want)
    # another set classified on the same context leaves the resident columns alone
    other = rk.synth(20_000, 2_000_000, seed=5)
    gpu_ctx.classify(other, 2_000_000, 2_000_000, 0.3, 0.3)
    assert db.device_view() == view
    assert results_equal(gpu_ctx.classify_db(db, 0.3, 0.3), want)
    db.close()
    # free, then a fresh load
    db2 = rk.FragmentsDatabase(path, ctx=gpu_ctx, keep_device=True)
    assert results_equal(gpu_ctx.classify_db(db2, 0.3, 0.3), want)
    db2.close()


def test_device_view_needs_keep_device(corpus, gpu_ctx):
    db = rk.FragmentsDatabase(corpus, ctx=gpu_ctx)
    with pytest.raises(rk.RkError):
        db.device_view()
    db.close()


def test_cli_device_parse(corpus, tmp_path):
    out = tmp_path / "out.csv"
    p = subprocess.run([rk.CLI_PATH, "--device-parse", "--timing", corpus, str(out), "0.3", "0.3"],
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, p.stdout + p.stderr
    assert '"ingress"' in p.stderr
    with gzip.open(os.path.join(GOLDEN, "corpus10k.out.csv.gz"), "rb") as f:
        assert out.read_bytes() == f.read()


def test_cli_device_parse_usage(corpus, tmp_path):
    for extra in (["--soa"], ["--gpus", "2"]):
        p = subprocess.run([rk.CLI_PATH, "--device-parse"] + extra +
                           [corpus, str(tmp_path / "o.csv"), "0.3", "0.3"],
                           capture_output=True, text=True, timeout=60)
        assert p.returncode == 1 and "--device-parse" in p.stderr
