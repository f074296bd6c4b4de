"""The shared CSV row function (csrc/rk_csv_row.h), compiled for the host,
against the host formatter (rk::db_format_row) and snprintf: every row of the
golden outputs and 300k rows of a seeded grammar of edge values, then the float
function alone over 5 M values.  The status is checked as an exact two-way
predicate (tests/cpp/csv_row_check.cpp), so no row is left out; a second,
stand-alone build of the same check runs under AddressSanitizer and UBSan from
the first run's dumps (CPU only)."""
import glob
import gzip
import os
import shutil
import subprocess

import pytest

from conftest import EDGE, GOLDEN, ROOT

import repkiller_amd as rk

CSRC = os.path.join(ROOT, "repkiller_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "csv_row_check.cpp")


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    d = tmp_path_factory.mktemp("csv_row")
    corpus = d / "corpus10k.out.csv"
    with gzip.open(os.path.join(GOLDEN, "corpus10k.out.csv.gz"), "rb") as f, open(corpus, "wb") as o:
        shutil.copyfileobj(f, o)
    libdir = os.path.dirname(rk.LIB_PATH)
    exe = d / "csv_row_check"
    subprocess.run(["g++", "-O2", "-std=c++17", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    SRC, "-L", libdir, "-lrepkiller_amd", f"-Wl,-rpath,{libdir}", "-lpthread",
                    "-o", str(exe)], check=True)
    inputs = sorted(glob.glob(os.path.join(EDGE, "*.out.csv"))) + [str(corpus)]
    p = subprocess.run([str(exe), "full", str(d)] + inputs, capture_output=True, text=True,
                       timeout=300)
    return d, p


def test_row_function_matches_host_formatter(workdir):
    d, p = workdir
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches 0" in p.stdout
    # both statuses are reached, by rows and by floats alone
    words = p.stdout.split()
    for key in ("device", "host", "floats_exact", "floats_refused"):
        assert int(words[words.index(key) + 1]) > 1000, p.stdout
    assert int(words[words.index("rows") + 1]) > 310_000


def test_row_function_sanitized(workdir):
    d, first = workdir
    assert first.returncode == 0, first.stdout + first.stderr
    exe = d / "csv_row_check_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-DRK_NO_LIB", "-I", CSRC, SRC, "-o", str(exe)],
                   check=True)
    p = subprocess.run([str(exe), "check", str(d)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches 0" in p.stdout
    assert p.stdout.splitlines()[-1] == first.stdout.splitlines()[-1]
