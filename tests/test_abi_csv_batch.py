"""Batched sets as files in the C ABI (rk_dbset_*): symbols, signatures as the
header states them, argument checks that need no device, and the CLI's usage
rule for --device-save (CPU only)."""
import ctypes
import os
import re
import subprocess

from conftest import EDGE, ROOT

import repkiller_amd as rk

HEADER = os.path.join(ROOT, "include", "repkiller_amd.h")
SYMBOLS = ("rk_dbset_load_csv_device", "rk_dbset_free", "rk_dbset_view", "rk_classify_dbset",
           "rk_dbset_write_csv_device", "rk_classify_dbset_to_csv", "rk_dbset_write_csv")


def header_text():
    with open(HEADER) as f:
        return re.sub(r"\s+", " ", f.read())


def test_symbols_exist():
    lib = rk.load_library()
    for sym in SYMBOLS:
        assert sym in rk.EXPORTS, sym
        assert ctypes.cast(getattr(lib, sym), ctypes.c_void_p).value, sym


def test_documented_signatures():
    text = header_text()
    for decl in (
        "typedef struct rk_dbset rk_dbset;",
        "int rk_dbset_load_csv_device(rk_ctx *ctx, const char *const *paths, uint32_t nsets, "
        "uint32_t flags, rk_dbset **out);",
        "void rk_dbset_free(rk_dbset *dbs);",
        "int rk_dbset_view(const rk_dbset *dbs, uint32_t *nsets, const uint64_t **set_off, "
        "const uint64_t **len_x_hdr, const uint64_t **len_y_hdr, const uint64_t **total_hdr, "
        "rk_frags_soa *host, rk_frags_soa *dev);",
        "int rk_classify_dbset(rk_ctx *ctx, const rk_dbset *dbs, double len_ratio, "
        "double pos_ratio, rk_batch_result *out);",
        "int rk_dbset_write_csv(const rk_dbset *dbs, uint32_t k, const char *path, "
        "const rk_result *res);",
        "int rk_dbset_write_csv_device(rk_ctx *ctx, const rk_dbset *dbs, const char *const *paths, "
        "const rk_batch_result *res, uint32_t flags);",
        "int rk_classify_dbset_to_csv(rk_ctx *ctx, const rk_dbset *dbs, double len_ratio, "
        "double pos_ratio, const char *const *paths, uint64_t *n_out, uint64_t *n_groups);",
    ):
        assert decl in text, decl
    # the comments cite the reference lines the entry points replace
    section = text[text.index("batched sets as files"):]
    for cite in ("FragmentsDatabase.cpp:17-101", "commonFunctions.cpp:101-146",
                 "repkiller.cpp:80-97"):
        assert cite in section, cite


def test_null_arguments():
    lib = rk.load_library()
    h = ctypes.c_void_p()
    paths = (ctypes.c_char_p * 1)(os.path.join(EDGE, "e03_strands.in.csv").encode())
    res = rk.BatchResult()
    assert lib.rk_dbset_load_csv_device(None, paths, 1, 0, ctypes.byref(h)) == -1
    assert lib.rk_dbset_view(None, None, None, None, None, None, None, None) == -1
    assert lib.rk_classify_dbset(None, None, 0.3, 0.3, ctypes.byref(res)) == -1
    assert lib.rk_dbset_write_csv_device(None, None, paths, ctypes.byref(res), 0) == -1
    assert lib.rk_classify_dbset_to_csv(None, None, 0.3, 0.3, paths, None, None) == -1
    one = rk.Result()
    assert lib.rk_dbset_write_csv(None, 0, b"/nonexistent/x.csv", ctypes.byref(one)) == -1
    lib.rk_dbset_free(None)  # a no-op, like free


def test_bad_arguments_are_refused_before_anything_is_touched():
    """With a context and a set that are not null, a bad flag, a null path list
    or a null output pointer is refused by the first check: the stand-ins below
    are zeroed memory that no entry point may read before it has checked."""
    lib = rk.load_library()
    ctx = ctypes.create_string_buffer(1 << 16)
    dbs = ctypes.create_string_buffer(1 << 12)
    h = ctypes.c_void_p()
    paths = (ctypes.c_char_p * 2)(b"/nonexistent/a.csv", None)
    res = rk.BatchResult()
    load = lib.rk_dbset_load_csv_device
    for flags in (2, 4, 5, 8, 1 << 31):  # bit 1 alone keeps nothing to classify
        assert load(ctx, paths, 1, flags, ctypes.byref(h)) == -1, flags
    assert load(ctx, paths, 1, 0, None) == -1
    assert load(ctx, None, 1, 0, ctypes.byref(h)) == -1
    assert load(ctx, paths, 2, 0, ctypes.byref(h)) == -1  # a null path in the list
    for flags in (2, 3, 1 << 16):
        assert lib.rk_dbset_write_csv_device(ctx, dbs, paths, ctypes.byref(res), flags) == -1
    assert lib.rk_dbset_write_csv_device(ctx, dbs, paths, None, 0) == -1
    assert lib.rk_classify_dbset(ctx, dbs, 0.3, 0.3, None) == -1


def test_cli_device_save_needs_device_parse(tmp_path):
    out = tmp_path / "out.csv"
    lst = tmp_path / "list.tsv"
    lst.write_text(f"{os.path.join(EDGE, 'e03_strands.in.csv')}\t{out}\n")
    p = subprocess.run([rk.CLI_PATH, "--batch", str(lst), "--device-save", "0.3", "0.3"],
                       capture_output=True, text=True)
    assert p.returncode == 1
    assert "--device-save" in p.stderr
    assert not out.exists()
    assert os.listdir(tmp_path) == ["list.tsv"]


def test_cli_help_names_the_batched_device_route():
    p = subprocess.run([rk.CLI_PATH], capture_output=True, text=True)
    assert p.returncode == 1
    assert re.search(r"--batch .*--device-parse \[--device-save\]", p.stdout), p.stdout
