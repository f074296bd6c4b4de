"""The device CSV egress in the C ABI: symbols, signatures as the header states
them, argument checks that need no device (CPU only)."""
import ctypes
import os
import re

from conftest import EDGE, ROOT

import repkiller_amd as rk

HEADER = os.path.join(ROOT, "include", "repkiller_amd.h")


def header_text():
    with open(HEADER) as f:
        return re.sub(r"\s+", " ", f.read())


def test_symbols_exist():
    lib = rk.load_library()
    for sym in ("rk_db_write_csv_device", "rk_classify_db_pairs_to_csv", "rk_get_egress_stats"):
        assert ctypes.cast(getattr(lib, sym), ctypes.c_void_p).value, sym
        assert sym in rk.EXPORTS


def test_documented_signatures():
    text = header_text()
    for decl in (
        "enum { RK_DB_KEEP_DEVICE = 1 };",
        "enum { RK_DB_KEEP_ROWS = 3 };",
        "enum { RK_RES_DEVICE = 1 }; /* res->out_order / gid / repval are device pointers */",
        "int rk_db_write_csv_device(rk_ctx *ctx, const rk_db *db, const char *path, "
        "const rk_result *res, uint32_t flags);",
        "/* classify from the resident columns and write pair i to paths[i]; the result "
        "arrays never leave the device. n_out / n_groups: nullable HOST arrays, npairs entries */",
        "int rk_classify_db_pairs_to_csv(rk_ctx *ctx, const rk_db *db, const double *len_ratio, "
        "const double *pos_ratio, uint32_t npairs, const char *const *paths, uint64_t *n_out, "
        "uint64_t *n_groups);",
        "typedef struct { uint64_t rows, bytes, host_rows; uint32_t chunks; "
        "double upload_ms, device_ms, host_fix_ms, d2h_write_ms, total_ms; } rk_egress_stats;",
        "int rk_get_egress_stats(const rk_ctx *ctx, rk_egress_stats *st);",
    ):
        assert decl in text, decl
    # every entry of the section cites the reference's save_all_frag_pairs
    section = text[text.index("device egress"):text.index("synthetic inputs")]
    assert section.count("commonFunctions.cpp:101-146") >= 3
    # the ctypes mirror has the struct's layout: 3 u64, u32 (+pad), 5 doubles
    assert ctypes.sizeof(rk.EgressStats) == 3 * 8 + 8 + 5 * 8
    assert rk.RK_DB_KEEP_ROWS == 3 and rk.RK_RES_DEVICE == 1 and rk.RK_DB_KEEP_DEVICE == 1


def test_keep_rows_follows_keep_device_in_the_header():
    with open(HEADER) as f:
        lines = [l.strip() for l in f]
    a = next(i for i, l in enumerate(lines) if l.startswith("enum { RK_DB_KEEP_DEVICE = 1 };"))
    b = lines.index("enum { RK_DB_KEEP_ROWS = 3 };")
    assert b > a


def test_null_arguments():
    lib = rk.load_library()
    db = rk.FragmentsDatabase(os.path.join(EDGE, "e03_strands.in.csv"))
    res = rk.Result(0, 0, 0, 0, 0)
    path = b"/nonexistent-dir/never-opened.csv"
    # the argument check returns before it looks behind any pointer: a context
    # that is only an address stands in where no device is at hand
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.cast(fake_ctx, ctypes.c_void_p)
    assert lib.rk_db_write_csv_device(None, db._h, path, ctypes.byref(res), 0) == -1
    assert lib.rk_db_write_csv_device(ctx, None, path, ctypes.byref(res), 0) == -1
    assert lib.rk_db_write_csv_device(ctx, db._h, None, ctypes.byref(res), 0) == -1
    assert lib.rk_db_write_csv_device(ctx, db._h, path, None, 0) == -1
    assert lib.rk_db_write_csv_device(None, None, None, None, 0) == -1
    lr, pr = ctypes.c_double(0.3), ctypes.c_double(0.3)
    paths = (ctypes.c_char_p * 1)(path)
    assert lib.rk_classify_db_pairs_to_csv(None, db._h, ctypes.byref(lr), ctypes.byref(pr), 1,
                                           paths, None, None) == -1
    assert lib.rk_classify_db_pairs_to_csv(ctx, None, ctypes.byref(lr), ctypes.byref(pr), 1,
                                           paths, None, None) == -1
    assert lib.rk_classify_db_pairs_to_csv(ctx, db._h, None, ctypes.byref(pr), 1, paths, None,
                                           None) == -1
    assert lib.rk_classify_db_pairs_to_csv(ctx, db._h, ctypes.byref(lr), ctypes.byref(pr), 1,
                                           None, None, None) == -1
    assert lib.rk_classify_db_pairs_to_csv(ctx, db._h, ctypes.byref(lr), ctypes.byref(pr), 0,
                                           paths, None, None) == -1
    st = rk.EgressStats()
    assert lib.rk_get_egress_stats(None, ctypes.byref(st)) == -1
    assert lib.rk_get_egress_stats(ctx, None) == -1
    assert not os.path.exists(path.decode())
    db.close()


def test_load_flags_without_a_context():
    lib = rk.load_library()
    h = ctypes.c_void_p()
    path = os.path.join(EDGE, "e03_strands.in.csv").encode()
    assert lib.rk_db_load_csv_device(None, path, 3, ctypes.byref(h)) == -1
    assert not h.value
    # an unknown bit, and bit 1 alone, are refused before anything is read
    fake_ctx = ctypes.create_string_buffer(4096)
    ctx = ctypes.cast(fake_ctx, ctypes.c_void_p)
    for flags in (2, 4, 7, 0x80000003):
        assert lib.rk_db_load_csv_device(ctx, path, flags, ctypes.byref(h)) == -1, flags
        assert not h.value
