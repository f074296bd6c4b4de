"""The device CSV ingress in the C ABI: symbols, signatures as the header states
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
    for sym in ("rk_db_load_csv_device", "rk_db_device_view", "rk_get_ingress_stats",
                "rk_csv_max_line"):
        assert ctypes.cast(getattr(lib, sym), ctypes.c_void_p).value, sym


def test_documented_signatures():
    text = header_text()
    for decl in (
        "enum { RK_DB_KEEP_DEVICE = 1 };",
        "int rk_db_load_csv_device(rk_ctx *ctx, const char *path, uint32_t flags, rk_db **db);",
        "int rk_db_device_view(const rk_db *db, rk_frags_soa *soa_dev);",
        "typedef struct { uint64_t body_bytes, lines, accepted, host_lines; uint32_t windows; "
        "double h2d_ms, device_ms, host_fix_ms, d2h_ms, total_ms; } rk_ingress_stats;",
        "int rk_get_ingress_stats(const rk_ctx *ctx, rk_ingress_stats *st);",
        "uint32_t rk_csv_max_line(void);",
    ):
        assert decl in text, decl
    # the ctypes mirror has the struct's layout: 4 u64, u32 (+pad), 5 doubles
    assert ctypes.sizeof(rk.IngressStats) == 4 * 8 + 8 + 5 * 8
    assert rk.RK_DB_KEEP_DEVICE == 1


def test_null_arguments():
    lib = rk.load_library()
    h = ctypes.c_void_p()
    path = os.path.join(EDGE, "e03_strands.in.csv").encode()
    assert lib.rk_db_load_csv_device(None, path, 0, ctypes.byref(h)) == -1
    assert lib.rk_db_load_csv_device(None, None, 0, ctypes.byref(h)) == -1
    assert lib.rk_db_load_csv_device(None, path, 0, None) == -1
    soa = rk.FragsSoA()
    assert lib.rk_db_device_view(None, ctypes.byref(soa)) == -1
    st = rk.IngressStats()
    assert lib.rk_get_ingress_stats(None, ctypes.byref(st)) == -1


def test_device_view_of_a_host_database():
    lib = rk.load_library()
    db = rk.FragmentsDatabase(os.path.join(EDGE, "e03_strands.in.csv"))
    soa = rk.FragsSoA()
    assert lib.rk_db_device_view(db._h, ctypes.byref(soa)) == -1
    assert lib.rk_db_device_view(db._h, None) == -1
    db.close()


def test_max_line_and_tile():
    lib = rk.load_library()
    assert lib.rk_csv_max_line() >= 256
    assert lib.rk_csv_tile() >= 16 and lib.rk_csv_tile() % 16 == 0
