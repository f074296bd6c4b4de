"""The byte-stream arithmetic of a batched load (rk_csv_stream.h): pieces with
and without an appended newline read as one stream, against a plain
concatenation, in a stand-alone host program built with the address and
undefined-behaviour sanitizers (tests/cpp/csv_stream_check.cpp; CPU only)."""
import os
import subprocess

from conftest import ROOT

CSRC = os.path.join(ROOT, "repkiller_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "cpp", "csv_stream_check.cpp")


def test_stream_arithmetic_sanitized(tmp_path):
    exe = tmp_path / "csv_stream_check_san"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, SRC, "-o", str(exe)], check=True)
    p = subprocess.run([str(exe), "1500"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "mismatches 0" in p.stdout
