"""The layout of a host-buffer call's staging block under AddressSanitizer + UBSan (CPU build):
tests/cpp/test_io_layout.cpp checks umihip_io_layout.hpp alone -- alignment, no overlap, absent and empty
arrays, the total, and the totals of umi_count_matrix and umi_dedup_stats against the sums written out by hand."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_io_layout_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "test_io_layout")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_io_layout.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "io layout ok" in r.stdout
