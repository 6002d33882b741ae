"""The planner's super-bin rule under AddressSanitizer + UBSan (CPU build): tests/cpp/test_plan_super.cpp drives
choose_super_bases and plan_segment's super-bin table of umihip_plan.hpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_super_bin_rule_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "test_plan_super")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_plan_super.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "super plan ok" in r.stdout
