"""The planner's cross rule under AddressSanitizer + UBSan (CPU build): tests/cpp/test_plan_cross.cpp drives
choose_cross and plan_segment's cross bits and map offsets of umihip_plan.hpp."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cross_rule_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "test_plan_cross")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-D__HIP_PLATFORM_AMD__",
                           "-I/opt/rocm/include", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_plan_cross.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cross plan ok" in r.stdout
