"""The reference that the sort and scan primitives are tested against, checked on the CPU.
tests/cpp/test_primitives_ref.cpp runs under AddressSanitizer + UBSan (CPU build only: the GPU pool
has no sanitizer runs): the reference sort of tests/cpp/primitives_ref.hpp equals an independent
counting sort, every input generator produces what its name says, and every checker rejects a
host-made wrong answer at the right index.  The `refusals` group of tests/cpp/test_primitives.hip
makes no HIP call, so it runs here too; the other groups run in tests/test_gpu_primitives.py."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reference_and_checkers_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "test_primitives_ref")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_primitives_ref.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "primitives reference ok" in r.stdout


def test_host_side_refusals_without_a_gpu():
    subprocess.check_call(["make", "-s", "-C", ROOT, "primtest"])
    r = subprocess.run([os.path.join(ROOT, "build", "test_primitives"), "refusals"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    assert "refusals ok:" in r.stdout
