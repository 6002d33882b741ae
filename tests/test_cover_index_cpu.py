"""The cover lookup of umi_assign_genes_classes under AddressSanitizer + UBSan (CPU build): tests/cpp/test_cover_index.cpp
runs the prefix array of covered bases, gene_cover, the genes' own exons and gene_read_class of
csrc/umihip_gene_index.hpp -- the code the kernel runs -- against a per-base brute force."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cover_index_against_brute_force_under_asan_and_ubsan(tmp_path):
    exe = str(tmp_path / "test_cover_index")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_cover_index.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "cover index ok" in r.stdout
