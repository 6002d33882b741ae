"""The host decisions of read staging under AddressSanitizer + UBSan (CPU build): tests/cpp/test_stage_plan.cpp
checks stage_sort_plan and stage_order_plan of umihip_stage_plan.hpp against the table that the plain-Python
statement of the rules (tests/stage_edge_inputs.py) prints."""
import os
import subprocess

import stage_edge_inputs as si

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_stage_plan_against_the_python_rule_under_asan_and_ubsan(tmp_path):
    table = str(tmp_path / "stage_plan_table.txt")
    with open(table, "w") as f:
        f.write("\n".join(si.plan_table()) + "\n")
    exe = str(tmp_path / "test_stage_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_stage_plan.cpp")])
    r = subprocess.run([exe, table], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "stage plan ok" in r.stdout
