"""The library's own sort and scan (umihip_radix.hip), called directly by tests/cpp/test_primitives.hip
(`make primtest`) and compared with the plain references of tests/cpp/primitives_ref.hpp at the sizes
where tiles, rounds, look-back windows and spine rounds begin and end.  One process per group; the
first group that fails ends the test, and nothing more is started on the GPU after it."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROUPS = ["refusals", "scan", "spine", "sort32", "sort64", "hist", "reuse"]


@pytest.mark.gpu
def test_sort_and_scan_primitives_match_the_reference():
    exe = os.path.join(ROOT, "build", "test_primitives")
    if not os.path.exists(exe):
        subprocess.check_call(["make", "-s", "-C", ROOT, "primtest"])
    for group in GROUPS:
        # (120 s: a guard against a hang; a group takes a few seconds)
        out = subprocess.run([exe, group], capture_output=True, text=True, timeout=120)
        tail = (out.stdout + out.stderr)[-3000:]
        assert out.returncode == 0, "group %s exited %d:\n%s" % (group, out.returncode, tail)
        assert "%s ok: " % group in out.stdout, "group %s printed no ok line:\n%s" % (group, tail)
