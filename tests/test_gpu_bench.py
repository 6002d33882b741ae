"""bench.py's two kinds of run on config 2 (shrunk): a plain run times the top-level workload's steps and
leaves every other field null; --full adds the phase split, the roofline, the sustained block, the
brute-force step, device staging and the host-buffer call.  Both time the same steps on the same
seeded input, so their dumped kept masks are equal."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--reads", "200000", "--dump-outputs", str(out_dir)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def test_bench_plain_run_and_full_run(tmp_path):
    plain = _bench(tmp_path / "plain")
    assert plain["full"] is False and plain["value"] > 0 and plain["ms_per_step"] > 0
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["higher_is_better"] is True
    assert plain["unit"] == "UMI-pair comparisons/s" and plain["dtype"] == "u32"
    for f in ("ms_per_step_with_events", "roofline", "phases_ms", "sustained", "value_bruteforce",
              "staging_device", "host_buffer_path"):
        assert plain[f] is None, f
    assert plain["configs"] == {} and "cpu_baseline" not in plain and "end_to_end" not in plain

    full = _bench(tmp_path / "full", "--full", "--also", "none", "--no-cpu-baseline")
    assert full["full"] is True and full["value"] > 0
    assert full["ms_per_step_with_events"] > 0 and full["roofline"]["bound"] in ("valu", "hbm")
    assert set(full["phases_ms"]) == {"prep", "pairs", "collapse", "finalize"}
    for f in ("sustained", "value_bruteforce", "staging_device", "host_buffer_path"):
        assert full[f] is not None, f
    assert full["configs"] == {} and "cpu_baseline" not in full

    assert plain["kept_rank0"] == full["kept_rank0"]
    a, b = np.load(tmp_path / "plain" / "kept.npy"), np.load(tmp_path / "full" / "kept.npy")
    assert a.shape == (plain["config"]["unique_umis_rank0"],) and (a == b).all()
