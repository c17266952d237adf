"""bench.py on the card, plain and with --full: a plain run prints the headline line without the legs beside it, and
--full still runs them (parity of the timed output against the oracle, the CPU baseline, the device-copy yardstick).
Small batches: checks of what the line carries, not measurements."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
QUICK = ["--steps", "3", "--warmup", "1", "--batch", "4096", "--ramp-seconds", "0"]


def _line(argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH] + QUICK + argv, capture_output=True, text=True, timeout=600, env=env,
                       cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])
    return json.loads(lines[0])


def test_plain_line_is_the_headline_only():
    d = _line([])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["value"] > 0
    assert d["unit"] == "GSample/s" and d["higher_is_better"] is True and d["dtype"] == "f32"
    assert not {"parity", "cpu_baseline", "also", "gather"} & set(d)
    assert d["roofline"]["device_copy_same_buffers_GBps"] is None and "traffic_detail" not in d["roofline"]


def test_full_line_still_checks_and_compares():
    d = _line(["--full", "--no-also", "--cpu-seconds", "0.5"])
    assert d["parity"]["ok"] is True and d["parity"]["rows"] == 256 and d["parity"]["max_rel_err"] <= 1e-5
    assert d["cpu_baseline"]["value"] > 0
    assert d["roofline"]["device_copy_same_buffers_GBps"] > 0
    assert "also" not in d
