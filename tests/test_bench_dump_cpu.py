"""bench.py --dump-outputs without a GPU: the row sample is fixed and within the byte budget, and the flag is refused
where there is no batched output to write."""
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_dump_rows_is_a_fixed_sample_within_the_budget():
    import bench
    row_bytes = 2 * 4096 * 4  # fft4096: the re and im rows of one f32 transform
    a = bench.dump_rows(65536, row_bytes)
    b = bench.dump_rows(65536, row_bytes)
    assert a.tolist() == b.tolist()
    assert len(a) == bench.DUMP_BYTES // row_bytes and len(a) * row_bytes <= 64 * 10 ** 6
    assert len(set(a.tolist())) == len(a) and a.tolist() == sorted(a.tolist())
    assert 0 <= a.min() and a.max() < 65536 and a.max() >= 65536 // 2  # drawn from the whole batch
    assert bench.dump_rows(100, row_bytes).tolist() == list(range(100))  # small outputs: every row


@pytest.mark.parametrize("extra", [["--dry-run"], ["--workload", "stream"], ["--workload", "single1024"]])
def test_dump_outputs_refused_without_batched_outputs(tmp_path, extra):
    p = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(tmp_path / "d")] + extra, capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 2 and "--dump-outputs needs" in p.stderr, p.stderr[-2000:]
    assert not (tmp_path / "d").exists()
