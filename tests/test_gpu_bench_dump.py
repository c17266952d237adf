"""bench.py --dump-outputs on the card: the files hold what the timed path computed in its last step -- checked row for
row against the oracle on the same seeded inputs, regenerated here -- within the byte budget, and the line carries
the timed steps and ms_per_step.  Small batches: checks of the dump, not measurements."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
QUICK = ["--steps", "3", "--warmup", "1", "--ramp-seconds", "0", "--no-measure-traffic", "--no-also", "--no-cpu-baseline"]


def _run_dump(out_dir, argv):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    p = subprocess.run([sys.executable, BENCH, "--dump-outputs", str(out_dir)] + QUICK + argv, capture_output=True,
                       text=True, timeout=600, env=env, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, (p.stdout[-2000:], p.stderr[-2000:])
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    files = sorted(os.listdir(out_dir))
    assert files == sorted(name + ".npy" for name in d["dump_outputs"]["files"])
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 * 10 ** 6
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    for name, a in arrays.items():
        assert list(a.shape) == d["dump_outputs"]["files"][name]
    return d, arrays


def test_dump_fft4096_is_the_timed_transform_of_the_seeded_rows(tmp_path, oracle_mod):
    import bench
    batch, n = 4096, 4096
    d, got = _run_dump(tmp_path / "d", ["--batch", str(batch)])
    rows = bench.dump_rows(batch, 2 * n * 4).numpy()
    assert len(rows) < batch  # a sample: exercises the seeded selection
    assert set(got) == {"out_re", "out_im"} and all(a.dtype == np.float32 for a in got.values())
    assert got["out_re"].shape == (len(rows), n)
    re, im = bench.synth_batch(batch, n, "cuda:0", seed=1337)
    wre, wim = oracle_mod.Plan(n).forward_complex(re.cpu().numpy()[rows], im.cpu().numpy()[rows])
    want = wre + 1j * wim
    assert rel_err(got["out_re"].astype(np.float64) + 1j * got["out_im"].astype(np.float64), want) <= 1e-5


def test_dump_spectrum16k_amplitude_rows(tmp_path, oracle_mod):
    import bench
    frames, n = 2048, 16384
    d, got = _run_dump(tmp_path / "d", ["--workload", "spectrum16k", "--batch", str(frames), "--chunk", str(frames)])
    rows = bench.dump_rows(frames, (n // 2 + 1) * 4).numpy()
    assert set(got) == {"amplitude"} and got["amplitude"].dtype == np.float32
    assert got["amplitude"].shape == (len(rows), n // 2 + 1)
    x, _ = bench.synth_batch(frames, n, "cuda:0", seed=1337, complex_noise=False)
    want, _, _ = oracle_mod.Plan(n).spectrum_batch(x.cpu().numpy()[rows], window=oracle_mod.create_window("hann", n))
    assert rel_err(got["amplitude"], want) <= 1e-5


def test_dump_peaks16k_records(tmp_path, oracle_mod):
    import bench
    frames, n = 2048, 16384
    d, got = _run_dump(tmp_path / "d", ["--workload", "peaks16k", "--batch", str(frames), "--chunk", str(frames)])
    assert set(got) == {"peak_index", "peak_frequency", "peak_amplitude", "peak_phase"}
    assert got["peak_index"].dtype == np.float64 and got["peak_amplitude"].dtype == np.float32
    assert got["peak_index"].shape == (frames,)  # 20 bytes per frame: every row fits
    idx = got["peak_index"].astype(np.int64)
    assert np.array_equal(idx, got["peak_index"]) and idx.min() >= 0 and idx.max() <= n // 2
    x, _ = bench.synth_batch(frames, n, "cuda:0", seed=1337, complex_noise=False)
    want, _, wpk = oracle_mod.Plan(n).spectrum_batch(x.cpu().numpy(), window=oracle_mod.create_window("hann", n),
                                                     want_peak=True)
    rows = np.arange(frames)
    top, at = want.max(axis=1), want[rows, idx]
    assert (np.abs(at - want[rows, wpk]) <= 2e-5 * top).all()  # the oracle's peak, up to near-ties in f32
    assert (np.abs(got["peak_amplitude"] - at) <= 1e-5 * top).all()
    assert np.allclose(got["peak_frequency"], idx * 48000.0 / n, rtol=1e-6)
