"""The host f64 forms of the packed families that take a batch -- stft / istft, dct / idct, hilbert, firFilter, dft,
czt, wavedecHost / waverecHost, upfirdnHost / resamplePoly: a row of a batch equals the same call on that row alone,
bit for bit.  The device forms assert this in their own files; the host forms add their own staging (2-D copies with a
pitch where a row is shorter than the transform) and nothing else checks that per row.  One case each: 2 x (rows per
workgroup) + 1 rows at the smallest size of the family where a workgroup holds more than one row (the wavelet and
rate-change kernels run one row per workgroup: five rows), rows first, middle and last."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def packed_rows_per_wg(n):
    """FftTraits<log2(n/2)>::ROWS of the packed-real kernels on N-point rows (one thread per 32 samples)."""
    tp = n // 32
    return max(tp, 256) // tp


def chirp_rows_per_wg(m):
    """The same for the chirp-z kernels on an M-point convolution (one thread per 16 points)."""
    tp = m // 16
    return max(tp, 256) // tp


def same_rows(fn, x, batch):
    """fn on the batch against fn on rows first, middle and last alone."""
    got = fn(x)
    assert got.shape[0] == batch and np.isfinite(got.view(np.float64)).all()
    for r in (0, batch // 2, batch - 1):
        one = fn(x[r:r + 1])
        assert one.shape == got[r:r + 1].shape
        assert np.array_equal(got[r].view(np.float64), one[0].view(np.float64)), f"row {r} of {batch} differs from the call on it alone"
    return got


def test_dct_and_idct_rows():
    m = importlib.import_module("pragma_dsp_amd.dct")
    n = 64
    batch = 2 * packed_rows_per_wg(n) + 1
    assert packed_rows_per_wg(n) > 1
    x = np.random.default_rng(1).standard_normal((batch, n))
    y = same_rows(lambda a: m.dct(a, 2, "ortho"), x, batch)
    back = same_rows(lambda a: m.idct(a, 2, "ortho"), y, batch)
    assert np.abs(back - x).max() <= 1e-12


@pytest.mark.parametrize("mode", ["hilbert", "envelope"])
def test_hilbert_rows_shorter_than_the_transform(mode):
    m = importlib.import_module("pragma_dsp_amd.hilbert")
    n, ln = 64, 50  # rows of 50 samples staged with a pitch into 64-point transforms
    batch = 2 * packed_rows_per_wg(n) + 1
    x = np.random.default_rng(2).standard_normal((batch, ln))
    same_rows(lambda a: getattr(m, mode)(a, n), x, batch)


@pytest.mark.parametrize("mode", ["full", "same"])
def test_fir_filter_rows(mode):
    m = importlib.import_module("pragma_dsp_amd.filters")
    taps = np.random.default_rng(3).standard_normal(9)
    n = m.block_size(taps.size)
    assert packed_rows_per_wg(n) > 1, n
    batch = 2 * packed_rows_per_wg(n) + 1
    x = np.random.default_rng(4).standard_normal((batch, 50))  # shorter than a block, and 150: three blocks a row
    same_rows(lambda a: m.firFilter(a, taps, mode), x, batch)
    x3 = np.random.default_rng(5).standard_normal((batch, 150))
    same_rows(lambda a: m.firFilter(a, taps, mode), x3, batch)


def test_stft_frames_and_istft_frames():
    m = importlib.import_module("pragma_dsp_amd.stft")
    n, hop = 64, 24
    frames = 2 * packed_rows_per_wg(n) + 1
    x = np.random.default_rng(6).standard_normal((frames - 1) * hop + n)
    spec = m.stft(x, n, hop, "hann")
    assert spec.shape == (frames, n // 2 + 1)
    for f in (0, frames // 2, frames - 1):  # frame f is the one-frame transform of its own samples
        one = m.stft(x[f * hop:f * hop + n], n, hop, "hann")
        assert np.array_equal(spec[f].view(np.float64), one[0].view(np.float64)), f"frame {f} of {frames}"
    # hop = N: no frame overlaps another, so a frame's stretch of the output is the inverse of that frame alone
    out = m.istft(spec, n, "hamming")
    assert out.shape == (frames * n,) and np.isfinite(out).all()
    for f in (0, frames // 2, frames - 1):
        one = m.istft(spec[f:f + 1], n, "hamming")
        assert np.array_equal(out[f * n:(f + 1) * n], one), f"frame {f} of {frames}"


@pytest.mark.parametrize("ln,conv", [(2, 32), (17, 64)])
def test_dft_rows(ln, conv):
    m = importlib.import_module("pragma_dsp_amd.dft")
    assert chirp_rows_per_wg(conv) > 1
    batch = 2 * chirp_rows_per_wg(conv) + 1
    rng = np.random.default_rng(7 + ln)
    z = rng.standard_normal((batch, ln)) + 1j * rng.standard_normal((batch, ln))
    y = same_rows(m.dft, z, batch)
    assert np.abs(y - np.fft.fft(z, axis=1)).max() <= 1e-12 * ln
    same_rows(m.idft, y, batch)
    same_rows(m.dft, z.real.copy(), batch)  # real rows: no imaginary plane is staged


def test_czt_rows():
    m = importlib.import_module("pragma_dsp_amd.czt")
    ln, bins, conv = 20, 12, 32  # 20 + 12 - 1 = 31 points of convolution on a 32-point transform
    batch = 2 * chirp_rows_per_wg(conv) + 1
    rng = np.random.default_rng(8)
    z = rng.standard_normal((batch, ln)) + 1j * rng.standard_normal((batch, ln))
    same_rows(lambda a: m.czt(a, bins, np.exp(-2j * np.pi * 0.013), np.exp(2j * np.pi * 0.1)), z, batch)
    same_rows(lambda a: m.zoom_fft(a, [0.2, 0.4], bins), z.real.copy(), batch)


def test_wavelet_rows():
    m = importlib.import_module("pragma_dsp_amd.wavelet")
    batch, n, levels = 5, 96, 3
    x = np.random.default_rng(9).standard_normal((batch, n))
    c = same_rows(lambda a: m.wavedecHost(a, "db4", levels), x, batch)
    back = same_rows(lambda a: m.waverecHost(a, "db4", levels), c, batch)
    assert np.abs(back - x).max() <= 1e-12


def test_rate_change_rows():
    m = importlib.import_module("pragma_dsp_amd.resample")
    batch = 5
    x = np.random.default_rng(10).standard_normal((batch, 101))
    h = np.random.default_rng(11).standard_normal(13)
    same_rows(lambda a: m.upfirdnHost(h, a, 3, 2), x, batch)
    same_rows(lambda a: m.resamplePoly(a, 3, 2), x, batch)
