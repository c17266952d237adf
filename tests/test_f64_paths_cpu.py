"""The CPU half of tests/test_gpu_f64_paths.py: its long-double reference against the C oracle and scipy.fft, the
extended-precision check it relies on, and the reach of its path tables (expected_path_f64 over every case)."""
import numpy as np
import pytest

from test_gpu_f64_paths import (REQUIRED_F64, SPEC_CASES, TOP_MODES, TOP_N, TOP_SPEC_N, TRANSFORM_CASES,
                                _frame_geometry, check_long_double, expected_path_f64, ld_fft, lg, reference_transform,
                                split)


def test_long_double_is_extended():
    check_long_double()
    assert ld_fft(np.zeros((2, 8), dtype=np.longdouble), real=True).dtype == np.clongdouble


def test_split_is_exact_to_the_long_double():
    x = np.fft.fft(np.arange(64, dtype=np.longdouble) / 3)
    hi, lo = split(x)
    assert hi.dtype == np.complex128 and lo.dtype == np.complex128
    assert (hi.astype(np.clongdouble) + lo == x).all()


@pytest.mark.parametrize("n", [1, 2, 8, 1024, 1 << 13, 1 << 16])
def test_long_double_reference_matches_the_oracle_and_scipy(oracle_mod, n):
    """Forward (complex and real input) and inverse: the long-double reference and two f64 FFTs agree within the f64
    FFTs' own error: 3 * 2^-53 * log2 N of each row's rms per bin at most (measured: the oracle 1.9, scipy.fft 0.8)."""
    import scipy.fft
    rng = np.random.default_rng(n)
    re, im = rng.standard_normal((3, n)), rng.standard_normal((3, n))
    re[2] = 0.0
    re[2, n // 3] = 1.0
    p = oracle_mod.Plan(n)
    for kind in ("complex", "real", "inverse"):
        ref = reference_transform(kind, re, None if kind == "real" else im)
        if kind == "complex":
            o = p.forward_complex(re, im)
            s = scipy.fft.fft(re + 1j * im, axis=-1)
        elif kind == "real":
            o = p.forward(re)
            s = scipy.fft.fft(re, axis=-1)
        else:
            o = p.inverse(re, im)
            s = scipy.fft.ifft(re + 1j * im, axis=-1)
        hi, lo = split(ref)
        rms = np.sqrt((np.abs(hi) ** 2).mean(axis=-1, keepdims=True))
        for name, got in (("oracle", o[0] + 1j * o[1]), ("scipy", s)):
            err = float((np.abs((got - hi) - lo) / rms).max())
            assert err <= 3 * 2.0 ** -53 * lg(n), (n, kind, name, err / lg(n))


def test_path_tables_reach_every_path():
    """The expected paths of every case in the f64 tables, without running them: each case reaches the names it is
    there for, and together they reach each name in REQUIRED_F64."""
    seen = set()
    for name, logs, batch, kinds, offs, out_mode, sw, intended in TRANSFORM_CASES:
        for L in logs:
            for kind in kinds:
                if kind == "real":
                    o = (offs[0], None, offs[0] if out_mode == "inplace" else offs[2], offs[3])
                else:
                    o = offs if out_mode != "inplace" else (offs[0], offs[1], offs[0], offs[1])
                if out_mode == "overlap":
                    o = (o[0], o[1], offs[0] + (batch << L) // 2 + offs[2], offs[3])
                path = expected_path_f64(kind, 1 << L, batch, o, aliasing=out_mode != "disjoint", switches=sw)
                assert intended <= path, (name, L, kind, sorted(path))
                seen |= path
    for n in TOP_N:
        for kind in ("complex", "real", "inverse"):
            for _, offs, out_mode in TOP_MODES:
                o = offs if kind != "real" else (offs[0], None, offs[2], offs[3])
                seen |= expected_path_f64(kind, n, 1, o, aliasing=out_mode != "disjoint")
    for name, logs, batch, frame, smode, f_off, windows, w_off, sidess, outsets, sw, want in SPEC_CASES:
        for L in logs:
            n = 1 << L
            length, stride, _ = _frame_geometry(n, frame, smode)
            for window in windows:
                if n == 1 and window is not None:
                    continue
                wo = (0 if window[0] == "plan" else w_off) if window else None
                for sides in sidess:
                    for outs in outsets:
                        path = expected_path_f64("spectrum", n, batch, (f_off, wo), frame_len=length, stride=stride,
                                                 window=window, sides=sides, outputs=set(outs), switches=sw)
                        assert any(p.startswith(w) for p in path for w in want), (name, L, window, sorted(path))
                        seen |= path
    for n in TOP_SPEC_N:
        for frame_len, f_off, outs in ((n, 0, ("amp", "idx")), (n + 5, 1, ("amp", "ph"))):
            seen |= expected_path_f64("spectrum", n, 1, (f_off, 0), frame_len=frame_len, stride=frame_len,
                                      window=("plan", "hann"), outputs=set(outs))
    assert "bigfft-n1-split2" in expected_path_f64("complex", 1 << 26, 1, (0, 0, 0, 0))
    missing = REQUIRED_F64 - seen
    assert not missing, sorted(missing)
