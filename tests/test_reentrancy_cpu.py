"""pdsp_last_error is per thread: eight threads leave a barrier together and each repeats refusals of
its own two families 2000 times -- refusals the library makes before it looks for a device -- reading back its own code
and text after every call.  Every text carries a number that changes with the iteration, so a text from another thread
and a stale one of the thread's own both show.  ctypes releases the GIL inside the C call, so the calls really overlap.
A refused call creates nothing: the counters of pdsp_dev_live_resources read the same before and after.

(With `thread_local` taken off g_err in pdsp_capi.hip this test fails: DESIGN.md, "Re-entrancy, the plan cache and handle
lifetimes".)"""
import ctypes as C
import threading

from pragma_dsp_amd import _capi

THREADS, ROUNDS = 8, 2000
SIZE, BAD, UNSUPPORTED, WINDOW, RATE = (_capi.ERR_SIZE_NOT_POW2, _capi.ERR_BAD_ARG, _capi.ERR_UNSUPPORTED_SIZE,
                                         _capi.ERR_WINDOW_TYPE, _capi.ERR_SAMPLE_RATE)


def families(lib, ntt, dwt, resampler):
    """Per thread two refusals: k -> (return code, expected code, expected text), k the number the text carries.  None of
    them needs a device."""
    out = C.c_void_p()
    ll = C.c_longlong()
    one = (C.c_double * 1)(1.0)
    return [
        # 0: the plan (a size that is no power of two) | the DCT host form (a type of 1, and others that are not 2 or 3)
        (lambda k: (lib.pdsp_plan_create(2 * k + 3, -1, C.byref(out)), SIZE, f"FFT size must be power of two, got {2 * k + 3}"),
         lambda k: (lib.pdsp_dct_host_f64(None, 1, 64, 1 - 4 * k, 0, None), BAD, f"DCT type must be 2 or 3, got {1 - 4 * k}")),
        # 1: the chirp-z transform of 0 (and fewer) bins | the any-length DFT beyond 4096
        (lambda k: (lib.pdsp_czt_create(8, -k, 0.125, 0.0, 1.0, -1, C.byref(out)), UNSUPPORTED,
                    f"CZT bins must be >= 1, got {-k}"),
         lambda k: (lib.pdsp_dft_host_f64(None, None, 1, 4097 + k, 0, None, None), UNSUPPORTED,
                    f"DFT length must be 2 ... 4096, got {4097 + k}")),
        # 2: an NTT row stride below N | an NTT size that is no power of two
        (lambda k: (lib.pdsp_ntt_forward_u64(ntt, 1, None, k % 64, None, 64, None), BAD,
                    f"strides must be >= N = 64, got {k % 64} (input) and 64 (output)"),
         lambda k: (lib.pdsp_ntt_create(64 * k + 65, -1, C.byref(out)), SIZE,
                    f"NTT size must be power of two, got {64 * k + 65}")),
        # 3: the Hilbert host form with more samples than N | the short-time host form with a hop below 1
        (lambda k: (lib.pdsp_hilbert_host_f64(None, 1, 65 + k, 64, 0, None), BAD, f"len must be 1 ... N = 64, got {65 + k}"),
         lambda k: (lib.pdsp_stft_host_f64(None, 400, 128, -k, 1, None, None), BAD, f"hop must be >= 1, got {-k}")),
        # 4: the resampler's ratio | its output length for an empty row
        (lambda k: (lib.pdsp_resampler_create(-1, -k, 1, one, 1, 0, C.byref(out)), BAD,
                    f"up and down must be >= 1, got up {-k}, down 1"),
         lambda k: (lib.pdsp_resample_output_len(resampler, -k, 0, C.byref(ll)), BAD, f"len must be >= 1, got {-k}")),
        # 5: the sliding DFT's window length | the spectrum host form's sample rate
        (lambda k: (lib.pdsp_sdft_create(16385 + k, 1, one, 1, 0, -1, C.byref(out)), UNSUPPORTED,
                    f"sliding DFT window length must be 2 ... 16384, got {16385 + k}"),
         lambda k: (lib.pdsp_spectrum_host_f64(None, 0, -1.0 - k, 64, 0, 0, None, None, None, None, None), RATE,
                    f"Sample rate must be positive, got {-1 - k}")),
        # 6: the wavelet transform's depth | a row that is no multiple of 2^levels
        (lambda k: (lib.pdsp_dwt_create(-1, b"db2", None, 0, -k, C.byref(out)), BAD, f"levels must be >= 1, got {-k}"),
         lambda k: (lib.pdsp_dwt_forward_f64(dwt, 1, None, 8 * k + 4, 8 * k + 4, None, 8 * k + 4, None), BAD,
                    f"len must be a positive multiple of 2^levels (levels = 3), got {8 * k + 4}")),
        # 7: the FIR host form's tap count | the window type of the short-time inverse
        (lambda k: (lib.pdsp_fir_filter_host_f64(None, 1, 16, None, -k, 0, None), BAD,
                    f"filter must have at least one tap, got {-k}"),
         lambda k: (lib.pdsp_istft_host_f64(None, None, 1, 128, 32, 4 + k, None), WINDOW,
                    f"Unsupported window type: {4 + k}")),
    ]


def test_last_error_is_per_thread_and_refusals_create_nothing(pdsp):
    lib = pdsp.lib
    handles = {}
    for name, create in (("ntt", lambda o: lib.pdsp_ntt_create(64, -1, o)),
                         ("dwt", lambda o: lib.pdsp_dwt_create(-1, b"db2", None, 0, 3, o)),
                         ("resampler", lambda o: lib.pdsp_resampler_create_poly(-1, 3, 2, None, 0, o))):
        handles[name] = C.c_void_p()
        assert create(C.byref(handles[name])) == _capi.OK, name  # no device needed: their tables go up on first use
    before = _capi.live_resources()
    barrier = threading.Barrier(THREADS)
    errors = []

    def worker(tid):
        try:
            pair = families(lib, handles["ntt"], handles["dwt"], handles["resampler"])[tid]
            barrier.wait(timeout=60)
            for i in range(ROUNDS):
                rc, code, text = pair[i & 1](i >> 1)
                got = lib.pdsp_last_error().decode()
                if rc != code or got != text:
                    errors.append((tid, i, rc, code, got, text))
                    return
        except Exception as exc:  # noqa: BLE001
            errors.append((tid, "exception", repr(exc)))

    threads = [threading.Thread(target=worker, args=(t,), daemon=True) for t in range(THREADS)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a worker is stuck"
    assert not errors, errors[:5]
    assert _capi.live_resources() == before
    assert before["tables"] == 0 and before["table_bytes"] == 0  # handles without a first call hold no device memory
    assert lib.pdsp_ntt_destroy(handles["ntt"]) == 0 and lib.pdsp_dwt_destroy(handles["dwt"]) == 0
    assert lib.pdsp_resampler_destroy(handles["resampler"]) == 0
    assert _capi.live_resources() == before


def test_live_resources_refuses_a_null_buffer(pdsp):
    assert pdsp.lib.pdsp_dev_live_resources(None) == _capi.ERR_BAD_ARG
    assert pdsp.lib.pdsp_last_error() == b"null buffer"
    assert set(_capi.live_resources()) == set(_capi.LIVE_FIELDS)
