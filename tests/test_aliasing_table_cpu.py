"""The table of tests/test_gpu_aliasing.py is complete: every device entry point of the transforms and spectra in
include/pdsp_hip.h (pdsp_fft_*_f32 / _f64, pdsp_spectrum*) has a row that pins its aliasing contract, and the rows
reach the kernels and sizes the contract was derived for.  A new entry point of these families fails here until it
has a row."""
import aliasing_cases as AC
import graph_capture_cases as G


def test_the_header_has_the_thirteen_entry_points():
    names = AC.aliasing_entry_points()
    assert len(names) == len(set(names)) == 13, names
    assert set(names) <= set(G.stream_entry_points())
    assert {n for n in G.stream_entry_points() if n.startswith(("pdsp_fft_forward", "pdsp_fft_inverse",
                                                                 "pdsp_spectrum"))} == set(names)


def test_the_parser_sees_through_comments_and_host_forms(tmp_path):
    h = tmp_path / "h.h"
    h.write_text("/* PDSP_API int pdsp_fft_commented_f32(int a, pdsp_stream stream); */\n"
                 "PDSP_API int pdsp_fft_new_form_f64(const pdsp_plan *plan, /* why */ double *out,\n"
                 "                                   pdsp_stream   stream);\n"
                 "PDSP_API int pdsp_fft_transform_host_f64(const double *re, int inverse);\n"
                 "PDSP_API int pdsp_spectrum_rows_host_f64(const double *const *rows, pdsp_stream stream);\n"
                 "PDSP_API int pdsp_fft_shift_f64(const double *in, long long n, double *out);\n"
                 "PDSP_API int pdsp_dct_f32(const pdsp_plan *plan, pdsp_stream stream);\n"
                 "PDSP_API int pdsp_spectrum_new(pdsp_stream stream);\n")
    assert AC.aliasing_entry_points(str(h)) == ["pdsp_fft_new_form_f64", "pdsp_spectrum_new"]


def test_every_entry_point_has_a_row():
    names = set(AC.aliasing_entry_points())
    declared = AC.declared_entries()
    assert declared <= names, sorted(declared - names)  # a row cannot declare what the header does not have
    missing = names - declared
    assert not missing, f"entry points whose aliasing contract no row pins: {sorted(missing)}"


def test_rows_are_well_formed():
    ids = [r.name for r in AC.ROWS]
    assert len(set(ids)) == len(ids)
    for r in AC.TRANSFORM_ROWS:
        assert r.entry == f"{AC.ENTRY[r.kind]}_{r.dt}" and r.dt in AC.DTS, r
        assert r.n <= (16384 if r.dt == "f32" or r.kernel == "fft_real_kernel" else 8192), r  # single-pass sizes
        # at least three workgroups and a partial last one (fft_real_kernel at 16384: the batch that picks it)
        per = AC.rows_per_workgroup(r.kernel, r.n)
        assert r.batch > 2 * per and (per == 1 or r.batch % per), r
        assert r.batch == (8 if (r.kernel, r.n) == ("fft_real_kernel", 16384) else 2 * per + 1), r
    for r in AC.SPECTRUM_ROWS:
        assert r.entry in ("pdsp_spectrum_f32", "pdsp_spectrum_f64", AC.SP) and r.outputs, r
        assert ("rec" in r.outputs) == (r.entry == AC.SP) and not (r.entry == AC.SP and "idx" in r.outputs), r
        assert r.batch >= 3 and r.stride >= 1, r


def test_rows_reach_the_required_kernels_and_sizes():
    seen = {}
    for r in AC.TRANSFORM_ROWS:
        if r.kind in AC.PLANAR:
            seen.setdefault((r.kernel, r.dt), set()).add(r.n)
    for key, sizes in AC.REQUIRED_TRANSFORMS.items():
        assert sizes <= seen.get(key, set()), (key, sorted(sizes - seen.get(key, set())))
    # every planar entry point on every kernel it can reach at these sizes
    for dt in AC.DTS:
        for kernel, n, _offs, _sw, kinds in AC.TRANSFORM_SPECS[dt]:
            for kind in kinds or AC.PLANAR:
                assert any((r.kernel, r.n, r.kind, r.dt) == (kernel, n, kind, dt) for r in AC.TRANSFORM_ROWS)
        # all four interleaved entry points at N = 1, 64, 4096 and the largest single-pass size
        for kind in ("ifwd", "iinv"):
            got = {r.n for r in AC.TRANSFORM_ROWS if (r.kind, r.dt) == (kind, dt)}
            assert got == {1, 64, 4096, 16384 if dt == "f32" else 8192}, (kind, dt, got)
    # N = 8 from misaligned planes, N = 64 with staged_small 0, N = 8192 / 16384 from a misaligned input
    by = {(r.dt, r.kernel, r.n): r for r in AC.TRANSFORM_ROWS if r.kind in ("complex", "real")}
    for dt in AC.DTS:
        assert all(by[dt, "fft_stockham_kernel", 8].offs), dt
        assert by[dt, "fft_stockham_kernel", 64].switches == {"staged_small": 0}, dt
        assert by[dt, "fft_stockham_kernel", 8192].offs[0] * (4 if dt == "f32" else 8) % 16, dt
    assert by["f32", "fft_stockham_kernel", 16384].offs[0] * 4 % 16
    spec = AC.SPECTRUM_ROWS
    for prefix in AC.REQUIRED_SPECTRUM_PREFIXES:
        assert any(r.kernel.startswith(prefix) for r in spec), prefix
    assert {r.n for r in spec if r.kernel == "spectrum_staged_kernel"} == {64, 512}
    packed = [r.kernel for r in spec if r.kernel.startswith("spectrum_packed_kernel-FAST")]
    assert {k.split("-")[3][:2] for k in packed} >= {"w0", "w1", "w2"}  # rect, table, fused window
    assert {r.sides for r in spec} == {"one", "two"}
    assert any(r.stride < r.n for r in spec if r.dt == "f32") and any(r.stride < r.n for r in spec if r.dt == "f64")
    # the three peak forms: fused into spectrum_packed_kernel and spectrum_dif16k_kernel, and peak_wave_kernel behind
    # the stored rows of the sizes below 64
    peaks = [r for r in spec if r.entry == AC.SP]
    assert any(r.kernel.startswith("spectrum_packed_kernel") and r.kernel.endswith("-peak") for r in peaks)
    assert any(r.kernel.startswith("spectrum_dif16k_kernel") and r.kernel.endswith("-peak") for r in peaks)
    assert any(r.n < 64 for r in peaks)
    assert any(r.outputs == ("rec",) for r in peaks)  # peaks-only output
