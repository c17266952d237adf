"""The table of tests/test_gpu_graph_capture.py is complete: every function of include/pdsp_hip.h that takes a stream
is captured and replayed by at least one row, and what is left out is forms of a call, not entry points.  A 49th
stream entry point fails here until it has a row.  And the Python half of the refusal ("Streams and graphs"):
BatchedFft.window() of a kind it has not cached raises on a capturing stream before any library call."""
import pytest

import graph_capture_cases as G
from test_batch_checks_cpu import Recorder


def test_the_header_has_48_stream_entry_points():
    names = G.stream_entry_points()
    assert len(names) == len(set(names)) == 48, names
    assert all(n.startswith("pdsp_") and not n.endswith("_host_f64") for n in names)


def test_the_parser_sees_through_comments_and_line_breaks(tmp_path):
    h = tmp_path / "h.h"
    h.write_text("/* PDSP_API int pdsp_commented(int a, pdsp_stream stream); */\n"
                 "// PDSP_API int pdsp_line_comment(pdsp_stream stream);\n"
                 "PDSP_API int pdsp_one(const pdsp_plan *plan, /* why */ float *out,\n"
                 "                      pdsp_stream   stream);\n"
                 "PDSP_API int pdsp_no_stream(pdsp_stream stream, int last);\n"
                 "PDSP_API const char *pdsp_text(void);\n"
                 "PDSP_API int pdsp_two(pdsp_stream stream);\n")
    assert G.stream_entry_points(str(h)) == ["pdsp_one", "pdsp_two"]


def test_every_stream_entry_point_has_a_row():
    names = set(G.stream_entry_points())
    declared = G.declared_entries()
    assert declared <= names, sorted(declared - names)  # a row cannot declare what the header does not have
    missing = names - declared - set(G.EXCLUDED)
    assert not missing, f"stream entry points no row captures: {sorted(missing)}"
    # an entry point is excluded only if no row could reach it: none today, and never one that a row does reach
    assert G.EXCLUDED == {}
    assert not set(G.EXCLUDED) & declared


def test_what_is_left_out_is_five_forms_of_calls():
    forms = G.EXCLUDED_FORMS
    assert sorted(r for _, _, r in forms) == [G.CLEAR] * 2 + [G.SCRATCH] * 3
    assert {(e, r) for e, _, r in forms} == {("pdsp_fft_*", G.SCRATCH), ("pdsp_spectrum_*", G.SCRATCH),
                                             ("pdsp_istft_*", G.SCRATCH), ("pdsp_spectrum_*", G.CLEAR),
                                             ("pdsp_fir_filter_*", G.CLEAR)}
    declared = G.declared_entries()
    for stem, condition, _ in forms:
        assert condition
        hit = [n for n in declared if n.startswith(stem[:-1])]
        assert hit, f"{stem}: the other forms of these entry points must have rows"


def test_rows_are_well_formed_and_within_the_size_limits():
    assert len(set(G.IDS)) == len(G.ROWS)
    for r in G.ROWS:
        assert r.entries and r.dt in ("f32", "f64", "u64"), r
        if r.dt in G.DTS:  # a row of one precision reaches that precision's entry points only
            assert all(e.endswith("_" + r.dt) for e in r.entries), r
        if r.family in ("fft", "spectrum", "peaks", "stft", "istft", "dct", "hilbert", "fir"):
            n = r.shape[0]
            limit = 16384 if r.dt == "f32" or r.family in ("spectrum", "stft") else 8192
            assert n <= limit, r
    # both precisions wherever the entry point has both
    names = set(G.stream_entry_points())
    for r in G.ROWS:
        for e in r.entries:
            other = e[:-3] + ("f64" if e.endswith("f32") else "f32")
            if e[-3:] in G.DTS and other in names:
                assert other in G.declared_entries(), other
    # every code of pdsp_complex_op_f32
    from pragma_dsp_amd import _capi
    assert {r.op for r in G.ROWS if r.family == "complex"} == set(_capi.COMPLEX_OPS)


class _Plan:
    """What BatchedFft.window() touches, without a device."""
    _sfx = "f32"
    _h = dtype = device = None
    size = 64

    def __init__(self):
        self._windows = {}


@pytest.mark.parametrize("capturing", [True, False])
def test_window_of_an_uncached_kind_is_refused_on_a_capturing_stream(pdsp, monkeypatch, capturing):
    import torch
    from pragma_dsp_amd import _capi, batch
    rec = Recorder()
    monkeypatch.setattr(batch, "lib", rec)
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: capturing)
    plan = _Plan()
    if not capturing:  # the stand-in is reached, and the kind is cached from then on
        batch.BatchedFft.window(plan, "hann")
        assert rec.calls == ["pdsp_plan_window_f32"] and "hann" in plan._windows
        return
    with pytest.raises(pdsp.PdspError) as e:
        batch.BatchedFft.window(plan, "hann")
    assert e.value.code == _capi.ERR_BAD_ARG and str(e.value).startswith("stream is capturing:")
    assert rec.calls == [] and plan._windows == {}
    with pytest.raises(pdsp.PdspError) as e:  # an unknown kind keeps its own error
        batch.BatchedFft.window(plan, "kaiser")
    assert e.value.code == _capi.ERR_WINDOW_TYPE and rec.calls == []
    plan._windows["hann"] = 1234  # a cached kind is served during a capture
    assert batch.BatchedFft.window(plan, "hann").data_ptr() == 1234 and rec.calls == []
