"""The two properties the host side of csrc is cut for ("The host side of the boundary, unit by unit").

Layering, by text: no host unit (pdsp_capi*.hip) includes a kernel header or pdsp_dispatch.inc, and no kernel unit,
kernel header or pdsp_dispatch.inc includes pdsp_host.h.  The Makefile names by hand what pdsp_internal.h includes, so
that list is compared with the #include lines.

Rebuild scope, by `make -n -W <file>` in csrc (what-if mode: nothing is built or touched): a change to pdsp_host.h
compiles host units only, a change to one family's host unit compiles that unit alone, and a change to a kernel header
compiles no host unit."""
import glob
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pragma-dsp_amd", "csrc")
LIB = os.path.join(CSRC, "libpdsp_hip.so")
OBJDIR = os.path.join(CSRC, "build")

INCLUDE = re.compile(r'^\s*#\s*include\s*"([^"]+)"', re.M)


def includes(path):
    return {os.path.basename(i) for i in INCLUDE.findall(open(path).read())}


def host_units():
    return sorted(glob.glob(os.path.join(CSRC, "pdsp_capi*.hip")))


def test_the_units_are_cut_by_family():
    names = {os.path.basename(p)[len("pdsp_capi"):-len(".hip")] for p in host_units()}
    assert names == {"", "_host", "_fir", "_stft", "_dct", "_hilbert", "_resample", "_chirp", "_dwt", "_ntt", "_sdft",
                     "_fft2d"}


def test_no_host_unit_includes_kernel_code():
    for p in host_units() + [os.path.join(CSRC, "pdsp_host.h")]:
        bad = {i for i in includes(p) if i.endswith("_kernel.h") or i == "pdsp_dispatch.inc"}
        assert not bad, f"{os.path.basename(p)} includes {sorted(bad)}"
    # the field arithmetic of the NTT is the one header beyond the contract that a host unit takes, and one unit takes it
    assert [os.path.basename(p) for p in host_units() if "pdsp_goldilocks.h" in includes(p)] == ["pdsp_capi_ntt.hip"]


def test_no_kernel_code_includes_the_host_header():
    kernel_side = glob.glob(os.path.join(CSRC, "pdsp_kernels_*.hip")) + [os.path.join(CSRC, "pdsp_dispatch.inc")] + \
        [p for p in glob.glob(os.path.join(CSRC, "*.h")) if os.path.basename(p) != "pdsp_host.h"]
    assert len(kernel_side) > 30
    for p in kernel_side:
        assert "pdsp_host.h" not in includes(p), os.path.basename(p)


def test_every_host_unit_depends_on_what_the_contract_includes():
    seen, todo = set(), ["pdsp_internal.h"]
    while todo:
        h = todo.pop()
        if h not in seen and os.path.exists(os.path.join(CSRC, h)):
            seen.add(h)
            todo += includes(os.path.join(CSRC, h))
    listed = re.search(r"^INTERNAL_HDRS\s*=(.*)$", open(os.path.join(CSRC, "Makefile")).read(), re.M).group(1).split()
    assert seen == {h for h in listed if not h.startswith("$")}


def what_if(changed=None):
    """The units `make` would compile, and whether it would link, were `changed` newer than everything."""
    cmd = ["make", "-n", "-C", CSRC] + (["-W", changed] if changed else []) + ["libpdsp_hip.so"]
    out = subprocess.run(cmd, capture_output=True, text=True, check=True).stdout
    compiled = re.findall(r"-c -o \S*?/(\w+)\.o ", out)
    return sorted(compiled), bool(re.search(r"-shared -o libpdsp_hip\.so", out))


@pytest.fixture(scope="module")
def built():
    if shutil.which("make") is None or not os.path.exists(LIB) or not os.path.isdir(OBJDIR):
        pytest.skip("needs make, the built library and its object directory")
    # a library newer than every source has nothing to build: a unit that compiles regardless is the Makefile's mistake
    srcs = [p for pat in ("*.hip", "*.h", "*.inc", "Makefile") for p in glob.glob(os.path.join(CSRC, pat))]
    assert os.path.getmtime(LIB) < max(map(os.path.getmtime, srcs)) or what_if() == ([], False)


def test_a_change_to_the_host_header_compiles_host_units_only(built):
    compiled, linked = what_if("pdsp_host.h")
    assert compiled == sorted(os.path.basename(p)[:-len(".hip")] for p in host_units()) and linked


def test_a_change_to_one_family_compiles_that_unit_alone(built):
    assert what_if("pdsp_capi_dwt.hip") == (["pdsp_capi_dwt"], True)


def test_a_change_to_a_kernel_header_compiles_no_host_unit(built):
    compiled, linked = what_if("pdsp_dwt_kernel.h")
    assert compiled and linked and not [u for u in compiled if u.startswith("pdsp_capi")]
    assert all(u.startswith("pdsp_kernels_") for u in compiled)
