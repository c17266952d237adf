"""The N-API addon's argument handling, export by export, driven directly under Node (tests/js/native_cases.js): arity,
every typed-array and number parameter given the wrong type, every refusal text of the addon's own letter for letter,
one library refusal per export handed on unchanged, and the host-only values.  No GPU is needed and none changes an
outcome: every expected throw is raised by the addon itself or by a library check made ahead of the device check, and
every expected value comes from a host-only call.  The three exports that take a plan are the exception: a plan needs
a device, so their rows (lists 'planned' and 'changed-planned') run only where planCreate succeeds."""
import json
import os
import subprocess

from js_host import ADDON, NODE, ROOT, needs_node

EXPORTS = ["applyWindow", "binFrequencies", "czt", "dct", "deviceCount", "dft", "dwt", "fftShift", "firFilter", "hilbert",
           "istft", "magnitude", "nextPow2", "ntt", "phase", "planCreate", "resampleDesign", "resamplePoly", "sdft",
           "spectrum", "spectrumBatch", "spectrumRows", "stft", "transform", "transformBatch", "transformRows", "upfirdn",
           "windowMake"]
PLANNED = {"transform", "transformBatch", "transformRows"}


@needs_node
def test_every_export_handles_its_arguments_as_pinned():
    p = subprocess.run([NODE, os.path.join(ROOT, "tests", "js", "native_cases.js"), ADDON], capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    log = json.loads(p.stdout.strip().splitlines()[-1])
    (_, _, exports, have_plan), rows = log[-1], log[:-1]
    assert exports.split(",") == sorted(EXPORTS + ["version"])
    bad = [r for r in rows if (r[3], r[4]) != (r[5], r[6])]
    assert not bad, bad
    lists = {name: [r for r in rows if r[0] == name] for name in ("pinned", "planned", "changed", "changed-planned")}
    assert sum(map(len, lists.values())) == len(rows)
    # every export has its arity row and at least one refusal beyond the argument types (deviceCount takes nothing)
    seen = lists["pinned"] + lists["planned"]
    for exp in EXPORTS:
        if exp == "deviceCount" or (exp in PLANNED and not have_plan):
            continue
        mine = [r for r in seen if r[1] == exp]
        assert any(r[2] == "too few arguments" for r in mine), exp
        assert any(not r[2].startswith(("too few", "argument ")) for r in mine), exp
    assert len(lists["pinned"]) == 242 and len(lists["changed"]) == 18
    assert [len(lists["planned"]), len(lists["changed-planned"])] == ([30, 2] if have_plan else [0, 0])
