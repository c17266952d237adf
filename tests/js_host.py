"""Shared plumbing of the tests that run a case list under Node: where the addon and node are, the skip mark for a
machine without them, and run_cases(), which hands a JSON case list to a driver under tests/js/ (built on
tests/js/_cases.js) and reads back its results."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ADDON = os.path.join(ROOT, "pragma-dsp_amd", "csrc", "pdsp_napi.node")
NODE = shutil.which("node")
needs_node = pytest.mark.skipif(NODE is None or not os.path.exists(ADDON), reason="node or the addon is not available")


def run_cases(driver, cases, tmp_path, tail=1, timeout=120):
    """Run tests/js/<driver> on `cases`: (results, then each of the `tail` entries the driver appends after them)."""
    cin, cout = tmp_path / "cases.json", tmp_path / "out.json"
    cin.write_text(json.dumps(cases))
    subprocess.run([NODE, os.path.join(ROOT, "tests", "js", driver), str(cin), str(cout)], check=True, timeout=timeout)
    res = json.loads(cout.read_text())
    return (res[:len(res) - tail], *res[len(res) - tail:])
