"""The N-API addon's surface that needs no device (webspeechanalyzer_amd/napi/): the 46 exports by name, and how each of the 45 other than
`create` answers four argument sets (none, six {}, the numbers 1 .. 6, four nulls): the thrown error's class and whole message, the kind of the
value returned, or the string a promise rejects with.  tests/golden/napi_surface.json holds what the addon did before the binding was cut into
files (tests/golden/gen/make_napi_surface.js records it); usage texts and refusals are part of what a JavaScript caller sees."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NODE = shutil.which("node")
PROBE = os.path.join(ROOT, "tests", "js", "napi_surface_probe.js")
ADDON = os.path.join(ROOT, "webspeechanalyzer_amd", "lib", "wsa_napi.node")
GOLDEN = os.path.join(ROOT, "tests", "golden", "napi_surface.json")
pytestmark = pytest.mark.skipif(NODE is None, reason="node not installed")


def test_exports_and_refusals_are_the_recorded_ones():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "csrc")], check=True)
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "webspeechanalyzer_amd", "napi")], check=True)
    want = json.load(open(GOLDEN))
    assert len(want["exports"]) == 46 and len(want["calls"]) == 45 and "create" not in want["calls"]
    r = subprocess.run([NODE, PROBE, ADDON], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    got = json.loads(r.stdout)
    assert got["exports"] == want["exports"]
    for name in want["exports"]:
        if name != "create":
            assert got["calls"][name] == want["calls"][name], name
    assert got == want
