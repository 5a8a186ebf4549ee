"""The host build of poseidon2_core.hpp as a stand-alone program under AddressSanitizer and UBSan
(tests/asan/p2_untied_main.cpp), on the known answers of tests/golden/p2_untied_kat.json, for risc0's Core<24, 21, 0>
and SP1's Core<16, 13, 1>.  p2::madk / mulk / smadk / smulk have one signature for the device form (inline asm whose
addend is an input operand of its own) and for the host branch; this guards the host branch.  Nothing of the program is
loaded into Python.

The fixture holds canonical integers: inputs (zeros, all p - 1, 0 .. W - 1, seeded random states) and the outputs of
the plain-integer reference tests/p2_edges.py:permute under the instance's preset tables; the test recomputes them, so
a fixture that drifted from the reference fails here and not in the program."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as o
import p2_edges as E

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KAT = os.path.join(ROOT, "tests", "golden", "p2_untied_kat.json")
INSTANCES = [(24, 0), (16, 1)]


def mont(v):
    return [int(x) for x in o.to_mont(np.array([int(x) for x in v], dtype=np.uint64))]


@pytest.fixture(scope="module")
def kat(orc):
    with open(KAT) as f:
        doc = json.load(f)
    out = []
    for w, m4 in INSTANCES:
        cases = doc["%d/%d" % (w, m4)]
        assert len(cases) >= 6 and all(len(c["in"]) == w and len(c["out"]) == w for c in cases)
        out.append((w, m4, E.preset_tables(w, m4), cases))
    return out


def test_fixture_is_the_reference(kat):
    for w, m4, tabs, cases in kat:
        for c in cases:
            assert E.permute(c["in"], m4, *tabs) == c["out"], (w, m4)


def test_host_permutation_under_sanitizers(kat, tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = str(tmp_path / "p2_untied_main")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "asan", "p2_untied_main.cpp")],
                   check=True, capture_output=True)
    lines = []
    for w, m4, tabs, cases in kat:
        lines.append("%d %d %d" % (w, m4, len(cases)))
        lines += [" ".join(map(str, mont(t))) for t in tabs]
        for c in cases:
            lines.append(" ".join(map(str, mont(c["in"]))))
            lines.append(" ".join(map(str, mont(c["out"]))))
    path = tmp_path / "cases.txt"
    path.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe, str(path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    assert "p2_untied_main ok: %d instances" % len(INSTANCES) in r.stdout
