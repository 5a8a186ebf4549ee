"""The in-flight pipeline behind rk_prove_session and rk_p3_prove_shards (raiko_amd/csrc/inflight.hpp) as a stand-alone
program (tests/asan/inflight_main.cpp), once under ThreadSanitizer and once under AddressSanitizer + UBSan.  The machine is
host threads around three callbacks, so it needs no GPU: the callbacks are fakes that count their calls.  The scenarios are
the ones a GPU run reaches only with a proof that really fails: a stage, a proof or a verification failing while others
are in flight, two failures at once, a callback that throws, a device whose remaining work is pinned elsewhere.  A
deadlock shows as the time limit of the subprocess; the last scenario line printed names where it stopped.  Nothing of the
program is loaded into Python."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENARIOS = ["options and counts", "normal run", "more workers than items", "pinned items", "stage fails", "prove fails",
             "verify fails", "two failures at once", "stage throws", "prove throws", "verify throws", "verify off"]


@pytest.mark.parametrize("name,flags", [("tsan", ["-fsanitize=thread"]),
                                        ("asan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_pipeline_under_sanitizers(name, flags, tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build the sanitizer program")
    exe = str(tmp_path / ("inflight_main_" + name))
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags +
                   ["-I", os.path.join(ROOT, "raiko_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "asan", "inflight_main.cpp")],
                   check=True, capture_output=True)
    try:
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    except subprocess.TimeoutExpired as e:
        pytest.fail("deadlock? the program printed:\n%s" % (e.stdout or b"").decode(errors="replace")[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert r.stderr == "", r.stderr[-4000:]
    for s in SCENARIOS:
        assert "scenario %s: ok" % s in r.stdout, r.stdout
    assert "inflight_main ok: %d scenarios" % len(SCENARIOS) in r.stdout
