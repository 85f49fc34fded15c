"""The host planner's per-segment analysis (pinot_amd/csrc/pgpu_segplan.h) against the code it replaced (CPU only).

tests/sanitize/segplan_fuzz.cpp holds a verbatim copy of the vector-based analyze / split_children / scan_runs /
prefix_ranges / lead_model / prefix_loss / lead_choice and plans every case with both: children, selectivities, scan
columns, id runs, the dense / residual split, rho, staged columns, prefix ranges at every lead width, the lead model
and the lead choice must agree exactly, doubles bit for bit.  Directed cases sit at every inline capacity of the
header (one below, at, one above), at the nesting limit, at PGPU_SLICE_RANGES and one more prefix ranges per width,
and on every malformed shape; seeded random programs of at most 40 nodes follow.  The harness is a stand-alone
program built with -fsanitize=address,undefined and -fno-sanitize-recover: an out-of-bounds access or overflow in
the inline storage or its spill fails the test.
"""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pinot_amd", "csrc")
SOURCE = os.path.join(ROOT, "tests", "sanitize", "segplan_fuzz.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="g++ not available")


@pytest.fixture(scope="module")
def fuzz(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("sanitize") / "segplan_fuzz")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-fno-omit-frame-pointer", "-I", CSRC, "-I", os.path.join(ROOT, "include"), SOURCE, "-o", out]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        pytest.fail(r.stderr[-4000:])
    return out


def _run(fuzz, *args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([fuzz, *args], capture_output=True, text=True, env=env, timeout=300)
    assert r.returncode == 0, (args, r.stdout[-2000:], r.stderr[-6000:])
    assert r.stdout.strip().endswith("ok")


def test_directed_cases(fuzz):
    _run(fuzz, "directed")


@pytest.mark.parametrize("seed", [1, 1_000_003, 20_000_033])
def test_random_programs(fuzz, seed):
    _run(fuzz, "random", str(seed), "20000")
