"""The step-and-window map of the device-resident I/O (csrc/mhpc_step_map.h) on the host: the
header that the control, plan export and plan import kernels and the runtime's validation run,
compiled by plain g++ into tests/native/step_map_hostcheck.cpp, over synthetic layouts -- C3-like
(80, 80 whole-body + 2 SRB), SRB-only, one whole-body phase, a rotated ko, a phase with N = 2 --
under both scopes.  Steps: every one maps to a distinct (phase, knot) with kk = ko + k, the
boundary steps land where the map states, steps outside 0..n-1 are refused with the output
untouched.  Windows of W = 1, W = 5 from 3 steps before a phase boundary, W past the last step and
W = all steps, in rows of 14 and 6, in the export's and in the import's direction: every element
of every [W][c] block is classified exactly once; every offset equals an independent restatement,
lies inside its array and inside its record's own field and is named once; a window across a
boundary never names a phase's last knot; the ALL scope uses 6 columns in the SRB phases of a
whole-body problem; the export-only kinds are never a destination."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "step_map_hostcheck.cpp")


def _run(name, flags):
    exe = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_step_map_hostcheck():
    _run("step_map_hostcheck", ["-O1"])


def test_step_map_hostcheck_sanitized():
    """The same stand-alone program under the address and undefined-behaviour sanitizers: an
    offset of the map outside an array is a report, not a silently read or overwritten
    neighbour."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    _run("step_map_hostcheck_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                    "-fno-sanitize-recover=all"])
