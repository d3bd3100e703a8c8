"""The control-step map of mhpc_control / mhpc_control_device (csrc/mhpc_control_map.h) on the
host: the header the control kernel and the runtime's step validation run, compiled by plain g++
into tests/native/control_map_hostcheck.cpp, over synthetic layouts -- C3-like (80, 80 whole-body
+ 2 SRB), SRB-only, one whole-body phase, a rotated ko, a phase with N = 2.  Every step of each
layout maps to a distinct (phase, knot < N - 1) at the layout's own ko, the steps either side of
each phase boundary land where the map states, n_steps is the sum of N - 1 over the control
phases, steps outside are refused, and every record the offsets name lies inside the arrays."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "control_map_hostcheck.cpp")


def _run(name, flags):
    exe = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_control_map_hostcheck():
    _run("control_map_hostcheck", ["-O1"])


def test_control_map_hostcheck_sanitized():
    """The same stand-alone program under the address and undefined-behaviour sanitizers: an
    offset of the map outside an array is a report, not a silent neighbour."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    _run("control_map_hostcheck_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                       "-fno-sanitize-recover=all"])
