"""The re-stride map of mhpc_copy_problems (csrc/mhpc_copy_map.h) on the host: the header the copy
kernel runs, compiled by plain g++ into tests/native/copy_map_hostcheck.cpp, copies one synthetic
problem of uniquely tagged elements between two sets of host arrays -- knot strides (7,7), (7,12),
(12,7), stores of differing shape or on one side only, 8- and 4-byte elements -- and every element
must land at the destination's index with nothing else written, every run inside both arrays."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "copy_map_hostcheck.cpp")


def _run(name, flags):
    exe = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_copy_map_hostcheck():
    _run("copy_map_hostcheck", ["-O1"])


def test_copy_map_hostcheck_sanitized():
    """The same stand-alone program under the address and undefined-behaviour sanitizers: an
    offset of the map outside an array is a report, not a silent neighbour."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    _run("copy_map_hostcheck_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                    "-fno-sanitize-recover=all"])
