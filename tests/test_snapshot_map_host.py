"""The snapshot's staging side and blob layout (csrc/mhpc_snapshot_map.h over mhpc_copy_map.h) on
the host: the headers the device path runs, compiled by plain g++ into
tests/native/snapshot_map_hostcheck.cpp, pack synthetic problems of uniquely tagged elements out of
arrays of stride 12 (and 7) into a payload of stride 7 in rounds of 3 over 8 entries, with and
without a store, and unpack them into strides 7 and 12, for 8- and 4-byte elements: every element
lands where the map says, nothing else is written, every zeroed tail is zero, every entry is
visited once, and the header's validation catches what it promises to."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "snapshot_map_hostcheck.cpp")


def _run(name, flags):
    exe = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_snapshot_map_hostcheck():
    _run("snapshot_map_hostcheck", ["-O1"])


def test_snapshot_map_hostcheck_sanitized():
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    _run("snapshot_map_hostcheck_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                        "-fno-sanitize-recover=all"])
