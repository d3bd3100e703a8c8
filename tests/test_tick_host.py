"""The scope of a list-driven solve (csrc/mhpc_plan.h: solve_scope, scope_clip, scope_split) on the
host: the pure part of mhpc_tick_problems' plan, compiled by plain g++ into
tests/native/tick_hostcheck.cpp, whose header comment lists the cases (a list over several groups
with an empty one, n = 1, the whole batch, an unsorted list, the fresh / rolled split, sub-batch
clipping inside a group)."""
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "tick_hostcheck.cpp")


@functools.lru_cache(maxsize=None)
def _build(name, flags):
    """One build of each variant a session."""
    exe = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", exe, SRC], check=True)
    return exe


def _run(name, flags):
    r = subprocess.run([_build(name, flags)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


def _has_sanitizers():
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main(){return 0;}", capture_output=True, text=True)
    return probe.returncode == 0


def test_tick_hostcheck():
    _run("tick_hostcheck", ("-O1",))


def test_tick_hostcheck_fp32():
    """The header as the fp32 runtime compiles it (real = float)."""
    _run("tick_hostcheck32", ("-O1", "-DMHPC_FP32"))


def test_tick_hostcheck_sanitized():
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    if not _has_sanitizers():
        pytest.skip("this g++ has no sanitizer runtime")
    _run("tick_hostcheck_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
