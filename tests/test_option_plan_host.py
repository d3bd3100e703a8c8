"""The option plan (csrc/mhpc_plan.h: option_cap, check_option, plan_options, scope_caps, solve_ops)
on the host: the pure part of mhpc_set_option_sets and of the launch schedule a scope gets, compiled
by plain g++ into tests/native/option_hostcheck.cpp, whose header comment lists the cases (iteration
caps from the reference's loops for 0, fractional and huge budgets; the record checks; the op
counts of a schedule; the maxima over a list against the maxima over the batch; merging, dropping
and slot reuse of the option table, the 33rd record refused)."""
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "option_hostcheck.cpp")


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


def test_option_hostcheck():
    _run("option_hostcheck", ("-O1",))


def test_option_hostcheck_fp32():
    """The header as the fp32 runtime compiles it (real = float)."""
    _run("option_hostcheck32", ("-O1", "-DMHPC_FP32"))


def test_option_hostcheck_sanitized():
    """The same stand-alone program under the address and undefined-behaviour sanitizers."""
    if not _has_sanitizers():
        pytest.skip("this g++ has no sanitizer runtime")
    _run("option_hostcheck_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
