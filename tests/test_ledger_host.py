"""What the calls on some problems of a live batch share (csrc/mhpc_plan.h: ProblemList,
pack_rows, solve_scope as mhpc_reset_problems uses it, Ledger) on the host: compiled by plain g++
into tests/native/ledger_hostcheck.cpp, whose header comment lists the cases (the problem list's
refusals in both wordings; the row packer over mixed and SRB-only batches in range, list and group
order; reset's order and go[] against the sort and count the runtime had; the ledger against the
members it replaced over random sequences of transitions, and its hand-worked cases)."""
import functools
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "ledger_hostcheck.cpp")


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


def test_ledger_hostcheck():
    _run("ledger_hostcheck", ("-O1",))


def test_ledger_hostcheck_fp32():
    """The header as the fp32 runtime compiles it (real = float)."""
    _run("ledger_hostcheck32", ("-O1", "-DMHPC_FP32"))


def test_ledger_hostcheck_sanitized():
    """The same stand-alone program under the address and undefined-behaviour sanitizers: the row
    packer reads nothing past an SRB-only problem's six entries (the caller's array ends there)."""
    if not _has_sanitizers():
        pytest.skip("this g++ has no sanitizer runtime")
    _run("ledger_hostcheck_san", ("-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"))
