"""The ledger event of mhpc_import_plan(_device) (csrc/mhpc_plan.h, Ledger::guessed) on the host:
compiled by plain g++ into tests/native/import_ledger_hostcheck.cpp.  A guess for a problem of a
handle that is just initialised, updated, solved, or solved with reset problems: the problem stops
being fresh; right after initialize everyone else becomes fresh and the next solve starts with the
rollout; after an update or a solve only the flag changes; `open` and the command marks are left
alone; the counts follow the flags; the first op of the next solve, problem by problem."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "import_ledger_hostcheck.cpp")


def _run(name, flags):
    exe = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_import_ledger_hostcheck():
    _run("import_ledger_hostcheck", ["-O1"])


def test_import_ledger_hostcheck_fp32():
    """The header as the fp32 runtime compiles it (real = float)."""
    _run("import_ledger_hostcheck32", ["-O1", "-DMHPC_FP32"])


def test_import_ledger_hostcheck_sanitized():
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    _run("import_ledger_hostcheck_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                         "-fno-sanitize-recover=all"])
