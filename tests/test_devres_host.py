"""The owners of a handle's device memory, streams and events (csrc/mhpc_devres.h) on the host,
against a fake device with a failure injectable at every allocation and creation
(tests/native/devres_hostcheck.cpp): one release per object, none from a moved-from owner, a failed
creation leaves the owner as it was, a stream set is all or nothing, a grown vector of sets holds
only complete ones, the seven-array grow-and-swap of ensure_knot_arrays keeps the old arrays on a
failure, and a struct with Handle's resource members releases memory before events before streams,
the main stream last.  A stand-alone program built by plain g++ (the header needs the HIP API's
declarations, not its runtime), run as it is and under the address and undefined-behaviour
sanitizers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "devres_hostcheck.cpp")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def _run(name, flags):
    exe = os.path.join(ROOT, "tests", "_build", name)
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(ROCM, "include"), "-o", exe, SRC], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-4000:]


def test_devres_hostcheck():
    _run("devres_hostcheck", ["-O1"])


def test_devres_hostcheck_sanitized():
    """A double release or a use of a released object is a report, not a count."""
    probe = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", os.devnull],
                           input="int main(){return 0;}", capture_output=True, text=True)
    if probe.returncode != 0:
        pytest.skip("this g++ has no sanitizer runtime")
    _run("devres_hostcheck_san", ["-O1", "-g", "-fsanitize=address,undefined",
                                  "-fno-sanitize-recover=all"])
