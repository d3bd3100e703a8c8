"""The owner of the runtime's per-call device temporaries (csrc/mhpc_devtemp.h) on the host,
against a fake device with injectable failures (tests/native/devtemp_hostcheck.cpp): values
round-trip as static_cast gives them, and after a failure at any allocation or copy the error
is sticky, nothing else touches the device, no caller array is written and every allocation is
freed exactly once.  Plain g++: the header needs the HIP API's declarations, not its runtime."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "devtemp_hostcheck.cpp")
EXE = os.path.join(ROOT, "tests", "_build", "devtemp_hostcheck")
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")


def test_devtemp_hostcheck():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-D__HIP_PLATFORM_AMD__",
                    "-I" + os.path.join(ROCM, "include"), "-o", EXE, SRC], check=True)
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-4000:] + r.stderr[-2000:]
