"""Per-problem user commands, host side: the three entry points in the header and the ctypes
mirror, and the wrapper's argument handling (float rounding, scalar broadcast) -- no GPU."""
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mhpc_set_commands", "mhpc_get_commands", "mhpc_get_reference_problems")


def test_header_declares_the_command_calls():
    src = open(os.path.join(ROOT, "include", "mhpc_capi.h")).read()
    for n in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*mhpc_handle\s*\*" % n, src), n


def test_ctypes_mirror_has_the_command_calls():
    import ctypes
    from mhpc_minimal_env_amd import capi
    sig = {n: (r, a) for n, r, a in capi.SIGNATURES}
    dp = ctypes.POINTER(ctypes.c_double)
    assert sig["mhpc_set_commands"] == (ctypes.c_int, [ctypes.c_void_p, dp, dp])
    assert sig["mhpc_get_commands"] == (ctypes.c_int, [ctypes.c_void_p, dp, dp])
    assert sig["mhpc_get_reference_problems"] == (
        ctypes.c_int, [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, dp])


def test_cpp_surface_has_the_command_members():
    src = open(os.path.join(ROOT, "include", "mhpc_locomotion.hpp")).read()
    for n in ("set_commands", "get_commands", "get_reference_problems"):
        assert re.search(r"\b%s\s*\(" % n, src), n
    assert "std::vector<float>& vel" in src


def test_shard_rows_slices_commands_like_x0():
    from mhpc_minimal_env_amd import sharding
    vel = np.linspace(0.5, 2.5, 11)
    parts = [sharding.shard_rows(vel, 4, r) for r in range(4)]
    np.testing.assert_array_equal(np.concatenate(parts), vel)
    for r, p in enumerate(parts):
        off, cnt = sharding.shard_offsets(11, 4, r)
        np.testing.assert_array_equal(p, vel[off:off + cnt])


class _Bare:
    """MHPCLocomotion without a handle: only what _command_array reads."""
    batch = 5


def _arr(v, name="vel"):
    from mhpc_minimal_env_amd import locomotion as L
    return L.MHPCLocomotion._command_array(_Bare(), v, name)


def test_command_array_rounds_through_float():
    a = _arr([0.1, 1.5, 2.0, -0.02, 1e-9])
    assert a.dtype == np.float64 and a.flags["C_CONTIGUOUS"]
    np.testing.assert_array_equal(a, np.array([0.1, 1.5, 2.0, -0.02, 1e-9],
                                              dtype=np.float32).astype(np.float64))
    assert a[0] != 0.1  # USRCMD is float: 0.1 is not representable


def test_command_array_broadcasts_a_scalar_and_keeps_none():
    assert _arr(None) is None
    np.testing.assert_array_equal(_arr(0.02), np.full(5, float(np.float32(0.02))))
    np.testing.assert_array_equal(_arr(np.float32(2.5)), np.full(5, 2.5))


def test_command_array_rejects_a_wrong_length():
    for bad in ([1.0, 2.0], np.zeros((5, 1)), np.zeros(6)):
        with pytest.raises(ValueError):
            _arr(bad, "height")
