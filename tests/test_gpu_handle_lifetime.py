"""Tearing down a fully populated handle leaves the device and the process in order.  Handle A
creates every resource a handle can own -- sub-batch stream sets, the profiling event pool, the
phase-buffer store, the tick's events, the control steps' array, both staging buffers of a
snapshot in three rounds -- and is closed; handle B, created after that, runs a plain initialize
and solve and must equal, bit for bit, a handle C that did the same before A existed.  C3 at
batch 5, fp64 and fp32.  (No free-memory figure: the device is shared.  No provoked failure: the
failure paths are tests/test_devres_host.py's.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

B = 5


def _desc(prec):
    from mhpc_minimal_env_amd import configs
    d = configs.c3_desc()
    d.precision = prec
    return d


def _plain(prec):
    """A new handle's initialize + solve: every array the getters give."""
    from mhpc_minimal_env_amd import configs, locomotion as L
    desc = _desc(prec)
    loco = L.MHPCLocomotion(desc=desc, option=L.HSDDP_OPTION(), batch=B, device=0)
    try:
        loco.set_initial_condition(configs.x0_for(desc, B))
        loco.initialization()
        res = {"status": loco.solve_mhpc().copy()}
        res.update(loco.concatenated())
        res.update(loco.get_scalars())
    finally:
        loco.close()
    return res


def _populated(prec):
    """Handle A: every lazily created resource, then close."""
    from mhpc_minimal_env_amd import configs, locomotion as L
    desc, gait = _desc(prec), L.Gait(L.GaitType2D.PRONK)
    x0 = configs.x0_for(desc, B)
    loco = L.MHPCLocomotion(desc=desc, gait=gait, option=L.HSDDP_OPTION(), batch=B, device=0)
    try:
        loco.set_kernel_variant(sub_batches=2, snap_round=2)
        loco.set_profiling(True)
        loco.set_initial_condition(x0)
        loco.initialization()
        assert (loco.solve_mhpc() == 0).all()
        loco.update_problems([gait], None, np.array([1, 0, 2, 1, 0], dtype=np.int32))
        assert loco.solve_mhpc().shape == (B,)
        assert loco.tick_problems([3, 0], x0=x0[[1, 2]], gaits=[gait], steps=[1, 0]).shape == (2,)
        u = loco.control(np.array([0, 1, 2, 0, 1], dtype=np.int32), loco.get_x0())["u"]
        assert u.shape == (B, 4) and np.isfinite(u).all()
        blob = loco.snapshot_problems(list(range(B)))  # rounds of 2, 2, 1: both staging buffers
        assert blob.size == loco.snapshot_size(list(range(B)))
        assert sum(k["launches"] for k in loco.kernel_stats().values()) > 0  # the event pool was used
    finally:
        loco.close()


@pytest.mark.parametrize("prec", [64, 32])
def test_handle_after_a_populated_one(need_gpu, prec):
    before = _plain(prec)
    assert (before["status"] == 0).all()
    _populated(prec)
    after = _plain(prec)
    assert sorted(after) == sorted(before)
    for k in before:
        a, b = np.ascontiguousarray(after[k]), np.ascontiguousarray(before[k])
        assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), \
            f"fp{prec}: {k} of a handle created after the close differs"
