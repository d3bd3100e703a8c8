"""Policy rollouts (mhpc_rollout_policy & co.), the parts that need no GPU: the C-ABI boundary,
and the numpy yardstick of tests/test_gpu_policy.py checked against the oracle's own solve."""
import ctypes
import os
import re

import numpy as np
import pytest

import _policy_ref as PR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mhpc_rollout_policy", "mhpc_rollout_policy_phase", "mhpc_advance_x0", "mhpc_get_x0")


def test_header_declares_and_library_exports_the_policy_entry_points():
    from mhpc_minimal_env_amd import capi
    text = open(os.path.join(ROOT, "include", "mhpc_capi.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % s, code), s
    assert re.search(r"#define\s+MHPC_MAX_POLICY_SAMPLES\s+4096\b", code)
    assert capi.MHPC_MAX_POLICY_SAMPLES == 4096
    # the header names the reference code the entry points replace
    assert "SinglePhase.cpp:117-144" in text and "MultiPhaseDDP.cpp:56-76" in text
    if not os.path.exists(capi.LIB_PATH):
        pytest.fail("libmhpc_amd.so not built (run __graft_entry__.build())")
    lib = ctypes.CDLL(capi.LIB_PATH)
    assert not [s for s in NEW if not hasattr(lib, s)]
    sigs = {n: a for n, _, a in capi.SIGNATURES}
    assert len(sigs["mhpc_rollout_policy"]) == 8 and len(sigs["mhpc_rollout_policy_phase"]) == 9
    assert len(sigs["mhpc_advance_x0"]) == 3 and len(sigs["mhpc_get_x0"]) == 2


def test_cpp_surface_has_the_four_members():
    text = open(os.path.join(ROOT, "include", "mhpc_locomotion.hpp")).read()
    for m in ("rollout_policy", "rollout_policy_phase", "advance_x0", "get_x0"):
        assert re.search(r"\b%s\s*\(" % m, text), m


def test_perturbations_are_seeded_and_scaled():
    x0 = np.zeros((3, 14))
    a, b = PR.perturbed_states(x0, 5), PR.perturbed_states(x0, 5)
    assert (a == b).all() and (a[:, 0] == 0).all()
    assert np.abs(a[..., :7]).max() <= 1e-2 and np.abs(a[..., 7:]).max() <= 1e-1
    assert np.abs(a[:, 1:, 7:]).max() > 1e-2  # velocities really use the larger scale
    s = PR.perturbed_states(np.zeros((2, 6)), 4)
    assert np.abs(s[..., :3]).max() <= 1e-2 and np.abs(s[..., 3:]).max() <= 1e-1


def _c3_solution(batch):
    import oracle as O
    from mhpc_minimal_env_amd import configs, locomotion as L
    desc = configs.c3_desc()
    x0 = configs.x0_for(desc, batch)
    r = O.solve(desc, L.HSDDP_OPTION().to_c(), x0, nthreads=2)
    nominal = []  # [problem][phase] from the phase-concatenated rows
    for b in range(batch):
        ox = ou = ok = 0
        ph = []
        for p in range(desc.n_phases):
            n, N = desc.xsize(p), desc.N[p]
            ph.append({"x": r["X"][b, ox:ox + N * n].reshape(N, n),
                       "u": r["U"][b, ou:ou + N * 4].reshape(N, 4),
                       "K": r["K"][b, ok:ok + N * 4 * n].reshape(N, 4, n)})
            ox, ou, ok = ox + N * n, ou + N * 4, ok + N * 4 * n
        nominal.append(ph)
    return desc, x0, nominal


def test_yardstick_reproduces_the_oracles_nominal_and_stays_finite():
    """The numpy restatement rolled from x0 with the oracle's X, U, K (zero perturbation, so
    u = u_nom) reproduces the oracle's X over the whole-body phases of C3 to <= 1e-12
    relative; from the tests' perturbed states every sample stays finite."""
    import oracle as O
    if not O.available():
        pytest.skip("oracle not built")
    from _util import rel_err
    B = 2
    desc, x0, nominal = _c3_solution(B)
    for b in range(B):
        got = PR.rollout_wb(desc, nominal[b], x0[b], desc.n_wb)
        for p in range(desc.n_wb):
            e = rel_err(got[p]["x"], nominal[b][p]["x"])
            eu = rel_err(got[p]["u"][:-1], nominal[b][p]["u"][:-1])
            print("problem", b, "phase", p, f"x {e:.2e} u {eu:.2e}")
            assert e <= 1e-12 and eu <= 1e-12
    xs = PR.perturbed_states(x0, 3)
    for b in range(B):
        for s in range(xs.shape[1]):
            got = PR.rollout_wb(desc, nominal[b], xs[b, s], desc.n_wb)
            assert all(np.isfinite(q[k]).all() for q in got for k in ("x", "u", "y", "x_end"))
