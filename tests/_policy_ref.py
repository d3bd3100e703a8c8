"""Yardstick of the policy-rollout tests: a numpy restatement of the reference's
set_initial_condition(x) + forward_sweep_dynamics_only(0) over whole-body phases
(HSDDPSolver/source/SinglePhase.cpp:117-144: u = u_nom + K (x - x_nom), model dynamics;
Dynamics/source/PlanarQuadruped.cpp:8-27: x_next = x + xdot dt with xdot, y from Dyn_BS /
Dyn_FL / Dyn_FS; :58-76: resetmap = identity after a stance mode, Imp_F after mode 2, Imp_B
after mode 4) on the reference's own CasADi kernels (oracle.casadi_ref), plus the seeded
perturbations the tests start from.  tests/test_policy.py checks this yardstick itself
against the oracle's solve on the CPU; tests/test_gpu_policy.py checks the HIP kernel
against it."""
import numpy as np

DYN = {1: "Dyn_BS", 2: "Dyn_FL", 3: "Dyn_FS", 4: "Dyn_FL"}
IMP = {2: "Imp_F", 4: "Imp_B"}

# perturbation scale: 1e-2 on positions and angles, 1e-1 on velocities
SCALE_WB = np.array([1e-2] * 7 + [1e-1] * 7)
SCALE_SRB = np.array([1e-2] * 3 + [1e-1] * 3)


def perturbed_states(x0, n_samples, seed=20261019):
    """xs [B][n_samples][r]: sample 0 is x0 itself, the others x0 + scale * U(-1, 1)."""
    x0 = np.asarray(x0, dtype=np.float64)
    B, r = x0.shape
    scale = SCALE_WB if r == 14 else SCALE_SRB
    rng = np.random.default_rng(seed)
    xs = x0[:, None, :] + scale * rng.uniform(-1.0, 1.0, size=(B, n_samples, r))
    xs[:, 0, :] = x0
    return np.ascontiguousarray(xs)


def rollout_wb(desc, nominal, x_start, n_phases):
    """One sample through whole-body phases 0..n_phases-1 of `desc`.  nominal[p] = {"x" [N][14],
    "u" [N][4], "K" [N][4][14]} of the problem.  Returns a list of per-phase dicts: x [N][14],
    u, y [N][4] (last knot's u, y zero) and x_end, the state after the phase's resetmap."""
    from oracle import casadi_ref as C
    assert n_phases <= desc.n_wb
    dt = desc.dt_wb
    x = np.array(x_start, dtype=np.float64)
    out = []
    for p in range(n_phases):
        mode, N = desc.mode_seq[p], desc.N[p]
        nom = nominal[p]
        X, U, Y = np.zeros((N, 14)), np.zeros((N, 4)), np.zeros((N, 4))
        for k in range(N - 1):
            u = nom["u"][k] + nom["K"][k] @ (x - nom["x"][k])
            xdot, y = C.call(DYN[mode], x, u)
            X[k], U[k], Y[k] = x, u, y
            x = x + xdot * dt
        X[N - 1] = x
        if mode in IMP:
            x = C.call(IMP[mode], x)[0]
        out.append({"x": X, "u": U, "y": Y, "x_end": x.copy()})
    return out
