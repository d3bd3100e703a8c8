"""Generate the committed golden fixtures (run in the container that holds /root/reference).

  kat_model.npz      per-function known-answer vectors of the reference's OWN CasADi kernels
                     (oracle/_ref, compiled from /root/reference/CasadiGen/source): random
                     (x, u) per mode, x ~ U(-1,1) for q and U(-3,3) for qdot, u ~ U(-20,20)
                     (SURVEY.md §8c(i)); dense outputs scattered like casadi_interface.
  kat_model_traj.npz the same kernels at knots of the oracle's C5 solution (make_kat_traj):
                     states the solver visits, with contact forces, torques and the
                     barrier active, a quarter of them from its worst-conditioned problem.
  solve_<cfg>.npz    full HSDDP solves of the CPU oracle (restatement + CasADi kernels) for
                     the BASELINE configs at small batch: inputs (x0) and every output incl.
                     the decision trace.

The reference cannot travel to the GPU box, so these files are what the GPU tests check
against when the oracle cannot run there.  Usage: python tests/golden/make_golden.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "oracle")]

import casadi_ref as cr  # noqa: E402
import oracle as O  # noqa: E402
from mhpc_minimal_env_amd import configs, locomotion as L  # noqa: E402

KAT_N = 64
KAT_SEED = 20261015


def make_kat():
    rng = np.random.default_rng(KAT_SEED)
    n = KAT_N
    x = np.concatenate([rng.uniform(-1, 1, (n, 7)), rng.uniform(-3, 3, (n, 7))], axis=1)
    u = rng.uniform(-20, 20, (n, 4))
    xs = rng.uniform(-1, 1, (n, 6))
    us = rng.uniform(-50, 50, (n, 4))
    ps = rng.uniform(-1, 1, (n, 4))
    ss = np.array([[0, 1], [1, 0], [0, 0], [1, 1]] * (n // 4), dtype=float)
    return eval_kat(x, u, xs, us, ps, ss)


def eval_kat(x, u, xs, us, ps, ss):
    """Every reference kernel at the whole-body points (x, u) and the SRB points (xs, us,
    footholds ps, contact flags ss)."""
    n = len(x)
    out = {"x": x, "u": u}
    for nm in ("Dyn_BS", "Dyn_FL", "Dyn_FS"):
        r = [cr.call(nm, x[i], u[i]) for i in range(n)]
        out[nm + ".xdot"] = np.stack([a[0] for a in r])
        out[nm + ".y"] = np.stack([a[1] for a in r])
        r = [cr.call(nm + "_par", x[i], u[i]) for i in range(n)]
        for j, k in enumerate(("Ac", "Bc", "C", "D")):
            out[f"{nm}_par.{k}"] = np.stack([a[j] for a in r])
    for nm in ("Imp_F", "Imp_B"):
        r = [cr.call(nm, x[i]) for i in range(n)]
        out[nm + ".xplus"] = np.stack([a[0] for a in r])
        out[nm + ".y"] = np.stack([a[1] for a in r])
        out[nm + "_par.Px"] = np.stack([cr.call(nm + "_par", x[i])[0] for i in range(n)])
    for nm in ("WB_FL1_terminal_constr", "WB_FL2_terminal_constr"):
        r = [cr.call(nm, x[i]) for i in range(n)]
        out[nm + ".h"] = np.array([np.ravel(a[0])[0] for a in r])
        out[nm + ".hx"] = np.stack([np.ravel(a[1]) for a in r])
        out[nm + ".hxx"] = np.stack([a[2] for a in r])
    for nm in ("Jacob_F", "Jacob_B"):
        r = [cr.call(nm, x[i]) for i in range(n)]
        out[nm + ".J"] = np.stack([a[0] for a in r])
        out[nm + ".Jd"] = np.stack([a[1] for a in r])
    n = len(xs)
    out.update({"srb.x": xs, "srb.u": us, "srb.p": ps, "srb.s": ss})
    r = [cr.call("FBDynamics", xs[i], us[i], ps[i], ss[i]) for i in range(n)]
    out["FBDynamics.xdot"] = np.stack([a[0] for a in r])
    r = [cr.call("FBDynamics_par", xs[i], us[i], ps[i], ss[i]) for i in range(n)]
    out["FBDynamics_par.Ac"] = np.stack([a[0] for a in r])
    out["FBDynamics_par.Bc"] = np.stack([a[1] for a in r])
    return out


TRAJ_WORST = 50  # the worst-conditioned problem of x0_for(c5_desc(), 64) (tests/_conditioning.py)


def _spread(total, n):
    return np.round(np.linspace(0, total - 1, n)).astype(int)


def make_kat_traj():
    """The same kernels at states the solver visits: knots of the oracle's C5 solution for
    x0_for(c5_desc(), 64).  64 whole-body knots (x, u, their phase's mode in "mode", "pre_td"
    = the phase's last knot, the state the touchdown impact maps): 16 of problem TRAJ_WORST
    spread evenly over its whole-body phases, the last knot of each flight phase among them,
    and 48 spread evenly over the other problems and over the whole-body knots, every third
    one the last knot of a flight phase.  64 SRB knots (x, u, foothold, contact flags) alike."""
    desc = configs.c5_desc()
    B = KAT_N
    sol = O.solve(desc, L.HSDDP_OPTION().to_c(), configs.x0_for(desc, B), nthreads=4)
    P = desc.n_phases
    N = [desc.N[p] for p in range(P)]
    mode = [desc.mode_seq[p] for p in range(P)]
    xsz = [desc.xsize(p) for p in range(P)]
    xoff = np.concatenate([[0], np.cumsum([N[p] * xsz[p] for p in range(P)])])
    uoff = np.concatenate([[0], np.cumsum([N[p] * 4 for p in range(P)])])

    def knot(b, p, k):
        x = sol["X"][b, xoff[p] + k * xsz[p]: xoff[p] + (k + 1) * xsz[p]]
        u = sol["U"][b, uoff[p] + k * 4: uoff[p] + (k + 1) * 4]
        return x.copy(), u.copy()

    others = [b for b in range(B) if b != TRAJ_WORST]
    prob = [TRAJ_WORST] * 16 + [others[i] for i in _spread(len(others), 48)]

    # whole-body knots
    wb = [(p, k) for p in range(desc.n_wb) for k in range(N[p])]
    last = [wb.index((p, N[p] - 1)) for p in range(desc.n_wb) if mode[p] in (2, 4)]
    pick = list(_spread(len(wb), 16))
    for l in last:  # the nearest spread knot moves onto the flight phase's last knot
        pick[int(np.argmin([abs(i - l) for i in pick]))] = l
    rest = list(_spread(len(wb), 48))
    for j in range(0, 48, 3):
        rest[j] = last[(j // 3) % len(last)]
    rows = [(b,) + wb[i] for b, i in zip(prob, pick + rest)]
    xu = [knot(*r) for r in rows]
    x, u = np.stack([a[0] for a in xu]), np.stack([a[1] for a in xu])

    # SRB knots; foothold and contact flags as FootholdPlanner and PlanarFloatingBase set them
    fb = [(p, k) for p in range(desc.n_wb, P) for k in range(N[p])]
    srows = [(b,) + fb[i] for b, i in zip(prob, list(_spread(len(fb), 16)) + list(_spread(len(fb), 48)))]
    xs, us, ps, ss = [], [], [], []
    for b, p, k in srows:
        xk, uk = knot(b, p, k)
        x0p, _ = knot(b, p, 0)
        f = np.zeros(4)
        stance = desc.dt_fb * N[p]
        if mode[p] == 1:
            f[2:] = np.cos(x0p[2]) * (-0.19) + x0p[0] + desc.vel_cmd * stance / 2, -0.404
        elif mode[p] == 3:
            f[:2] = np.cos(x0p[2]) * 0.19 + x0p[0] + desc.vel_cmd * stance / 2, -0.404
        xs.append(xk), us.append(uk), ps.append(f)
        ss.append([float(mode[p] == 3), float(mode[p] == 1)])
    out = eval_kat(x, u, np.stack(xs), np.stack(us), np.stack(ps), np.array(ss))
    out["mode"] = np.array([mode[p] for _, p, _ in rows], dtype=np.int32)
    out["pre_td"] = np.array([k == N[p] - 1 and mode[p] in (2, 4) for _, p, k in rows])
    out["problem"] = np.array([b for b, _, _ in rows], dtype=np.int32)
    out["srb.mode"] = np.array([mode[p] for _, p, _ in srows], dtype=np.int32)
    return out


SOLVES = {
    # name: (desc factory, batch)
    "c1": (configs.c1_desc, 2),
    "c2": (configs.c2_desc, 2),
    "c3": (configs.c3_desc, 8),
    "c5": (configs.c5_desc, 2),
}


def make_solve(name):
    fn, B = SOLVES[name]
    desc = fn()
    opt = L.HSDDP_OPTION()
    x0 = configs.x0_for(desc, B)
    res = O.solve(desc, opt.to_c(), x0, nthreads=4)
    res["x0"] = x0
    res["desc"] = np.array(str(desc.describe()))
    return res


def make_edge(name):
    """Solves that reach the rare branches (tests/_edge_cases.py): inputs + oracle outputs."""
    sys.path.insert(0, os.path.dirname(HERE))
    import _edge_cases as E
    desc, opt, x0 = E.inputs(name)
    res = O.solve(desc, opt.to_c(), x0, nthreads=4)
    # per-problem scalars and decision traces only (the trajectories of 64 problems would be
    # megabytes; the GPU tests compare those against the live oracle)
    keep = {k: res[k] for k in ("J", "dV_exp", "viol", "V", "dV", "status", "trace", "counters")}
    keep["x0"] = x0
    keep["desc"] = np.array(str(desc.describe()))
    return keep


def main():
    assert O.available(), "build the oracle and oracle/_ref first (make -C oracle)"
    sys.path.insert(0, os.path.dirname(HERE))
    import _edge_cases as E
    for name in E.CASES:
        np.savez_compressed(os.path.join(HERE, f"edge_{name}.npz"), **make_edge(name))
    np.savez_compressed(os.path.join(HERE, "kat_model.npz"), **make_kat())
    np.savez_compressed(os.path.join(HERE, "kat_model_traj.npz"), **make_kat_traj())
    for name in SOLVES:
        np.savez_compressed(os.path.join(HERE, f"solve_{name}.npz"), **make_solve(name))
    # smoke fixture: first 4 problems of C3 (same x0 stream as __graft_entry__.smoke)
    desc = configs.c3_desc()
    x0 = L.random_x0(4)
    res = O.solve(desc, L.HSDDP_OPTION().to_c(), x0, nthreads=4)
    res["x0"] = x0
    np.savez_compressed(os.path.join(HERE, "smoke_c3_b4.npz"), **res)
    print("golden fixtures written to", HERE)


if __name__ == "__main__":
    main()
