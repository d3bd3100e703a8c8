"""Is the device's derivative chain (k_partials, k_partials_impact, the cost-derivative records,
k_bws_srb / k_bws) the derivative of what its value chain (k_cost, k_rollout, k_eps_rollout,
k_policy_rollout) computes?  The two identities of tests/_gradient_identities.py

  I1  dJ/deps at eps = 0 = dV_exp                  I2  d J_closed-loop / d x0 = Vx[phase 0][knot 0]

through MHPCLocomotion alone: solve_mhpc, get_scalars()["dV_exp"], Vx, rollout_costs,
rollout_policy.  No oracle on the device side: a term misread the same way in the oracle and in
the kernels, or a derivative kernel that reads a neighbour's parameters where the value kernel
reads the problem's own, fails here and nowhere else.

The oracle only sets the yardstick: tests/test_oracle_gradients.py measures how well the
reference's algorithm itself satisfies each form on the same problems (TABLE there); the device
is held to 10 x that measured residual, and to no less than the rounding term of the step-size
model.  The factor covers the device's other rounding of J (another model arithmetic at 1e-11,
summed over up to 1e3 knots, divided by h) and leaves three decades below the smallest real
first-order inconsistency seen (the negative control, 1e-3 at the reference's sigma).

Residuals, worst problem, oracle (CPU) | device (MI355X, first measured):
  workload  i1_plain          i1_reb            i1_al_ls          i2_plain          i2_reb
  c3        1.4e-9 | 9.8e-10  2.2e-9 | 2.1e-9   2.9e-8 | 3.9e-10  3.6e-8 | 1.2e-9   1.1e-7 | 8.0e-9
  c5        1.2e-9 | 1.2e-9   1.2e-9 | 1.2e-9   3.1e-9 | 1.3e-9   7.9e-8 | 9.1e-8   1.3e-7 | 1.2e-7
  short_a   1.1e-9 | 1.1e-9   1.3e-9 | 1.1e-9                     1.1e-7 | 4.2e-8   1.0e-7 | 4.3e-8
  short_b   1.2e-9 | 1.0e-9   1.2e-9 | 1.0e-9                     1.9e-7 | 1.0e-8   1.3e-7 | 1.1e-8
  long      1.4e-9 | 1.4e-9   1.9e-9 | 1.9e-9                     1.3e-8 | 2.0e-9   1.9e-8 | 3.6e-9
  mixed                       2.1e-9 | 2.1e-9                                       1.3e-7 | 6.1e-8
  tick 2    1.2e-8 | 1.2e-8                                       2.3e-6 | 2.1e-7
  negative control (AL on, rollout_costs after the solve, sigma = 150), smallest problem:
  c3 3.4e-2 | 3.4e-2, c5 1.4e-2 | 1.4e-2
The I1 residuals by rollout_costs are the same ~1e-9 on both sides and on every problem, whatever
the arithmetic.  Where the oracle's residual is the larger one (the line-search form, I2) it is
the term that grows as 1 / h in the oracle's step-size scans; the device shows less of it.

fp32 handles are out of scope: with float states the rounding term is ~1e-7 |J| / h, so no step
size resolves the derivative better than about 1e-2 of dV, which is the level
tests/test_gpu_fp32.py already bounds.  Do not add them here with a loose bound.
"""
import numpy as np
import pytest

import _gradient_identities as GI
import test_oracle_gradients as Y
from _util import SOLVE_TOL

pytestmark = pytest.mark.gpu


def device_backend(desc, x0, constraints=None):
    from mhpc_minimal_env_amd import locomotion as L

    def prepare(opt):
        loco = L.MHPCLocomotion(desc=desc, option=opt, batch=x0.shape[0], device=0)
        if constraints is not None:
            loco.set_constraint_params(constraints)
        loco.set_initial_condition(x0)
        loco.initialization()
        return loco
    return GI.DeviceBackend(prepare)


def device_bound(r, oracle_residual):
    """Per problem: 10 x the oracle's residual of the case, floored by the rounding term."""
    return np.maximum(10.0 * oracle_residual, r["floor"])


def check(what, r, oracle_residual):
    bnd = device_bound(r, oracle_residual)
    print(f"{what}: device worst {r['err'].max():.2e} (oracle {oracle_residual:.2e}, bound "
          f"{bnd.max():.1e}) per problem", " ".join(f"{e:.1e}" for e in r["err"]),
          f"| |J| {np.abs(r['J']).min():.3g}..{np.abs(r['J']).max():.3g}"
          + (f" |dV| {np.abs(r['dV']).min():.3g}..{np.abs(r['dV']).max():.3g}" if "dV" in r else ""))
    assert (r["err"] <= bnd).all(), (what, r["err"], bnd)


FORMS = ["i1_plain", "i1_reb", "i2_plain", "i2_reb"]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", Y.WORKLOADS)
def test_identity(need_gpu, name, form):
    """The oracle's cases, and (a) the phase extremes: the descriptor's shortest phases and
    phases past the line search's 128-knot stage."""
    desc, x0 = Y.workload(name)
    be = device_backend(desc, x0)
    try:
        r = Y.measure(be, form, reb_on=name in Y.REB_ON)
    finally:
        be.close()
    check(f"{name} {form}", r, Y.measured(name, form))


@pytest.mark.parametrize("name", ["c3", "c5"])
def test_al_through_the_line_search(need_gpu, name):
    desc, x0 = Y.workload(name)
    be = device_backend(desc, x0, Y.al_constraints())
    try:
        s = Y.share(be, "al")
        print(name, "AL share of dV at sigma", Y.AL_SIGMA, s)
        assert (s >= 0.01).all(), s
        r = Y.measure(be, "i1_al_ls")
        print("   one-sided", r["err_one_sided"].max())
        check(f"{name} i1_al_ls", r, Y.measured(name, "i1_al_ls"))
        # (d) the negative control, as on the oracle
        n = Y.measure(be, "neg")
    finally:
        be.close()
    print(name, "negative control", n["err"])
    assert (n["err"] >= 1e3 * 10.0 * Y.measured(name, "i1_al_ls")).all(), n["err"]


@pytest.mark.parametrize("name", ["c3", "c5", "long"])
def test_evaluators_agree(need_gpu, name):
    """(e) sample 0 of rollout_policy, rollout_costs(eps = 0) and the solve's J are one cost."""
    desc, x0 = Y.workload(name)
    be = device_backend(desc, x0)
    try:
        for case in ("plain", "reb"):
            e = GI.evaluators_agree(be, GI.option(case))
            print(name, case, "evaluators differ by", e.max())
            assert (e <= SOLVE_TOL).all(), e
    finally:
        be.close()


def test_reb_share(need_gpu):
    for name in Y.REB_ON:
        desc, x0 = Y.workload(name)
        be = device_backend(desc, x0)
        try:
            s = Y.share(be, "reb")
        finally:
            be.close()
        print(name, "ReB share of dV", s)
        assert (s >= 0.01).all(), (name, s)


@pytest.mark.parametrize("form", ["i1_reb", "i2_reb"])
def test_mixed_handle(need_gpu, form):
    """(b) ten unlike problems in one handle: five layouts, three parameter sets that differ in
    the whole-body Q / R / S / Qf scales, mu and tq_lim, a speed and height command each.  Every
    problem satisfies the identity by its own dV_exp / Vx; the barrier is on for the C3 problems,
    which meet all three sets."""
    from mhpc_minimal_env_amd import locomotion as L
    descs, lop, sop, vel, hgt, x0 = GI.mixed_problems()
    ss = GI.mixed_sets()

    def prepare(opt):
        loco = L.MHPCLocomotion(desc=descs[0], option=opt, batch=len(lop), device=0)
        loco.set_commands(vel, hgt)
        loco.set_param_sets([s[0] for s in ss], [s[1] for s in ss], sop)
        loco.set_layouts(descs, lop)
        loco.set_initial_condition(x0)
        loco.initialization()
        assert loco.num_layouts() == 5 and loco.num_param_sets() == 3
        return loco

    be = GI.DeviceBackend(prepare)
    try:
        opt = GI.option("reb")
        r = GI.i1_rollout(be, opt) if form == "i1_reb" else GI.i2_policy(be, opt)
    finally:
        be.close()
    reb = GI.assert_all_rejected(r["solve"]["trace"], opt, "mixed")
    assert (reb[list(Y.MIXED_REB_ON)] == 1).all(), reb
    check(f"mixed {form}", r, Y.measured("mixed", form))


@pytest.mark.parametrize("form", ["i1_plain", "i2_plain"])
def test_second_tick(need_gpu, form):
    """(c) the second tick of a receding-horizon loop: a full solve, update_problem (rotated phase
    buffers, warm start), then the all-rejected options through set_options.  The rotated
    buffers make it the least linear problem here (J of 4e5 to 9e5); the oracle's receding-horizon
    loop shows the same I1 residual problem by problem."""
    from mhpc_minimal_env_amd import locomotion as L
    desc, gait, x0 = Y.tick2_inputs()

    def prepare(opt):
        loco = L.MHPCLocomotion(desc=desc, gait=gait, option=L.HSDDP_OPTION(), batch=Y.B, device=0)
        loco.set_initial_condition(x0)
        loco.initialization()
        assert (loco.solve_mhpc() == 0).all()
        x1 = loco.get_phase(0)["x"][:, -1, :]  # where the first phase of the own plan ends
        loco.set_initial_condition(x1)
        loco.update_problem()
        assert list(loco.desc.mode_seq)[:4] == [2, 3, 4, 1]
        loco.set_options(opt)
        return loco

    be = GI.DeviceBackend(prepare)
    try:
        r = Y.measure(be, form)
        if form == "i1_plain":
            e = GI.evaluators_agree(be, GI.option("plain"))
            assert (e <= SOLVE_TOL).all(), e
    finally:
        be.close()
    check(f"tick 2 {form}", r, Y.measured("tick2", form))
