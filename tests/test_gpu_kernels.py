"""Kernel-level parity: the HIP model (through the C-ABI), in its fp64 and its fp32 build, vs
the reference's CasADi kernels (committed known-answer vectors: random states,
tests/golden/kat_model.npz, knots of a C5 solution, tests/golden/kat_model_traj.npz, and
states off the range of both, tests/golden/kat_model_wide.npz: the nominal posture, angles of
several turns, and link-angle sums of 1e3 to 3e5 whose bound is KAT_TOL plus four times the
reference's own spread under a one-ulp move of a position).

The wide fixture, fp64, first measured on MI355X (rel_err over all 64 rows; the worst row as
a fraction of its bound): xdot 1.3e-9 (0.09), Ac 1.4e-9 (0.14), xplus 2.0e-10 (0.20),
hx 3.3e-12 (0.17), J 4.2e-12 (0.17), Jd 2.5e-11 (0.17); fp32 (rows 0-47): beside the bounds
in _util.KAT_TOL_F32.

fp32 bounds: _util.KAT_TOL_F32 (4 x the host float build's error).  Device vs host float
build, norm_err, first measured on MI355X (random / trajectory fixture):
  quantity  device vs reference      device vs host float
  xdot      1.6e-05 / 2.4e-05        1.8e-05 / 3.8e-05
  y         8.4e-06 / 3.6e-07        6.2e-06 / 4.2e-07
  Ac        3.5e-05 / 5.1e-05        2.2e-05 / 6.4e-05
  Bc        1.8e-06 / 3.0e-07        1.8e-06 / 3.5e-07
  C         3.6e-05 / 2.9e-06        3.6e-05 / 5.8e-06
  D         1.2e-05 / 1.0e-06        5.0e-06 / 3.2e-06
  xplus     1.8e-05 / 2.5e-06        4.1e-05 / 1.6e-06
  Px        2.4e-05 / 9.5e-06        2.7e-05 / 7.9e-06
  h         1.5e-07 / 9.0e-08        1.2e-07 / 6.0e-08
  hx        5.2e-08 / 3.9e-08        6.0e-08 / 3.0e-08
  hxx       5.0e-08 / 7.1e-08        3.0e-08 / 3.0e-08
  J         5.2e-08 / 6.4e-08        6.0e-08 / 3.0e-08
  Jd        1.9e-07 / 3.3e-07        1.2e-07 / 1.2e-07
  srb.xdot  7.0e-07 / 1.1e-06        0 / 0
  srb.Ac    4.5e-07 / 1.2e-07        0 / 0
  srb.Bc    1.4e-07 / 2.9e-07        0 / 0
The two float builds differ by about as much as either differs from the fp64 reference
(independent roundings of the same size); the SRB model is the same bits on both.
"""
import numpy as np
import pytest

from _util import (DYN_NAME, IMP_NAME, JAC_NAME, KAT_FIXTURES, KAT_TOL, KAT_TOL_F32, KAT_WIDE,
                   TD_NAME, assert_abs_within, assert_rows_within, assert_structure, golden,
                   kat_for, kat_row_bounds, kat_rows, norm_err, rel_err)

pytestmark = pytest.mark.gpu

PAR_KEYS = (("Ac", (14, 14)), ("Bc", (14, 4)), ("C", (4, 14)), ("D", (4, 4)))


@pytest.fixture(scope="module")
def kat(need_gpu):
    return golden("kat_model.npz")


@pytest.fixture(scope="module")
def L():
    from mhpc_minimal_env_amd import capi
    return capi


def device_outputs(L, kat, precision):
    """Every eval hook of one build at every point of the fixture, keyed like
    test_model_host.host_outputs: dyn<mode>.xdot/.y, ift<mode>.Ac/Bc/C/D, imp<foot>.xplus/.Px,
    td<foot>.h/.hv/.hx/.hxx, jac<foot>.J/.Jd, srb.xdot/.Ac/.Bc."""
    lib, d = L.lib(), L.dptr
    f32 = precision == 32
    x, u = np.ascontiguousarray(kat["x"]), np.ascontiguousarray(kat["u"])
    n = len(x)
    o = {}
    for mode in (1, 2, 3, 4):
        xd, y = np.zeros((n, 14)), np.zeros((n, 4))
        if f32:
            L.check(lib.mhpc_eval_wb_dynamics_f32(0, n, mode, 0, d(x), d(u), d(xd), d(y)))
        else:
            L.check(lib.mhpc_eval_wb_dynamics(0, n, mode, d(x), d(u), d(xd), d(y)))
        o[f"dyn{mode}.xdot"], o[f"dyn{mode}.y"] = xd, y
        m = [np.zeros((n,) + s) for _, s in PAR_KEYS]
        fn = lib.mhpc_eval_wb_partials_f32 if f32 else lib.mhpc_eval_wb_partials
        L.check(fn(0, n, mode, d(x), d(u), *[d(a) for a in m]))
        for a, (k, _) in zip(m, PAR_KEYS):
            o[f"ift{mode}.{k}"] = a
    for foot in (0, 1):
        xp, Px = np.zeros((n, 14)), np.zeros((n, 14, 14))
        fn = lib.mhpc_eval_wb_impact_f32 if f32 else lib.mhpc_eval_wb_impact
        L.check(fn(0, n, foot, d(x), d(xp), d(Px)))
        h, hx, hxx = np.zeros((n, 2)), np.zeros((n, 14)), np.zeros((n, 14, 14))
        J, Jd = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
        fn = lib.mhpc_eval_wb_touchdown_f32 if f32 else lib.mhpc_eval_wb_touchdown
        L.check(fn(0, n, foot, d(x), d(h), d(hx), d(hxx), d(J), d(Jd)))
        o.update({f"imp{foot}.xplus": xp, f"imp{foot}.Px": Px, f"td{foot}.h": h[:, 0].copy(),
                  f"td{foot}.hv": h[:, 1].copy(), f"td{foot}.hx": hx, f"td{foot}.hxx": hxx,
                  f"jac{foot}.J": J, f"jac{foot}.Jd": Jd})
    ns = len(kat["srb.x"])
    xd, A, B = np.zeros((ns, 6)), np.zeros((ns, 6, 6)), np.zeros((ns, 6, 4))
    fn = lib.mhpc_eval_srb_f32 if f32 else lib.mhpc_eval_srb
    L.check(fn(0, ns, *[d(np.ascontiguousarray(kat[k])) for k in ("srb.x", "srb.u", "srb.p", "srb.s")],
               d(xd), d(A), d(B)))
    o.update({"srb.xdot": xd, "srb.Ac": A, "srb.Bc": B})
    return o


_cache = {}


def make_case(L, precision, name):
    """(precision, fixture name, fixture, the device's outputs, the host float build's)."""
    if (precision, name) not in _cache:
        kat = kat_for(name, precision)
        host = None
        if precision == 32:
            import test_model_host
            host = test_model_host.make_case(32, name)[3]
        _cache[precision, name] = (precision, name, kat, device_outputs(L, kat, precision), host)
    return _cache[precision, name]


@pytest.fixture(scope="module")
def base(need_gpu, L):
    """The fp64 build on the random fixture."""
    return make_case(L, 64, KAT_FIXTURES[0])


# the fp32 build on every fixture, the fp64 build on the trajectory and the wide fixture
@pytest.fixture(scope="module", params=[(32, KAT_FIXTURES[0]), (32, KAT_FIXTURES[1]),
                                        (64, KAT_FIXTURES[1]), (32, KAT_FIXTURES[2]),
                                        (64, KAT_FIXTURES[2])],
                ids=lambda pf: f"fp{pf[0]}-{pf[1][:-4]}")
def case(request, need_gpu, L):
    return make_case(L, *request.param)


def check(case, key, refkey, rows, kind, q):
    """Output key against reference output refkey.  fp64: the per-element bound KAT_TOL[kind]
    (or, a number, that bound) on every fixture, on the wide fixture's last rows plus four times
    the reference's own spread (kat_row_bounds); fp32: the bound KAT_TOL_F32 of quantity q,
    norm-relative, and the difference to the host float build printed."""
    precision, name, kat, o, host = case
    got, ref = np.asarray(o[key])[rows], np.asarray(kat[refkey])[rows]
    if got.ndim == 1:
        got, ref = got[:, None], ref[:, None]
    if precision == 64:
        tol = KAT_TOL[kind] if isinstance(kind, str) else kind
        worst = assert_rows_within(got, ref, kat_row_bounds(kat, refkey, tol, rows), key)
        print(f"fp64 {name[:-4]} {key}: error {rel_err(got, ref):.2e}, {worst:.2f} of the bound")
    else:
        e = norm_err(got, ref)
        dh = norm_err(got, np.asarray(host[key])[rows].reshape(got.shape))
        print(f"fp32 {name[:-4]} {key}: device vs reference {e:.2e} (bound "
              f"{KAT_TOL_F32[name][q]:.0e}), device vs host float {dh:.2e}")
        assert e <= KAT_TOL_F32[name][q], (key, e)


def check_dynamics(case, mode):
    kat = case[2]
    rows, name = kat_rows(kat, mode=mode), DYN_NAME[mode]
    assert len(rows) > 0
    check(case, f"dyn{mode}.xdot", name + ".xdot", rows, "value", "xdot")
    check(case, f"dyn{mode}.y", name + ".y", rows, "value", "y")


def check_partials(case, mode):
    kat, o = case[2], case[3]
    rows, name = kat_rows(kat, mode=mode), DYN_NAME[mode]
    assert len(rows) > 0
    for k, _ in PAR_KEYS:
        check(case, f"ift{mode}.{k}", f"{name}_par.{k}", rows, "jac", k)
        assert_structure(o[f"ift{mode}.{k}"][rows], f"{name}_par.{k}")


def check_impact(case, foot):
    kat, o = case[2], case[3]
    rows, name = kat_rows(kat, foot=foot), IMP_NAME[foot]
    assert len(rows) > 0
    check(case, f"imp{foot}.xplus", name + ".xplus", rows, "value", "xplus")
    check(case, f"imp{foot}.Px", name + "_par.Px", rows, "jac", "Px")
    assert_structure(o[f"imp{foot}.Px"][rows], name + "_par.Px")


def check_touchdown_and_foot_jacobian(case, foot):
    kat, o = case[2], case[3]
    rows, td, jac = kat_rows(kat), TD_NAME[foot], JAC_NAME[foot]
    # line search (value-only routine) and backward sweep (derivative routine) agree
    np.testing.assert_array_equal(o[f"td{foot}.h"], o[f"td{foot}.hv"])
    if case[0] == 64:
        assert_abs_within(o[f"td{foot}.h"], kat[td + ".h"], kat, td + ".h", 1e-14)
    else:
        check(case, f"td{foot}.h", td + ".h", rows, None, "h")
    check(case, f"td{foot}.hx", td + ".hx", rows, 1e-14, "hx")
    check(case, f"td{foot}.hxx", td + ".hxx", rows, 1e-14, "hxx")
    check(case, f"jac{foot}.J", jac + ".J", rows, 1e-14, "J")
    check(case, f"jac{foot}.Jd", jac + ".Jd", rows, 1e-13, "Jd")


def check_srb(case):
    kat, o = case[2], case[3]
    if case[0] == 64:
        # same operation order as FBDynamics.c / FBDynamics_par.c -> bitwise
        np.testing.assert_array_equal(o["srb.xdot"], kat["FBDynamics.xdot"])
        np.testing.assert_array_equal(o["srb.Ac"], kat["FBDynamics_par.Ac"])
        np.testing.assert_array_equal(o["srb.Bc"], kat["FBDynamics_par.Bc"])
    else:
        rows = np.arange(len(kat["srb.x"]))
        check(case, "srb.xdot", "FBDynamics.xdot", rows, None, "srb.xdot")
        check(case, "srb.Ac", "FBDynamics_par.Ac", rows, None, "srb.Ac")
        check(case, "srb.Bc", "FBDynamics_par.Bc", rows, None, "srb.Bc")
    assert_structure(o["srb.Ac"], "FBDynamics_par.Ac")
    assert_structure(o["srb.Bc"], "FBDynamics_par.Bc")


# ---- the fp64 build on the random fixture -------------------------------------------------
@pytest.mark.parametrize("mode,name", [(1, "Dyn_BS"), (2, "Dyn_FL"), (3, "Dyn_FS"), (4, "Dyn_FL")])
def test_wb_dynamics(base, mode, name):
    check_dynamics(base, mode)


@pytest.mark.parametrize("mode,name", [(1, "Dyn_BS"), (2, "Dyn_FL"), (3, "Dyn_FS"), (4, "Dyn_FL")])
def test_wb_partials(base, mode, name):
    check_partials(base, mode)


@pytest.mark.parametrize("foot,name", [(0, "Imp_F"), (1, "Imp_B")])
def test_wb_impact(base, foot, name):
    check_impact(base, foot)


def test_srb_bit_exact(base):
    check_srb(base)


@pytest.mark.parametrize("foot,td,jac", [(0, "WB_FL1_terminal_constr", "Jacob_F"),
                                         (1, "WB_FL2_terminal_constr", "Jacob_B")])
def test_touchdown_and_foot_jacobian(base, foot, td, jac):
    """Touchdown constraint (MHPCConstraints.cpp:91-107) and foot Jacobian
    (PlanarQuadruped.cpp:103-117) on the device vs the reference's CasADi kernels."""
    check_touchdown_and_foot_jacobian(base, foot)


# ---- the fp32 build, and the trajectory fixture -------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_wb_dynamics_cases(case, mode):
    check_dynamics(case, mode)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_wb_partials_cases(case, mode):
    check_partials(case, mode)


@pytest.mark.parametrize("foot", [0, 1])
def test_wb_impact_cases(case, foot):
    check_impact(case, foot)


@pytest.mark.parametrize("foot", [0, 1])
def test_touchdown_and_foot_jacobian_cases(case, foot):
    check_touchdown_and_foot_jacobian(case, foot)


def test_srb_cases(case):
    check_srb(case)


# ---- the line search's lane-pair dynamics -------------------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_wb_dynamics_pair_bitwise(kat, L, mode):
    pair_bitwise(kat, L, mode)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_wb_dynamics_pair_bitwise_wide(need_gpu, L, mode):
    """The same off the sampled range (kat_model_wide.npz): the pair's sin_cos_n<3> and the
    single lane's sin_cos_n<5> on angles of several turns and on link-angle sums on both sides
    of the 1e5 switch to the library path."""
    pair_bitwise(kat_for(KAT_WIDE, 64), L, mode)


def pair_bitwise(kat, L, mode):
    """The line search's lane-pair dynamics (mhpc_model_pair.h) reproduces the single-lane
    model bit for bit on both lanes of every pair (so forward_sweep(0) as a cost evaluation
    of the stored nominal stays exact whichever rollout variant produced it)."""
    x, u = np.ascontiguousarray(kat["x"]), np.ascontiguousarray(kat["u"])
    n = len(x)
    xd, y = np.zeros((n, 14)), np.zeros((n, 4))
    L.check(L.lib().mhpc_eval_wb_dynamics(0, n, mode, L.dptr(x), L.dptr(u), L.dptr(xd), L.dptr(y)))
    xd2, y2 = np.zeros((n, 2, 14)), np.zeros((n, 2, 4))
    L.check(L.lib().mhpc_eval_wb_dynamics_pair(0, n, mode, L.dptr(x), L.dptr(u), L.dptr(xd2),
                                               L.dptr(y2)))
    for lane in (0, 1):
        np.testing.assert_array_equal(xd2[:, lane], xd, err_msg=f"lane {lane} xdot")
        np.testing.assert_array_equal(y2[:, lane], y, err_msg=f"lane {lane} y")


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_wb_dynamics_pair_bitwise_fp32(kat, L, mode):
    pair_bitwise_fp32(kat, L, mode)


@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_wb_dynamics_pair_bitwise_fp32_wide(need_gpu, L, mode):
    """The same on the rows of kat_model_wide.npz that a float can hold."""
    pair_bitwise_fp32(kat_for(KAT_WIDE, 32), L, mode)


def pair_bitwise_fp32(kat, L, mode):
    """The same in the fp32 instantiation (C5 fp32 runs both line-search variants too)."""
    x, u = np.ascontiguousarray(kat["x"]), np.ascontiguousarray(kat["u"])
    n = len(x)
    xd, y = np.zeros((n, 14)), np.zeros((n, 4))
    L.check(L.lib().mhpc_eval_wb_dynamics_f32(0, n, mode, 0, L.dptr(x), L.dptr(u), L.dptr(xd),
                                              L.dptr(y)))
    xd2, y2 = np.zeros((n, 2, 14)), np.zeros((n, 2, 4))
    L.check(L.lib().mhpc_eval_wb_dynamics_f32(0, n, mode, 1, L.dptr(x), L.dptr(u), L.dptr(xd2),
                                              L.dptr(y2)))
    assert np.isfinite(xd).all()
    for lane in (0, 1):
        np.testing.assert_array_equal(xd2[:, lane], xd, err_msg=f"lane {lane} xdot")
        np.testing.assert_array_equal(y2[:, lane], y, err_msg=f"lane {lane} y")
