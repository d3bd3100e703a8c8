"""The hand-written device model (mhpc_model.h) compiled for the host, in double and in
float (the fp32 instantiation's arithmetic), vs the reference's CasADi kernels (committed
known-answer vectors: random states and knots of a C5 solution) -- the CPU-side check of the
physics."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _util import (DYN_NAME, IMP_NAME, JAC_NAME, KAT_FIXTURES, KAT_TOL, KAT_TOL_F32, TD_NAME,
                   assert_abs_within, assert_rows_within, assert_structure, kat_for, kat_row_bounds, kat_rows,
                   norm_err, rel_err)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "model_hostcheck.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")
PAR_KEYS = (("Ac", (14, 14)), ("Bc", (14, 4)), ("C", (4, 14)), ("D", (4, 4)))


def build_hostcheck(precision):
    """libmodel_hostcheck.so (double) / libmodel_hostcheck_f32.so (-DMHPC_FP32, without
    contraction like the device's whole-body model)."""
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libmodel_hostcheck.so" if precision == 64 else "libmodel_hostcheck_f32.so")
    extra = [] if precision == 64 else ["-DMHPC_FP32", "-ffp-contract=off"]
    subprocess.run(["g++", "-O2", "-std=c++17", *extra, "-fPIC", "-shared", "-o", so, SRC], check=True)
    lib = ctypes.CDLL(so)
    lib.hc_wb_touchdown_value.restype = ctypes.c_double
    return lib


def P(a):
    return np.ascontiguousarray(a).ctypes.data_as(ctypes.POINTER(ctypes.c_double))


def host_outputs(hc, kat):
    """Every model function at every point of the fixture, dense row-major like the
    fixture's reference outputs: dyn<mode>.xdot/.y, par<mode>.* (dual numbers through the
    forward dynamics) and ift<mode>.* (implicit differentiation, the partials kernel's method),
    imp<foot>.xplus/.lam/.Px, td<foot>.h/.hv/.hx/.hxx, jac<foot>.J/.Jd, srb.xdot/.Ac/.Bc."""
    x, u = kat["x"], kat["u"]
    n = len(x)
    o = {}
    for mode in (1, 2, 3, 4):
        xd, y = np.zeros((n, 14)), np.zeros((n, 4))
        par = {k: np.zeros((n,) + s) for k, s in PAR_KEYS}
        ift = {k: np.zeros((n,) + s) for k, s in PAR_KEYS}
        for i in range(n):
            hc.hc_wb_dynamics(P(x[i]), P(u[i]), mode, P(xd[i]), P(y[i]))
            for fn, dst in ((hc.hc_wb_partials, par), (hc.hc_wb_partials_ift, ift)):
                m = [np.zeros(s[0] * s[1]) for _, s in PAR_KEYS]
                fn(P(x[i]), P(u[i]), mode, *[P(a) for a in m])
                for a, (k, s) in zip(m, PAR_KEYS):
                    dst[k][i] = a.reshape(s, order="F")
        o[f"dyn{mode}.xdot"], o[f"dyn{mode}.y"] = xd, y
        for k, _ in PAR_KEYS:
            o[f"par{mode}.{k}"], o[f"ift{mode}.{k}"] = par[k], ift[k]
    for foot in (0, 1):
        xp, lam, Px = np.zeros((n, 14)), np.zeros((n, 2)), np.zeros((n, 14, 14))
        h, hv, hx, hxx = np.zeros((n, 1)), np.zeros(n), np.zeros((n, 14)), np.zeros((n, 14, 14))
        J, Jd = np.zeros((n, 2, 7)), np.zeros((n, 2, 7))
        for i in range(n):
            hc.hc_wb_impact(P(x[i]), foot, P(xp[i]), P(lam[i]))
            px = np.zeros(196)
            hc.hc_wb_impact_par(P(x[i]), foot, P(px))
            Px[i] = px.reshape(14, 14, order="F")
            hc.hc_wb_touchdown(P(x[i]), foot, P(h[i]), P(hx[i]), P(hxx[i]))
            hv[i] = hc.hc_wb_touchdown_value(P(x[i]), foot)
            hc.hc_wb_foot_jacobian(P(x[i]), foot, P(J[i]), P(Jd[i]))
        o.update({f"imp{foot}.xplus": xp, f"imp{foot}.lam": lam, f"imp{foot}.Px": Px,
                  f"td{foot}.h": h[:, 0], f"td{foot}.hv": hv, f"td{foot}.hx": hx,
                  f"td{foot}.hxx": hxx, f"jac{foot}.J": J, f"jac{foot}.Jd": Jd})
    ns = len(kat["srb.x"])
    xd, A, B = np.zeros((ns, 6)), np.zeros((ns, 6, 6)), np.zeros((ns, 6, 4))
    for i in range(ns):
        args = [P(kat[k][i]) for k in ("srb.x", "srb.u", "srb.p", "srb.s")]
        hc.hc_srb_dynamics(*args, P(xd[i]))
        hc.hc_srb_jacobians(*args, P(A[i]), P(B[i]))
    o.update({"srb.xdot": xd, "srb.Ac": A, "srb.Bc": B})
    return o


_cache = {}


def make_case(precision, name):
    """(precision, fixture name, fixture, the host build's outputs on it), computed once."""
    if precision not in _cache:
        _cache[precision] = build_hostcheck(precision)
    if (precision, name) not in _cache:
        kat = kat_for(name, precision)
        _cache[precision, name] = (precision, name, kat, host_outputs(_cache[precision], kat))
    return _cache[precision, name]


@pytest.fixture(scope="module")
def base():
    """The double build on the random fixture."""
    return make_case(64, KAT_FIXTURES[0])


# the float build on every fixture, the double build on the trajectory and the wide fixture
@pytest.fixture(scope="module", params=[(32, KAT_FIXTURES[0]), (32, KAT_FIXTURES[1]),
                                        (64, KAT_FIXTURES[1]), (32, KAT_FIXTURES[2]),
                                        (64, KAT_FIXTURES[2])],
                ids=lambda pf: f"fp{pf[0]}-{pf[1][:-4]}")
def case(request):
    return make_case(*request.param)


def check(case, got, key, rows, kind, q, part=4, cols=slice(None)):
    """Against reference output `key` (its columns cols).  fp64: the per-element bound
    KAT_TOL[kind] (kind a number: that bound) on every fixture, on the wide fixture's last rows
    plus four times the reference's own spread (kat_row_bounds); fp32: a quarter of the device
    bound KAT_TOL_F32 of quantity q, norm-relative."""
    precision, name, kat, _ = case
    got, ref = np.asarray(got)[rows], np.asarray(kat[key])[rows]
    if got.ndim == 1:
        got, ref = got[:, None], ref[:, None]
    ref = ref[:, cols]
    if precision == 64:
        tol = KAT_TOL[kind] if isinstance(kind, str) else kind
        worst = assert_rows_within(got, ref, kat_row_bounds(kat, key, tol, rows), key)
        print(f"fp64 {name[:-4]} {key}: {worst:.2f} of the bound, error {rel_err(got, ref):.2e}")
    else:
        assert norm_err(got, ref) <= KAT_TOL_F32[name][q] / part, (q, norm_err(got, ref))


def check_dynamics_and_jacobians(case, mode):
    """Values, and the Jacobians by both of the model's derivative paths: forward-mode dual
    numbers through the whole forward dynamics, and implicit differentiation of the KKT
    system at the knot's solution (wb_partial_column, what the partials kernel computes)."""
    precision, _, kat, o = case
    rows, name = kat_rows(kat, mode=mode), DYN_NAME[mode]
    assert len(rows) > 0
    check(case, o[f"dyn{mode}.xdot"], name + ".xdot", rows, "value", "xdot")
    check(case, o[f"dyn{mode}.y"], name + ".y", rows, "value", "y")
    for k, _ in PAR_KEYS:
        # fp32: the table is derived from the kernel's method (ift); dual numbers through the
        # forward dynamics round differently (Ac up to 1.7x its error) and get the whole bound
        for path, part in (("ift", 4), ("par", 1)):
            check(case, o[f"{path}{mode}.{k}"], f"{name}_par.{k}", rows, "jac", k, part)
            assert_structure(o[f"{path}{mode}.{k}"][rows], f"{name}_par.{k}")
    if precision == 64:  # the two paths are the same derivative
        worst = max(rel_err(o[f"par{mode}.{k}"][rows], o[f"ift{mode}.{k}"][rows]) for k, _ in PAR_KEYS)
        assert worst < 1e-10, worst


def check_impact(case, foot):
    _, _, kat, o = case
    rows, name = kat_rows(kat, foot=foot), IMP_NAME[foot]
    assert len(rows) > 0
    check(case, o[f"imp{foot}.xplus"], name + ".xplus", rows, "value", "xplus")
    check(case, o[f"imp{foot}.lam"], name + ".y", rows, "value", "lam",
          cols=slice(2 * foot, 2 * foot + 2))
    check(case, o[f"imp{foot}.Px"], name + "_par.Px", rows, "jac", "Px")
    assert_structure(o[f"imp{foot}.Px"][rows], name + "_par.Px")


def check_touchdown_constraint(case, foot):
    precision, name, kat, o = case
    td = TD_NAME[foot]
    # h from the derivative routine (backward sweep) and from the value-only one (line search):
    # the same bits
    np.testing.assert_array_equal(o[f"td{foot}.h"], o[f"td{foot}.hv"])
    if precision == 64:
        rows = np.arange(len(kat["x"]))
        assert_abs_within(o[f"td{foot}.h"], kat[td + ".h"], kat, td + ".h", 1e-14)
        assert_abs_within(o[f"td{foot}.hv"], kat[td + ".h"], kat, td + ".h", 1e-14)
        check(case, o[f"td{foot}.hx"], td + ".hx", rows, 1e-14, "hx")
        check(case, o[f"td{foot}.hxx"], td + ".hxx", rows, 1e-14, "hxx")
    else:
        tol = KAT_TOL_F32[name]
        assert norm_err(o[f"td{foot}.h"][:, None], kat[td + ".h"][:, None]) <= tol["h"] / 4
        assert norm_err(o[f"td{foot}.hv"][:, None], kat[td + ".h"][:, None]) <= tol["h"] / 4
        assert norm_err(o[f"td{foot}.hx"], kat[td + ".hx"]) <= tol["hx"] / 4
        assert norm_err(o[f"td{foot}.hxx"], kat[td + ".hxx"]) <= tol["hxx"] / 4


def check_foot_jacobian(case, foot):
    precision, name, kat, o = case
    jac = JAC_NAME[foot]
    if precision == 64:
        rows = np.arange(len(kat["x"]))
        check(case, o[f"jac{foot}.J"], jac + ".J", rows, 1e-14, "J")
        check(case, o[f"jac{foot}.Jd"], jac + ".Jd", rows, 1e-13, "Jd")
    else:
        tol = KAT_TOL_F32[name]
        assert norm_err(o[f"jac{foot}.J"], kat[jac + ".J"]) <= tol["J"] / 4
        assert norm_err(o[f"jac{foot}.Jd"], kat[jac + ".Jd"]) <= tol["Jd"] / 4


def check_srb(case):
    """fp64: the reference's operation order, bit for bit."""
    precision, name, kat, o = case
    if precision == 64:
        np.testing.assert_array_equal(o["srb.xdot"], kat["FBDynamics.xdot"])
        np.testing.assert_array_equal(o["srb.Ac"], kat["FBDynamics_par.Ac"])
        np.testing.assert_array_equal(o["srb.Bc"], kat["FBDynamics_par.Bc"])
    else:
        tol = KAT_TOL_F32[name]
        assert norm_err(o["srb.xdot"], kat["FBDynamics.xdot"]) <= tol["srb.xdot"] / 4
        assert norm_err(o["srb.Ac"], kat["FBDynamics_par.Ac"]) <= tol["srb.Ac"] / 4
        assert norm_err(o["srb.Bc"], kat["FBDynamics_par.Bc"]) <= tol["srb.Bc"] / 4
    assert_structure(o["srb.Ac"], "FBDynamics_par.Ac")
    assert_structure(o["srb.Bc"], "FBDynamics_par.Bc")


# ---- the double build on the random fixture ----------------------------------------------
@pytest.mark.parametrize("mode,name", [(1, "Dyn_BS"), (2, "Dyn_FL"), (3, "Dyn_FS")])
def test_dynamics_and_jacobians(base, mode, name):
    assert DYN_NAME[mode] == name
    check_dynamics_and_jacobians(base, mode)


@pytest.mark.parametrize("mode,name", [(1, "Dyn_BS"), (2, "Dyn_FL"), (3, "Dyn_FS"), (4, "Dyn_FL")])
def test_jacobians_by_implicit_differentiation(base, mode, name):
    """The partials kernel's method (implicit differentiation of the KKT system at the
    knot's solution, wb_partial_column) vs the reference's CasADi Jacobians and vs
    forward-mode dual numbers through the whole forward dynamics (the same derivative)."""
    assert DYN_NAME[mode] == name
    check_dynamics_and_jacobians(base, mode)


@pytest.mark.parametrize("foot,name", [(0, "Imp_F"), (1, "Imp_B")])
def test_impact(base, foot, name):
    check_impact(base, foot)


@pytest.mark.parametrize("foot,name", [(0, "WB_FL1_terminal_constr"), (1, "WB_FL2_terminal_constr")])
def test_touchdown_constraint(base, foot, name):
    check_touchdown_constraint(base, foot)


@pytest.mark.parametrize("foot,name", [(0, "Jacob_F"), (1, "Jacob_B")])
def test_foot_jacobian(base, foot, name):
    check_foot_jacobian(base, foot)


def test_srb_bit_exact(base):
    check_srb(base)


# ---- the float build, and the trajectory fixture -----------------------------------------
@pytest.mark.parametrize("mode", [1, 2, 3, 4])
def test_dynamics_and_jacobians_cases(case, mode):
    check_dynamics_and_jacobians(case, mode)


@pytest.mark.parametrize("foot", [0, 1])
def test_impact_cases(case, foot):
    check_impact(case, foot)


@pytest.mark.parametrize("foot", [0, 1])
def test_touchdown_and_foot_jacobian_cases(case, foot):
    check_touchdown_constraint(case, foot)
    check_foot_jacobian(case, foot)


def test_srb_cases(case):
    check_srb(case)
