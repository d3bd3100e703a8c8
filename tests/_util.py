"""Shared helpers of the test-suite."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# fp64 tolerance of the HIP solve vs the oracle: |d| <= TOL * max(1, |ref|)
# with an identical decision trace.  The model arithmetic differs from CasADi's QR at
# ~1e-11 relative (tests/test_model_host.py), which the solve amplifies to <~1e-8.
SOLVE_TOL = 1e-6
# per-function tolerance of the hand-written model vs the CasADi kernels.  Measured worst
# cases over the 64 KAT states (host build, tests/test_model_host.py): values 1.5e-10
# (Dyn_FL, Imp_B), Jacobians 1.4e-9 (Dyn_FL_par); CasADi's QR leaves ~1e-10 noise itself.
KAT_TOL = {"value": 1e-9, "jac": 5e-9}
# The same bounds hold on the trajectory fixture (host build: values 7.0e-11, Jacobians
# 8.5e-10, the model's two derivative paths within 3.5e-11 of each other).

# The fp32 instantiation (real = float) vs the same fp64 reference vectors, per fixture and
# quantity, as norm_err.  Each entry is 4 x the worst case of the HOST float build
# (tests/native/model_hostcheck.cpp with -DMHPC_FP32, no contraction; the Jacobians by the
# partials kernel's method, wb_partial_column) rounded up to one digit; the measured host value
# stands beside it.  tests/test_model_host.py holds the host build to a quarter of each entry,
# so the table cannot drift from what it was derived from; tests/test_gpu_kernels.py holds
# the device to the entry.  The factor 4 covers what differs between the two builds: the
# device's sincosf, division and reciprocal rounding, and the contraction the fp32 partials
# and impact are compiled with (the whole-body dynamics is built without in both).
# Beside each entry: the host float build's error, then the device's error and the device's
# difference to the host float build as first measured on MI355X ("lam" has no device hook).
KAT_TOL_F32 = {
    "kat_model.npz": {
        "xdot": 5e-5,      # host 1.04e-5; device 1.6e-5, device vs host 1.8e-5
        "y": 4e-5,         # host 8.36e-6; device 8.4e-6, device vs host 6.2e-6
        "Ac": 2e-4,        # host 3.48e-5; device 3.5e-5, device vs host 2.2e-5
        "Bc": 8e-6,        # host 1.79e-6; device 1.8e-6, device vs host 1.8e-6
        "C": 2e-4,         # host 2.51e-5; device 3.6e-5, device vs host 3.6e-5
        "D": 5e-5,         # host 1.19e-5; device 1.2e-5, device vs host 5.0e-6
        "xplus": 2e-4,     # host 2.62e-5; device 1.8e-5, device vs host 4.1e-5
        "lam": 4e-5,       # host 8.65e-6
        "Px": 1e-4,        # host 2.26e-5; device 2.4e-5, device vs host 2.7e-5
        "h": 7e-7,         # host 1.50e-7; device 1.5e-7, device vs host 1.2e-7
        "hx": 3e-7,        # host 5.32e-8; device 5.2e-8, device vs host 6.0e-8
        "hxx": 2e-7,       # host 4.97e-8; device 5.0e-8, device vs host 3.0e-8
        "J": 3e-7,         # host 5.16e-8; device 5.2e-8, device vs host 6.0e-8
        "Jd": 7e-7,        # host 1.66e-7; device 1.9e-7, device vs host 1.2e-7
        "srb.xdot": 3e-6,  # host 7.00e-7; device 7.0e-7, device vs host 0
        "srb.Ac": 2e-6,    # host 4.51e-7; device 4.5e-7, device vs host 0
        "srb.Bc": 6e-7,    # host 1.40e-7; device 1.4e-7, device vs host 0
    },
    "kat_model_traj.npz": {
        "xdot": 1e-4,      # host 2.40e-5; device 2.4e-5, device vs host 3.8e-5
        "y": 2e-6,         # host 4.66e-7; device 3.6e-7, device vs host 4.2e-7
        "Ac": 2e-4,        # host 4.66e-5; device 5.1e-5, device vs host 6.4e-5
        "Bc": 1e-6,        # host 2.43e-7; device 3.0e-7, device vs host 3.5e-7
        "C": 2e-5,         # host 3.12e-6; device 2.9e-6, device vs host 5.8e-6
        "D": 9e-6,         # host 2.22e-6; device 1.0e-6, device vs host 3.2e-6
        "xplus": 2e-5,     # host 4.10e-6; device 2.5e-6, device vs host 1.6e-6
        "lam": 3e-6,       # host 7.25e-7
        "Px": 2e-5,        # host 3.21e-6; device 9.5e-6, device vs host 7.9e-6
        "h": 4e-7,         # host 9.05e-8; device 9.0e-8, device vs host 6.0e-8
        "hx": 2e-7,        # host 3.92e-8; device 3.9e-8, device vs host 3.0e-8
        "hxx": 3e-7,       # host 7.12e-8; device 7.1e-8, device vs host 3.0e-8
        "J": 3e-7,         # host 6.39e-8; device 6.4e-8, device vs host 3.0e-8
        "Jd": 2e-6,        # host 3.29e-7; device 3.3e-7, device vs host 1.2e-7
        "srb.xdot": 5e-6,  # host 1.12e-6; device 1.1e-6, device vs host 0
        "srb.Ac": 5e-7,    # host 1.17e-7; device 1.2e-7, device vs host 0
        "srb.Bc": 2e-6,    # host 2.92e-7; device 2.9e-7, device vs host 0
    },
    # Rows 0-47 only: a float cannot hold the angles of rows 48-63 (link-angle sums of 1e3 to
    # 3e5, where a float ulp is 6e-5 to 0.03 rad), so the fp32 builds are not run on them.  On
    # rows 32-47 (angles up to 60, float ulp 4e-6 rad) the rounding of the inputs alone is what
    # the entries of h, hx, hxx, J and Jd measure.
    "kat_model_wide.npz": {
        "xdot": 3e-5,      # host 5.15e-6; device 1.4e-6, device vs host 4.5e-7
        "y": 2e-4,         # host 2.76e-5; device 2.7e-5, device vs host 1.0e-6
        "Ac": 9e-5,        # host 2.13e-5; device 2.2e-5, device vs host 2.4e-5
        "Bc": 2e-5,        # host 3.36e-6; device 3.5e-6, device vs host 4.7e-7
        "C": 2e-4,         # host 4.66e-5; device 5.2e-5, device vs host 1.2e-5
        "D": 8e-5,         # host 1.94e-5; device 1.9e-5, device vs host 1.4e-6
        "xplus": 5e-5,     # host 1.17e-5; device 1.2e-5, device vs host 1.5e-6
        "lam": 6e-5,       # host 1.29e-5
        "Px": 9e-5,        # host 2.05e-5; device 2.3e-5, device vs host 1.2e-5
        "h": 4e-6,         # host 7.84e-7; device 7.7e-7, device vs host 1.1e-7
        "hx": 6e-6,        # host 1.28e-6; device 1.3e-6, device vs host 3.0e-8
        "hxx": 6e-6,       # host 1.33e-6; device 1.3e-6, device vs host 3.0e-8
        "J": 6e-6,         # host 1.33e-6; device 1.3e-6, device vs host 3.0e-8
        "Jd": 2e-5,        # host 3.84e-6; device 3.9e-6, device vs host 1.3e-7
        "srb.xdot": 3e-6,  # host 7.00e-7; device 7.0e-7, device vs host 0 (the SRB points of kat_model.npz)
        "srb.Ac": 2e-6,    # host 4.51e-7; device 4.5e-7, device vs host 0
        "srb.Bc": 6e-7,    # host 1.40e-7; device 1.4e-7, device vs host 0
    },
}


# The known-answer fixtures (tests/golden/make_golden.py): uniform-random states, knots of
# the oracle's C5 solution (each tagged with its phase's mode), and states off the range of
# both (the nominal posture, angles of several turns, link-angle sums up to 3e5).
KAT_FIXTURES = ("kat_model.npz", "kat_model_traj.npz", "kat_model_wide.npz")
KAT_WIDE = KAT_FIXTURES[2]
KAT_WIDE_COND = 48    # its rows from here on are bounded by the reference's own conditioning
KAT_COND_SKIP = 1e-6  # a row whose bound exceeds this says nothing (at most 4 rows may)
DYN_NAME = {1: "Dyn_BS", 2: "Dyn_FL", 3: "Dyn_FS", 4: "Dyn_FL"}  # mode 4 is flight too
IMP_NAME = {0: "Imp_F", 1: "Imp_B"}
TD_NAME = {0: "WB_FL1_terminal_constr", 1: "WB_FL2_terminal_constr"}
JAC_NAME = {0: "Jacob_F", 1: "Jacob_B"}


def golden(name):
    return dict(np.load(os.path.join(GOLDEN, name), allow_pickle=False))


def kat_for(name, precision):
    """Fixture `name` as a build of `precision` is checked on it: the fp32 build skips the
    wide fixture's rows from KAT_WIDE_COND on (a float cannot hold those angles: at 1e5 its
    ulp is 0.008 rad)."""
    kat = golden(name)
    if name == KAT_WIDE and precision == 32:
        n = len(kat["x"])
        kat = {k: (v[:KAT_WIDE_COND] if v.ndim and len(v) == n and not k.startswith(("srb.", "FBDynamics"))
                   else v) for k, v in kat.items() if not k.startswith("spread.")}
    return kat


def kat_row_bounds(kat, key, tol, rows):
    """Bound of each of `rows` for reference output `key`: tol, and on the rows the wide
    fixture stores a conditioning spread for (make_kat_wide: how far the reference's own output
    moves when a position moves by an ulp) tol + 4 x that spread."""
    rows = np.asarray(rows)
    b = np.full(len(rows), float(tol))
    if "spread." + key in kat:
        c = rows >= KAT_WIDE_COND
        b[c] += 4.0 * kat["spread." + key][rows[c] - KAT_WIDE_COND]
    return b


def assert_rows_within(got, ref, bounds, what):
    """rel_err of each row (a point's whole output) below its bound; rows whose bound exceeds
    KAT_COND_SKIP are not checked, and at most 4 may be such."""
    got = np.asarray(got, dtype=float).reshape(len(bounds), -1)
    ref = np.asarray(ref, dtype=float).reshape(len(bounds), -1)
    use = bounds <= KAT_COND_SKIP
    assert (~use).sum() <= 4, (what, bounds)
    if not use.any():
        return 0.0
    e = (np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max(axis=1)
    assert (e[use] < bounds[use]).all(), (what, int(np.argmax(e / bounds)), e.max())
    return float((e[use] / bounds[use]).max())


def assert_abs_within(got, ref, kat, key, tol):
    """|got - ref| < tol on every row of a per-point scalar; on the wide fixture's conditioned
    rows the row's bound (kat_row_bounds) instead, relative to max(1, |ref|)."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    rows = np.arange(len(ref))
    cond = rows >= KAT_WIDE_COND if "spread." + key in kat else np.zeros(len(ref), dtype=bool)
    assert np.max(np.abs(got - ref)[~cond]) < tol, key
    if cond.any():
        assert_rows_within(got[cond], ref[cond], kat_row_bounds(kat, key, tol, rows[cond]), key)


def kat_rows(kat, mode=None, foot=None):
    """Points of a fixture a dynamics mode / a touchdown impact of `foot` is checked at: all
    of the random fixture; of the trajectory fixture the knots of that mode, and for the
    impact the last knots of the flight phase that ends with that foot's touchdown."""
    if "mode" not in kat:
        return np.arange(len(kat["x"]))
    if mode is not None:
        return np.where(kat["mode"] == mode)[0]
    if foot is not None:
        return np.where(kat["pre_td"] & (kat["mode"] == (2 if foot == 0 else 4)))[0]
    return np.arange(len(kat["x"]))


def rel_err(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))


def norm_err(a, b):
    """Norm-relative error of [points][...] arrays, worst point: per point
    max|a - b| / max(1, max|b|) over the point's whole output array.  (Per element, rel_err
    says little in fp32: Ac holds entries of 3e4 beside entries of 1e-2.)"""
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    assert a.shape == b.shape, (a.shape, b.shape)
    if a.size == 0:
        return 0.0
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    return float(np.max(np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))))


def ulp_err(got, hi, lo, f32=False):
    """Error of got in ulps of the reference hi + lo (a double-double of prim_kat.npz), per
    element.  The ulp is that of hi (rounded to float when f32) and is not taken below the
    smallest normal number, so a subnormal result flushed to zero is within an ulp.  Where the
    reference is not finite the error is 0 if got is the same value (any NaN for NaN), else
    inf."""
    got, hi, lo = (np.asarray(v, dtype=np.float64) for v in (got, hi, lo))
    fin = np.isfinite(hi)
    h = np.where(fin, hi, 1.0)
    if f32:
        with np.errstate(over="ignore"):
            sp = np.spacing(np.abs(h).astype(np.float32)).astype(np.float64)
        sp = np.where(np.isfinite(sp), sp, 2.0 ** 104)  # a reference past the largest float
        unit = np.maximum(sp, 2.0 ** -126)
    else:
        unit = np.maximum(np.spacing(np.abs(h)), 2.0 ** -1022)
    with np.errstate(invalid="ignore"):
        e = np.abs((got - h) - lo) / unit
    same = (got == hi) | (np.isnan(got) & np.isnan(hi))
    e = np.where(fin, e, np.where(same, 0.0, np.inf))
    return np.where(np.isnan(e), np.inf, e)


_structure = {}


def kat_structure(key):
    """Entries of reference output `key` (e.g. "Dyn_BS_par.Ac") that are exactly 0, and
    exactly 1, at every one of the 64 random points: the function's sparsity pattern."""
    if key not in _structure:
        ref = golden(KAT_FIXTURES[0])[key]
        _structure[key] = ((ref == 0).all(axis=0), (ref == 1).all(axis=0))
    return _structure[key]


def assert_structure(got, key):
    """The structural zeros and ones of `key` are exact in got [points][...] (the sweep's
    structure-exploiting [A B] form relies on them; rel_err lets 1e-9 through)."""
    zero, one = kat_structure(key)
    got = np.asarray(got)
    assert got.shape[1:] == zero.shape, (key, got.shape)
    assert (got[:, zero] == 0).all(), (key, "structural zero", np.abs(got[:, zero]).max())
    assert (got[:, one] == 1).all(), (key, "structural one")
