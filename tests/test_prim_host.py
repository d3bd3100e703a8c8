"""The hand-written elementary functions that have a host path (mhpc_dual.h: sin_cos_short,
sin_cos, sin_cos_n; mhpc_model.h: div_const), compiled for the host in double and in float
without contraction, against the 60-digit references of tests/golden/prim_kat.npz; and the
fixture's own barrier and log references against plain numpy, so the fixture cannot be wrong
on its own.  The device paths of the same functions: tests/test_gpu_primitives.py."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from _util import golden, ulp_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "prim_hostcheck.cpp")
BUILD = os.path.join(ROOT, "tests", "_build")

# sin / cos bands of the fixture ("sc.band")
RANDOM, NEAR_KPI2, SMALL, SWITCH, BIG, NONFINITE = (0, 1, 2, 3), 4, 5, 6, 7, 8
# Host bound of the short reduction on random arguments, in ulps: the header's claim (1.49
# measured over 2 M points a band, 1.36 on the fixture's); the device test adds half an ulp for
# its contraction.
SINCOS_ULP_HOST = 1.5
# At the doubles around k pi/2 the result is near 0 and only the absolute error is bounded
# (in ulps of the result the error reaches 1.78e3, at a = 46066.743875913933).
SINCOS_ABS_NEAR_KPI2 = 2.0 ** -52


def P(a):
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))


@pytest.fixture(scope="module")
def kat():
    return golden("prim_kat.npz")


_libs = {}


def build(f32):
    """libprim_hostcheck.so (double) / libprim_hostcheck_f32.so (-DMHPC_FP32), built once."""
    if f32 in _libs:
        return _libs[f32]
    os.makedirs(BUILD, exist_ok=True)
    so = os.path.join(BUILD, "libprim_hostcheck_f32.so" if f32 else "libprim_hostcheck.so")
    extra = ["-DMHPC_FP32"] if f32 else []
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", *extra, "-fPIC", "-shared",
                    "-o", so, SRC], check=True)
    _libs[f32] = ctypes.CDLL(so)
    return _libs[f32]


@pytest.fixture(scope="module", params=[64, 32], ids=["fp64", "fp32"])
def hc(request):
    return request.param == 32, build(request.param == 32)


def sincos(lib, a, fn="hc_sin_cos", N=None):
    a = np.ascontiguousarray(a, dtype=np.float64)
    s, c = np.full(len(a), np.nan), np.full(len(a), np.nan)
    if N is None:
        getattr(lib, fn)(len(a), P(a), P(s), P(c))
    else:
        lib.hc_sin_cos_n(N, len(a), P(a), P(s), P(c))
    return s, c


def sincos_errors(kat, key, s, c, f32):
    """(ulp error, absolute error) per point, the worse of sin and cos."""
    es = ulp_err(s, kat[key + ".s.hi"], kat[key + ".s.lo"], f32)
    ec = ulp_err(c, kat[key + ".c.hi"], kat[key + ".c.lo"], f32)
    with np.errstate(invalid="ignore"):
        ab = np.maximum(np.abs((s - kat[key + ".s.hi"]) - kat[key + ".s.lo"]),
                        np.abs((c - kat[key + ".c.hi"]) - kat[key + ".c.lo"]))
    return np.maximum(es, ec), ab


def test_sin_cos_short_fp64(kat):
    """The short reduction on |a| <= 1e5, host double build: random arguments within
    SINCOS_ULP_HOST ulps in every band (measured 1.36 / 1.16 / 0.90 / 1.11 on the fixture's 512
    points each of [0,3], [3,60], [60,1e3], [1e3,1e5], absolute 1.08e-16; 1.49 over 2 M points);
    around k pi/2 within 2^-52 absolute (measured 6.6e-22 on the fixture: the error of the
    reduced argument, which is 1.78e3 ulps of the result at 46066.743875913933); sin(+-0) = 0
    (the reduction's FMA returns +0 for -0: the sign of a zero sine is not kept) and
    cos(+-0) = 1."""
    lib = build(False)
    a, band = kat["sc.a"], kat["sc.band"]
    use = np.abs(a) <= 1e5
    s, c = sincos(lib, a[use], "hc_sin_cos_short")
    sub = {k: v[use] for k, v in kat.items() if k.startswith("sc.")}
    ulp, ab = sincos_errors(sub, "sc", s, c, False)
    b = band[use]
    for r in RANDOM:
        print(f"sin_cos_short band {r}: {ulp[b == r].max():.3f} ulp, abs {ab[b == r].max():.3e}")
        assert ulp[b == r].max() <= SINCOS_ULP_HOST
    near = b == NEAR_KPI2
    print(f"sin_cos_short near k pi/2: abs {ab[near].max():.3e}, {ulp[near].max():.3e} ulp at "
          f"{a[use][near][np.argmax(ulp[near])]!r}")
    assert ab[near].max() <= SINCOS_ABS_NEAR_KPI2
    for r in (SMALL, SWITCH):
        print(f"sin_cos_short band {r}: {ulp[b == r].max():.3f} ulp")
        assert ulp[b == r].max() <= SINCOS_ULP_HOST
    zero = a[use] == 0
    assert zero.sum() == 2 and (s[zero] == 0).all()
    assert (c[zero] == 1).all()


def test_sin_cos(kat, hc):
    """sin_cos of both host builds on every point of its fixture: the double build equals the
    short reduction on |a| <= 1e5 and the C library beyond (within an ulp, 2^-51 absolute);
    the float build (sinf / cosf) within 1 ulp and 2^-22 absolute on |a| <= 60; NaN for +-inf
    and NaN in both."""
    f32, lib = hc
    key = "sc32" if f32 else "sc"
    a, band = kat[key + ".a"], kat[key + ".band"]
    s, c = sincos(lib, a)
    ulp, ab = sincos_errors(kat, key, s, c, f32)
    nf = band == NONFINITE
    assert np.isnan(s[nf]).all() and np.isnan(c[nf]).all()
    if f32:
        fin = ~nf & (band != NEAR_KPI2)
        print(f"sinf / cosf: {ulp[fin].max():.3f} ulp, abs on |a| <= 60 {ab[np.abs(a) <= 60].max():.3e}")
        assert ulp[fin].max() <= 1.0
        assert ab[np.abs(a) <= 60].max() <= 2.0 ** -22
        assert ab[~nf].max() <= 2.0 ** -23  # half a float ulp of 1 everywhere
        return
    small = np.abs(a) <= 1e5
    s0, c0 = sincos(lib, a[small], "hc_sin_cos_short")
    assert (s[small] == s0).all() and (c[small] == c0).all()
    big = band == BIG
    print(f"library path: {ulp[big].max():.3f} ulp, abs {ab[big].max():.3e}")
    assert ulp[big].max() <= 1.0 and ab[big].max() <= 2.0 ** -51
    sw = band == SWITCH
    assert ulp[sw].max() <= SINCOS_ULP_HOST and ab[sw].max() <= 2.0 ** -51


@pytest.mark.parametrize("N", [5, 3])
def test_sin_cos_n_is_sin_cos_per_angle(kat, hc, N):
    """sin_cos_n<N> returns, per angle, the bits of sin_cos -- also in groups that hold
    arguments on both sides of 1e5 and non-finite ones (the fixture's points shuffled)."""
    f32, lib = hc
    a = kat["sc32.a" if f32 else "sc.a"]
    a = np.random.default_rng(N).permutation(a)[:len(a) // N * N]
    s, c = sincos(lib, a)
    sn, cn = sincos(lib, a, N=N)
    assert (s.view(np.int64) == sn.view(np.int64)).all()
    assert (c.view(np.int64) == cn.view(np.int64)).all()


def test_div_const_is_the_ieee_quotient(hc):
    """div_const(a, c, RN(1 / c)) equals a / c bit for bit for both SRB constants, over every
    binade whose quotient and residual stay normal, in both signs, and at +-0."""
    f32, lib = hc
    t = np.float32 if f32 else np.float64
    cs = np.zeros(2)
    lib.hc_div_const_c(P(cs))
    rng = np.random.default_rng(7)
    e = np.repeat(np.arange(-100, 100) if f32 else np.arange(-900, 1000), 16)
    a = np.ldexp(rng.uniform(1, 2, len(e)), e) * rng.choice([-1.0, 1.0], len(e))
    a = np.concatenate([a, [0.0, -0.0]]).astype(t).astype(np.float64)
    for which in (0, 1):
        out = np.full(len(a), np.nan)
        lib.hc_div_const(len(a), which, P(a), P(out))
        ref = (a.astype(t) / t(cs[which])).astype(np.float64)
        assert (out.view(np.int64) == ref.view(np.int64)).all(), which


def barrier_numpy(g, delta):
    """SinglePhase::reduced_barrier (SinglePhase.cpp:298-317) restated operation by operation,
    k = 2."""
    k = 2
    with np.errstate(all="ignore"):
        inside = g > delta
        t = (g - k * delta) / ((k - 1) * delta)
        one, half = g.dtype.type(1), g.dtype.type((k - 1) / k)
        log = lambda v: np.log(v.astype(np.float64)).astype(v.dtype)  # numpy's float log: 2 ulps
        B = np.where(inside, -log(g), half * (np.power(t, k) - one) - log(delta))
        Bz = np.where(inside, -one / g, np.power(t, k - 1) / delta)
        Bzz = np.where(inside, np.power(g, g.dtype.type(-2)), np.power(t, k - 2))
    return inside, B, Bz, Bzz


def barrier_errors(kat, key, got, f32):
    """Error of B, Bz, Bzz [n][3] against the fixture in ulps of the working type.  B on the
    relaxed side is a difference that carries log(delta) with the log's own error of an ulp:
    its error is taken in units of ulp(B) + ulp(log(delta)).  (Inside, B is the log itself.)"""
    e = {nm: ulp_err(got[:, j], kat[f"{key}.{nm}.hi"], kat[f"{key}.{nm}.lo"], f32)
         for j, nm in enumerate(("B", "Bz", "Bzz"))}
    t = np.float32 if f32 else np.float64
    tiny = 2.0 ** (-126 if f32 else -1022)
    rel = ~kat[key + ".in"]
    B = kat[key + ".B.hi"][rel]
    lg = np.abs(np.log(kat[key + ".delta"][rel]))
    unit = lambda v: np.maximum(np.spacing(np.abs(v).astype(t)).astype(np.float64), tiny)
    e["B"][rel] = np.abs(got[rel, 0] - B) / (unit(B) + unit(lg))
    return e


@pytest.mark.parametrize("key", ["bar", "bar32"])
def test_fixture_barrier_is_the_reference_formula(kat, key):
    """The fixture's barrier references against the reference's formulas in plain numpy, in the
    fixture's working type: the same side, and every output within an ulp (numpy's log and pow
    are the C library's, within an ulp of the correctly rounded ones of the fixture); the
    special values (g = +inf: -inf, -0, +0; g g overflowing: Bzz = 0) exactly."""
    f32 = key == "bar32"
    t = np.float32 if f32 else np.float64
    g, d = kat[key + ".g"], kat[key + ".delta"]
    inside, B, Bz, Bzz = barrier_numpy(g.astype(t), d.astype(t))
    assert (inside == kat[key + ".in"]).all()
    e = barrier_errors(kat, key, np.stack([B, Bz, Bzz], axis=1).astype(np.float64), f32)
    for nm, v in e.items():
        print(f"{key}.{nm}: numpy restatement within {v.max():.2f} ulp")
        assert v.max() <= 1.0, (nm, g[np.argmax(v)], d[np.argmax(v)])
    inf = g == np.inf
    assert inf.sum() == 2
    assert (kat[key + ".B.hi"][inf] == -np.inf).all()
    assert (kat[key + ".Bz.hi"][inf] == 0).all() and np.signbit(kat[key + ".Bz.hi"][inf]).all()
    assert (kat[key + ".Bzz.hi"][inf] == 0).all() and not np.signbit(kat[key + ".Bzz.hi"][inf]).any()
    over = kat[key + ".band"] == 4
    assert over.sum() == 2 and (kat[key + ".Bzz.hi"][over] == 0).all()
    # the side at delta itself is the relaxed one, one ulp above it the inside
    edge = kat[key + ".band"] == 2
    assert (kat[key + ".in"][edge] == (g[edge] > d[edge])).all()
    assert sorted(kat[key + ".in"][edge].tolist()) == [False, False, False, False, True, True]


def test_fixture_elementary_references_match_libm(kat):
    """sin, cos, log and 1 / a of the fixture within an ulp of numpy's (the C library's) values:
    a reference generated wrongly would be off by far more."""
    for key in ("sc", "sc32"):
        fin = np.isfinite(kat[key + ".a"])
        a = kat[key + ".a"][fin]
        assert ulp_err(np.sin(a), kat[key + ".s.hi"][fin], kat[key + ".s.lo"][fin]).max() <= 1.0
        assert ulp_err(np.cos(a), kat[key + ".c.hi"][fin], kat[key + ".c.lo"][fin]).max() <= 1.0
    for key in ("log", "log32"):
        assert ulp_err(np.log(kat[key + ".a"]), kat[key + ".hi"], kat[key + ".lo"]).max() <= 1.0
        one = kat[key + ".a"] == 1
        assert one.sum() == 1 and (kat[key + ".hi"][one] == 0).all()
    for key in ("rcp", "rcp32"):
        a = kat[key + ".a"]
        with np.errstate(all="ignore"):
            q = 1.0 / a
        assert (q[~np.isnan(a)] == kat[key + ".hi"][~np.isnan(a)]).all()
        fin = np.isfinite(q)
        assert (np.abs(kat[key + ".lo"][fin]) <= np.spacing(np.abs(q[fin])) / 2).all()
        assert (kat[key + ".lo"][~fin] == 0).all()
