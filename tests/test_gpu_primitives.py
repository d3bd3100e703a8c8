"""The hand-written elementary functions of the device code, evaluated on the device through
mhpc_eval_primitive exactly as the solve kernels call them, against 60-digit references
(tests/golden/prim_kat.npz): sin_cos / sin_cos_n (short reduction, library path, and waves
that hold both), pivot_rcp, the backward sweep's recip, log_pos, reduced_barrier, div_const.
Both libraries (fp64, fp32).  The host paths of the same functions: tests/test_prim_host.py.

Every bound is stated beside the value first measured on MI355X."""
import numpy as np
import pytest

from _util import golden, ulp_err
from test_prim_host import barrier_errors

pytestmark = pytest.mark.gpu

RANDOM, NEAR_KPI2, SMALL, SWITCH, BIG, NONFINITE = (0, 1, 2, 3), 4, 5, 6, 7, 8

# sin_cos, fp64, |a| <= 1e5: the host bound of the short reduction (test_prim_host.py) plus half
# an ulp for the contracted polynomial tails of the device build.  Measured: 1.16.
SINCOS_ULP_SHORT = 1.5 + 0.5
# |a| > 1e5 (the library's sincos): the measured ulp error, 0.655, plus a half.
SINCOS_ULP_LIB = 0.655 + 0.5
# fp32 library (sincosf): twice the measured 1.253 float ulps.
SINCOS_ULP_F32 = 2 * 1.253
LOG_ULP_F32 = 2 * 2.215          # logf: twice the measured 2.215 float ulps
BARRIER_ULP_F32 = 2 * 2.0        # twice the measured 2 float ulps (of B; Bz 0, Bzz 1)
RECIP_ULP_F32 = 1.0              # one Newton step from v_rcp_f32; measured 0.500


@pytest.fixture(scope="module")
def kat(need_gpu):
    return golden("prim_kat.npz")


@pytest.fixture(scope="module")
def L(need_gpu):
    from mhpc_minimal_env_amd import capi
    return capi


def prim(L, name, a, b=None, f32=False):
    """One launch of primitive `name` at the points a (and b): out [n][w] (w = 1: [n])."""
    fn, w = L.PRIMITIVES[name]
    a = np.ascontiguousarray(a, dtype=np.float64)
    assert 1 <= len(a) <= 4096
    b = None if b is None else np.ascontiguousarray(b, dtype=np.float64)
    out = np.full((len(a), w), np.nan)
    f = L.lib().mhpc_eval_primitive_f32 if f32 else L.lib().mhpc_eval_primitive
    L.check(f(0, fn, len(a), L.dptr(a), L.dptr(b), L.dptr(out)), name)
    return out[:, 0] if w == 1 else out


def bits(v):
    return np.ascontiguousarray(v, dtype=np.float64).view(np.int64)


def same_bits(a, b):
    """Bitwise equal, any NaN equal to any NaN."""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def sincos_errors(kat, key, out, f32):
    s, c = out[:, 0], out[:, 1]
    es = ulp_err(s, kat[key + ".s.hi"], kat[key + ".s.lo"], f32)
    ec = ulp_err(c, kat[key + ".c.hi"], kat[key + ".c.lo"], f32)
    with np.errstate(invalid="ignore"):
        ab = np.maximum(np.abs((s - kat[key + ".s.hi"]) - kat[key + ".s.lo"]),
                        np.abs((c - kat[key + ".c.hi"]) - kat[key + ".c.lo"]))
    return np.maximum(es, ec), ab


def test_sin_cos_fp64(kat, L):
    """sin_cos of the fp64 library on every point of the fixture.
    |a| <= 1e5 (short reduction): random bands within SINCOS_ULP_SHORT = 2.0 ulp (measured
    0.97 / 1.16 / 0.93 / 1.11 on [0,3], [3,60], [60,1e3], [1e3,1e5], 1.08e-16 absolute); the
    doubles around k pi/2 within 2^-52 absolute (no relative bound holds there; measured
    6.6e-22, which is 1.78e3 ulps of the result); +-0, subnormals, 2^-30, pi/4 +- 1 ulp and both sides of the
    switch at 1e5 within their side's bound.
    |a| > 1e5 (library path): 2^-51 absolute (measured 7.3e-17) and SINCOS_ULP_LIB = 1.155
    ulp (measured 0.655; at the switch 0.46 below and 0.29 above).
    +-inf and NaN give NaN in both outputs."""
    a, band = kat["sc.a"], kat["sc.band"]
    out = prim(L, "sin_cos", a)
    ulp, ab = sincos_errors(kat, "sc", out, False)
    short = np.abs(a) <= 1e5
    for r in RANDOM + (SMALL,):
        print(f"sin_cos fp64 band {r}: {ulp[band == r].max():.3f} ulp, abs {ab[band == r].max():.3e}")
    near = band == NEAR_KPI2
    print(f"sin_cos fp64 near k pi/2: abs {ab[near].max():.3e}, {ulp[near].max():.3e} ulp")
    lib = ~short & np.isfinite(a)
    print(f"sin_cos fp64 library path: {ulp[lib].max():.3f} ulp, abs {ab[lib].max():.3e}")
    sw = band == SWITCH
    print(f"sin_cos fp64 switch: below {ulp[sw & short].max():.3f} ulp, above {ulp[sw & ~short].max():.3f} ulp")
    for r in RANDOM + (SMALL,):
        assert ulp[band == r].max() <= SINCOS_ULP_SHORT, r
    assert ab[near].max() <= 2.0 ** -52
    assert ab[lib].max() <= 2.0 ** -51
    assert ulp[lib].max() <= SINCOS_ULP_LIB
    assert (sw & short).sum() == 4 and (sw & ~short).sum() == 2
    assert ulp[sw & short].max() <= SINCOS_ULP_SHORT and ulp[sw & ~short].max() <= SINCOS_ULP_LIB
    nf = band == NONFINITE
    assert nf.sum() == 3 and np.isnan(out[nf]).all()
    zero = a == 0
    assert (out[zero, 0] == 0).all() and (out[zero, 1] == 1).all()


def test_sin_cos_fp32(kat, L):
    """sincosf of the fp32 library on float arguments: SINCOS_ULP_F32 = 2.506 float ulps, twice
    the measured 1.253, away from k pi/2; everywhere on |a| <= 60 at most 2^-22 absolute (what
    the KAT_TOL_F32 entries of h and J need; measured 5.5e-8); NaN for +-inf and
    NaN."""
    a, band = kat["sc32.a"], kat["sc32.band"]
    out = prim(L, "sin_cos", a, f32=True)
    ulp, ab = sincos_errors(kat, "sc32", out, True)
    nf = band == NONFINITE
    fin = ~nf & (band != NEAR_KPI2)
    print(f"sin_cos fp32: {ulp[fin].max():.3f} ulp, abs on |a| <= 60 {ab[np.abs(a) <= 60].max():.3e}, "
          f"abs overall {ab[~nf].max():.3e}")
    assert ulp[fin].max() <= SINCOS_ULP_F32
    assert ab[np.abs(a) <= 60].max() <= 2.0 ** -22
    assert np.isnan(out[nf]).all()


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_sin_cos_mixed_waves(kat, L, f32):
    """The wave-uniform library fallback with its per-lane select: 512 arguments of
    |a| <= 1e5 and 512 above it (+-inf and NaN among them) evaluated in waves wholly on one
    side, interleaved small / big within every wave, and with a single big lane (lane 0, lane
    63) in a small wave -- every argument gets the same bits in all of them.  sin_cos_n<5> and
    sin_cos_n<3>, with the default constants and with the knot loops' register copy, in groups
    that straddle 1e5: per angle the bits of sin_cos."""
    key = "sc32" if f32 else "sc"
    a = kat[key + ".a"]
    rng = np.random.default_rng(5)
    isbig = ~(np.abs(a) <= 1e5)
    sw = kat[key + ".band"] == SWITCH                # both sides of the switch are in
    small = np.concatenate([a[sw & ~isbig], rng.permutation(a[~isbig & ~sw])])[:512]
    big = np.resize(np.concatenate([a[sw & isbig], rng.permutation(a[isbig & ~sw])]), 512)
    assert len(small) == 512 and isbig.sum() >= 64
    pool = np.concatenate([small, big])              # sorted: waves 0-7 small, 8-15 big
    ref = prim(L, "sin_cos", pool, f32=f32)
    inter = np.empty(1024, dtype=int)                # even lanes small, odd lanes big
    inter[0::2], inter[1::2] = np.arange(512), 512 + np.arange(512)
    single = []                                      # 63 small lanes and one big one
    for w in range(16):
        lanes = list(rng.integers(0, 512, 63))
        lanes.insert(0 if w < 8 else 63, 512 + w)
        single += lanes
    for name, idx in (("interleaved", inter), ("single big lane", np.array(single))):
        got = prim(L, "sin_cos", pool[idx], f32=f32)
        assert same_bits(got, ref[idx]).all(), name
    perm = rng.permutation(1024)[:1020]              # a multiple of 5 and of 3
    for name in ("sin_cos_n5", "sin_cos_n3", "sin_cos_n5_vk", "sin_cos_n3_vk"):
        got = prim(L, name, pool[perm], f32=f32)
        assert same_bits(got, ref[perm]).all(), name
    groups = (~(np.abs(pool[perm]) <= 1e5)).reshape(-1, 5).sum(axis=1)
    assert ((groups > 0) & (groups < 5)).sum() >= 100  # groups of five that straddle 1e5


def test_log_pos_fp64(kat, L):
    """log_pos of the fp64 library within 1 ulp on every binade from 2^-1074 to 2^1023
    (measured 0.583; subnormal arguments 0.477), on 1 +- 1e-3 (0.499) and around the sqrt(1/2)
    switch (0.605); log_pos(1) = +0 exactly."""
    a, band = kat["log.a"], kat["log.band"]
    got = prim(L, "log_pos", a)
    e = ulp_err(got, kat["log.hi"], kat["log.lo"])
    sub = a < 2.0 ** -1022
    for nm, m in (("binades", band == 0), ("subnormal", sub), ("1 +- 1e-3", band == 1),
                  ("1 +- 1 ulp", band == 2), ("sqrt(1/2) +- 8 ulp", band == 3), ("delta", band == 4)):
        print(f"log_pos fp64 {nm}: {e[m].max():.3f} ulp")
    assert sub.sum() >= 52
    assert e.max() <= 1.0, a[np.argmax(e)]
    one = a == 1
    assert one.sum() == 1 and got[one][0] == 0 and not np.signbit(got[one][0])


def test_log_pos_fp32(kat, L):
    """logf of the fp32 library on float arguments of every binade: LOG_ULP_F32 = 4.43 float
    ulps, twice the measured 2.215 (subnormal arguments 1.365); logf(1) = +0."""
    a = kat["log32.a"]
    got = prim(L, "log_pos", a, f32=True)
    e = ulp_err(got, kat["log32.hi"], kat["log32.lo"], True)
    print(f"log_pos fp32: {e.max():.3f} ulp; subnormal arguments {e[a < 2.0 ** -126].max():.3f} ulp")
    assert e.max() <= LOG_ULP_F32, a[np.argmax(e)]
    assert got[a == 1][0] == 0 and not np.signbit(got[a == 1][0])


def check_barrier_cases(kat, key, got, f32):
    g, band, inside = kat[key + ".g"], kat[key + ".band"], kat[key + ".in"]
    # the side taken at delta and its two neighbours: Bzz = 1 exactly on the relaxed side only
    edge = band == 2
    assert edge.sum() == 6 and ((got[edge, 2] == 1.0) == ~inside[edge]).all()
    over = band == 4  # g g overflows: Bzz = 0
    assert over.sum() == 2 and (got[over, 2] == 0).all()


@pytest.mark.parametrize("f32", [
    pytest.param(False, id="fp64", marks=pytest.mark.xfail(strict=True, reason=(
        "log_pos(+inf) is NaN (f / (2 + f) = inf / inf), so B = NaN where the reference's "
        "-log(g) is -inf; a select on log_pos' result costs 0.5 % of the C3 solve (5.402 against "
        "5.377 ms a step, three alternating runs each) and no constraint is known to reach "
        "g = +inf"))),
    pytest.param(True, id="fp32")])
def test_reduced_barrier_at_inf(kat, L, f32):
    """g = +inf: the reference's log and pow give B, Bz, Bzz = -inf, -0, +0.  The fp32 library
    (logf) does; the fp64 library returns NaN, -0, +0 (measured)."""
    key = "bar32" if f32 else "bar"
    inf = kat[key + ".g"] == np.inf
    assert inf.sum() == 2
    got = prim(L, "reduced_barrier", kat[key + ".g"][inf], kat[key + ".delta"][inf], f32=f32)
    print(f"{key} g = +inf: B, Bz, Bzz = {got.tolist()}")
    assert (got[:, 1] == 0).all() and np.signbit(got[:, 1]).all()
    assert (got[:, 2] == 0).all() and not np.signbit(got[:, 2]).any()
    assert (got[:, 0] == -np.inf).all()


def test_reduced_barrier_fp64(kat, L):
    """reduced_barrier(g, delta) of the fp64 library for both default relaxations, against the
    reference's own operations with a correctly rounded log and pow: B, Bz and Bzz within 1 ulp,
    B of the relaxed side within 1 ulp of B plus 1 ulp of the log(delta) it carries (measured: B
    1 ulp on both sides, Bz 0, Bzz 1); the side at g = delta (relaxed) and one ulp on either side as the reference
    takes it; Bzz = 0 where g g overflows."""
    got = prim(L, "reduced_barrier", kat["bar.g"], kat["bar.delta"])
    e = barrier_errors(kat, "bar", got, False)
    fin = kat["bar.g"] != np.inf  # g = +inf: test_reduced_barrier_at_inf
    e = {nm: np.where(fin, v, 0.0) for nm, v in e.items()}
    for nm, v in e.items():
        for side in (True, False):
            m = kat["bar.in"] == side
            i = np.argmax(np.where(m, v, -1))
            print(f"reduced_barrier fp64 {nm} {'inside' if side else 'relaxed'}: {v[m].max():.3f} ulp "
                  f"at g = {kat['bar.g'][i]!r}, delta = {kat['bar.delta'][i]}")
    check_barrier_cases(kat, "bar", got, False)
    assert e["B"].max() <= 1.0
    assert e["Bz"].max() <= 1.0
    assert e["Bzz"].max() <= 1.0


def test_reduced_barrier_fp32(kat, L):
    """The fp32 library's barrier (logf, float arithmetic) on float arguments: BARRIER_ULP_F32
    = 4 float ulps per output, twice the measured 2 (B; Bz 0, Bzz 1); the same special cases."""
    got = prim(L, "reduced_barrier", kat["bar32.g"], kat["bar32.delta"], f32=True)
    e = barrier_errors(kat, "bar32", got, True)
    fin = kat["bar32.g"] != np.inf
    e = {nm: np.where(fin, v, 0.0) for nm, v in e.items()}
    for nm, v in e.items():
        print(f"reduced_barrier fp32 {nm}: {v.max():.3f} ulp")
    check_barrier_cases(kat, "bar32", got, True)
    assert max(v.max() for v in e.values()) <= BARRIER_ULP_F32


def show(tag, a, got, ref):
    for x, y, z in zip(a, got, ref):
        print(f"  {tag}({x!r}) = {y!r}  (IEEE {z!r})")


RCP_CASES = pytest.mark.parametrize("name,f32", [("pivot_rcp", False), ("sweep_recip", False),
                                                 ("sweep_recip", True)],
                                    ids=["pivot_rcp", "recip", "recip-of-the-fp32-library"])


@RCP_CASES
def test_reciprocals_fp64(kat, L, name, f32):
    """pivot_rcp (fp64 library) and the sweep's recip(double) (both libraries: the fp32
    library's default sweep computes in double): within 1 ulp on [2^-1020, 2^1020] in both
    signs (measured 0.500 for all three), powers of two exact.  pivot_rcp at +-0, +-inf and NaN
    is the IEEE value.  What recip returns at +-0 (never reached, the caller tests the pivot),
    +-inf and NaN is printed (measured: the IEEE values +-inf, +-0, NaN, the estimate where its
    refinement is not finite), and at +-inf and NaN it is no finite non-zero number."""
    a, band, hi, lo = kat["rcp.a"], kat["rcp.band"], kat["rcp.hi"], kat["rcp.lo"]
    got = prim(L, name, a, f32=f32)
    e = ulp_err(got, hi, lo)
    print(f"{name}: random mantissas {e[band == 0].max():.3f} ulp")
    assert e[band == 0].max() <= 1.0
    assert same_bits(got[band == 1], hi[band == 1]).all()
    sp = band == 2
    show(name, a[sp], got[sp], hi[sp])
    if name == "pivot_rcp":
        assert same_bits(got[sp], hi[sp]).all()
    else:
        nz = sp & (a != 0)
        assert nz.sum() == 3 and (~np.isfinite(got[nz]) | (got[nz] == 0)).all()


@RCP_CASES
def test_reciprocals_fp64_subnormal_and_near_overflow(kat, L, name, f32):
    """Subnormal arguments, |a| > 2^1020 and |a| < 2^-1020: the IEEE value, or within an ulp
    floored at 2^-1022 (what the device did is printed).  Measured: all 54 points are the IEEE
    value or within the floored ulp for all three.  Below 2^-1024 the estimate is +-inf, its
    refinement inf - inf, and both functions return the estimate, 1 / a = +-inf; recip(double)
    returned NaN at those 20 points (first +-4.9406564584124654e-324) before it had
    pivot_rcp's guard."""
    a, band, hi, lo = kat["rcp.a"], kat["rcp.band"], kat["rcp.hi"], kat["rcp.lo"]
    rest = band >= 3
    got = prim(L, name, a[rest], f32=f32)
    e = ulp_err(got, hi[rest], lo[rest])
    show(name, a[rest], got, hi[rest])
    ok = same_bits(got, hi[rest]) | (e <= 1.0)
    print(f"{name}: {(~ok).sum()} of {rest.sum()} points fail: {a[rest][~ok].tolist()}")
    assert ok.all(), a[rest][~ok]


def test_reciprocals_fp32(kat, L):
    """The fp32 library on float arguments.  pivot_rcp keeps the IEEE quotient: equal to 1 / a
    in float on every binade, at powers of two, at +-0, +-inf, NaN, and at subnormal and
    near-overflow arguments.  recip(float) of the float sweep (one Newton step): RECIP_ULP_F32 =
    1 float ulp on [2^-124, 2^124] (measured 0.500), powers of two exact, no finite
    non-zero value at +-inf and NaN; what it returns at subnormal and near-overflow arguments is
    printed (the float estimate takes a subnormal argument for zero: +-inf)."""
    a, band, hi, lo = kat["rcp32.a"], kat["rcp32.band"], kat["rcp32.hi"], kat["rcp32.lo"]
    with np.errstate(all="ignore"):
        ieee = (np.float32(1) / a.astype(np.float32)).astype(np.float64)
    for name in ("pivot_rcp", "sweep_recip_f32"):
        got = prim(L, name, a, f32=True)
        e = ulp_err(got, hi, lo, True)
        print(f"{name} fp32: random mantissas {e[band == 0].max():.3f} ulp")
        sp = band == 2
        show(name, a[sp], got[sp], ieee[sp])
        rest = band >= 3
        show(name, a[rest], got[rest], ieee[rest])
        if name == "pivot_rcp":
            assert same_bits(got, ieee).all(), a[~same_bits(got, ieee)]
        else:
            assert e[band == 0].max() <= RECIP_ULP_F32
            assert same_bits(got[band == 1], ieee[band == 1]).all()
            nz = sp & (a != 0)
            assert (~np.isfinite(got[nz]) | (got[nz] == 0)).all()


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_div_const_is_the_ieee_quotient(L, f32):
    """div_const on the device, both SRB constants: the IEEE quotient a / c bit for bit over
    the binades whose quotient and residual stay normal, in both signs, and at +-0 (the same
    points as the host check).  At +-inf it returns NaN where the division gives +-inf (a
    rollout that far gone is lost either way): printed, not asserted."""
    t = np.float32 if f32 else np.float64
    rng = np.random.default_rng(7)
    e = np.repeat(np.arange(-100, 100) if f32 else np.arange(-900, 1000), 2)
    a = np.ldexp(rng.uniform(1, 2, len(e)), e) * rng.choice([-1.0, 1.0], len(e))
    a = np.concatenate([a, [0.0, -0.0, np.inf, -np.inf]]).astype(t).astype(np.float64)
    # kSrbMass, kSrbInertia (mhpc_model.h)
    for which, c in ((0.0, 8.2520000000000007), (1.0, 0.23216549759999999)):
        got = prim(L, "div_const", a, np.full(len(a), which), f32=f32)
        with np.errstate(all="ignore"):
            ref = (a.astype(t) / t(c)).astype(np.float64)
        fin = np.isfinite(a)
        print(f"div_const c = {c}: at +-inf {got[~fin].tolist()}")
        assert same_bits(got[fin], ref[fin]).all(), c
