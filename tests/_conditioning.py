"""How far the fp64 oracle's own C5 outputs move when each initial state is perturbed by an
fp32 rounding: the conditioning of every problem of configs.x0_for(c5_desc(), 64), measured on
the CPU alone.  The fp32 solve's error divided by this sensitivity is nearly flat over the
problems (tests/test_gpu_fp32.py), so it tells conditioning from an fp32 defect."""
import numpy as np

ARRAYS = ("X", "U", "K", "DU", "G")
N_DRAWS = 7        # x0 * (1 + U(-1, 1) * EPS), besides x0 rounded to float32
EPS = 6e-8         # half an fp32 ulp, relative
WORST = 50         # the problem every array's sensitivity ranks first

_cache = {}


def array_errors(got, ref, same=slice(None)):
    """Per problem and phase-concatenated array: ||a - b||_inf / max(1, ||b||_inf)."""
    out = {}
    for k in ARRAYS:
        a = np.asarray(got[k], float)[same]
        b = np.asarray(ref[k], float)[same]
        out[k] = np.abs(a - b).max(axis=1) / np.maximum(1.0, np.abs(b).max(axis=1))
    return out


def perturbations(x0):
    """The eight fixed perturbed copies of x0."""
    rng = np.random.default_rng(0)
    out = [x0.astype(np.float32).astype(np.float64)]
    for _ in range(N_DRAWS):
        out.append(x0 * (1.0 + rng.uniform(-1, 1, x0.shape) * EPS))
    return out


def c5_sensitivity(B=64, nthreads=8):
    """(ref, sens, traces_kept): the oracle's C5 solution of x0_for(c5_desc(), B),
    sens[k][b] = the largest array_errors of the eight perturbed oracle solves against it, and
    whether every perturbed solve kept every problem's decision trace."""
    if B not in _cache:
        import oracle as O
        from mhpc_minimal_env_amd import configs, locomotion as L
        desc, opt = configs.c5_desc(64), L.HSDDP_OPTION().to_c()
        x0 = configs.x0_for(desc, B)
        ref = O.solve(desc, opt, x0, nthreads=nthreads)
        sens = {k: np.zeros(B) for k in ARRAYS}
        kept = True
        for xp in perturbations(x0):
            got = O.solve(desc, opt, np.ascontiguousarray(xp), nthreads=nthreads)
            kept = kept and bool((got["trace"] == ref["trace"]).all())
            for k, e in array_errors(got, ref).items():
                sens[k] = np.maximum(sens[k], e)
        _cache[B] = (ref, sens, kept)
    return _cache[B]
