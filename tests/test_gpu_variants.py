"""Every launch variant of the backward sweep and of the line search, and the batch sizes at
which the automatic choice switches between them, against the oracle and against each other.

The launch shape is chosen from the batch size (k_bws two rows per problem up to 2048 problems,
one row per problem above; k_rollout pair / pipelined / fused, staged or not), so a problem's result must not depend on the
batch it is solved in (per-problem outputs on G GPUs bitwise-identical to 1
GPU).  Here:
  * every (bws, rollout) variant pinned through mhpc_set_kernel_variant at batch 256 (C3) and
    64 (C5, fp64 and fp32): bitwise identical to each other, and the fp64 ones within the
    solve tolerance of the oracle with an identical decision trace (MultiPhaseDDP.cpp:154-289);
  * the north-star batch 4096 with the automatic choice (k_bws one row per problem, fused
    line search): a spread sample of 64 problems (including the last, partial block) against
    the oracle, and bitwise against the same initial states solved at batch 8 (two rows per
    problem, pair)."""
import itertools

import numpy as np
import pytest

from _util import SOLVE_TOL

pytestmark = pytest.mark.gpu

KEYS = ("X", "U", "Y", "K", "DU", "G", "J", "dV_exp", "viol", "V", "dV", "trace", "status")


def _oracle():
    import oracle as O
    return O if O.available() else None


def solve(desc, x0, bws="auto", rollout="auto", rows=None, overlap="auto", sub_batches=0,
          ro_store=0, sweep_bits=0):
    from mhpc_minimal_env_amd import locomotion as L
    loco = L.MHPCLocomotion(desc=desc, option=L.HSDDP_OPTION(), batch=x0.shape[0], device=0)
    try:
        loco.set_kernel_variant(bws=bws, rollout=rollout, overlap=overlap, sub_batches=sub_batches,
                                ro_store=ro_store, sweep_bits=sweep_bits)
        loco.set_initial_condition(x0)
        loco.initialization()
        status = loco.solve_mhpc().copy()
        out = loco.concatenated()
        out.update(loco.get_scalars())
        out["status"] = status
    finally:
        loco.close()
    if rows is not None:
        out = {k: np.asarray(v)[rows] for k, v in out.items()}
    return out


def assert_bitwise(a, b, what):
    for k in KEYS:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=f"{what}: {k}")


def assert_oracle(got, ref, tol=SOLVE_TOL):
    np.testing.assert_array_equal(got["trace"], ref["trace"])
    np.testing.assert_array_equal(got["status"], ref["status"])
    for k in ("X", "U", "Y", "K", "DU", "G", "J", "dV_exp", "viol", "V", "dV"):
        a, b = np.asarray(got[k], float), np.asarray(ref[k], float)
        err = float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b))))
        assert err <= tol, (k, err)


ALL_VARIANTS = [(b, r, "auto") for b, r in
                itertools.product(("rows4", "rows2", "rows1", "pairs2"),
                                  ("pair", "pipe_staged", "pipe", "fused_staged", "fused"))]
# the backward sweep as one launch after the partials (the default splits it into an SRB
# launch beside the partials and a WB launch after them)
ALL_VARIANTS += [("rows4", "pair", "off"), ("rows2", "fused", "off"), ("rows1", "pipe", "off"),
                 ("pairs2", "fused_staged", "off"), ("auto", "auto", "off")]


def test_variant_rejected_when_it_does_not_apply(need_gpu):
    from mhpc_minimal_env_amd import capi, configs, locomotion as L
    opt = L.HSDDP_OPTION()
    opt.alpha = 0.01  # 1, 1e-2, ..., 1e-8: 5 candidates -> no staged / pair variants
    loco = L.MHPCLocomotion(desc=configs.c3_desc(), option=opt, batch=2, device=0)
    try:
        for v in ("pair", "pipe_staged", "fused_staged"):
            with pytest.raises(RuntimeError):
                loco.set_kernel_variant(rollout=v)
        loco.set_kernel_variant(bws="rows2", rollout="fused")
        assert capi.lib().mhpc_set_kernel_variant(loco._h, 7, 0) == capi.MHPC_ERR_INVALID
        assert capi.lib().mhpc_set_kernel_variant(loco._h, 2, 3) == capi.MHPC_ERR_INVALID
        assert capi.lib().mhpc_set_kernel_variant(loco._h, 0, 5) == capi.MHPC_ERR_INVALID
        assert capi.lib().mhpc_set_kernel_variant(loco._h, capi.MHPC_VARIANT_SUBBATCH,
                                                  capi.MHPC_MAX_SUBBATCH + 1) == capi.MHPC_ERR_INVALID
        assert capi.lib().mhpc_set_kernel_variant(loco._h, capi.MHPC_VARIANT_RO_STORE, 33) == capi.MHPC_ERR_INVALID
        assert capi.lib().mhpc_set_kernel_variant(loco._h, capi.MHPC_VARIANT_RO_STORE, -1) == capi.MHPC_ERR_INVALID
    finally:
        loco.close()


def test_c3_every_variant_bitwise_and_vs_oracle(need_gpu):
    from mhpc_minimal_env_amd import configs, locomotion as L
    desc = configs.c3_desc()
    x0 = configs.x0_for(desc, 256, offset=5000)
    base = solve(desc, x0)
    O = _oracle()
    if O is not None:
        assert_oracle(base, O.solve(desc, L.HSDDP_OPTION().to_c(), x0, nthreads=8))
    for bws, ro, ov in ALL_VARIANTS:
        assert_bitwise(solve(desc, x0, bws, ro, overlap=ov), base,
                       f"C3 bws={bws} rollout={ro} overlap={ov}")


# fsweep: the fp32 library's float build of the backward sweep (MHPC_VARIANT_SWEEP_BITS = 32)
@pytest.mark.parametrize("precision,sweep_bits", [pytest.param(64, 0, id="64"),
                                                  pytest.param(32, 0, id="32"),
                                                  pytest.param(32, 32, id="32-fsweep")])
def test_c5_every_variant_bitwise(need_gpu, precision, sweep_bits):
    from mhpc_minimal_env_amd import configs, locomotion as L
    desc = configs.c5_desc(precision)
    x0 = configs.x0_for(desc, 64, offset=7000)
    base = solve(desc, x0, sweep_bits=sweep_bits)
    if precision == 64 and _oracle() is not None:
        assert_oracle(base, _oracle().solve(desc, L.HSDDP_OPTION().to_c(), x0, nthreads=8))
    for bws, ro, ov in ALL_VARIANTS:
        assert_bitwise(solve(desc, x0, bws, ro, overlap=ov, sweep_bits=sweep_bits), base,
                       f"C5/{precision} sweep bits {sweep_bits} bws={bws} rollout={ro} overlap={ov}")


def test_long_phases_unstaged_line_search(need_gpu):
    """Phases longer than the line search's LDS reference stage (ST_RMAX = 128 knots) run the
    unstaged kernels, also when a staged variant is pinned (launch_rollout): the same results
    bit for bit, and the oracle's."""
    from mhpc_minimal_env_amd import locomotion as L
    desc = L.make_problem_desc(2, 2, [1, 2, 3, 4], [0.15] * 4, 0.001, 0.001, 1.5)
    assert min(desc.N[p] for p in range(4)) > 128
    x0 = configs_x0(desc, 12, offset=4242)
    base = solve(desc, x0)
    O = _oracle()
    if O is not None:
        assert_oracle(base, O.solve(desc, L.HSDDP_OPTION().to_c(), x0, nthreads=8))
    for ro in ("pair", "fused_staged", "pipe", "fused"):
        assert_bitwise(solve(desc, x0, rollout=ro), base, f"long phases, rollout={ro}")
    # the unstaged re-roll (an accepted trial without records, one trial stored)
    assert_bitwise(solve(desc, x0, ro_store=1), base, "long phases, one trial stored")


@pytest.mark.parametrize("name,precision", [("c3", 64), ("c5", 64), ("c5", 32)])
def test_unstored_trials_rolled_out_again(need_gpu, name, precision):
    """Only the first ro_store line-search trials (and the last) store their knot records; an
    accepted trial without them is rolled out again into its slot (k_rollout mode 2).  With
    one stored trial most C5 decisions (trial 2 accepted) take the re-roll, in every variant;
    the results equal storing every trial bit for bit."""
    from mhpc_minimal_env_amd import configs
    desc = configs.c3_desc() if name == "c3" else configs.c5_desc(precision)
    x0 = configs.x0_for(desc, 48, offset=777)
    every = solve(desc, x0, ro_store=32)
    for ro in ("auto", "pair", "fused_staged", "pipe", "fused"):
        assert_bitwise(solve(desc, x0, rollout=ro, ro_store=1), every,
                       f"{name}/{precision} rollout={ro}, one trial stored")
    assert_bitwise(solve(desc, x0), every, f"{name}/{precision} default stored trials")


def configs_x0(desc, B, offset):
    from mhpc_minimal_env_amd import configs
    return configs.x0_for(desc, B, offset=offset)


@pytest.mark.parametrize("name,precision,sweep_bits", [pytest.param("c3", 64, 0, id="c3-64"),
                                                       pytest.param("c5", 32, 0, id="c5-32"),
                                                       pytest.param("c5", 32, 32, id="c5-32-fsweep")])
def test_sub_batches_bitwise(need_gpu, name, precision, sweep_bits):
    """The batch as 2..4 concurrently scheduled sub-batches (own stream pairs, staggered,
    ragged last block; MHPC_VARIANT_SUBBATCH) computes every problem bit for bit as one
    schedule over the whole batch does -- also with the sub-batch sizes' own launch shapes."""
    from mhpc_minimal_env_amd import configs
    desc = configs.c3_desc() if name == "c3" else configs.c5_desc(precision)
    x0 = configs.x0_for(desc, 203, offset=9000)
    what = f"{name}/{precision} sweep bits {sweep_bits}"

    def run(xs, **kw):
        return solve(desc, xs, sweep_bits=sweep_bits, **kw)

    base = run(x0, sub_batches=1)
    for n in (2, 3, 4):
        assert_bitwise(run(x0, sub_batches=n), base, f"{what} {n} sub-batches")
    assert_bitwise(run(x0, bws="rows4", rollout="fused", sub_batches=2), base,
                   f"{what} 2 sub-batches, 1-wave sweep, fused line search")
    # batches barely larger than the block count: the even partition leaves no empty block
    for B in (5, 6):
        xs = np.ascontiguousarray(x0[:B])
        assert_bitwise(run(xs, sub_batches=4), run(xs, sub_batches=1),
                       f"{what} batch {B} in 4 sub-batches")


def test_no_ddp_iterations_joins_partials(need_gpu):
    """max_DDP_iter = 0: the schedule is forward_sweep(0), partials, AL update per AL
    iteration; the partials' second stream is joined back before the solve returns, so a
    second handle's results and this one's repeat solve are deterministic."""
    from mhpc_minimal_env_amd import configs, locomotion as L
    desc = configs.c3_desc()
    x0 = configs.x0_for(desc, 16, offset=300)
    outs = []
    for _ in range(2):
        opt = L.HSDDP_OPTION()
        opt.max_DDP_iter = 0
        loco = L.MHPCLocomotion(desc=desc, option=opt, batch=16, device=0)
        try:
            loco.set_initial_condition(x0)
            loco.initialization()
            loco.solve_mhpc()
            o = loco.concatenated()
            o.update(loco.get_scalars())
            o["status"] = np.zeros(16)
            outs.append(o)
        finally:
            loco.close()
    assert_bitwise(outs[0], outs[1], "max_DDP_iter = 0, repeated")
    O = _oracle()
    if O is not None:
        opt = L.HSDDP_OPTION()
        opt.max_DDP_iter = 0
        ref = O.solve(desc, opt.to_c(), x0, nthreads=8)
        for k in ("J", "viol"):
            a, b = np.asarray(outs[0][k], float), np.asarray(ref[k], float)
            assert float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))) <= SOLVE_TOL, k


def _sample(B, n=64):
    """n problem indices spread over the batch: every block position, the last (partial)
    line-search block and the last problem."""
    idx = np.unique(np.concatenate([np.linspace(0, B - 1, n - 4).astype(int),
                                    [1, 2, B - 2, B - 1]]))
    return idx


@pytest.mark.parametrize("name,precision", [("c3", 64), ("c5", 64), ("c5", 32)])
def test_batch_4096_matches_batch_8_and_oracle(need_gpu, name, precision):
    from mhpc_minimal_env_amd import configs, locomotion as L
    desc = configs.c3_desc() if name == "c3" else configs.c5_desc(precision)
    B = 4096 + 7  # ragged: the last line-search block / pair block is partial
    x0 = configs.x0_for(desc, B)
    idx = _sample(B)
    big = solve(desc, x0, rows=idx)
    # the same problems in batches of 8 (1-wave bws, pair line search): bitwise equal
    for c in range(0, len(idx), 8):
        small = solve(desc, np.ascontiguousarray(x0[idx[c:c + 8]]))
        part = {k: np.asarray(v)[c:c + 8] for k, v in big.items()}
        assert_bitwise(part, small, f"{name}/{precision} batch {B} vs 8, problems {idx[c:c + 8]}")
    O = _oracle()
    if O is None:
        pytest.skip("oracle not built")
    ref = O.solve(configs.c5_desc(64) if name == "c5" else desc, L.HSDDP_OPTION().to_c(),
                  np.ascontiguousarray(x0[idx]), nthreads=8)
    if precision == 64:
        assert_oracle(big, ref)
    else:  # fp32 vs the fp64 oracle: the bounds of tests/test_gpu_fp32.py
        from test_gpu_fp32 import FP32_J_TOL, FP32_TRACE_MIN_SAMPLE
        same = (big["trace"] == ref["trace"]).all(axis=1)
        rel = np.abs(big["J"] - ref["J"]) / np.maximum(1.0, np.abs(ref["J"]))
        print(f"fp32 batch-{B} sample: traces {same.sum()}/{len(same)}, J rel err median "
              f"{np.median(rel):.2e} max {rel.max():.2e} (same-trace max {rel[same].max():.2e})")
        assert same.mean() >= FP32_TRACE_MIN_SAMPLE and rel[same].max() <= FP32_J_TOL
