"""Timing of mhpc_rollout_policy on the GPU: one launch over batch x n_samples lanes against
the only way to get the same numbers without it -- n_samples successive mhpc_set_x0 +
mhpc_rollout_costs([0]) calls, each a launch over `batch` lanes.

Case (default): C3, batch 1024, 64 samples per problem, every phase (n_phases = 0).
Reported: the device time (`ms` of mhpc_rollout_policy, HIP events around the launch) and the
wall time of the call (host packing and copies included), the wall time of the loop of
set_x0 + rollout_costs calls and the sum of their device times, median and spread over the
repeats, the two alternating in one process after a warm-up of both; the ratio; lanes per CU.
Before timing, the two ways' costs are compared bit for bit.  Fails without a GPU.

usage: python tools/policy_rollout_timing.py [--batch 1024] [--samples 64] [--repeats 7]
                                             [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def perturbed(x0, n_samples, seed=20261019):
    scale = np.array([1e-2] * 7 + [1e-1] * 7)
    rng = np.random.default_rng(seed)
    xs = x0[:, None, :] + scale * rng.uniform(-1.0, 1.0, size=(x0.shape[0], n_samples, 14))
    xs[:, 0, :] = x0
    return np.ascontiguousarray(xs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("policy_rollout_timing: no GPU visible")
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    from mhpc_minimal_env_amd import capi, configs, locomotion as L

    desc = configs.c3_desc()
    loco = L.MHPCLocomotion(desc=desc, option=L.HSDDP_OPTION(), batch=a.batch, device=0)
    x0 = configs.x0_for(desc, a.batch)
    loco.set_initial_condition(x0)
    loco.initialization()
    loco.solve_mhpc()
    xs = perturbed(x0, a.samples)
    cols = [np.ascontiguousarray(xs[:, s]) for s in range(a.samples)]
    lib = capi.lib()

    def one_launch():
        t = time.perf_counter()
        r = loco.rollout_policy(xs, 0)
        return time.perf_counter() - t, r["ms"], r["J"]

    def many_launches():
        J = np.zeros((a.batch, a.samples))
        dev = 0.0
        t = time.perf_counter()
        for s in range(a.samples):
            capi.check(lib.mhpc_set_x0(loco._h, capi.dptr(cols[s])), "mhpc_set_x0")
            r = loco.rollout_costs([0.0])
            J[:, s] = r["J"][:, 0]
            dev += r["ms"]
        return time.perf_counter() - t, dev, J

    for _ in range(a.warmup):
        _, _, J1 = one_launch()
        _, _, J2 = many_launches()
    same = bool((J1.view(np.uint64) == J2.view(np.uint64)).all())
    rows = {"policy_wall_ms": [], "policy_device_ms": [], "loop_wall_ms": [], "loop_device_ms": []}
    for _ in range(a.repeats):  # alternating, so that both see the same neighbours on the host
        w, d, _ = one_launch()
        rows["policy_wall_ms"].append(1e3 * w)
        rows["policy_device_ms"].append(d)
        w, d, _ = many_launches()
        rows["loop_wall_ms"].append(1e3 * w)
        rows["loop_device_ms"].append(d)
    loco.close()
    med = {k: float(np.median(v)) for k, v in rows.items()}
    res = {
        "case": {"config": "C3", "batch": a.batch, "n_samples": a.samples, "n_phases": 0,
                 "repeats": a.repeats, "warmup": a.warmup},
        "costs_bitwise_equal": same,
        "median": med,
        "min": {k: float(np.min(v)) for k, v in rows.items()},
        "max": {k: float(np.max(v)) for k, v in rows.items()},
        "loop_wall_over_policy_device": med["loop_wall_ms"] / med["policy_device_ms"],
        "loop_wall_over_policy_wall": med["loop_wall_ms"] / med["policy_wall_ms"],
        "loop_device_over_policy_device": med["loop_device_ms"] / med["policy_device_ms"],
        "compute_units": ncu,
        "lanes": a.batch * a.samples,
        "lanes_per_cu": a.batch * a.samples / ncu,
        "loop_lanes_per_cu_per_launch": a.batch / ncu,
    }
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    if not same:
        sys.exit("policy_rollout_timing: the two ways' costs differ")


if __name__ == "__main__":
    main()
