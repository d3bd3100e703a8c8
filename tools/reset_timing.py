"""Timing of per-problem re-initialisation on the GPU: mhpc_reset_problems for 1, 32 and all
problems of a live batch beside mhpc_initialize of the same handle, at batch 64 and 4096.

Case: C3, one parameter set.  The handle is initialised, solved, stepped once
(mhpc_update_problem, so the phase-buffer store exists and a reset clears its rows too) and
solved again; then each call is repeated on that state (a reset is idempotent and leaves the
call-order flags alone), mhpc_initialize last (it drops the store).  Both are called through the
C ABI directly, with the index list and x0 rows prepared once.

Reported per batch and call, median and min / max over the repeats:
  wall_ms    host wall time of the call, profiling off
  device_ms  the call's launches by HIP events (mhpc_set_profiling, the k_init row of
             mhpc_get_kernel_stats), in a second pass.  For a reset that is the x0 scatter, k_init
             and (with several sets) k_init_params on the main stream plus the list-driven
             memory_reset, which runs beside them on the second stream: their sum, an upper bound
             of the critical path.  For mhpc_initialize it is k_init alone: its batch-wide
             k_reset_arrays on the second stream is not bracketed.
  host_ms    wall_ms - device_ms: validation, plan_groups (a map over the batch's
             descriptors), the uploads of the group table, the grouped order and the list, the
             stream synchronisations.  An estimate: the device sum counts overlapped launches
             twice, so it can exceed the wall time of a reset of many problems.
and the growth of a one-problem reset's device part from batch 64 to 4096 beside the run-to-run
spread (max - min) of mhpc_initialize's device part: a reset launch that still walks the whole
batch would show there.  Recorded, not gated.  Fails without a GPU.

usage: python tools/reset_timing.py [--batches 64 4096] [--repeats 21] [--out FILE.json]
(FILE.md is written beside it)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def measure(batch, repeats, warmup):
    from mhpc_minimal_env_amd import capi, configs, locomotion as L
    lib = capi.lib()
    desc = configs.c3_desc()
    gait = L.Gait(L.GaitType2D.PRONK)
    loco = L.MHPCLocomotion(desc=desc, gait=gait, option=L.HSDDP_OPTION(), batch=batch, device=0)
    x0 = configs.x0_for(desc, batch)
    loco.set_initial_condition(x0)
    loco.initialization()
    loco.solve_mhpc()
    loco.update_problem()
    loco.solve_mhpc()

    calls = {}
    for n in sorted({1, min(32, batch), batch}):
        pr = np.ascontiguousarray(np.linspace(0, batch - 1, n).astype(np.int32))
        rows = np.ascontiguousarray(x0[pr])
        calls[f"reset_{n if n < batch else 'all'}"] = (
            lambda pr=pr, rows=rows: lib.mhpc_reset_problems(loco._h, int(pr.size), capi.iptr(pr),
                                                             capi.dptr(rows), 0, None, None))
    calls["initialize"] = lambda: lib.mhpc_initialize(loco._h)  # last: it drops the store

    def k_init_ms():
        return loco.kernel_stats()["k_init"]["ms"]

    out = {}
    for name, call in calls.items():
        wall, dev = [], []
        loco.set_profiling(False)
        for i in range(warmup + repeats):
            t = time.perf_counter()
            capi.check(call(), name)
            if i >= warmup:
                wall.append(1e3 * (time.perf_counter() - t))
        loco.set_profiling(True)
        for i in range(warmup + repeats):
            before = k_init_ms()
            capi.check(call(), name)
            if i >= warmup:
                dev.append(k_init_ms() - before)
        loco.set_profiling(False)
        out[name] = {"wall_ms": stats(wall), "device_ms": stats(dev),
                     "host_ms": float(np.median(wall) - np.median(dev))}
    loco.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 4096])
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        sys.exit("reset_timing: no GPU visible")
    res = {"case": {"config": "C3", "param_sets": 1, "state": "initialize, solve, update_problem, solve",
                    "repeats": a.repeats, "warmup": a.warmup},
           "compute_units": torch.cuda.get_device_properties(0).multi_processor_count,
           "batch": {str(b): measure(b, a.repeats, a.warmup) for b in a.batches}}
    lo, hi = str(min(a.batches)), str(max(a.batches))
    ini = res["batch"][hi]["initialize"]["device_ms"]
    res["reset_1_device_growth_ms"] = (res["batch"][hi]["reset_1"]["device_ms"]["median"] -
                                       res["batch"][lo]["reset_1"]["device_ms"]["median"])
    res["initialize_device_spread_ms"] = ini["max"] - ini["min"]
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
        md = ["# mhpc_reset_problems beside mhpc_initialize (tools/reset_timing.py)", "",
              f"C3, one parameter set, {a.repeats} repeats; median [min .. max] in ms.  device = the",
              "call's launches by HIP events (a reset: their sum, the memory_reset overlaps the warm",
              "start; initialize: k_init alone), host = wall - device (an estimate: below zero where",
              "the overlapped launches sum to more than the call lasts).", "",
              "| batch | call | wall | device | host |", "|---|---|---|---|---|"]
        for b, calls in res["batch"].items():
            for name, r in calls.items():
                w, d = r["wall_ms"], r["device_ms"]
                md.append(f"| {b} | {name} | {w['median']:.3f} [{w['min']:.3f} .. {w['max']:.3f}] | "
                          f"{d['median']:.3f} [{d['min']:.3f} .. {d['max']:.3f}] | {r['host_ms']:.3f} |")
        md += ["", f"Device part of a one-problem reset, batch {lo} -> {hi}: "
               f"{res['reset_1_device_growth_ms']:+.3f} ms; run-to-run spread of mhpc_initialize's "
               f"device part at batch {hi}: {res['initialize_device_spread_ms']:.3f} ms."]
        with open(os.path.splitext(a.out)[0] + ".md", "w") as f:
            f.write("\n".join(md) + "\n")


if __name__ == "__main__":
    main()
