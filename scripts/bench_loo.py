"""Leave-one-out predictions (BatchedKalman.loo_predict, C ABI mk_loo): device-event time of one call, warmed up, over
--reps repetitions, and cells/s -- beside the two backward walks it shares its structure with, timed in the same process on
the same batch:
  narrow  configs[1]'s workload, 4096 x (8 series, 2 factors), T = 1000: loglik_grad (the same record filter + adjoint walk,
          with the parameter sums) and simulate_smoothed (filter + projecting smoother)
  wide    configs[3]'s workload, 4096 x (32, 4), T = 2000, 30 % missing: simulate_smoothed (the same tape, the projection)
Prints one JSON line.  --once: one LOO call per shape and nothing else (for a kernel trace: rocprofv3 --kernel-trace --stats).
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SHAPES = {"narrow": (4096, 8, 2, 1000, 0.0), "wide": (4096, 32, 4, 2000, 0.3)}


def timed(fn, warmup, reps):
    """Median / min of per-call device-event times (ms)."""
    import torch

    for _ in range(warmup):
        fn()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in ev]
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "reps": reps}


def run_shape(which, warmup, reps, once):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    bufs = kf.alloc_loo(B)
    if once:
        kf.loo_predict(phi, q, buffers=bufs)
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    out = {"shape": [B, N, K, T], "missing": missing, "cells": B * T * N}
    out["loo"] = timed(lambda: kf.loo_predict(phi, q, buffers=bufs), warmup, reps)
    out["loo"]["cells_per_s"] = round(out["cells"] / (out["loo"]["median_ms"] * 1e-3), 1)
    assert int(bufs["status"].abs().sum().item()) == 0
    del bufs
    torch.cuda.empty_cache()
    if which == "narrow":
        out["loglik_grad"] = timed(lambda: kf.loglik_grad(phi, q), warmup, reps)
        out["loo_over_loglik_grad"] = round(out["loo"]["median_ms"] / out["loglik_grad"]["median_ms"], 3)
        kf._grad_work = kf._grad_upd = None
        torch.cuda.empty_cache()
    pb = kf.alloc_projection(B)
    out["simulate_smoothed"] = timed(lambda: kf.simulate_smoothed(phi, q, buffers=pb), warmup, reps)
    out["simulate_smoothed"]["tape_path"] = bool(pb.get("_tape", False))
    out["loo_over_simulate_smoothed"] = round(out["loo"]["median_ms"] / out["simulate_smoothed"]["median_ms"], 3)
    del pb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one LOO call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "loo_predict", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
