"""Smoothed state disturbances (BatchedKalman.disturbances, C ABI mk_disturbances): device-event time of one call, warmed up,
over --reps repetitions, and state-steps/s -- beside loglik_grad, the same recording forward pass and the same backward walk with
the parameter sums instead of the two stores, on the same batch:
  narrow  configs[1]'s workload, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s workload, 4096 x (32, 4), T = 2000, 30 % missing
Prints one JSON line.  --grad-only: loglik_grad alone -- uses nothing this entry point added, so the same file runs on the commit
before it (the ratio quoted in DESIGN.md is against THAT figure).  --once: one call per shape and nothing else (for a kernel
trace: rocprofv3 --kernel-trace --stats).
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


def run_shape(which, warmup, reps, once, grad_only):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    out = {"shape": [B, N, K, T], "missing": missing, "state_steps": B * T * (N + K)}
    if not grad_only:
        bufs = kf.alloc_disturbances(B)
        if once:
            kf.disturbances(phi, q, buffers=bufs)
            torch.cuda.synchronize()
            return {"shape": [B, N, K, T], "calls": 1}
        out["disturbances"] = timed(lambda: kf.disturbances(phi, q, buffers=bufs), warmup, reps)
        out["disturbances"]["state_steps_per_s"] = round(out["state_steps"] / (out["disturbances"]["median_ms"] * 1e-3), 1)
        assert int(bufs["status"].abs().sum().item()) == 0
        del bufs
        torch.cuda.empty_cache()
    if once:
        kf.loglik_grad(phi, q)
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    out["loglik_grad"] = timed(lambda: kf.loglik_grad(phi, q), warmup, reps)
    if not grad_only:
        out["disturbances_over_loglik_grad"] = round(out["disturbances"]["median_ms"] / out["loglik_grad"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--grad-only", action="store_true", help="loglik_grad alone (runs on the commit before mk_disturbances too)")
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "loglik_grad" if a.grad_only else "disturbances", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.grad_only)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
