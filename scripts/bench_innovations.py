"""One-step-ahead innovations (BatchedKalman.innovations, C ABI mk_innovations) and their whiteness statistics
(innovation_stats, mk_innovation_stats): device-event times, warmed up, over --reps repetitions, at
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The call's two kernels are timed separately by the library's own hipEvents (the recording forward pass in the filter slot,
innov_step_kernel in the smoother slot; accumulated over the repetitions, no host synchronisation in between), the statistics
kernel and the whole calls by events on the stream -- beside loglik, the filter with both record sets, loglik_grad (narrow)
and simulate_smoothed of the same batch in the same process.  Also printed: the step kernel's achieved read bandwidth, the
B T rs 8 bytes of filtered records it reads over its time.  Prints one JSON line.  --once: one call per shape and nothing
else (for a kernel trace).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_loo import SHAPES, timed  # noqa: E402  (the batches and the event timer of the leave-one-out benchmark)


def run_shape(which, warmup, reps, once):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    bufs = kf.alloc_innovations(B)
    if once:
        kf.innovations(phi, q, buffers=bufs)
        kf.innovation_stats(bufs["v"], bufs["f"])
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    rs = int(bufs["_work"].shape[2])
    out = {"shape": [B, N, K, T], "missing": missing, "cells": B * T * N, "record_stride": rs,
           "record_bytes": B * T * rs * 8}
    out["innovations"] = timed(lambda: kf.innovations(phi, q, buffers=bufs), warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    # the two kernels of the call, by the library's events, accumulated over the same number of calls
    kf.enable_timing(True, accumulate=True)
    kf.kernel_ms_totals()
    for _ in range(reps):
        kf.innovations(phi, q, buffers=bufs)
    torch.cuda.synchronize()
    f_ms, nf, s_ms, ns = kf.kernel_ms_totals()
    kf.enable_timing(False)
    out["recording_pass_ms"] = round(f_ms / nf, 3)
    out["step_kernel_ms"] = round(s_ms / ns, 3)
    out["step_kernel_read_GBps"] = round(out["record_bytes"] / (s_ms / ns * 1e-3) / 1e9, 1)
    out["step_over_recording"] = round((s_ms / ns) / (f_ms / nf), 3)
    out["stats"] = timed(lambda: kf.innovation_stats(bufs["v"], bufs["f"], nlags=10, t_first=1), warmup, reps)
    del bufs
    torch.cuda.empty_cache()
    out["loglik"] = timed(lambda: kf.loglik(phi, q), warmup, reps)
    fb = kf._alloc_outputs(B, ("F", "Pf", "Xp", "Pp"))
    out["filter_records"] = timed(lambda: kf.filter(phi, q, buffers=fb), warmup, reps)
    del fb
    torch.cuda.empty_cache()
    if which == "narrow":   # as in bench_loo.py: the wide batch's gradient workspace (records + update tape) is not allocated here
        out["loglik_grad"] = timed(lambda: kf.loglik_grad(phi, q), warmup, reps)
        kf._grad_work = kf._grad_upd = None
        torch.cuda.empty_cache()
    pb = kf.alloc_projection(B)
    out["simulate_smoothed"] = timed(lambda: kf.simulate_smoothed(phi, q, buffers=pb), warmup, reps)
    del pb
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "innovations", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
