"""Residual diagnostics (BatchedKalman.residual_series / residual_cross, C ABI mk_residual_series / mk_residual_cross):
device-event times of the two kernels, warmed up, over --reps repetitions, on the innovations of
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
with nlags = 10 and t_first = 1 -- beside innov_stats_kernel (innovation_stats, nlags = 10) on the same v / f buffers in the same
process.  Also printed: the bytes of v and f one pass reads (16 B T N) and the rate each kernel would need to read them once.
Prints one JSON line.  --once: one call of each kernel per shape and nothing else (for a kernel trace).
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


def run_shape(which, warmup, reps, once, nlags):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    bufs = kf.alloc_innovations(B, outputs=("v", "f"))
    kf.innovations(d["phi"], d["q"], buffers=bufs, outputs=("v", "f"))
    assert int(bufs["status"].abs().sum().item()) == 0
    v, f = bufs["v"], bufs["f"]
    del bufs   # the forward pass's workspace is not needed any more
    torch.cuda.empty_cache()
    stats = kf.residual_series(v, f, t_first=1)
    if once:
        kf.residual_cross(v, f, stats, nlags=nlags, t_first=1)
        kf.innovation_stats(v, f, nlags=nlags, t_first=1)
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    out = {"shape": [B, N, K, T], "missing": missing, "cells": B * T * N, "nlags": nlags, "cell_bytes": 16 * B * T * N}
    out["series"] = timed(lambda: kf.residual_series(v, f, t_first=1), warmup, reps)
    out["cross"] = timed(lambda: kf.residual_cross(v, f, stats, nlags=nlags, t_first=1), warmup, reps)
    out["innov_stats"] = timed(lambda: kf.innovation_stats(v, f, nlags=nlags, t_first=1), warmup, reps)
    for key in ("series", "cross", "innov_stats"):
        out[key]["cell_bytes_GBps"] = round(out["cell_bytes"] / (out[key]["median_ms"] * 1e-3) / 1e9, 1)
    out["series_over_innov_stats"] = round(out["series"]["median_ms"] / out["innov_stats"]["median_ms"], 3)
    # the cross kernel's work: two LDS reads and one multiply-add per (lag, i, j, step of every tile)
    tiles = -(-T // 64)
    fma = B * (nlags + 1) * N * N * tiles * 64
    out["cross"]["fma_per_s"] = round(fma / (out["cross"]["median_ms"] * 1e-3), 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--nlags", type=int, default=10)
    ap.add_argument("--once", action="store_true", help="one call per kernel and shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "residuals", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.nlags)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
