"""Multi-step-ahead forecasts and forecast skill (BatchedKalman.forecast, C ABI mk_forecast): device-event times, warmed up,
over --reps repetitions, at horizon H = 14 and
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The kernels are timed by the library's own hipEvents (the recording forward pass in the filter slot, the forecast kernels in
the smoother slot; accumulated over the repetitions, no host synchronisation in between): one series of calls asks for the
fan and the track (forecast_path_kernel alone), one for the skill table (forecast_skill_kernel + the reduction over the
chunks) -- beside innovations (innov_step_kernel) of the same batch in the same process.  Also printed: the achieved read
bandwidth of each kernel against the B T rs 8 bytes of filtered records.  Prints one JSON line.  --once: one call per shape and
nothing else (for a kernel trace).
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


def kernels_ms(kf, call, reps):
    """(filter slot ms, smoother slot ms) per call, by the library's events accumulated over ``reps`` calls."""
    import torch

    kf.enable_timing(True, accumulate=True)
    kf.kernel_ms_totals()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    f_ms, nf, s_ms, ns = kf.kernel_ms_totals()
    kf.enable_timing(False)
    return f_ms / nf, s_ms / ns


def run_shape(which, warmup, reps, once, horizon):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    bufs = kf.alloc_forecast(B, horizon, ("fan", "track", "skill"))
    path = lambda: kf.forecast(phi, q, horizon=horizon, outputs=("fan", "track"), track_horizon=horizon, buffers=bufs)  # noqa: E731
    skill = lambda: kf.forecast(phi, q, horizon=horizon, outputs=("skill",), buffers=bufs)  # noqa: E731
    if once:
        path()
        skill()
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 2}
    rs = int(kf._L.mk_record_stride(N + K))
    out = {"shape": [B, N, K, T], "missing": missing, "horizon": horizon, "record_stride": rs, "record_bytes": B * T * rs * 8}
    out["forecast_path"] = timed(path, warmup, reps)
    out["forecast_skill"] = timed(skill, warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    f_ms, p_ms = kernels_ms(kf, path, reps)
    out["recording_pass_ms"] = round(f_ms, 3)
    out["path_kernel_ms"] = round(p_ms, 3)
    _, s_ms = kernels_ms(kf, skill, reps)
    out["skill_kernel_ms"] = round(s_ms, 3)
    out["path_kernel_read_GBps"] = round(out["record_bytes"] / (p_ms * 1e-3) / 1e9, 1)
    out["skill_kernel_read_GBps"] = round(out["record_bytes"] / (s_ms * 1e-3) / 1e9, 1)
    del bufs
    torch.cuda.empty_cache()
    ib = kf.alloc_innovations(B)
    out["innovations"] = timed(lambda: kf.innovations(phi, q, buffers=ib), warmup, reps)
    _, i_ms = kernels_ms(kf, lambda: kf.innovations(phi, q, buffers=ib), reps)
    out["innov_step_kernel_ms"] = round(i_ms, 3)
    out["skill_over_innov_step"] = round(s_ms / i_ms, 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--horizon", type=int, default=14)
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "forecast", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.horizon)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
