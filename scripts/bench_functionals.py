"""Exact window means (BatchedKalman.functionals, C ABI mk_functionals): device-event times, warmed up, over --reps repetitions,
with monthly windows (30 steps each, W = T // 30) and the N unit contrasts, at
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The library's own hipEvents give the recording forward pass (filter slot) and the smoother + functional_walk_kernel together
(smoother slot, two launches).  The two are told apart by DIFFERENCE: mk_filter_smooth into the same two record sets, in the same
process, spends the same forward pass and the same smoother, so walk = slot(functionals) - slot(filter_smooth).  Beside them:
draw_window_statistics at --draws draws (what the sd of a window mean cost before), and for model 0, series 0 the exact sd of every
window mean beside the sd of the draws' window means.  Prints one JSON line.  --once: one call per shape and nothing else (for a
kernel trace); --models: a smaller batch; --draws 0: no draws.
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


def slots_ms(kf, call, reps):
    """(filter slot ms, smoother slot ms) PER CALL, by the library's events accumulated over ``reps`` calls (a call may launch
    more than one kernel into a slot)."""
    import torch

    kf.enable_timing(True, accumulate=True)
    kf.kernel_ms_totals()
    for _ in range(reps):
        call()
    torch.cuda.synchronize()
    f_ms, _, s_ms, _ = kf.kernel_ms_totals()
    kf.enable_timing(False)
    return f_ms / reps, s_ms / reps


def run_shape(which, warmup, reps, once, models, draws):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    B = min(B, models) if models else B
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    W = T // 30
    wins = torch.tensor([(30 * w, 30 * (w + 1), 0, 0) for w in range(W)], dtype=torch.int64)
    bufs = kf.alloc_functionals(B, W, N)
    call = lambda: kf.functionals(phi, q, wins, buffers=bufs)  # noqa: E731
    if once:
        call()
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    rs = int(kf._L.mk_record_stride(N + K))
    out = {"shape": [B, N, K, T], "missing": missing, "windows": W, "contrasts": N, "walks": B * W, "record_stride": rs,
           "record_bytes_both_sets": 2 * B * T * rs * 8}
    out["functionals"] = timed(call, warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    f_ms, s_ms = slots_ms(kf, call, reps)
    out["recording_pass_ms"] = round(f_ms, 3)
    out["smoother_and_walk_ms"] = round(s_ms, 3)
    exact_sd = bufs["var"][0, :, 0].sqrt().cpu().numpy()
    del bufs
    torch.cuda.empty_cache()
    # mk_filter_smooth into the same two record sets (filtered and smoothed records, no predicted ones)
    res = {"mle": torch.empty(B, dtype=torch.float64, device=kf.device), "status": torch.zeros(B, dtype=torch.int32, device=kf.device),
           "sigmacount": torch.empty(B, dtype=torch.int64, device=kf.device), "_rs": rs}
    res["_rec_filt"], res["F"], res["Pf"], res["sigmas"], res["detfs"] = kf._alloc_records(B)
    res["_rec_smooth"], res["S"], res["Ps"], _, _ = kf._alloc_records(B)
    fs = lambda: kf.filter_smooth(phi, q, warmup=0, buffers=res)  # noqa: E731
    out["filter_smooth"] = timed(fs, warmup, reps)
    ff_ms, fs_ms = slots_ms(kf, fs, reps)
    out["filter_smooth_filter_ms"], out["filter_smooth_smoother_ms"] = round(ff_ms, 3), round(fs_ms, 3)
    walk_ms = s_ms - fs_ms
    out["walk_ms_by_difference"] = round(walk_ms, 3)
    out["walk_over_smoother"] = round(walk_ms / fs_ms, 3)
    out["walk_records_read_GBps"] = round(out["record_bytes_both_sets"] / (walk_ms * 1e-3) / 1e9, 1) if walk_ms > 0 else None
    out["functionals_call_over_filter_smooth"] = round(out["functionals"]["median_ms"] / out["filter_smooth"]["median_ms"], 3)
    del res
    torch.cuda.empty_cache()
    if draws:
        steps = wins[:, :2].numpy().copy()
        dr = lambda: kf.draw_window_statistics(phi, q, draws, steps)  # noqa: E731
        out["draw_window_statistics"] = dict(timed(dr, 1, max(1, reps // 5)), draws=draws)
        summary = dr()["summary"]          # [R,N,W,5,5+P]: functional 0 = mean, statistic 2 = sd
        out["model0_series0_exact_sd"] = [round(float(v), 5) for v in exact_sd]
        out["model0_series0_draws_sd"] = [round(float(v), 5) for v in summary[0, 0, :, 0, 2].cpu().numpy()]
        out["draws_over_functionals"] = round(out["draw_window_statistics"]["median_ms"] / out["functionals"]["median_ms"], 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--draws", type=int, default=200, help="draws of draw_window_statistics (0: skip)")
    ap.add_argument("--models", type=int, default=0, help="cap on the number of models (0: the configuration's own)")
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "functionals", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.models, a.draws)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
