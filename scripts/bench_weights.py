"""Observation weights of smoothed series (BatchedKalman.observation_weights, C ABI mk_observation_weights): device-event times,
warmed up, over --reps repetitions, with M = 8 targets per model spread over the record, at
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The library's own hipEvents give the recording forward pass (filter slot) and the clear of the gain tape + the gain writer
(innov_step_kernel with its tape output) + weights_walk_kernel together (smoother slot).  The three are told apart in two ways:
by DIFFERENCE -- the same call with 2 M targets costs one more walk of M targets, so walk(M) = slot(2M) - slot(M) and clear +
writer = 2 slot(M) - slot(2M) -- and, where torch's profiler sees the library's kernels, by the per-kernel device times it
reports.  Beside them, in the same process: innovations (innov_step_kernel writing v and f) and simulate_smoothed (the filter
and the projecting smoother: M targets of a model cost about as much as how many whole smoothing passes?).  Also printed: the
bytes of tape the walks read (each target reads its instance's tape twice, forward from its step and backward over the whole
record) over the walk's time.  Prints one JSON line.  --once: one call per shape and nothing else (for a kernel trace);
--models: a smaller batch.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_forecast import kernels_ms  # noqa: E402  (the library's event timer, accumulated over the repetitions)
from bench_loo import SHAPES, timed  # noqa: E402  (the batches and the event timer of the leave-one-out benchmark)


def profiled_kernels(call, reps):
    """name -> mean device ms per call of every kernel torch's profiler attributes to ``reps`` calls, or None where it cannot."""
    try:
        import torch
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(reps):
                call()
            torch.cuda.synchronize()
        out = {}
        for e in prof.key_averages():
            us = getattr(e, "device_time_total", None)
            if us is None:
                us = getattr(e, "cuda_time_total", 0.0)
            if us:
                out[e.key[:60]] = round(us / 1e3 / reps, 3)
        return out or None
    except Exception as err:   # a profiler that is not there is not this script's business
        return {"unavailable": str(err)[:120]}


def run_shape(which, warmup, reps, once, M, models):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    B = min(B, models) if models else B
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]

    def targets(m):   # spread over the record, over the series
        return torch.tensor([[(2 * i + 1) * T // (2 * m), i % N] for i in range(m)], dtype=torch.int64)

    bufs = kf.alloc_observation_weights(B, M)
    call = lambda: kf.observation_weights(phi, q, targets(M), buffers=bufs)  # noqa: E731
    if once:
        call()
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    n = N + K
    rs, ws = int(kf._L.mk_record_stride(n)), int(kf._L.mk_weights_work_stride(N, K))
    gs = (n + 3) & ~1
    tape_bytes = B * T * N * gs * 8
    out = {"shape": [B, N, K, T], "missing": missing, "targets_per_model": M, "record_stride": rs, "work_stride": ws,
           "record_bytes": B * T * rs * 8, "tape_bytes": tape_bytes}
    out["observation_weights"] = timed(call, warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    f_ms, s_ms = kernels_ms(kf, call, reps)
    out["recording_pass_ms"] = round(f_ms, 3)
    out["clear_writer_walk_ms"] = round(s_ms, 3)
    out["profiled_kernels_ms"] = profiled_kernels(call, max(1, reps // 4))
    del bufs
    torch.cuda.empty_cache()
    bufs2 = kf.alloc_observation_weights(B, 2 * M)
    call2 = lambda: kf.observation_weights(phi, q, targets(2 * M), buffers=bufs2)  # noqa: E731
    for _ in range(warmup):
        call2()
    _, s2_ms = kernels_ms(kf, call2, reps)
    del bufs2
    torch.cuda.empty_cache()
    walk_ms = s2_ms - s_ms
    out["clear_writer_walk_2M_ms"] = round(s2_ms, 3)
    out["walk_ms_by_difference"] = round(walk_ms, 3)
    out["clear_and_gain_writer_ms_by_difference"] = round(2.0 * s_ms - s2_ms, 3)
    # every target reads its instance's tape once backward over the whole record and once forward from its own step
    fwd = sum((T - int(t)) for t, _ in targets(M).tolist()) / float(T)
    out["walk_tape_bytes_read"] = int(tape_bytes * (M + fwd))
    out["walk_tape_read_GBps"] = round(out["walk_tape_bytes_read"] / (walk_ms * 1e-3) / 1e9, 1) if walk_ms > 0 else None
    out["walk_cell_steps_per_s"] = round(B * M * T * N * (1.0 + fwd / M) / (walk_ms * 1e-3), 1) if walk_ms > 0 else None
    ib = kf.alloc_innovations(B, ("v", "f"))
    inn = lambda: kf.innovations(phi, q, buffers=ib, outputs=("v", "f"))  # noqa: E731
    out["innovations"] = timed(inn, warmup, reps)
    _, i_ms = kernels_ms(kf, inn, reps)
    out["innov_step_kernel_ms"] = round(i_ms, 3)
    del ib
    torch.cuda.empty_cache()
    pb = kf.alloc_projection(B)
    sim = lambda: kf.simulate_smoothed(phi, q, buffers=pb)  # noqa: E731
    out["simulate_smoothed"] = timed(sim, warmup, reps)
    sf_ms, ss_ms = kernels_ms(kf, sim, reps)
    out["simulate_smoothed_filter_ms"], out["simulate_smoothed_smoother_ms"] = round(sf_ms, 3), round(ss_ms, 3)
    out["weights_call_over_simulate_smoothed"] = round(out["observation_weights"]["median_ms"] / out["simulate_smoothed"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--targets", type=int, default=8, help="M, targets per model")
    ap.add_argument("--models", type=int, default=0, help="cap on the number of models (0: the configuration's own)")
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "observation_weights", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.targets, a.models)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
