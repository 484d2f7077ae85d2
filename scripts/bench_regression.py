"""Intervention effects by GLS (BatchedKalman.regression, C ABI mk_regression): device-event times, warmed up, over --reps
repetitions, with M = 8 effects per model (pulses, temporary offsets, permanent shifts and ramps spread over the record and the
series), at
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The library's own hipEvents give the recording forward pass (filter slot) and the clear of the gain tape + the gain writer
(innov_step_kernel with its tape output) + regress_replay_kernel together (smoother slot).  The three are told apart in two
ways: by DIFFERENCE -- observation_weights spends the same clear and the same writer, and with 2 M targets one more walk of M
targets, so clear + writer = 2 slot_w(M) - slot_w(2M) and replay = slot - (clear + writer) -- and, where torch's profiler sees the
library's kernels, by the per-kernel device times it reports.  Beside them, in the same process: innovations (innov_step_kernel
writing v and f) and simulate_smoothed (the filter and the projecting smoother).  Also printed: the bytes of tape the replay
reads (once) over its time, and adjust_observations.  Prints one JSON line.  --once: one call per shape and nothing else (for a
kernel trace); --models: a smaller batch.
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
from bench_weights import profiled_kernels  # noqa: E402


def effects(M, T, N):
    """[M,4]: in turn a pulse, a temporary offset, a permanent shift and a ramp that holds, spread over the record and the series."""
    import torch

    rows = []
    for i in range(M):
        t0 = (2 * i + 1) * T // (2 * M)
        kind, t1 = [(0, t0 + 1), (0, min(T, t0 + T // (4 * M) + 2)), (0, T), (1, min(T, t0 + T // (4 * M) + 2))][i % 4]
        rows.append((i % N, kind, t0, t1))
    return torch.tensor(rows, dtype=torch.int64)


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
    ef = effects(M, T, N)
    bufs = kf.alloc_regression(B, M)
    call = lambda: kf.regression(phi, q, ef, buffers=bufs)  # noqa: E731
    if once:
        call()
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    n = N + K
    rs, ws = int(kf._L.mk_record_stride(n)), int(kf._L.mk_regression_work_stride(N, K))
    tape_bytes = B * T * N * ((n + 3) & ~1) * 8
    out = {"shape": [B, N, K, T], "missing": missing, "effects_per_model": M, "record_stride": rs, "work_stride": ws,
           "record_bytes": B * T * rs * 8, "tape_bytes": tape_bytes}
    out["regression"] = timed(call, warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    out["effects_dropped"] = int((bufs["dropped"] != 0).sum().item())
    f_ms, s_ms = kernels_ms(kf, call, reps)
    out["recording_pass_ms"] = round(f_ms, 3)
    out["clear_writer_replay_ms"] = round(s_ms, 3)
    out["profiled_kernels_ms"] = profiled_kernels(call, max(1, reps // 4))
    beta = bufs["beta"][: kf.R].clone()
    adj = lambda: kf.adjust_observations(ef, beta)  # noqa: E731
    out["adjust_observations"] = timed(adj, warmup, reps)
    kf.unadjust_observations()
    del bufs
    torch.cuda.empty_cache()

    def targets(m):
        return torch.tensor([[(2 * i + 1) * T // (2 * m), i % N] for i in range(m)], dtype=torch.int64)

    slots = []
    for m in (M, 2 * M):   # the clear and the gain writer by difference, from the weights' calls
        wb = kf.alloc_observation_weights(B, m)
        wcall = lambda: kf.observation_weights(phi, q, targets(m), buffers=wb)  # noqa: E731
        for _ in range(warmup):
            wcall()
        slots.append(kernels_ms(kf, wcall, reps)[1])
        del wb
        torch.cuda.empty_cache()
    clear_writer = 2.0 * slots[0] - slots[1]
    replay_ms = s_ms - clear_writer
    out["clear_and_gain_writer_ms_by_difference"] = round(clear_writer, 3)
    out["replay_ms_by_difference"] = round(replay_ms, 3)
    out["replay_tape_read_GBps"] = round(tape_bytes / (replay_ms * 1e-3) / 1e9, 1) if replay_ms > 0 else None
    out["replay_cell_columns_per_s"] = round(B * T * N * (M + 1) / (replay_ms * 1e-3), 1) if replay_ms > 0 else None
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
    out["regression_call_over_simulate_smoothed"] = round(out["regression"]["median_ms"] / out["simulate_smoothed"]["median_ms"], 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--effects", type=int, default=8, help="M, effects per model")
    ap.add_argument("--models", type=int, default=0, help="cap on the number of models (0: the configuration's own)")
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "regression", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.effects, a.models)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
