"""Per-step scores by the tangent filter (BatchedKalman.scores, C ABI mk_scores): device-event times, warmed up, over --reps
repetitions, at
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The library's own hipEvents give the recording forward pass (filter slot) and the clear of the gain tape + the gain writer
(innov_step_kernel writing the tape and v) + score_tangent_kernel + score_stats_kernel together (smoother slot); torch's profiler,
where it sees the library's kernels, tells the four apart by their device times.  Beside them, in the same process, the same
batch's loglik_grad (the adjoint gradient: what the total of the scores costs when the steps are not wanted) and innovations
(innov_step_kernel writing v and f), and 2 n times the measured innovations call: what central differences of the per-step
contributions would cost.  Prints one JSON line.  --once: one call per shape and nothing else (for a kernel trace); --models: a
smaller batch.
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


def run_shape(which, warmup, reps, once, models):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    B = min(B, models) if models else B
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q, alpha = d["phi"], d["q"], d["alpha"]
    n = N + K
    c = torch.cat([1.0 - (d["loadings"] ** 2).sum(2), torch.ones((B, K), dtype=torch.float64, device=phi.device)], 1)
    dphi = phi / (alpha * alpha)
    dq = -2.0 * phi * dphi * c
    bufs = kf.alloc_scores(B)
    call = lambda: kf.scores(phi, q, dphi, dq, buffers=bufs)  # noqa: E731
    if once:
        call()
        torch.cuda.synchronize()
        return {"shape": [B, N, K, T], "calls": 1}
    rs, ws = int(kf._L.mk_record_stride(n)), int(kf._L.mk_scores_work_stride(N, K))
    tape_bytes = B * T * N * ((n + 3) & ~1) * 8
    out = {"shape": [B, N, K, T], "missing": missing, "parameters": n, "record_stride": rs, "work_stride": ws,
           "record_bytes": B * T * rs * 8, "tape_bytes": tape_bytes, "tangent_groups": B * n}
    out["scores"] = timed(call, warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    f_ms, s_ms = kernels_ms(kf, call, reps)
    out["recording_pass_ms"] = round(f_ms, 3)
    out["clear_writer_tangent_stats_ms"] = round(s_ms, 3)
    out["profiled_kernels_ms"] = profiled_kernels(call, max(1, reps // 2))
    del bufs
    torch.cuda.empty_cache()
    if kf.has_adjoint():
        grad = lambda: kf.loglik_grad(phi, q)  # noqa: E731
        out["loglik_grad"] = timed(grad, warmup, reps)
        out["scores_call_over_loglik_grad"] = round(out["scores"]["median_ms"] / out["loglik_grad"]["median_ms"], 2)
    ib = kf.alloc_innovations(B, ("v", "f"))
    inn = lambda: kf.innovations(phi, q, buffers=ib, outputs=("v", "f"))  # noqa: E731
    out["innovations"] = timed(inn, warmup, reps)
    _, i_ms = kernels_ms(kf, inn, reps)
    out["innov_step_kernel_ms"] = round(i_ms, 3)
    out["central_differences_2n_innovations_ms"] = round(2 * n * out["innovations"]["median_ms"], 1)
    out["scores_call_over_central_differences"] = round(out["scores"]["median_ms"] / (2 * n * out["innovations"]["median_ms"]), 3)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", type=int, default=0, help="cap on the number of models (0: the configuration's own)")
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "scores", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.models)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
