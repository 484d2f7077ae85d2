"""The level-shift scan (BatchedKalman.level_shifts, C ABI mk_level_shifts): device-event times, warmed up, over --reps
repetitions, at
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The workspace (records, gain tape, innovations) of the wide batch is 21 KB per (model, step), so its models are taken in chunks
(--chunk, default 4096 narrow / 1024 wide); the figures are per chunk and, scaled by the number of chunks, per batch.  The three
stages are timed separately: the recording forward pass by the library's own hipEvents (filter slot); the clear of the tape + the
gain writer and shift_scan_kernel by the per-kernel device times of torch's profiler (their sum is the library's smoother slot,
printed beside them).  In the same process, on the same chunk: block_predict with one block per model, for the time of
block_checkpoint_kernel -- the same (r, N) walk without the Omega work -- and loo_predict and simulate_smoothed.  Prints one JSON
line.  --once: one call per shape and nothing else (for a kernel trace); --models: a smaller batch.
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

CHUNK = {"narrow": 4096, "wide": 1024}


def run_shape(which, warmup, reps, once, models, chunk):
    import torch

    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, N, K, T, missing = SHAPES[which]
    B = min(B, models) if models else B
    C = min(B, chunk or CHUNK[which])
    d = make_dfm_batch_torch(C, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    bufs = kf.alloc_level_shifts(C)
    call = lambda: kf.level_shifts(phi, q, buffers=bufs)  # noqa: E731
    if once:
        call()
        torch.cuda.synchronize()
        return {"shape": [C, N, K, T], "calls": 1}
    chunks = -(-B // C)
    out = {"shape": [B, N, K, T], "missing": missing, "models_per_chunk": C, "chunks_per_batch": chunks,
           "work_stride": int(kf._L.mk_shift_work_stride(N, K)), "output_bytes_per_chunk": 2 * C * T * N * 8}
    out["level_shifts"] = timed(call, warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    seen = torch.isfinite(kf.obs)
    assert bool((torch.isfinite(bufs["num"]) == seen).all()) and bool((bufs["den"][seen] > 0).all())
    out["candidates_per_chunk"] = int(seen.sum().item())
    f_ms, s_ms = kernels_ms(kf, call, reps)
    out["recording_pass_ms"] = round(f_ms, 3)
    out["clear_writer_scan_ms"] = round(s_ms, 3)
    pick = lambda prof, *words: round(sum(v for k, v in prof.items() if any(w in k for w in words)), 3)  # noqa: E731
    prof = profiled_kernels(call, max(1, reps // 4))
    out["profiled_kernels_ms"] = prof
    if prof and "unavailable" not in prof:
        out["clear_and_gain_writer_ms"] = pick(prof, "innov_step_kernel", "Memset", "memset", "fill")
        out["shift_scan_kernel_ms"] = pick(prof, "shift_scan_kernel")
    out["level_shifts_batch_ms"] = round(out["level_shifts"]["median_ms"] * chunks, 3)
    out["candidates_per_s"] = round(out["candidates_per_chunk"] / (out["level_shifts"]["median_ms"] * 1e-3), 1)
    del bufs
    torch.cuda.empty_cache()
    # the same walk without the Omega work: the checkpoint kernel of block_predict, one block per model
    blocks = torch.tensor([(0, T // 2, T // 2 + 1)], dtype=torch.int64)
    bb = kf.alloc_block_predict(C, 1, 1)
    blk = lambda: kf.block_predict(phi, q, blocks, buffers=bb)  # noqa: E731
    blk()
    prof = profiled_kernels(blk, max(1, reps // 4))
    if prof and "unavailable" not in prof:
        out["block_checkpoint_kernel_ms"] = pick(prof, "block_checkpoint_kernel")
        if out.get("shift_scan_kernel_ms") and out["block_checkpoint_kernel_ms"]:
            out["scan_over_checkpoint_walk"] = round(out["shift_scan_kernel_ms"] / out["block_checkpoint_kernel_ms"], 2)
    del bb
    torch.cuda.empty_cache()
    if kf.loo_supported():
        lb = kf.alloc_loo(C)
        loo = lambda: kf.loo_predict(phi, q, buffers=lb)  # noqa: E731
        out["loo_predict"] = timed(loo, warmup, reps)
        del lb
        torch.cuda.empty_cache()
    pb = kf.alloc_projection(C)
    sim = lambda: kf.simulate_smoothed(phi, q, buffers=pb)  # noqa: E731
    out["simulate_smoothed"] = timed(sim, warmup, reps)
    out["level_shifts_over_simulate_smoothed"] = round(out["level_shifts"]["median_ms"] / out["simulate_smoothed"]["median_ms"], 2)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", type=int, default=0, help="cap on the number of models (0: the configuration's own)")
    ap.add_argument("--chunk", type=int, default=0, help="models per call (0: 4096 narrow, 1024 wide)")
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "level_shifts", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.models, a.chunk)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
