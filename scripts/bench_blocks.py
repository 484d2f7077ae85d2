"""Leave-block-out predictions (BatchedKalman.block_predict, C ABI mk_block_predict): device-event times, warmed up, over --reps
repetitions, with EVERY series tiled with 30-step blocks from step 1 (W = N * ceil((T - 1) / 30) blocks per model), at
  narrow  configs[1]'s batch, 4096 x (8 series, 2 factors), T = 1000
  wide    configs[3]'s batch, 4096 x (32, 4), T = 2000, 30 % missing
The checkpoints of a full tiling are W * (n + n^2) doubles per model (94 GB for the wide batch), so the models are taken in
chunks (--chunk, default 4096 narrow / 512 wide) as MetranBatch.gap_fill_skill takes them; the figures are per chunk and, scaled
by the number of chunks, per batch.  The four stages are timed separately: the recording forward pass by the library's own
hipEvents (filter slot); the clear of the tape + the gain writer, block_checkpoint_kernel and block_walk_kernel by the per-kernel
device times of torch's profiler (their sum is the library's smoother slot, printed beside them).  In the same process, on the
same chunk: loo_predict, simulate_smoothed, and regression with 16 pulse effects per model -- the only route to a leave-block-out
prediction before this one (one block of 16 cells per call; a tiling needs W calls).  Prints one JSON line.  --once: one call
per shape and nothing else (for a kernel trace); --models: a smaller batch.
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

LENGTH = 30
CHUNK = {"narrow": 4096, "wide": 512}


def tiling(N, T, length=LENGTH, t_first=1):
    """[W,3]: every series tiled with consecutive blocks of ``length`` steps from ``t_first``."""
    import torch

    return torch.tensor([(j, t0, min(t0 + length, T)) for j in range(N) for t0 in range(t_first, T, length)], dtype=torch.int64)


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
    blocks = tiling(N, T)
    W = int(blocks.shape[0])
    bufs = kf.alloc_block_predict(C, W, LENGTH)
    call = lambda: kf.block_predict(phi, q, blocks, buffers=bufs)  # noqa: E731
    if once:
        call()
        torch.cuda.synchronize()
        return {"shape": [C, N, K, T], "calls": 1}
    n = N + K
    chunks = -(-B // C)
    out = {"shape": [B, N, K, T], "missing": missing, "models_per_chunk": C, "chunks_per_batch": chunks, "block_length": LENGTH,
           "blocks_per_model": W, "work_stride": int(kf._L.mk_block_work_stride(N, K)),
           "checkpoint_bytes_per_chunk": C * W * (n + n * n) * 8, "output_bytes_per_chunk": C * W * (2 * LENGTH + 4) * 8}
    out["block_predict"] = timed(call, warmup, reps)
    assert int(bufs["status"].abs().sum().item()) == 0
    out["degenerate_blocks"] = int((bufs["flags"] != 0).sum().item())
    out["blocks_with_observations"] = int((bufs["summary"][..., 0] > 0).sum().item())
    f_ms, s_ms = kernels_ms(kf, call, reps)
    out["recording_pass_ms"] = round(f_ms, 3)
    out["clear_writer_checkpoint_walk_ms"] = round(s_ms, 3)
    prof = profiled_kernels(call, max(1, reps // 4))
    out["profiled_kernels_ms"] = prof
    if prof and "unavailable" not in prof:
        pick = lambda *words: round(sum(v for k, v in prof.items() if any(w in k for w in words)), 3)  # noqa: E731
        out["clear_and_gain_writer_ms"] = pick("innov_step_kernel", "Memset", "memset", "fill")
        out["block_checkpoint_kernel_ms"] = pick("block_checkpoint_kernel")
        out["block_walk_kernel_ms"] = pick("block_walk_kernel")
    out["block_predict_batch_ms"] = round(out["block_predict"]["median_ms"] * chunks, 3)
    out["blocks_per_s"] = round(C * W / (out["block_predict"]["median_ms"] * 1e-3), 1)
    del bufs
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
    del pb
    torch.cuda.empty_cache()
    # the route that existed: one block of 16 cells per model and call, as 16 pulse effects
    t0 = T // 2
    ef = torch.tensor([(0, 0, t0 + c, t0 + c + 1) for c in range(16)], dtype=torch.int64)
    rb = kf.alloc_regression(C, 16)
    reg = lambda: kf.regression(phi, q, ef, t_first=0, buffers=rb)  # noqa: E731
    out["regression_16_pulses"] = timed(reg, warmup, reps)
    out["regression_calls_for_the_tiling"] = N * -(-(T - 1) // 16)
    out["regression_route_chunk_ms"] = round(out["regression_16_pulses"]["median_ms"] * out["regression_calls_for_the_tiling"], 1)
    out["block_predict_over_simulate_smoothed"] = round(out["block_predict"]["median_ms"] / out["simulate_smoothed"]["median_ms"], 2)
    out["masked_resmooth_route_chunk_ms"] = round(out["simulate_smoothed"]["median_ms"] * W, 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--models", type=int, default=0, help="cap on the number of models (0: the configuration's own)")
    ap.add_argument("--chunk", type=int, default=0, help="models per call (0: 4096 narrow, 512 wide)")
    ap.add_argument("--once", action="store_true", help="one call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "block_predict", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once, a.models, a.chunk)
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
