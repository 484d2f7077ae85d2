"""Posterior draws (BatchedKalman.draw_smoothed; C ABI mk_draw_perturb / mk_draw_combine around the existing smoothing pass):
device-event times, warmed up, over --reps repetitions, of the three parts of one chunk of draws -- perturb, the smoothing
pass of the perturbed records, combine -- and of the whole call, beside simulate_smoothed on the same number of instances in
the same process (existing code: the yardstick):
  narrow  configs[1]'s batch, 4096 paths of (8 series, 2 factors), T = 1000: 1024 models x 4 draws
  wide    configs[3]'s batch, 4096 paths of (32, 4), T = 2000, 30 % missing: 4096 models x 1 draw (its tape is 84 GB)
Also perturb's algorithmic bytes (read 8N, write 8N + 8N per path-step) against its time.  Prints one JSON line per shape as
it finishes, then the whole result as one line.
--once: one draw_smoothed call per shape and nothing else (for a kernel trace)."""
import argparse
import ctypes
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# models, draws per chunk, N, K, T, missing
SHAPES = {"narrow": (1024, 4, 8, 2, 1000, 0.0), "wide": (4096, 1, 32, 4, 2000, 0.3)}


def timed(fn, warmup, reps):
    """Median / min / max of per-call device-event times (ms)."""
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
    return {"median_ms": round(statistics.median(ms), 3), "min_ms": round(min(ms), 3), "max_ms": round(max(ms), 3), "reps": reps}


def run_shape(which, warmup, reps, once):
    import torch

    from metran_amd._lib import check
    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, S, N, K, T, missing = SHAPES[which]
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    if once:
        kf.draw_smoothed(phi, q, S, seed=1, chunk=S)
        torch.cuda.synchronize()
        return {"shape": [B, S, N, K, T], "calls": 1}
    out = {"shape": {"models": B, "draws": S, "N": N, "K": K, "T": T}, "missing": missing, "paths": S * B}
    # the yardstick: the existing projection on S * B instances (instance id reads record id % B)
    pb = kf.alloc_projection(S * B)
    rphi, rq = phi.repeat(S, 1), q.repeat(S, 1)
    out["simulate_smoothed"] = timed(lambda: kf.simulate_smoothed(rphi, rq, buffers=pb), warmup, reps)
    out["simulate_smoothed"]["tape_path"] = bool(pb.get("_tape", False))
    del pb
    torch.cuda.empty_cache()
    # one warm call sets up the sub-engine and its workspace; the parts are then timed on those
    res = kf.draw_smoothed(phi, q, S, seed=1, chunk=S)
    assert int(res["status"].abs().sum().item()) == 0
    del res
    prob, keep, _ = kf._problem(phi, q, 1, None, None)
    sub, ws = kf._draw_kf, kf._draw_ws
    held = {}

    def perturb():
        held["y"], held["zx"], _ = kf._draw_perturb(prob, B, S, 1, 0, 0, False, None, True, False)

    out["perturb"] = timed(perturb, warmup, reps)
    sub.obs = held["y"]
    check(sub._L.mk_observations_changed(sub._ctx))
    out["smoothing_pass"] = timed(lambda: sub.simulate_smoothed(rphi, rq, buffers=ws["buffers"]), warmup, reps)
    sim = ws["buffers"]["sim_means"]

    def combine():
        kf._bind_stream()
        check(kf._L.mk_draw_combine(kf._ctx, ctypes.byref(prob), S, 0, 1, kf._p(held["zx"]), kf._p(sim)))

    out["combine"] = timed(combine, warmup, reps)
    held.clear()
    out["draw_smoothed"] = timed(lambda: kf.draw_smoothed(phi, q, S, seed=1, chunk=S), warmup, reps)
    extra = out["perturb"]["median_ms"] + out["combine"]["median_ms"]
    out["perturb_plus_combine_over_smoothing_pass"] = round(extra / out["smoothing_pass"]["median_ms"], 4)
    out["draw_smoothed_over_simulate_smoothed"] = round(out["draw_smoothed"]["median_ms"] / out["simulate_smoothed"]["median_ms"], 4)
    nbytes = 3 * 8 * N * S * B * T                                 # read y, write y* and Z x+
    out["perturb"]["algorithmic_bytes"] = nbytes
    out["perturb"]["GB_per_s"] = round(nbytes / (out["perturb"]["median_ms"] * 1e-3) / 1e9, 1)
    out["perturb"]["ms_at_8_TB_per_s"] = round(nbytes / 8e12 * 1e3, 3)
    normals = (N + K) * S * B * (T + 1)
    out["perturb"]["normals_per_s"] = round(normals / (out["perturb"]["median_ms"] * 1e-3), 1)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--once", action="store_true", help="one draw_smoothed call per shape, no timing (for a kernel trace)")
    a = ap.parse_args()
    import torch

    res = {"metric": "draw_smoothed", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps, a.once)
        print(json.dumps({which: res[which]}), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
