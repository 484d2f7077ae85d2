"""Window statistics of posterior draws (BatchedKalman.draw_window_statistics; C ABI mk_path_functionals / mk_ensemble_summary
inside the chunk loop of draw_smoothed): device-event times, warmed up, over --reps repetitions, of the parts of one chunk of
draws -- perturb, the smoothing pass of the perturbed records, combine, the path functionals -- of the final ensemble summary
and of the whole call, with the call's peak device memory beside what get_simulation_draws of the same number of draws would
hold; monthly windows (W = 33 over T = 1000):
  narrow  configs[1]'s batch, 4096 paths of (8 series, 2 factors), T = 1000: 1024 models x 4 draws per chunk, 64 draws
  wide    configs[3]'s batch, 4096 paths of (32, 4), T = 2000, 30 % missing: 4096 models x 1 draw per chunk, 8 draws
Also the path kernel's algorithmic bytes (it reads the combined draws once) against its time.  Prints one JSON line per shape
as it finishes, then the whole result as one line."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from bench_draws import timed  # noqa: E402  (scripts/ is on the path when this file runs)

# models, draws per chunk, draws of the whole call, N, K, T, missing
SHAPES = {"narrow": (1024, 4, 64, 8, 2, 1000, 0.0), "wide": (4096, 1, 8, 32, 4, 2000, 0.3)}
PROBS = (0.025, 0.5, 0.975)


def run_shape(which, warmup, reps):
    import numpy as np
    import torch

    from metran_amd._lib import check
    from metran_amd.engine import BatchedKalman
    from metran_amd.synthetic import make_dfm_batch_torch

    B, S, total, N, K, T, missing = SHAPES[which]
    d = make_dfm_batch_torch(B, N, K, T, seed=2000, device=torch.device("cuda", 0), missing=missing)
    kf = BatchedKalman(0, layout="time_major")
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = d["phi"], d["q"]
    W = int(round(T / 30.4375))
    edges = np.rint(np.linspace(0, T, W + 1)).astype(np.int64)
    windows = np.stack([edges[:-1], edges[1:]], axis=1)
    thresholds = torch.zeros((B, N), dtype=torch.float64, device="cuda")
    out = {"shape": {"models": B, "draws_per_chunk": S, "draws": total, "N": N, "K": K, "T": T, "W": W}, "missing": missing}
    # the whole call first: it sets up the sub-engine and its workspace, and its peak is that of a fresh engine
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    res = kf.draw_window_statistics(phi, q, total, windows, thresholds, probs=PROBS, seed=1, chunk=S)
    torch.cuda.synchronize()
    assert int(res["status"].abs().sum().item()) == 0
    out["peak_bytes"] = int(torch.cuda.max_memory_allocated() - before)
    out["functionals_bytes"] = 8 * total * B * N * W * 5
    out["ensemble_bytes"] = 8 * total * B * T * N                    # what get_simulation_draws of the same draws returns
    out["peak_over_ensemble"] = round(out["peak_bytes"] / out["ensemble_bytes"], 4)
    del res
    out["draw_window_statistics"] = timed(lambda: kf.draw_window_statistics(phi, q, total, windows, thresholds, probs=PROBS, seed=1, chunk=S),
                                          1, max(2, reps // 3))
    prob, keep, _ = kf._problem(phi, q, 1, None, None)
    sub, ws = kf._draw_kf, kf._draw_ws
    rphi, rq = phi.repeat(S, 1), q.repeat(S, 1)
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
    win = kf._step_windows(windows)
    functionals = torch.empty((total, B, N, W, 5), dtype=torch.float64, device="cuda")

    def path_functionals():
        kf._bind_stream()
        check(kf._L.mk_path_functionals(kf._ctx, ctypes.byref(prob), S, 0, 1, kf._p(sim), W, kf._p(win), kf._p(thresholds),
                                        kf._p(functionals)))

    out["path_functionals"] = timed(path_functionals, warmup, reps)
    nbytes = 8 * N * S * B * T
    out["path_functionals"]["algorithmic_bytes"] = nbytes
    out["path_functionals"]["GB_per_s"] = round(nbytes / (out["path_functionals"]["median_ms"] * 1e-3) / 1e9, 1)
    out["path_functionals_over_combine"] = round(out["path_functionals"]["median_ms"] / out["combine"]["median_ms"], 4)
    chunk_ms = sum(out[k]["median_ms"] for k in ("perturb", "smoothing_pass", "combine", "path_functionals"))
    out["path_functionals_share_of_chunk"] = round(out["path_functionals"]["median_ms"] / chunk_ms, 4)
    held.clear()
    functionals.normal_()
    summary = torch.empty((B * N * W * 5, 5 + len(PROBS)), dtype=torch.float64, device="cuda")
    probs = (ctypes.c_double * len(PROBS))(*PROBS)

    def summarise():
        kf._bind_stream()
        check(kf._L.mk_ensemble_summary(kf._ctx, total, B * N * W * 5, kf._p(functionals), len(PROBS), probs, kf._p(summary)))

    out["ensemble_summary"] = timed(summarise, 1, max(2, reps // 3))
    out["ensemble_summary"]["cells"] = B * N * W * 5
    out["ensemble_summary_over_all_chunks"] = round(out["ensemble_summary"]["median_ms"] / (chunk_ms * total / S), 4)
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--shapes", default="narrow,wide")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    import torch

    res = {"metric": "draw_window_statistics", "device": torch.cuda.get_device_name(0)}
    for which in a.shapes.split(","):
        res[which] = run_shape(which, a.warmup, a.reps)
        print(json.dumps({which: res[which]}), flush=True)
        torch.cuda.empty_cache()
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
