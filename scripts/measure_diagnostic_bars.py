#!/usr/bin/env python
"""Measure the multipliers of the diagnostic routes' bars (tests/hard_models.py: disturbance_tolerances, forecast_tolerances,
weights_tolerance) on the CPU: over the models of the property sweep, the largest difference between the float64 and the
extended-precision run of each numpy restatement, relative to the scale of the quantity, in units of
``hard_models.conditioning`` (2 eps scale / min q).  hard_models.MEASURED holds the figures printed in the last line; the bars
use 4 times them.

    python scripts/measure_diagnostic_bars.py [--seeds 30] [--jobs 8]

Per seed range and route: the largest ratio with its model, the largest ratio among the models whose conditioning exceeds
1e-10 ("hard": where the conditioning term, not the flat bar, is what holds), and the largest gap itself.
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ROUTES = ("dist_r", "dist_n", "forecast_mean", "forecast_var", "weights_series", "weights_states")


def sweep(seed):
    """{route: [(ratio, gap, conditioning, where), ..]} of one sweep (seed None = the default one)."""
    import diagnostic_sweep as ds
    import hard_models

    rows = {k: [] for k in ROUTES}
    for key, g in hard_models.groups(seed=seed):
        for b in range(key[3]):
            c = hard_models.conditioning(g, b, ds.oracle_ref(g, b))
            where = (seed,) + key + (b, g["patterns"][b], float(g["q"][b].min()))
            for k, gap in ds.restatement_gaps(key, g, b).items():
                rows[k].append((gap / c, gap, c, where))
        g.pop("_cache", None)
    return rows


def report(name, rows):
    worst = {}
    for k in ROUTES:
        r = rows[k]
        top = max(r, key=lambda t: t[0])
        hard = [t for t in r if t[2] > 1e-10]
        toph = max(hard, key=lambda t: t[0]) if hard else (0.0, 0.0, 0.0, None)
        gap = max(r, key=lambda t: t[1])
        print("%-12s %-15s ratio %.3g at %s | hard models (%d): %.3g at %s | largest gap %.3g at %s (ratio %.3g)"
              % (name, k, top[0], top[3], len(hard), toph[0], toph[3], gap[1], gap[3], gap[0]), flush=True)
        worst[k] = top[0]
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=30, help="further sweeps, METRAN_SWEEP_SEED = 1 .. SEEDS")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    a = ap.parse_args()
    from multiprocessing import Pool

    t0 = time.perf_counter()
    seeds = [None] + list(range(1, a.seeds + 1))
    with Pool(a.jobs) as pool:
        res = pool.map(sweep, seeds, chunksize=1)
    print("%d sweeps, %d models, %.0f s" % (len(seeds), sum(len(r[ROUTES[0]]) for r in res), time.perf_counter() - t0))
    worst = report("default", res[0])
    for lo in range(1, len(seeds), 10):
        part = {k: sum((r[k] for r in res[lo:lo + 10]), []) for k in ROUTES}
        w = report("seeds %d-%d" % (seeds[lo], seeds[min(lo + 9, len(seeds) - 1)]), part)
        worst = {k: max(worst[k], w[k]) for k in ROUTES}
    print("MEASURED = {%s}" % ", ".join('"%s": %.2g' % (k, worst[k]) for k in ROUTES))


if __name__ == "__main__":
    main()
