#!/usr/bin/env python
"""Measure the multipliers of the diagnostic routes' bars (tests/hard_models.py: disturbance_tolerances, forecast_tolerances,
weights_tolerance, regression_tolerances, score_tolerances) on the CPU: over the models of the property sweep, the largest
difference between the float64 and the extended-precision run of each numpy restatement, relative to the scale of the quantity,
in units of ``hard_models.conditioning`` (2 eps scale / min q).  hard_models.MEASURED holds the figures printed in the last line;
the bars use 4 times them.

    python scripts/measure_diagnostic_bars.py [--seeds 30] [--jobs 8] [--fit-states 22]

Per seed range and route: the largest ratio with its model, the largest ratio among the models whose conditioning exceeds
1e-10 ("hard": where the conditioning term, not the flat bar, is what holds), and the largest gap itself.

The three fitting routes (regression, window functionals, scores) run on every model of the default sweep that
tests/diagnostic_sweep.py compares (``compared``; the scores on ``score_compared``) and, for the further seeds, on the shapes up to
N + K = ``--fit-states`` (the restatements' arithmetic does not depend on the shape; the extended-precision score restatement holds
[n,n,n] arrays per cell).  regress_beta and regress_cov are also divided by the unit-diagonal condition number of the kept
effects, the form of their bar; the ``_raw`` rows are not (for the judgement whether that factor belongs in the bar).  The
functional rows are in units of hard_models.functional_tolerances itself, not of the conditioning: that bar has no measured part,
the rows show what the float64 walk loses of it.
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
FITS = ("regress_normal", "regress_beta", "regress_cov", "regress_gain", "score_score", "score_grad", "score_opg", "score_cusum")
INFORMATIVE = ("regress_beta_raw", "regress_cov_raw")           # in units of the conditioning, not in MEASURED
AS_THEY_ARE = ("functional_mean", "functional_var", "regress_cond")   # not divided by the conditioning
FIT_STATES = 22


def sweep(job):
    """{route: [(ratio, gap, conditioning, where), ..]} of one sweep (seed None = the default one)."""
    import diagnostic_sweep as ds
    import hard_models

    seed, fit_states = job
    rows = {k: [] for k in ROUTES + FITS + INFORMATIVE + AS_THEY_ARE}
    for key, g in hard_models.groups(seed=seed):
        fits = seed is None or key[0] + key[1] <= fit_states
        cmp_, sc_ = (set(ds.compared(key, g)), set(ds.score_compared(key, g))) if fits else ((), ())
        for b in range(key[3]):
            c = hard_models.conditioning(g, b, ds.oracle_ref(g, b))
            where = (seed,) + key + (b, g["patterns"][b], float(g["q"][b].min()))
            for k, gap in ds.restatement_gaps(key, g, b, fits=b in cmp_, scores_too=b in sc_).items():
                rows[k].append((gap if k in AS_THEY_ARE else gap / c, gap, c, where))
        g.pop("_cache", None)
    return rows


def report(name, rows, keys):
    worst = {}
    for k in keys:
        r = rows[k]
        if not r:
            continue
        top = max(r, key=lambda t: t[0])
        hard = [t for t in r if t[2] > 1e-10]
        toph = max(hard, key=lambda t: t[0]) if hard else (0.0, 0.0, 0.0, None)
        gap = max(r, key=lambda t: t[1])
        print("%-12s %-16s (%5d) ratio %.3g at %s | hard models (%d): %.3g at %s | largest gap %.3g at %s (ratio %.3g)"
              % (name, k, len(r), top[0], top[3], len(hard), toph[0], toph[3], gap[1], gap[3], gap[0]), flush=True)
        worst[k] = top[0]
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seeds", type=int, default=30, help="further sweeps, METRAN_SWEEP_SEED = 1 .. SEEDS")
    ap.add_argument("--jobs", type=int, default=min(8, os.cpu_count() or 1))
    ap.add_argument("--fit-states", type=int, default=FIT_STATES,
                    help="the further sweeps run the fitting routes on the shapes up to N + K = this")
    a = ap.parse_args()
    from multiprocessing import Pool

    t0 = time.perf_counter()
    seeds = [None] + list(range(1, a.seeds + 1))
    with Pool(a.jobs) as pool:
        res = pool.map(sweep, [(s, a.fit_states) for s in seeds], chunksize=1)
    print("%d sweeps, %d models, %.0f s; fitting routes: the compared models of the default sweep, of the shapes up to N + K = %d beyond"
          % (len(seeds), sum(len(r[ROUTES[0]]) for r in res), time.perf_counter() - t0, a.fit_states))
    keys = ROUTES + FITS + INFORMATIVE + AS_THEY_ARE
    worst = report("default", res[0], keys)
    for lo in range(1, len(seeds), 10):
        part = {k: sum((r[k] for r in res[lo:lo + 10]), []) for k in keys}
        w = report("seeds %d-%d" % (seeds[lo], seeds[min(lo + 9, len(seeds) - 1)]), part, keys)
        worst = {k: max(worst.get(k, 0.0), w.get(k, 0.0)) for k in keys}
    print("functional walk, float64 against longdouble: %.2g (mean) and %.2g (variance) of hard_models.functional_tolerances; "
          "largest unit-diagonal condition number of the kept effects %.3g" % tuple(worst[k] for k in AS_THEY_ARE))
    print("MEASURED = {%s}" % ", ".join('"%s": %.2g' % (k, worst[k]) for k in ROUTES + FITS))


if __name__ == "__main__":
    main()
