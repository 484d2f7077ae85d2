#!/usr/bin/env python
"""Measure the bars of tests/test_scores_gpu.py on the CPU: on its inputs (``input_sets``: every shape, length and compared
instance), separately for the records of one or two steps and for the longer ones, the largest difference between the float64
and the extended-precision run of tests/score_ref.py, per output, relative
to the output's scale (the expression with every term replaced by its absolute value; for ``score`` the scale of the (instance,
parameter) pair's largest step).  The test's bars are 16 times these (the kernel's tree-order sums differ from numpy's order),
floored at 1e-13; the figures printed here are the ones in its docstring.

    python scripts/measure_scores_bar.py
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import score_ref  # noqa: E402
import test_scores_gpu as ts  # noqa: E402


def main():
    worst = {cls: {key: (-1.0, ()) for key in score_ref.OUTPUTS} for cls in ("short", "long")}
    for p, dphi, dq, t_first, compared in ts.input_sets():
        T, N = p["obs"].shape[1:]
        K = p["loadings"].shape[2]
        cls = "short" if T <= ts.SHORT else "long"
        t0 = time.perf_counter()
        for b in compared:
            r64 = ts._reference(p, b, dphi, dq, t_first, dtype=np.float64)
            rld = ts._reference(p, b, dphi, dq, t_first, dtype=np.longdouble)
            assert r64["count"] == rld["count"]
            diff = score_ref.differences(r64, rld)
            for key in score_ref.OUTPUTS:
                worst[cls][key] = max(worst[cls][key], (diff[key], (N, K, T, b)))
        print("(%d,%d) T=%d t_first=%d: %.1f s, worst so far (%s) %s" % (N, K, T, t_first, time.perf_counter() - t0, cls,
                                                                        ", ".join("%s %.3g" % (k, worst[cls][k][0]) for k in score_ref.OUTPUTS)), flush=True)
    for cls, name in (("long", "MEASURED"), ("short", "MEASURED_SHORT")):
        for key in score_ref.OUTPUTS:
            w, where = worst[cls][key]
            print("%s[%r] = %.3g at %s;  16 x = %.3g;  bar = max(that, 1e-13) = %.3g" % (name, key, w, where, 16 * w, max(16 * w, 1e-13)))


if __name__ == "__main__":
    main()
