#!/usr/bin/env python
"""Generate ``weights_ref_impulses.npz`` from the *reference itself*: the observation weights of three smoothed values of one
(3 series, 1 factor), T = 40, 30 %-missing model, by UNIT-IMPULSE DIFFERENCES through the reference's own filter
(``seqkalmanfilter``, the numba source un-jitted), ``kalmansmoother`` and ``simulate``:

    w[m, s, i] = simulate(y + e_{s,i})[t*_m, j*_m] - simulate(y)[t*_m, j*_m]      for every observed cell (s, i)

(the smoother is linear in the data for fixed parameters, so a difference quotient with step 1 is the weight up to rounding).
The targets: an observed cell, a cell of an empty step, and t* = 0.  Run ONCE where the reference is present:

    python tests/golden/make_weights_golden.py

The reference package is imported unmodified through ``_refshim``; nothing at test time reads it
(tests/test_weights_host.py compares tests/weights_ref.py with the fixture)."""
import os
import sys

import numpy as np
import pandas as pd

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import _refshim  # noqa: E402

metran = _refshim.install()
import metran.kalmanfilter as kfm  # noqa: E402

from metran_amd.params import observation_matrix  # noqa: E402
from metran_amd.synthetic import make_dfm  # noqa: E402


def simulate(obs, phi, q, loadings):
    """The reference's projected smoothed means [T,N] of one model (standardised units)."""
    N = obs.shape[1]
    kf = kfm.SPKalmanFilter(engine="numpy")
    kf.filtermethod = kfm.seqkalmanfilter
    kf.set_observations(pd.DataFrame(obs))
    Z = observation_matrix(loadings)
    kf.set_matrices(np.diag(phi), np.diag(q), Z, np.zeros(N))
    kf.run_smoother()
    return np.asarray(kf.simulate(Z, method="smoother")[0], float)


def main():
    N, K, T = 3, 1, 40
    y, alpha, loadings, phi, q = make_dfm(N, K, T, 31, 0, 0.3, "observed")
    y = y.copy()
    y[17] = np.nan                                        # an empty step
    seen = np.isfinite(y)
    t_obs = int(np.nonzero(seen[20:, 1])[0][0]) + 20      # an observed cell of series 1
    targets = np.array([[t_obs, 1], [17, 2], [0, 0]], dtype=np.int64)
    base = simulate(y, phi, q, loadings)
    w = np.full((len(targets), T, N), np.nan)
    for s in range(T):
        for i in range(N):
            if not seen[s, i]:
                continue
            bumped = y.copy()
            bumped[s, i] += 1.0
            sim = simulate(bumped, phi, q, loadings)
            for m, (ts, col) in enumerate(targets):
                w[m, s, i] = sim[ts, col] - base[ts, col]
    out = dict(obs=y, phi=phi, q=q, loadings=loadings, targets=targets, weights=w,
               base=np.array([base[ts, col] for ts, col in targets]))
    np.savez_compressed(os.path.join(HERE, "weights_ref_impulses.npz"), **out)
    print("weights_ref_impulses.npz", {k: v.shape for k, v in out.items()}, "observed cells:", int(seen.sum()))


if __name__ == "__main__":
    main()
