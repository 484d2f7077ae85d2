"""The rank-K covariance step of the record smoother (smoother_record_kernel LR), restated in numpy.

Where a model observes all N series at step t and has no observation variances, the N scalar updates leave Pf[t] Z^T = 0, so
Pf[t] = B C B^T with B = [-Gamma ; I_K], J = Pf Phi Pp^-1 = B J_f (J_f: the K factor rows of J) and

    Ps[t] = Pf[t] + J D J^T = Pf[t] + u B^T,      u = J (J_f D)^T,      D = Ps[t+1] - Pp[t+1].

Checked here, on the CPU: the restatement against the oracle's smoother (1e-9, the smoother bar of tests/test_hip_parity.py) and
against the general step; the hard models of tests/hard_models.py at ``smoother_tolerance``; and that the two ways of applying
the step where it does not hold -- with observation variances, or at a step with a missing cell -- fall outside the bar, which
is what the kernel's two guards (d_obsvar == NULL, every cell of the step finite) are for."""
import numpy as np
import pytest

import hard_models as hm
import oracle
from metran_amd.synthetic import make_dfm_batch

SMOOTH_ATOL = 1e-9   # tests/test_hip_parity.py
# low-rank against general step, same J: both are sums of at most n^2 products of entries of J (|J| <~ 1 here) and D (<~ 1), in
# another order -- n^2 eps ~ 2e-14 at n = 10 per step, and the recursion is a contraction (|J| < 1).  The issue's run measured 1.1e-16.
STEP_ATOL = 1e-12
SHAPES = [(1, 1), (4, 1), (8, 2), (7, 3)]


def smooth(F, Pf, phi, q, G, full, lowrank):
    """kalmansmoother (kalmanfilter.py:403-476) of one model from its filtered moments, Phi and Q diagonal; ``full[t]``: take the
    rank-K form of the covariance step at t (ignored unless ``lowrank``)."""
    T, n = F.shape
    N = G.shape[0]
    S, Ps = F.copy(), Pf.copy()
    for t in range(T - 2, -1, -1):
        W = Pf[t] * phi[None, :]                       # Pf Phi
        Pp = phi[:, None] * W + np.diag(q)             # Pp[t+1]
        J = np.linalg.solve(Pp, W.T).T                 # Pf Phi Pp^-1 (Pp symmetric)
        D = Ps[t + 1] - Pp
        S[t] = F[t] + J @ (S[t + 1] - phi * F[t])
        if lowrank and full[t]:
            u = J @ (D @ J[N:].T)                      # n x K
            Ps[t] = Pf[t]
            Ps[t][:, :N] -= u @ G.T
            Ps[t][:, N:] += u
        else:
            Ps[t] = Pf[t] + J @ D @ J.T
    return S, Ps


def _full_steps(obs):
    return np.isfinite(obs).all(axis=-1)


@pytest.mark.parametrize("missing", [0.0, 0.1])
@pytest.mark.parametrize("N,K", SHAPES)
def test_lowrank_step_against_oracle_and_general_step(N, K, missing):
    d = make_dfm_batch(6, N, K, 60, seed=4100 + 10 * N + K, missing=missing)
    ref = oracle.dfm_batch(d["obs"], d["phi"], d["q"], d["loadings"])
    taken = 0
    for b in range(6):
        full = _full_steps(d["obs"][b])
        taken += int(full[:-1].sum())
        S, Ps = smooth(ref["F"][b], ref["Pf"][b], d["phi"][b], d["q"][b], d["loadings"][b], full, True)
        Sg, Psg = smooth(ref["F"][b], ref["Pf"][b], d["phi"][b], d["q"][b], d["loadings"][b], full, False)
        np.testing.assert_allclose(S, ref["S"][b], rtol=0, atol=SMOOTH_ATOL)
        np.testing.assert_allclose(Ps, ref["Ps"][b], rtol=0, atol=SMOOTH_ATOL)
        np.testing.assert_allclose(Ps, Psg, rtol=0, atol=STEP_ATOL)
        np.testing.assert_array_equal(S, Sg)            # J and the mean are untouched
    assert taken > (200 if missing == 0.0 else 6)       # the low-rank form was what ran (10 % missing at N = 8: 43 % of the steps)
    if missing:
        assert taken < 6 * 59                           # ... next to general steps


def test_hard_models():
    """Near-unit persistence, communalities up to 0.999, every missingness pattern: the models without observation variances
    (the others never take the step) at the sweep's own bar."""
    checked = steps = 0
    for (N, K, T, B), g in hm.groups(per_shape=20, shapes=[(8, 2), (5, 1), (2, 1), (3, 1), (4, 1), (6, 2), (7, 2)]):
        if g["obsvar"] is not None:
            continue
        for b in range(B):
            ref = hm.oracle_model(oracle, g, b)
            if not (np.isfinite(ref["S"]).all() and np.isfinite(ref["Ps"]).all()):
                continue
            full = _full_steps(g["obs"][b])
            S, Ps = smooth(ref["F"], ref["Pf"], g["phi"][b], g["q"][b], g["loadings"][b], full, True)
            tol = hm.smoother_tolerance(g, b, ref)
            assert float(np.abs(S - ref["S"]).max()) <= tol, (N, K, T, b, g["patterns"][b])
            assert float(np.abs(Ps - ref["Ps"]).max()) <= tol, (N, K, T, b, g["patterns"][b])
            checked += 1
            steps += int(full[:-1].sum())
    assert checked >= 20 and steps >= 100, (checked, steps)


@pytest.mark.parametrize("N,K", [(4, 1), (8, 2)])
def test_the_step_needs_zero_observation_variances(N, K):
    d = make_dfm_batch(3, N, K, 40, seed=4300 + N, missing=0.0)
    obsvar = np.full((3, N), 0.1)
    ref = oracle.dfm_batch(d["obs"], d["phi"], d["q"], d["loadings"], obsvar=obsvar)
    for b in range(3):
        full = _full_steps(d["obs"][b])
        _, Psg = smooth(ref["F"][b], ref["Pf"][b], d["phi"][b], d["q"][b], d["loadings"][b], full, False)
        np.testing.assert_allclose(Psg, ref["Ps"][b], rtol=0, atol=SMOOTH_ATOL)   # the restatement itself is right ...
        _, Ps = smooth(ref["F"][b], ref["Pf"][b], d["phi"][b], d["q"][b], d["loadings"][b], full, True)
        assert float(np.abs(Ps - ref["Ps"][b]).max()) > 1e3 * SMOOTH_ATOL            # ... and Pf has full rank: no u B^T


@pytest.mark.parametrize("N,K", [(4, 1), (8, 2)])
def test_the_step_needs_every_cell_of_the_step(N, K):
    d = make_dfm_batch(3, N, K, 40, seed=4400 + N, missing=0.0)
    obs = d["obs"].copy()
    obs[:, 17, N - 1] = np.nan                                                       # one cell of one step
    ref = oracle.dfm_batch(obs, d["phi"], d["q"], d["loadings"])
    for b in range(3):
        full = _full_steps(obs[b])
        assert not full[17] and full.sum() == 39
        _, Ps = smooth(ref["F"][b], ref["Pf"][b], d["phi"][b], d["q"][b], d["loadings"][b], full, True)
        np.testing.assert_allclose(Ps, ref["Ps"][b], rtol=0, atol=SMOOTH_ATOL)     # guarded: the general step at t = 17
        _, Ps = smooth(ref["F"][b], ref["Pf"][b], d["phi"][b], d["q"][b], d["loadings"][b], np.ones(40, bool), True)
        assert float(np.abs(Ps - ref["Ps"][b]).max()) > 1e3 * SMOOTH_ATOL            # unguarded
