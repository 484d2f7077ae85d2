"""The numpy restatement of the intervention effects by GLS (tests/regress_ref.py), pinned WITHOUT a GPU: to a second
definition by dense Gaussian conditioning, to the oracle's own filter (its sigmas and its objective of the adjusted records) and
to the leave-one-out restatement (a pulse is a deletion residual); the conditioning cap of the GPU tier's inputs; its
deliberately wrong variants shown to be far outside the bars; and the MetranBatch accessors over a stand-in engine that answers
from the restatement.

Counting: the restatement counts the cells of the steps t >= t_first; the reference's ``get_mle(warmup)`` skips the first
``warmup`` steps that HOLD AN OBSERVATION (its sigmas are kept for those steps only).  The two name the same cells when warmup =
the number of non-empty steps before t_first, which is what the comparisons with the oracle use."""
import numpy as np
import pandas as pd
import pytest

import loo_ref
import oracle
import regress_ref
from batch_standin import stand_in, two_models
from regress_engine import RegressEngine

F64 = np.float64
PARITY_BAR = 1e-9    # the project's parity bar against the oracle / the reference
LEVEL, RAMP = regress_ref.LEVEL, regress_ref.RAMP


def _model(N, K, T, seed, full):
    """(y, phi, q, G, R, x0, P0): 30 % missing, step 2 empty, (0, 0) and (T - 1, N - 1) observed; ``full``: observation variances
    and initial moments given."""
    rng = np.random.default_rng(seed)
    n = N + K
    y = rng.normal(size=(T, N))
    y[rng.random((T, N)) < 0.3] = np.nan
    y[2] = np.nan
    y[0, 0], y[T - 1, N - 1] = 0.4, -0.7
    phi, q = rng.uniform(0.5, 0.95, n), rng.uniform(0.1, 0.5, n)
    G = rng.uniform(-0.6, 0.6, (N, K))
    A = rng.normal(size=(n, n))
    return (y, phi, q, G, rng.uniform(0.05, 0.4, N) if full else None, rng.normal(size=n) if full else None,
            A @ A.T / n + 0.5 * np.eye(n) if full else None)


def _small_effects(N, T):
    """A pulse at (0, 0), a shift, a ramp and a whole-record level, on different series where there are enough."""
    return np.array([(0, LEVEL, 0, 1), (1 % N, LEVEL, T // 2, T), (2 % N, RAMP, 1, T - 1), ((N - 1), LEVEL, 0, T)], dtype=np.int64)


def _dense(y, phi, q, G, R, x0, P0, X, t_first):
    """A by dense conditioning: with Sigma the covariance and mu the mean of all observed cells and Sigma_11, mu_1 those of the
    steps before t_first, W = [y - mu | X]:  A = W' Sigma^-1 W - W_1' Sigma_11^-1 W_1.  Also cond(Sigma) and sqrt(F_pp F_qq) of
    the first term F, the size of the numbers the difference is taken of."""
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    Z = np.concatenate([np.eye(N), G], axis=1)
    R = np.zeros(N) if R is None else R
    a = np.zeros(n) if x0 is None else x0
    P = np.eye(n) if P0 is None else P0
    Phi = np.diag(phi)
    mu = np.empty((T, n))
    V = np.zeros((T, n, T, n))
    for t in range(T):
        a = Phi @ a
        P = Phi @ P @ Phi.T + np.diag(q)
        mu[t] = a
        V[t, :, t, :] = P
        for s in range(t):
            V[t, :, s, :] = Phi @ V[t - 1, :, s, :]
            V[s, :, t, :] = V[t, :, s, :].T
    cells = [(t, j) for t in range(T) for j in range(N) if np.isfinite(y[t, j])]
    H = np.zeros((len(cells), T * n))
    for i, (t, j) in enumerate(cells):
        H[i, t * n:(t + 1) * n] = Z[j]
    Sy = H @ V.reshape(T * n, T * n) @ H.T + np.diag([R[j] for (_, j) in cells])
    W = np.array([[y[t, j] - (H @ mu.reshape(-1))[i]] + [X[m, t, j] for m in range(X.shape[0])] for i, (t, j) in enumerate(cells)])
    A = W.T @ np.linalg.solve(Sy, W)
    whole = np.sqrt(np.diag(A))
    n1 = sum(1 for (t, _) in cells if t < t_first)
    if n1:
        A = A - W[:n1].T @ np.linalg.solve(Sy[:n1, :n1], W[:n1])
    return A, float(np.linalg.cond(Sy)), np.outer(whole, whole)


DENSE_CASES = [(3, 1, 6, 1, False), (3, 1, 6, 2, True), (4, 2, 5, 3, False), (2, 2, 6, 4, True)]


@pytest.mark.parametrize("t_first", [0, 1, 2])
@pytest.mark.parametrize("case", DENSE_CASES, ids=["%dx%d-T%d-%s" % (c[0], c[1], c[2], "full" if c[4] else "plain") for c in DENSE_CASES])
def test_restatement_is_dense_gaussian_conditioning(case, t_first):
    """The replay's A is what one dense solve on the joint covariance of the observed cells gives, minus the part of the steps
    before t_first.  The bar is the dense definition's own error: 64 eps cond(Sigma), entrywise relative to the size of the two
    quadratic forms whose difference it is (a pulse before t_first keeps little of its own: that difference cancels)."""
    N, K, T, seed, full = case
    m = _model(N, K, T, seed, full)
    ef = _small_effects(N, T)
    Ad, cond, size = _dense(*m, regress_ref.regressors(T, N, ef), t_first)
    bar = 64 * np.finfo(float).eps * cond
    for dtype in (F64, np.longdouble):
        res = regress_ref.regression(*m, effects=ef, t_first=t_first, dtype=dtype)
        A = res["normal"].astype(F64)
        assert np.max(np.abs(A - Ad) / size) <= bar, (np.max(np.abs(A - Ad) / size), bar)
        kept = ~res["dropped"]
        assert kept.sum() >= 2
        S, s = Ad[1:, 1:][np.ix_(kept, kept)], Ad[0, 1:][kept]
        beta = np.linalg.solve(S, s)
        tol = bar * np.linalg.cond(S)
        assert np.max(np.abs(res["beta"][kept].astype(F64) - beta) / np.maximum(1, np.abs(beta))) <= tol
        assert np.max(np.abs(res["cov"][np.ix_(kept, kept)].astype(F64) - np.linalg.inv(S))) <= tol * np.max(np.abs(np.linalg.inv(S)))
        assert abs(float(res["gain"]) - s @ beta) <= tol * max(1.0, s @ beta)
        assert np.isnan(res["beta"][~kept]).all() and np.isnan(res["cov"][~kept]).all() and np.isnan(res["cov"][:, ~kept]).all()


def _oracle_filter(y, phi, q, G, R, x0, P0):
    N, K = G.shape
    n = N + K
    ob, oi, oc = oracle.set_observations(y)
    sg, df, sc, *_ = oracle.seqkalmanfilter(ob, np.diag(phi), np.diag(q), np.concatenate([np.eye(N), G], axis=1), np.zeros(N) if R is None else R,
                                            oi, oc, np.zeros(n) if x0 is None else x0, np.eye(n) if P0 is None else P0)
    return sg[:sc], df[:sc], oc


def _warmup_of(y, t_first):
    return int(np.isfinite(y[:t_first]).any(axis=1).sum())


ORACLE_CASES = [(3, 1, 14, 1, False), (3, 1, 14, 2, True), (4, 2, 9, 3, True)]


@pytest.mark.parametrize("t_first", [0, 1, 3])
@pytest.mark.parametrize("case", ORACLE_CASES, ids=["%dx%d-T%d-%s" % (c[0], c[1], c[2], "full" if c[4] else "plain") for c in ORACLE_CASES])
def test_restatement_agrees_with_the_oracles_filter(case, t_first):
    """A[0,0] is the oracle filter's sum of sigmas over the counted steps, and the oracle's objective of y - X beta is the base
    objective minus the gain (t_first = 3 lies behind the empty step 2: the warm-up that names the same cells is 2)."""
    N, K, T, seed, full = case
    m = _model(N, K, T, seed, full)
    y = m[0]
    ef = _small_effects(N, T)
    res = regress_ref.regression(*m, effects=ef, t_first=t_first, dtype=F64)
    w = _warmup_of(y, t_first)
    assert w == (2 if t_first == 3 else t_first)
    sg, df, oc = _oracle_filter(*m)
    assert abs(float(res["normal"][0, 0]) - sg[w:].sum()) <= PARITY_BAR * sg[w:].sum()
    base = oracle.get_mle(sg, df, oc, w)
    sg2, df2, oc2 = _oracle_filter(regress_ref.adjusted(y, ef, res["beta"]), *m[1:])
    after = oracle.get_mle(sg2, df2, oc2, w)
    assert float(res["gain"]) > 0 and abs((base - after) - float(res["gain"])) <= PARITY_BAR * abs(base)
    worse = oracle.get_mle(*_oracle_filter(regress_ref.adjusted(y, ef, res["beta"] + 0.01), *m[1:]), w)   # the kept effects moved
    assert worse > after                                           # ... and beta is where the quadratic is smallest


@pytest.mark.parametrize("case", ORACLE_CASES, ids=["%dx%d-T%d-%s" % (c[0], c[1], c[2], "full" if c[4] else "plain") for c in ORACLE_CASES])
def test_a_pulse_is_the_deletion_residual(case):
    """A pulse at an observed cell with t_first = 0: the estimate is the observation minus its leave-one-out prediction and its
    variance the deletion variance of the cell (tests/loo_ref.py: the variance of z_j x_t from the others, plus the observation
    variance)."""
    N, K, T, seed, full = case
    m = _model(N, K, T, seed, full)
    y, R = m[0], m[4]
    lm, lv = loo_ref.loo_adjoint(*m)
    cells = [(t, j) for t in (0, 1, 5, T - 1) for j in range(N) if np.isfinite(y[t, j])]
    assert len(cells) >= 4
    for t, j in cells:
        res = regress_ref.regression(*m, effects=[(j, LEVEL, t, t + 1)], t_first=0, dtype=F64)
        resid, var = y[t, j] - lm[t, j], lv[t, j] + (0.0 if R is None else R[j])
        assert not res["dropped"][0] and res["support"][0] == 1
        assert abs(float(res["beta"][0]) - resid) <= PARITY_BAR * max(1.0, abs(resid)), (t, j)
        assert abs(float(res["cov"][0, 0]) - var) <= PARITY_BAR * max(1.0, var), (t, j)


def test_conditioning_cap_of_the_gpu_tiers_inputs():
    """Every input set of tests/test_regression_gpu.py: the unit-diagonal S of the effects that are kept has a condition number
    of at most 1e4, and the pivot of every effect is either at rounding level (an exact duplicate: below 1e-14) or far from the
    threshold of 1e-12 (above 1e-6) -- never anything near it.  A cap, not a measurement."""
    import test_regression_gpu as tr

    worst = 0.0
    for p, ef, t_first in tr.input_sets():
        for b in range(p["phi"].shape[0]):
            res, _ = tr._reference(p, b, ef, t_first, dtype=F64)
            worst = max(worst, regress_ref.unit_condition(res["normal"], res["dropped"]))
            S = res["normal"][1:, 1:]
            live = np.nonzero((res["support"] > 0) & (np.diag(S) > 0))[0]
            piv = _pivots(S[np.ix_(live, live)])
            assert all(pv < 1e-14 or pv > 1e-6 for pv in piv), (p["obs"].shape, b, piv)
    assert worst <= 1e4, worst


def _pivots(S):
    """The pivots of the unit-diagonal matrix in effect order, a pivot below 1e-12 dropped (as regress_ref.solve takes them)."""
    sd = np.sqrt(np.diag(S))
    U = S / np.outer(sd, sd)
    out = []
    for k in range(U.shape[0]):
        out.append(U[k, k])
        keep = U[k, k] >= regress_ref.MIN_PIVOT
        col = U[k + 1:, k] / np.sqrt(U[k, k]) if keep else np.zeros(U.shape[0] - k - 1)
        U[k + 1:, k + 1:] -= np.outer(col, col)
    return out


@pytest.mark.parametrize("bad", ["descending", "inclusive", "ramp_from_zero", "late_sums", "skip_before", "records"])
def test_wrong_variants_are_far_outside_the_bars(bad):
    """On an input of the GPU tier ((8,2), T = 17, M = 16, observation variances and initial moments given, t_first = 1) each wrong
    variant is more than a thousand bars from the restatement, in A or in the solve."""
    import test_regression_gpu as tr

    N, K, T = 8, 2, 17
    p = tr._data(N, K, T, seed=100 * N + T, full=True)
    ef = tr._effects(N, T, 16)
    ef[1] = ef[1][::-1]                                            # the two records' lists differ in every slot but the middle
    b = 2
    good, gain = tr._reference(p, b, ef, 1, dtype=F64)
    if bad == "records":
        wrong, _ = tr._reference(p, b, ef[::-1], 1, gain, dtype=F64)
    else:
        wrong = regress_ref.regression(*tr._args(p, b), effects=ef[b % tr.R_], t_first=1, dtype=F64, gain=gain, **{bad: True})
    dg = np.sqrt(np.abs(np.diag(good["normal"])))
    scale = np.outer(dg, dg)
    scale[scale == 0] = 1.0
    da = np.max(np.abs(wrong["normal"] - good["normal"]) / scale)
    both = ~np.isnan(good["beta"]) & ~np.isnan(wrong["beta"])
    ds = np.max(np.abs(wrong["beta"] - good["beta"])[both] / np.maximum(1, np.abs(good["beta"][both])))
    assert da > 1000 * tr.BAR_A or ds > 1000 * tr.BAR_S, (bad, da, ds)
    assert da > 1000 * tr.BAR_A, (bad, da)


def test_metran_batch_interventions_over_a_stand_in_engine():
    """Units, timestamps, end = None, the unused slots of a model with fewer effects, the cache, and the adjustment with and
    without a mask."""
    models, G = two_models()
    mb = stand_in(RegressEngine, models, G)
    kf = mb.kf
    alpha = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    idx0, idx1 = mb.batch.index[0], mb.batch.index[1]
    L1 = int(mb.batch.lengths[1])
    assert L1 < mb.T
    wanted = [(0, "s1", "level", idx0[20]), (1, "s2", "ramp", 5, 15), (0, "s0", "level", idx0[10], idx0[11]), (0, "s2", "level", 3, 3 + 4)]
    frame = mb.fit_interventions(wanted, alpha=alpha)
    assert kf.calls == 1
    assert list(frame.index) == [(0, 0), (0, 1), (0, 2), (1, 0)]
    assert list(frame.columns) == ["series", "kind", "start", "end", "n_obs", "estimate", "stderr", "t", "pvalue", "dropped"]
    assert list(frame["series"]) == ["s1", "s0", "s2", "s2"] and list(frame["kind"]) == ["level", "level", "level", "ramp"]
    assert frame.loc[(0, 0), "start"] == idx0[20] and frame.loc[(0, 0), "end"] is not frame.loc[(0, 1), "end"]
    assert pd.isna(frame.loc[(0, 0), "end"]) and frame.loc[(0, 1), "end"] == idx0[11] and frame.loc[(1, 0), "end"] == idx1[15]
    table = frame.attrs["effects"]
    assert table.shape == (2, 3, 4) and table[0].tolist() == [[1, 0, 20, int(mb.batch.lengths[0])], [0, 0, 10, 11], [2, 0, 3, 7]]
    assert table[1].tolist() == [[2, 1, 5, 15], [-1, 0, 0, 1], [-1, 0, 0, 1]]          # the unused slots of the model with one effect
    # the numbers: the restatement on the standardised records, scaled by the series' std
    std = mb._std.numpy()
    phi, q = kf.params_from_alpha(torch_(alpha))
    for r in range(2):
        ref = regress_ref.regression(kf.obs_np[r], phi[r].numpy(), q[r].numpy(), G[r], effects=table[r], t_first=1, dtype=F64)
        for m in range(3 if r == 0 else 1):
            row, j = frame.loc[(r, m)], table[r, m, 0]
            assert row["n_obs"] == ref["support"][m] and not row["dropped"]
            assert row["estimate"] == float(ref["beta"][m]) * std[r, j] and row["stderr"] == float(np.sqrt(ref["cov"][m, m])) * std[r, j]
            assert row["t"] == row["estimate"] / row["stderr"] and 0 <= row["pvalue"] <= 1
        pm = frame.attrs["models"].loc[r]
        assert pm["gain"] == float(ref["gain"]) and pm["df"] == (3 if r == 0 else 1) and 0 <= pm["pvalue"] <= 1
    same = mb.fit_interventions(wanted, alpha=alpha, standardized=True)
    assert kf.calls == 1                                           # a second identical request launches nothing
    assert np.allclose(same["estimate"].values * std[[0, 0, 0, 1], [1, 0, 2, 2]], frame["estimate"].values, rtol=1e-15)
    mb.fit_interventions(wanted, alpha=alpha, t_first=2)
    assert kf.calls == 2
    # the objective: obj - gain is the oracle's objective of the adjusted records
    pm = frame.attrs["models"]
    before = mb.get_mle(alpha).numpy()
    obs0 = kf.obs_np.copy()
    assert np.array_equal(pm["obj"].values, before)
    mb.adjust_observations(frame)
    assert mb._cache == {} and not np.array_equal(kf.obs_np, obs0, equal_nan=True)
    after = mb.get_mle(alpha).numpy()
    assert np.all(np.abs((before - after) - pm["gain"].values) <= PARITY_BAR * np.abs(before))
    assert np.allclose(pm["obj_adjusted"].values, after, rtol=PARITY_BAR)
    mb.fit_interventions(wanted, alpha=alpha)
    assert kf.calls == 3                                           # adjust_observations cleared the cache
    adjusted = kf.obs_np.copy()
    # ... with a mask: set after the adjustment it hides adjusted values; unmasking gives adjusted, unmasked records
    mb.unadjust_observations()
    assert np.array_equal(kf.obs_np, obs0, equal_nan=True) and mb._cache == {}
    mask = np.zeros(obs0.shape, dtype=bool)
    mask[:, 12:16, 1] = True
    mb.mask_observations(mask)
    mb.adjust_observations(frame)
    assert np.array_equal(kf.obs_np, np.where(mask, np.nan, adjusted), equal_nan=True)
    mb.unmask_observations()
    assert np.array_equal(kf.obs_np, adjusted, equal_nan=True)
    mb.unadjust_observations()
    assert np.array_equal(kf.obs_np, np.where(mask, np.nan, obs0), equal_nan=True)
    mb.unmask_observations()
    assert np.array_equal(kf.obs_np, obs0, equal_nan=True)
    # refusals of the facade
    with pytest.raises(ValueError):
        mb.fit_interventions([], alpha=alpha)
    with pytest.raises(ValueError):
        mb.fit_interventions([(0, "s1", "step", 3)], alpha=alpha)
    with pytest.raises(ValueError):
        mb.fit_interventions([(0, "s1", "level", 9, 9)], alpha=alpha)
    with pytest.raises(KeyError):
        mb.fit_interventions([(0, "nobody", "level", 9)], alpha=alpha)
    with pytest.raises(IndexError):
        mb.fit_interventions([(2, "s1", "level", 9)], alpha=alpha)
    fresh = stand_in(RegressEngine, models, G)
    with pytest.raises(ValueError):
        fresh.adjust_observations()


def test_a_dropped_effect_in_the_facade():
    """An exact duplicate: the later one is dropped -- NaN estimate, ``dropped`` set, one degree of freedom fewer -- and subtracts
    nothing in ``adjust_observations``."""
    models, G = two_models()
    mb = stand_in(RegressEngine, models, G)
    alpha = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    frame = mb.fit_interventions([(0, "s1", "level", 20), (0, "s1", "level", 20), (1, "s0", "level", 7)], alpha=alpha)
    assert list(frame["dropped"]) == [False, True, False] and np.isnan(frame.loc[(0, 1), "estimate"]) and np.isnan(frame.loc[(0, 1), "stderr"])
    assert list(frame.attrs["models"]["df"]) == [1, 1]
    one = mb.fit_interventions([(0, "s1", "level", 20), (1, "s0", "level", 7)], alpha=alpha)
    assert one.loc[(0, 0), "estimate"] == frame.loc[(0, 0), "estimate"]
    obs0 = mb.kf.obs_np.copy()
    mb.adjust_observations(frame)
    with_duplicate = mb.kf.obs_np.copy()
    mb.adjust_observations(one)
    assert np.array_equal(mb.kf.obs_np, with_duplicate, equal_nan=True) and not np.array_equal(with_duplicate, obs0, equal_nan=True)


def torch_(a):
    import torch

    return torch.as_tensor(a, dtype=torch.float64)
