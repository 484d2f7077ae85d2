"""The restatements of the smoothed state disturbances (tests/disturbance_ref.py), pinned WITHOUT a GPU: the kernel's walk in
numpy against the definition from the oracle's smoothed moments and against the dense joint Gaussian; four deliberately wrong
read-outs shown to be far outside every bar; a level shift injected into one state is found where it was put; and the
MetranBatch accessors over a stand-in engine that answers from the restatement."""
import numpy as np
import pytest

import disturbance_ref as dr
import oracle
from metran_amd.synthetic import make_dfm_batch

SMOOTH_BAR = 1e-9     # the smoother's existing bar (tests/test_hip_parity.py: SMOOTH_ATOL), in the units of q r and q - q^2 N
RAW_TOL = 1e-12       # the GPU tier's bar on the raw pair against dist_adjoint (tests/test_loo_gpu.py's against its restatement)
VARIANTS = ("after_phi", "before_updates", "no_rr", "shifted")


def _models():
    """(y, phi, q, G, R, x0, P0): missing data, an empty step, a one-series step and a full step; with and without R, x0 / P0."""
    out = []
    for (N, K, T, seed, with_r, with_init) in ((8, 2, 24, 1, False, False), (5, 1, 6, 2, False, True), (12, 3, 16, 3, True, False),
                                               (32, 4, 10, 4, False, False), (3, 1, 5, 5, False, False)):
        d = make_dfm_batch(1, N, K, T, seed=seed, missing=0.3)
        y = d["obs"][0].copy()
        y[2] = np.nan                                         # an empty step
        y[1, 1:] = np.nan                                     # one observed series
        y[1, 0] = 0.25
        y[3] = np.where(np.isfinite(y[3]), y[3], -0.5)        # all observed
        rng = np.random.default_rng(seed)
        n = N + K
        R = rng.uniform(0.05, 0.4, N) * (rng.random(N) < 0.6) if with_r else None
        x0 = rng.normal(size=n) if with_init else None
        A = rng.normal(size=(n, n))
        P0 = A @ A.T / n + 0.5 * np.eye(n) if with_init else None
        out.append((y, d["phi"][0], d["q"][0], d["loadings"][0], R, x0, P0))
    return out


MODELS = _models()
IDS = ["%dx%d" % m[3].shape for m in MODELS]


def _oracle(y, phi, q, G, R, x0, P0):
    N, K = G.shape
    n = N + K
    Z = np.concatenate([np.eye(N), G], axis=1)
    o, oi, oc = oracle.set_observations(y)
    _, _, _, F, Pf, Xp, Pp = oracle.seqkalmanfilter(o, np.diag(phi), np.diag(q), Z, np.zeros(N) if R is None else R, oi, oc,
                                                    np.zeros(n) if x0 is None else x0, np.eye(n) if P0 is None else P0)
    S, Ps = oracle.kalmansmoother(F, Pf, Xp, Pp, np.diag(phi))
    return F, Pf, Xp, Pp, S, Ps


@pytest.mark.parametrize("m", range(len(MODELS)), ids=IDS)
def test_adjoint_walk_is_the_definition(m):
    """q r and q - q^2 N of the walk are S_t - phi o S_{t-1} and the variance through the lag-one covariance, for t >= 1."""
    y, phi, q, G, R, x0, P0 = MODELS[m]
    r, ninfo = dr.dist_adjoint(y, phi, q, G, R, x0, P0)
    mean, var = dr.moments(q, r, ninfo)
    dmean, dvar = dr.dist_definition(phi, q, *_oracle(y, phi, q, G, R, x0, P0))
    assert np.isnan(dmean[0]).all() and np.isfinite(dmean[1:]).all()
    em, ev = np.abs(mean[1:] - dmean[1:]).max(), np.abs(var[1:] - dvar[1:]).max()
    print("dist_adjoint against dist_definition %s: mean %.2e, variance %.2e" % (IDS[m], em, ev))
    assert em <= SMOOTH_BAR and ev <= SMOOTH_BAR
    # the share of the disturbance's variance that the data determine lies in [0, 1]
    share = q * ninfo
    assert (share >= 0).all() and (share <= 1 + 1e-12).all()
    # behind the last observation nothing is determined
    last = np.nonzero(np.isfinite(y).any(1))[0][-1]
    assert not r[last + 1:].any() and not ninfo[last + 1:].any()


@pytest.mark.parametrize("m", [i for i, mod in enumerate(MODELS) if mod[0].shape[0] <= 6 and sum(mod[3].shape) <= 6],
                         ids=lambda i: IDS[i])
def test_adjoint_walk_is_the_joint_gaussian(m):
    """... and, t = 0 and the caller's x0 / P0 included, the conditional moments of the dense joint Gaussian."""
    y, phi, q, G, R, x0, P0 = MODELS[m]
    r, ninfo = dr.dist_adjoint(y, phi, q, G, R, x0, P0)
    mean, var = dr.moments(q, r, ninfo)
    jmean, jvar = dr.dist_joint(y, phi, q, G, R, x0, P0)
    em, ev = np.abs(mean - jmean).max(), np.abs(var - jvar).max()
    print("dist_adjoint against dist_joint %s: mean %.2e, variance %.2e" % (IDS[m], em, ev))
    assert em <= SMOOTH_BAR and ev <= SMOOTH_BAR
    dmean, dvar = dr.dist_definition(phi, q, *_oracle(y, phi, q, G, R, x0, P0))
    assert np.abs(jmean[1:] - dmean[1:]).max() <= SMOOTH_BAR and np.abs(jvar[1:] - dvar[1:]).max() <= SMOOTH_BAR


def test_the_joint_reference_covers_both_small_models():
    assert [IDS[i] for i, mod in enumerate(MODELS) if mod[0].shape[0] <= 6 and sum(mod[3].shape) <= 6] == ["5x1", "3x1"]


@pytest.mark.parametrize("variant", VARIANTS)
@pytest.mark.parametrize("m", range(len(MODELS)), ids=IDS)
def test_wrong_read_outs_are_far_outside_the_bars(m, variant):
    """Each mistake moves the moments by at least 1000 of the smoother's bars, and the raw pair by at least 1000 of its own."""
    y, phi, q, G, R, x0, P0 = MODELS[m]
    r, ninfo = dr.dist_adjoint(y, phi, q, G, R, x0, P0)
    br, bn = dr.dist_adjoint(y, phi, q, G, R, x0, P0, variant=variant)
    mean, var = dr.moments(q, r, ninfo)
    bmean, bvar = dr.moments(q, br, bn)
    assert max(np.abs(bmean - mean).max(), np.abs(bvar - var).max()) >= 1000 * SMOOTH_BAR
    far_r = np.abs(br - r).max() / (RAW_TOL * max(1.0, np.abs(r).max()))
    far_n = np.abs(bn - ninfo).max() / (RAW_TOL * max(1.0, np.abs(ninfo).max()))
    assert max(far_r, far_n) >= 1000


def test_unit_spread_on_simulated_data():
    """u = r / sqrt(N) has unit spread on data simulated from the model."""
    d = make_dfm_batch(1, 5, 1, 1500, seed=12, missing=0.2)
    r, ninfo = dr.dist_adjoint(d["obs"][0], d["phi"][0], d["q"][0], d["loadings"][0])
    u = r[50:-50] / np.sqrt(ninfo[50:-50])
    assert np.isfinite(u).all()
    # 1400 correlated values a state: the sample spread is within a few percent of 1 (3 / sqrt(2 * 1400 / 10), ten steps of memory)
    assert np.all(np.abs(u.std(axis=0) - 1.0) < 0.18) and np.all(np.abs(u.mean(axis=0)) < 0.25)


# ---- a level shift is found where it was put ----
SHIFT_T, SHIFT_STATE, SHIFT_SIZE = 37, 2, 3.0


def _shift_record():
    """(y, y with a disturbance of SHIFT_SIZE injected into state SHIFT_STATE at step SHIFT_T, phi, q, loadings): the shift
    decays with the state's own persistence, as a disturbance of the state equation does."""
    d = make_dfm_batch(1, 5, 1, 90, seed=21, missing=0.0)
    y, phi = d["obs"][0].copy(), d["phi"][0]
    ys = y.copy()
    k = np.arange(y.shape[0] - SHIFT_T)
    ys[SHIFT_T:, SHIFT_STATE] += SHIFT_SIZE * phi[SHIFT_STATE] ** k
    return y, ys, phi, d["q"][0], d["loadings"][0]


def test_level_shift_is_the_largest_residual():
    y, ys, phi, q, G = _shift_record()
    u = {}
    for key, obs in (("plain", y), ("shift", ys)):
        r, ninfo = dr.dist_adjoint(obs, phi, q, G)
        u[key] = np.abs(r / np.sqrt(ninfo))[1:]
    assert np.unravel_index(np.argmax(u["shift"]), u["shift"].shape) == (SHIFT_T - 1, SHIFT_STATE)
    assert np.unravel_index(np.argmax(u["plain"]), u["plain"].shape) != (SHIFT_T - 1, SHIFT_STATE)
    assert u["shift"][SHIFT_T - 1, SHIFT_STATE] > 5.0 > u["plain"].max()
    # the smoothed disturbance itself recovers most of the shift
    r, _ = dr.dist_adjoint(ys, phi, q, G)
    r0, _ = dr.dist_adjoint(y, phi, q, G)
    assert abs(q[SHIFT_STATE] * (r - r0)[SHIFT_T, SHIFT_STATE] - SHIFT_SIZE) < 0.5 * SHIFT_SIZE


# ---- MetranBatch over a stand-in engine ----
def _stand_in(models, loadings):
    """A MetranBatch whose engine answers ``disturbances`` from dist_adjoint (the constructor itself needs a GPU)."""
    import torch

    from batch_standin import stand_in
    from oracle_engine import OracleEngine

    class DisturbanceEngine(OracleEngine):
        calls = 0
        status_bits = 0

        def disturbances(self, phi, q, x0=None, P0=None, buffers=None):
            self.calls += 1
            phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
            rr, nn = [], []
            for i, r in enumerate(self._records(phi.shape[0])):
                a, b = dr.dist_adjoint(self.obs_np[r], phi[i], q[i], self.load_np[r])
                rr.append(a)
                nn.append(b)
            return {"r": torch.from_numpy(np.stack(rr)), "ninfo": torch.from_numpy(np.stack(nn)),
                    "status": torch.full((phi.shape[0],), self.status_bits, dtype=torch.int32)}

    return stand_in(DisturbanceEngine, models, loadings)


def test_metran_batch_accessors_over_a_stand_in_engine():
    from scipy.stats import norm

    from batch_standin import two_models
    from metran_amd._lib import MetranHipError
    from metran_amd.params import phi_q_from_alpha

    models, G = two_models()
    mb = _stand_in(models, G)
    alpha = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    phi, q = phi_q_from_alpha(alpha, G, 1.0)
    raw = [dr.dist_adjoint(mb.kf.obs_np[r], phi[r], q[r], G[r]) for r in range(2)]
    L = [int(v) for v in mb.batch.lengths]
    assert L[1] < L[0] == mb.T

    # units: mean = q r, variance = q - q^2 N clipped at 0, padding steps included
    mean, var = (t.numpy() for t in mb.get_state_disturbances(alpha))
    assert mean.shape == var.shape == (2, mb.T, 4)
    for r in range(2):
        np.testing.assert_allclose(mean[r], q[r] * raw[r][0], rtol=0, atol=1e-15)
        np.testing.assert_allclose(var[r], np.maximum(q[r] - q[r] ** 2 * raw[r][1], 0.0), rtol=0, atol=1e-15)
    assert (var >= 0).all() and (var <= q[:, None, :] + 1e-15).all()
    assert mb.kf.calls == 1

    # the residuals: r / sqrt(N) from the raw pair, NaN beyond the model's own length and below the information threshold
    u = mb.get_auxiliary_residuals(alpha).numpy()
    assert mb.kf.calls == 1 and "dist" in mb._cache          # one cached run per parameter set
    for r in range(2):
        share = q[r] * raw[r][1]
        ok = (share >= 1e-6) & (np.arange(mb.T) < L[r])[:, None]
        assert np.array_equal(np.isfinite(u[r]), ok)
        # (one square root and one division, in torch there and in numpy here: two roundings)
        np.testing.assert_allclose(u[r][ok], raw[r][0][ok] / np.sqrt(raw[r][1][ok]), rtol=4 * np.finfo(float).eps, atol=0)
    assert np.isnan(u[1, L[1]:]).all() and np.isfinite(u[1, 1:L[1] - 8]).all()
    last = [np.nonzero(np.isfinite(mb.kf.obs_np[r]).any(1))[0][-1] for r in range(2)]
    assert all(np.isnan(u[r, last[r] + 1:]).all() for r in range(2))   # behind the last observation: no information
    strict = mb.get_auxiliary_residuals(alpha, min_information=0.3).numpy()
    for r in range(2):
        ok = (q[r] * raw[r][1] >= 0.3) & (np.arange(mb.T) < L[r])[:, None]
        assert np.array_equal(np.isfinite(strict[r]), ok) and 0 < ok.sum() < np.isfinite(u[r]).sum()
    assert mb.kf.calls == 1
    mb.get_auxiliary_residuals(alpha * 1.01)
    assert mb.kf.calls == 2                                   # another parameter set: another run

    # one state's frame, on the model's own index with get_state's columns
    frame = mb.get_state_disturbance(1, 3, alpha=alpha)
    assert mb.kf.calls == 3 and list(frame.columns) == ["mean", "lower", "upper"]
    assert frame.shape[0] == L[1] and frame.index.equals(mb.batch.index[1])
    np.testing.assert_array_equal(frame["mean"].values, mean[1, :L[1], 3])
    half = norm.ppf(0.975) * np.sqrt(var[1, :L[1], 3])
    np.testing.assert_allclose(frame["upper"].values - frame["mean"].values, half, rtol=0, atol=1e-14)
    np.testing.assert_allclose(frame["mean"].values - frame["lower"].values, half, rtol=0, atol=1e-14)
    assert mb.get_state_disturbance(0, 0, alpha=alpha, ci=None).name == "s0_sdf"
    with pytest.raises(IndexError):
        mb.get_state_disturbance(0, 4, alpha=alpha)

    # the screen: one row per (model, state), Sidak-corrected two-sided normal p-value of the largest residual
    table = mb.screen_breaks(alpha)
    assert list(table.columns) == ["max_abs_u", "time", "nobs", "pvalue"] and list(table.index.names) == ["model", "state"]
    assert list(table.index) == [(r, name) for r in range(2) for name in ("s0_sdf", "s1_sdf", "s2_sdf", "cdf1")]
    for r in range(2):
        for i, name in enumerate(("s0_sdf", "s1_sdf", "s2_sdf", "cdf1")):
            col = np.abs(u[r, 1:L[r], i])
            m = int(np.isfinite(col).sum())
            row = table.loc[(r, name)]
            assert row["nobs"] == m and row["max_abs_u"] == np.nanmax(col)
            assert row["time"] == mb.batch.index[r][1 + int(np.nanargmax(col))]
            want = 1.0 - (1.0 - 2.0 * norm.sf(np.nanmax(col))) ** m
            assert abs(row["pvalue"] - want) <= 1e-12
    t0 = mb.screen_breaks(alpha, t_first=0)
    assert (t0["nobs"].values >= table["nobs"].values).all() and (t0["nobs"].values > table["nobs"].values).any()
    none = mb.screen_breaks(alpha, min_information=2.0)      # a share above 1 does not exist: no residual anywhere
    assert (none["nobs"] == 0).all() and none[["max_abs_u", "pvalue"]].isna().all().all() and none["time"].isna().all()
    # the p-value formula keeps its accuracy where 1 - (1 - p)^m would cancel
    tiny = -np.expm1(30 * np.log1p(-2.0 * norm.cdf(-9.0)))
    assert abs(tiny / (30 * 2.0 * norm.sf(9.0)) - 1.0) < 1e-12

    mb.kf.status_bits = 1   # FLAG_NONPOSITIVE_F
    with pytest.raises(MetranHipError, match="innovation variance"):
        mb.get_auxiliary_residuals(alpha * 1.02)


def test_screen_breaks_ranks_the_shifted_state_first():
    import pandas as pd

    y, ys, phi, q, G = _shift_record()
    idx = pd.date_range("2003-05-01", periods=y.shape[0], freq="D")
    alpha = (-1.0 / np.log(phi))[None]
    tables = {}
    for key, obs in (("plain", y), ("shift", ys)):
        mb = _stand_in([[pd.Series(obs[:, j], index=idx, name="w%d" % j) for j in range(obs.shape[1])]], G[None])
        tables[key] = mb.screen_breaks(alpha)
    first = tables["shift"].sort_values("pvalue").index[0]
    assert first == (0, "w%d_sdf" % SHIFT_STATE)
    assert tables["shift"].loc[first, "time"] == idx[SHIFT_T] and tables["shift"].loc[first, "pvalue"] < 1e-4
    assert tables["shift"]["max_abs_u"].idxmax() == first
    # ... and the record without the shift does not point there
    plain = tables["plain"].loc[first]
    assert plain["time"] != idx[SHIFT_T] and plain["max_abs_u"] < 0.5 * tables["shift"].loc[first, "max_abs_u"]
