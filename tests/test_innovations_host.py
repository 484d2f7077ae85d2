"""The numpy restatement of the one-step-ahead innovations and their whiteness statistics (tests/innov_ref.py), pinned
WITHOUT a GPU: to the oracle (the C restatement of seqkalmanfilter) three ways, to the live reference where it is mounted, the
statistics to a direct numpy evaluation, scipy's chi-square and two known answers -- and three deliberately wrong variants
shown to be far outside every bar, so that the GPU tier's yardstick is known to be the right one and able to fail."""
import os
import re

import numpy as np
import pytest

import hard_models
import innov_ref
import oracle
from metran_amd.synthetic import make_dfm_batch

F64 = np.float64


def _models():
    """(y, phi, q, G, R, x0, P0): small models with empty, single-series and full steps, with and without R / x0 / P0."""
    out = []
    for (N, K, T, seed, extra) in ((5, 1, 30, 1, False), (8, 2, 24, 2, True), (4, 3, 17, 3, True), (3, 1, 1, 4, False)):
        d = make_dfm_batch(1, N, K, T, seed=seed, missing=0.3)
        y = d["obs"][0].copy()
        if T > 8:
            y[0] = np.nan                 # an empty first step
            y[3] = np.nan                 # an empty step
            y[5, 1:] = np.nan             # one observed series
            y[5, 0] = 0.25
            y[7] = np.where(np.isfinite(y[7]), y[7], -0.5)   # all observed
        rng = np.random.default_rng(seed)
        n = N + K
        R = rng.uniform(0.05, 0.4, N) * (rng.random(N) < 0.6) if extra else None
        x0 = rng.normal(size=n) if extra else None
        A = rng.normal(size=(n, n))
        P0 = A @ A.T / n + 0.5 * np.eye(n) if extra else None
        out.append((y, d["phi"][0], d["q"][0], d["loadings"][0], R, x0, P0))
    return out


MODELS = _models()


def _oracle(y, phi, q, G, R, x0, P0):
    N, K = G.shape
    n = N + K
    Z = np.concatenate([np.eye(N), G], axis=1)
    o, oi, oc = oracle.set_observations(y)
    sg, df, sc, F, Pf, Xp, Pp = oracle.seqkalmanfilter(o, np.diag(phi), np.diag(q), Z, np.zeros(N) if R is None else R, oi, oc,
                                                       np.zeros(n) if x0 is None else x0, np.eye(n) if P0 is None else P0)
    return dict(sigmas=sg, detfs=df, sc=int(sc), F=F, Pf=Pf, Xp=Xp, Pp=Pp, Z=Z)


def _step_sums(v, f):
    """sigma = sum_j v^2 / f and detf = sum_j log f per step with an observation, left to right (kalmanfilter.py:377-382)."""
    sig, det = [], []
    for t in range(v.shape[0]):
        js = np.nonzero(np.isfinite(v[t]))[0]
        if js.size == 0:
            continue
        s = d = type(v[t, 0])(0)
        for j in js:
            s = s + v[t, j] * v[t, j] / f[t, j]
            d = d + np.log(f[t, j])
        sig.append(s)
        det.append(d)
    return np.array(sig, dtype=F64), np.array(det, dtype=F64)


@pytest.mark.parametrize("m", range(len(MODELS)))
def test_step_sums_are_the_oracles(m):
    """sum_j v^2/f and sum_j log f of every observed step are the oracle's sigmas / detfs (compressed indexing), at the bar
    tests/test_oracle_golden.py holds the filter to -- with the restatement run in the oracle's own arithmetic (float64)."""
    y, phi, q, G, R, x0, P0 = MODELS[m]
    ref = _oracle(*MODELS[m])
    r = innov_ref.innovations(y, phi, q, G, R, x0, P0, dtype=F64)
    assert np.array_equal(np.isnan(r["v"]), ~np.isfinite(y)) and np.array_equal(np.isnan(r["f"]), ~np.isfinite(y))
    sig, det = _step_sums(r["v"], r["f"])
    assert len(sig) == ref["sc"]
    np.testing.assert_allclose(sig, ref["sigmas"][:ref["sc"]], rtol=4e-16 * y.shape[1], atol=0)
    np.testing.assert_allclose(det, ref["detfs"][:ref["sc"]], rtol=0, atol=1e-13)
    np.testing.assert_allclose(r["F"], ref["F"], rtol=0, atol=1e-14)
    # ... and the extended-precision run of the same recursion (the GPU tier's yardstick) is the same numbers to double rounding
    rl = innov_ref.innovations(y, phi, q, G, R, x0, P0)
    big = max(1.0, np.nanmax(np.abs(y)))
    seen = np.isfinite(y)
    np.testing.assert_allclose(r["v"][seen], rl["v"][seen].astype(F64), rtol=0, atol=1e-12 * big)
    np.testing.assert_allclose(r["f"][seen], rl["f"][seen].astype(F64), rtol=1e-12, atol=0)


@pytest.mark.parametrize("m", range(len(MODELS)))
def test_brute_force_cells(m):
    """Cell (t, j): with the cells (t, >= j) masked the oracle's filtered moments of step t are the state the update of series
    j starts from, so v = y - z_j F[t], f = z_j Pf[t] z_j' + r_j; the marginal forecast comes from its Xp[t], Pp[t]."""
    y, phi, q, G, R, x0, P0 = MODELS[m]
    N = y.shape[1]
    Rv = np.zeros(N) if R is None else R
    rng = np.random.default_rng(m)
    scale, offset = rng.uniform(0.5, 3.0, N), rng.normal(size=N)
    r = innov_ref.innovations(y, phi, q, G, R, x0, P0, scale, offset)
    full = _oracle(y, phi, q, G, R, x0, P0)
    Z = full["Z"]
    big = max(1.0, np.nanmax(np.abs(y)))
    cells = np.argwhere(np.isfinite(y))
    for t, j in cells[rng.choice(len(cells), size=min(12, len(cells)), replace=False)]:
        ym = y.copy()
        ym[t, j:] = np.nan
        o = _oracle(ym, phi, q, G, R, x0, P0)
        v = y[t, j] - Z[j] @ o["F"][t]
        f = Z[j] @ o["Pf"][t] @ Z[j] + Rv[j]
        assert abs(float(r["v"][t, j]) - v) <= 1e-12 * big, (t, j)
        assert abs(float(r["f"][t, j]) - f) <= 1e-12 * abs(f), (t, j)
    pm = np.einsum("jn,tn->tj", Z, full["Xp"]) * scale + offset
    pv = np.maximum(np.einsum("jn,tnm,jm->tj", Z, full["Pp"], Z) + Rv, 0.0) * scale ** 2
    np.testing.assert_allclose(r["pred_mean"].astype(F64), pm, rtol=0, atol=1e-12 * max(1.0, np.abs(pm).max()))
    np.testing.assert_allclose(r["pred_var"].astype(F64), pv, rtol=1e-12, atol=0)


@pytest.mark.parametrize("m", range(len(MODELS)))
def test_first_observed_series_is_the_marginal_forecast(m):
    y, phi, q, G, R, x0, P0 = MODELS[m]
    r = innov_ref.innovations(y, phi, q, G, R, x0, P0)
    for t in range(y.shape[0]):
        js = np.nonzero(np.isfinite(y[t]))[0]
        if js.size:
            j = js[0]
            assert abs(float(r["v"][t, j] - (y[t, j] - r["pred_mean"][t, j]))) <= 1e-15 * max(1.0, abs(y[t, j]))
            assert abs(float(r["f"][t, j] - r["pred_var"][t, j])) <= 1e-15 * abs(float(r["f"][t, j]))


def test_hard_models_step_sums():
    """The property sweep's hard models: the step sums against the oracle within that file's conditioning-aware bars."""
    for (N, K, T, B), g in hard_models.groups(per_shape=16, shapes=[(5, 1), (8, 2)]):
        for b in range(0, B, 2):
            ref = hard_models.oracle_model(oracle, g, b, smooth=False)
            Rb = None if g["obsvar"] is None else g["obsvar"][b]
            r = innov_ref.innovations(g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b], Rb,
                                      None if g["x0"] is None else g["x0"][b], None if g["P0"] is None else g["P0"][b])
            sig, _ = _step_sums(r["v"], r["f"])
            sc = ref["sigmacount"]
            atol, _ = hard_models.filter_tolerances(g, b, ref)
            assert len(sig) == sc
            np.testing.assert_allclose(sig, ref["sigmas"][:sc], rtol=1e-9, atol=atol, err_msg=str((N, K, T, b, g["patterns"][b])))


def test_live_reference_step_sums():
    """Where the reference is mounted: the same sums against the reference's own seqkalmanfilter."""
    from golden import _refshim

    if not _refshim.reference_available():
        pytest.skip("reference not mounted")
    metran = _refshim.install()
    from metran.kalmanfilter import seqkalmanfilter

    y, phi, q, G, R, x0, P0 = MODELS[1]
    N, K = G.shape
    n = N + K
    o, oi, oc = oracle.set_observations(y)
    Z = np.concatenate([np.eye(N), G], axis=1)
    # copies: run as plain Python the reference writes its filtered moments into the initial arrays it is handed
    sg, df, sc = seqkalmanfilter(o, np.diag(phi), np.diag(q), Z, R, oi, oc, x0.copy(), P0.copy())[:3]
    r = innov_ref.innovations(y, phi, q, G, R, x0, P0, dtype=F64)
    sig, det = _step_sums(r["v"], r["f"])
    assert metran is not None and len(sig) == int(sc)
    np.testing.assert_allclose(sig, sg[:int(sc)], rtol=4e-16 * N, atol=0)
    np.testing.assert_allclose(det, df[:int(sc)], rtol=0, atol=1e-13)


# ------------------------------------------------------------------------------------------------------------ statistics
def _direct(e, L):
    """Ljung-Box on a compacted series by the textbook formulas, numpy float64."""
    m = len(e)
    c = e - e.mean()
    acf = np.array([np.sum(c[: m - l] * c[l:]) / m for l in range(L + 1)])
    r = acf[1:] / acf[0]
    return m, e.mean(), acf[0], m * (m + 2) * np.sum(r ** 2 / (m - np.arange(1, L + 1))), r


def test_stats_against_direct_evaluation_and_chi2():
    from scipy.stats import chi2

    rng = np.random.default_rng(11)
    T, N, L = 200, 3, 10
    v = rng.normal(size=(T, N))
    f = rng.uniform(0.5, 2.0, (T, N))
    v[rng.random((T, N)) < 0.4] = np.nan
    f[5, 0] = np.nan          # a cell without a variance does not count
    f[6, 1] = -1.0            # nor one with a non-positive variance
    for t_first in (0, 1, 17):
        s = innov_ref.stats(v, f, L, t_first).astype(F64)
        for j in range(N):
            ok = np.isfinite(v[:, j]) & np.isfinite(f[:, j]) & (f[:, j] > 0) & (np.arange(T) >= t_first)
            m, mean, c0, Q, r = _direct(v[ok, j] / np.sqrt(f[ok, j]), L)
            assert s[j, 0] == m
            np.testing.assert_allclose(s[j, 1:4], [mean, c0, Q], rtol=1e-12)
            np.testing.assert_allclose(s[j, 4:], r, rtol=0, atol=1e-13)
            # the p-value of the facade: the upper tail of chi-square with L degrees of freedom
            assert abs(chi2.sf(s[j, 3], L) - (1.0 - chi2.cdf(Q, L))) <= 1e-12
    # white noise is not rejected, a strongly autocorrelated series is
    e = rng.normal(size=(2000, 1))
    ar = np.zeros(2000)
    for t in range(1, 2000):
        ar[t] = 0.8 * ar[t - 1] + e[t, 0]
    one = np.ones((2000, 1))
    assert chi2.sf(float(innov_ref.stats(e, one, 10)[0, 3]), 10) > 1e-3
    assert chi2.sf(float(innov_ref.stats(ar[:, None], one, 10)[0, 3]), 10) < 1e-12


def test_stats_known_answers():
    m, L = 21, 4
    alt = np.array([(-1.0) ** i for i in range(m)])[:, None]
    # ... with gaps between the cells: the lag counts successive valid cells
    v = np.full((3 * m, 1), np.nan)
    v[::3] = alt
    s = innov_ref.stats(v, np.ones_like(v), L)
    # an alternating +-1 series of even length m has mean 0 and c_0 = 1, so r_1 = -(m - 1)/m exactly
    m2 = 20
    v2 = np.full((2 * m2, 1), np.nan)
    v2[::2, 0] = [(-1.0) ** i for i in range(m2)]
    s2 = innov_ref.stats(v2, np.ones_like(v2), L)
    assert s2[0, 0] == m2 and s2[0, 1] == 0 and s2[0, 2] == 1
    assert abs(float(s2[0, 4]) + (m2 - 1) / m2) <= 1e-18
    assert s[0, 0] == m and float(s[0, 4]) < -0.9
    const = innov_ref.stats(np.full((30, 1), 0.5), np.full((30, 1), 0.25), L)   # e = 1 exactly
    assert const[0, 0] == 30 and const[0, 1] == 1 and const[0, 2] == 0 and np.isnan(const[0, 3:]).all()
    few = innov_ref.stats(np.arange(4.0)[:, None], np.ones((4, 1)), L)          # m = L: no statistics
    assert few[0, 0] == 4 and np.isfinite(few[0, 1:3]).all() and np.isnan(few[0, 3:]).all()
    none = innov_ref.stats(np.full((4, 1), np.nan), np.ones((4, 1)), L)
    assert none[0, 0] == 0 and np.isnan(none[0, 1:]).all()


# ------------------------------------------------------------------------------------------------ the tests can fail
def test_wrong_variants_are_far_outside_the_bars():
    y, phi, q, G, R, x0, P0 = MODELS[1]
    good = innov_ref.innovations(y, phi, q, G, R, x0, P0)
    seen = np.isfinite(y)
    big = max(1.0, np.nanmax(np.abs(y)))
    for kw in (dict(descending=True), dict(record_of_step=True)):
        bad = innov_ref.innovations(y, phi, q, G, R, x0, P0, **kw)
        assert float(np.max(np.abs(bad["v"][seen] - good["v"][seen]))) > 1e6 * 1e-12 * big, kw
        assert float(np.max(np.abs(bad["f"][seen] / good["f"][seen] - 1))) > 1e6 * 1e-12, kw
    bad = innov_ref.innovations(y, phi, q, G, R, x0, P0, record_of_step=True)
    assert float(np.max(np.abs(bad["pred_mean"] - good["pred_mean"]))) > 1e6 * 1e-12 * big
    # descending order changes v and f of the cells but not the step sums' meaning -- and not the marginal forecast
    bad = innov_ref.innovations(y, phi, q, G, R, x0, P0, descending=True)
    assert float(np.max(np.abs(bad["pred_mean"] - good["pred_mean"]))) <= 1e-15 * big
    # lags in calendar steps: far from lags in valid cells on a sparse record
    s = innov_ref.stats(good["v"], good["f"], 3)
    c = innov_ref.stats(good["v"], good["f"], 3, calendar=True)
    ok = np.isfinite(s[:, 4]) & np.isfinite(c[:, 4])
    assert ok.any() and float(np.max(np.abs(s[ok, 4:] - c[ok, 4:]))) > 1e6 * 1e-10


# ------------------------------------------------------------------------------------------- the kernel's time tile
TILE = 64   # innov_stats_kernel: time steps per pass of a wavefront (tests/test_innovations_gpu.py runs T = TILE - 1, TILE, TILE + 1)


def test_time_tile_is_what_the_kernel_source_says():
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metran_amd", "csrc", "innov_kernels.hip")).read()
    assert re.search(r"constexpr int kInnovTile = %d;" % TILE, src)
    assert "t0 += kInnovTile" in src and re.search(r"constexpr int innov_max_lags = 32;", open(os.path.join(
        os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "metran_amd", "csrc", "innov_kernels.h")).read())
