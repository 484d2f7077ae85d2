"""MetranBatch: the accessors of metran.Metran (metran/metran.py:605-989) for several models at once,
against the goldens produced by the reference itself on examples/data (tests/golden/make_golden.py)."""
import numpy as np
import pandas as pd
import pytest

from conftest import load_golden

pytestmark = pytest.mark.gpu


def _g1_series(g1):
    idx = pd.DatetimeIndex(g1["index_ns"].astype("datetime64[ns]"))
    raw = g1["obs"] * g1["oseries_std"] + g1["oseries_mean"]
    return [pd.Series(raw[:, j], index=idx, name="B21B021400%d" % (j + 1)).dropna() for j in range(raw.shape[1])]


def test_facade_on_examples_data(g1):
    from metran_amd.batch import MetranBatch

    gs = load_golden("g1_solve.npz")
    series = _g1_series(g1)
    short = [s.iloc[: len(s) // 2] for s in series]           # a second, shorter model: padded record
    mb = MetranBatch([series, short], factors=g1["loadings"])
    assert (mb.R, mb.T, mb.N, mb.K) == (2, 6255, 5, 1)
    astar = np.stack([g1["alpha_star"], g1["alpha_star"]])
    mle = mb.get_mle(astar).cpu().numpy()
    assert abs(mle[0] - 2332.327069381027) < 1e-6            # BASELINE.md G1 (standardisation done on the device)
    # get_simulation == the reference's (first 50 rows, mean/lower/upper), both methods of projection
    sim = mb.get_simulation(0, "B21B0214005", alpha=astar, ci=0.05)
    np.testing.assert_allclose(sim.values[:50, 0], g1["get_simulation_005"][:, 0], rtol=0, atol=1e-8)
    # the bounds carry sqrt(variance): at observed dates the variance is 0 up to ~1e-15 of rounding, whose
    # square root is ~5e-8
    np.testing.assert_allclose(sim.values[:50, 1:], g1["get_simulation_005"][:, 1:], rtol=0, atol=5e-7)
    assert list(sim.columns) == ["mean", "lower", "upper"] and sim.shape[0] == 6255
    m = mb.get_simulated_means(astar)[0].cpu().numpy()
    np.testing.assert_allclose(m, g1["sim_means"] + g1["oseries_mean"], rtol=0, atol=1e-8)
    v = mb.get_simulated_variances(astar)[0].cpu().numpy()
    np.testing.assert_allclose(v, g1["sim_vars"], rtol=0, atol=1e-8)
    mf = mb.get_simulated_means(astar, method="filter")[0].cpu().numpy()
    np.testing.assert_allclose(mf[g1["tsel"]], g1["simf_means"] + g1["oseries_mean"], rtol=0, atol=1e-8)
    vf = mb.get_simulated_variances(astar, method="filter")[0].cpu().numpy()
    np.testing.assert_allclose(vf[g1["tsel"]], g1["simf_vars"], rtol=0, atol=1e-8)
    # smoothed states with the reference's column names
    st = mb.get_state_means(0, astar)
    assert list(st.columns) == ["B21B021400%d_sdf" % i for i in range(1, 6)] + ["cdf1"]
    np.testing.assert_allclose(st.values[:5], g1["state_means_head"], rtol=0, atol=1e-8)
    np.testing.assert_allclose(st.values[-5:], g1["state_means_tail"], rtol=0, atol=1e-8)
    # decompose_simulation / get_state_variances / get_state (metran.py:682-756, 885-942) vs the reference's
    dec = mb.decompose_simulation(0, "B21B0214001", alpha=astar)
    assert list(dec.columns) == ["sdf", "cdf1"]
    np.testing.assert_allclose(dec.values[:50], g1["decompose_001"], rtol=0, atol=1e-8)
    sv = mb.get_state_variances(0, astar)
    assert list(sv.columns) == list(st.columns)
    np.testing.assert_allclose(sv.values[g1["tsel"]], np.diagonal(g1["Ps"], axis1=1, axis2=2), rtol=0, atol=1e-8)
    s0 = mb.get_state(0, 0, astar)
    from scipy.stats import norm

    assert list(s0.columns) == ["mean", "lower", "upper"]
    np.testing.assert_allclose(s0["mean"].values, g1["S"][:, 0], rtol=0, atol=1e-8)
    np.testing.assert_allclose((s0["upper"] - s0["mean"]).values[g1["tsel"]], norm.ppf(0.975) * np.sqrt(g1["Ps"][:, 0, 0]),
                               rtol=0, atol=1e-7)
    ff = mb.get_state_means(0, astar, method="filter")
    np.testing.assert_allclose(ff.values, g1["F"], rtol=0, atol=1e-8)
    # the result cache (metran.py:978-989): the accessors above launched one run per kind for this parameter set
    assert set(mb._cache) == {"project", "smoother", "filter"}
    before = {k: id(v[1]) for k, v in mb._cache.items()}
    mb.get_simulation(0, "B21B0214002", alpha=astar), mb.get_state(0, 3, astar), mb.decompose_simulation(1, "B21B0214003", astar)
    assert {k: id(v[1]) for k, v in mb._cache.items()} == before
    mb.get_state_means(0, astar * 1.01)   # another parameter set: recomputed
    assert id(mb._cache["smoother"][1]) != before["smoother"]
    # masking (metran.py:464-506): the projection at the masked date changes and the cache is dropped
    import torch

    mask = torch.zeros((2, 6255, 5), dtype=torch.uint8)
    mask[0, int(g1["mask_t"]), 4] = 1
    mb.mask_observations(mask)
    msim = mb.get_simulation(0, "B21B0214005", alpha=astar, ci=None)
    np.testing.assert_allclose(msim.values, g1["masked_sim_005"].ravel(), rtol=0, atol=1e-7)
    mb.unmask_observations()
    np.testing.assert_allclose(mb.get_simulation(0, "B21B0214005", alpha=astar, ci=None).values[:50],
                               g1["get_simulation_005"][:, 0], rtol=0, atol=1e-8)
    # the padded model returns frames of its own length
    assert mb.get_simulation(1, "B21B0214001", alpha=astar).shape[0] == int(mb.batch.lengths[1]) < 6255
    with pytest.raises(KeyError, match="Unknown name"):
        mb.get_simulation(0, "nope", alpha=astar)
    # solve() reaches the reference optimum for model 0 (Metran.solve on the same data: obj 2332.327, nfev 77)
    fit = mb.solve(stderr=True)
    assert bool(fit.converged.all())
    assert abs(float(fit.obj[0]) - float(gs["obj"])) < 1e-4
    np.testing.assert_allclose(fit.alpha[0].cpu().numpy(), gs["optimal"], rtol=1e-2)
    sim2 = mb.get_simulation(0, "B21B0214005")                # default parameters = the optimum just found
    np.testing.assert_allclose(sim2.values[:50], g1["get_simulation_005"], rtol=0, atol=2e-3)


# ---- the result cache on the real engine: launches, bits and what is held ----
def _narrow():
    """2 models x (3,1), T = 40: an ahead-of-time shape of at most 16 states -- ``project`` and ``smoother`` read filtered records."""
    from batch_standin import two_models

    models, G = two_models()
    return models, G, np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]]), {}


def _wide():
    """2 models x (32,4), T = 20, loadings given (no factor analysis): ``project`` and ``smoother`` read the filter's tape."""
    from metran_amd.synthetic import make_dfm_batch

    d = make_dfm_batch(2, 32, 4, 20, seed=7, missing=0.2)
    idx = pd.date_range("2002-03-01", periods=20, freq="D")
    models = []
    for r in range(2):
        obs = d["obs"][r].copy()
        obs[:6] = np.where(np.isfinite(obs[:6]), obs[:6], 0.1)      # every series has its cross-sectional pairs
        models.append([pd.Series(obs[:, j] * (1.0 + j) + j, index=idx, name="s%d" % j).dropna() for j in range(32)])
    return models, d["loadings"], np.full((2, 36), 9.0), {"min_pairs": 5}


def _same_bits(a, b):
    import torch

    if isinstance(a, torch.Tensor):
        return a.shape == b.shape and bool(torch.equal(a, b) or torch.equal(torch.nan_to_num(a, nan=1e300), torch.nan_to_num(b, nan=1e300)))
    if isinstance(a, (tuple, list)):
        return len(a) == len(b) and all(_same_bits(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return list(a) == list(b) and all(_same_bits(a[k], b[k]) and a[k].attrs == b[k].attrs for k in a)
    return type(a) is type(b) and a.equals(b) and a.index.equals(b.index)


@pytest.mark.parametrize("shape", [_narrow, _wide], ids=["3x1-T40", "32x4-T20"])
def test_cache_launches_once_and_holds_outputs_only(shape):
    """One accessor of every cached kind twice (and the accessors that derive something from a held result): the engine's launch
    counters move on the first call and not on the second; the second result has the bits of the first and of a fresh facade's;
    and no held tensor -- nor the storage behind it -- is larger than the largest array the kind's accessors read, which the
    forward pass's workspace, the filtered records and the tape all are (32 to 2560 doubles per model and step at these shapes)."""
    import torch

    from metran_amd.batch import MetranBatch

    models, G, alpha, kwargs = shape()
    mb, fresh = MetranBatch(models, factors=G, **kwargs), MetranBatch(models, factors=G, **kwargs)
    R, T, N, K = mb.R, mb.T, mb.N, mb.K
    n, name, H, steps = N + K, "s1", 5, [3, 11]
    assert (R, N, K) == (2,) + G.shape[1:] and T == {3: 40, 32: 20}[N]
    # kind -> (its accessors, the first of which runs the engine; the elements of the largest array those accessors read)
    kinds = {
        "project": ([lambda m: m.get_simulated_means(alpha), lambda m: m.get_simulated_variances(alpha, standardized=True),
                     lambda m: m.get_simulation(1, name, alpha)], R * T * N),
        # the decomposition holds one component per factor and series: cdf [R,K,T,N]
        "smoother": ([lambda m: m.get_state_means(1, alpha), lambda m: m.get_state_variances(0, alpha), lambda m: m.get_state(0, n - 1, alpha),
                      lambda m: m.decompose_simulation(1, name, alpha), lambda m: m.decompose_simulation(1, name, alpha, standardized=True)],
                     R * T * max(n, K * N)),
        # the projection of the filtered states reads the whole filtered covariance Pf [R,T,n,n]
        "filter": ([lambda m: m.get_state_variances(1, alpha, method="filter"), lambda m: m.get_simulated_variances(alpha, method="filter"),
                    lambda m: m.decompose_simulation(0, name, alpha, method="filter")], R * T * max(n * n, K * N)),
        "loo": ([lambda m: m.get_loo_simulated_means(alpha), lambda m: m.get_deletion_residuals(alpha)], R * T * N),
        "innov": ([lambda m: m.get_innovations(alpha), lambda m: m.get_prediction(1, name, alpha), lambda m: m.test_whiteness(alpha, nlags=3)],
                  R * T * N),
        "dist": ([lambda m: m.get_state_disturbances(alpha), lambda m: m.get_auxiliary_residuals(alpha)], R * T * n),
        # fan [R,H,N], track [R,T,N], skill [R,N,H,6]
        "forecast": ([lambda m: m.get_forecast_means(H, alpha), lambda m: m.get_forecast(1, name, H, alpha)], R * N * max(T, 6 * H)),
        # one model's weights [M,T,N]
        "weights": ([lambda m: m.get_observation_weights(1, name, steps, alpha), lambda m: m.get_weight_shares(1, name, steps, alpha)],
                    len(steps) * T * N),
    }
    # the weights run on a sub-engine of their model, whose launches the facade's engine does not count: its creation is counted
    subsets = []
    subset = mb.kf.subset
    mb.kf.subset = lambda index: subsets.append(index) or subset(index)
    mb.kf.enable_timing(accumulate=True)

    def launches():
        """Filter and smoother launches (the record readers are booked as smoothers) and sub-engines since the previous call."""
        _, nf, _, ns = mb.kf.kernel_ms_totals()
        count = nf + ns + len(subsets)
        subsets.clear()
        return count

    for kind, (accessors, _) in kinds.items():
        for i, accessor in enumerate(accessors):
            launches()
            one = accessor(mb)
            assert (launches() > 0) == (i == 0), (kind, i)    # the kind's first accessor runs the engine, the others read its result
            assert kind in mb._cache
            two = accessor(mb)
            assert launches() == 0, (kind, i)
            assert _same_bits(one, two) and _same_bits(two, accessor(fresh)), (kind, i)
    mb.get_prediction_at(0, name, 3, alpha), mb.forecast_skill(H, alpha)          # the other outputs of a forecast
    assert set(mb._cache) == set(kinds)

    def tensors(x):
        if isinstance(x, torch.Tensor):
            yield x
        for v in (x.values() if isinstance(x, dict) else x if isinstance(x, (tuple, list)) else ()):
            yield from tensors(v)

    for kind, (_, bound) in kinds.items():
        held = list(tensors(mb._cache[kind][1]))
        assert held, kind
        for t in held:
            assert t.numel() <= bound and t.untyped_storage().nbytes() <= 8 * bound, (kind, tuple(t.shape), bound)
