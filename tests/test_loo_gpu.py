"""Leave-one-out predictions on the GPU (C ABI mk_loo: adjoint_kernel's LOO mode for N + K <= 16, smoother_dk_kernel's for
16 < N + K <= 63): against the numpy restatement (tests/loo_ref.py), against masking one cell and smoothing with the
reference algorithm, against the reference's own masked example, end to end through MetranBatch, on the hard models of
the property sweep, and the refusal of shapes that are not served."""
import ctypes

import numpy as np
import pytest

import hard_models
import loo_ref
import oracle
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

SHAPES = [(8, 2), (5, 1), (7, 2), (12, 3), (32, 4), (17, 3), (19, 2), (48, 3)]


def _np(t):
    return t.detach().cpu().numpy()


@pytest.fixture(scope="module", params=["model_major", "time_major"])
def layout(request):
    return request.param


def _batch(N, K, T=40, B=6, seed=0):
    d = make_dfm_batch(B, N, K, T, seed=seed, missing=0.25)
    obs = d["obs"].copy()
    obs[:, 3] = np.nan                        # a step with no observation at all
    obs[0, 7, 1:] = np.nan                    # a step with one observed series
    obs[2, 11] = np.where(np.isfinite(obs[2, 11]), obs[2, 11], 0.5)   # a fully observed step
    return d, obs


@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
@pytest.mark.parametrize("with_r", [False, True], ids=["R0", "R"])
def test_kernels_match_restatement_and_masking(shape, with_r, layout):
    from metran_amd.engine import BatchedKalman

    N, K = shape
    d, obs = _batch(N, K, seed=N * 10 + K)
    B = obs.shape[0]
    rng = np.random.default_rng(N + K)
    R = rng.uniform(0.05, 0.4, (B, N)) * (rng.random((B, N)) < 0.6) if with_r else None
    scale = rng.uniform(0.5, 3.0, (B, N))
    offset = rng.normal(size=(B, N))
    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(obs).set_loadings(d["loadings"], R).set_scaling(scale, offset)
    assert kf.loo_supported()
    r = kf.loo_predict(d["phi"], d["q"])
    assert int(r["status"].abs().sum().item()) == 0
    gm, gv = _np(r["loo_means"]), _np(r["loo_vars"])
    seen = np.isfinite(obs)
    assert np.array_equal(np.isnan(gm), ~seen) and np.array_equal(np.isnan(gv), ~seen)
    assert np.isnan(gm[:, 3]).all() and np.isnan(gv[:, 3]).all()
    for b in range(B):
        Rb = None if R is None else R[b]
        m, v = loo_ref.loo_tape(obs[b], d["phi"][b], d["q"][b], d["loadings"][b], Rb)
        m = m * scale[b] + offset[b]
        v = np.maximum(v, 0.0) * scale[b] ** 2
        big = max(1.0, np.nanmax(np.abs(m)))
        np.testing.assert_allclose(gm[b][seen[b]], m[seen[b]], rtol=0, atol=1e-12 * big)
        np.testing.assert_allclose(gv[b][seen[b]], v[seen[b]], rtol=0, atol=1e-12 * max(1.0, np.nanmax(v)))
        if b < 2:
            cells = loo_ref.sample_cells(obs[b], rng, 4)
            bm, bv = loo_ref.loo_brute(oracle, obs[b], d["phi"][b], d["q"][b], d["loadings"][b], cells, Rb)
            np.testing.assert_allclose([gm[b][c] for c in cells], bm * scale[b][[c[1] for c in cells]] + offset[b][[c[1] for c in cells]],
                                       rtol=0, atol=1e-9 * big)
            np.testing.assert_allclose([gv[b][c] for c in cells], bv * scale[b][[c[1] for c in cells]] ** 2, rtol=0, atol=1e-9 * big * big)


def test_reference_masked_example(g1):
    """Metran's worked example: mask (mask_t, series 4), re-smooth, read get_simulation -- here one loo_predict call."""
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0)
    kf.set_observations(g1["obs"][None]).set_loadings(g1["loadings"][None])
    kf.set_scaling(g1["oseries_std"][None], g1["oseries_mean"][None])
    r = kf.loo_predict(g1["phi"][None], g1["q"][None])
    t = int(g1["mask_t"])
    got = float(_np(r["loo_means"])[0, t, 4])
    want = float(g1["masked_sim_005"].ravel()[t])
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)


def test_metran_batch_matches_mask_and_simulate(g1):
    """get_loo_simulation at a cell == mask_observations of that cell + get_simulation there (original units), for cells
    of a batch of two models of different lengths; the deletion residuals agree with both."""
    import pandas as pd
    import torch

    from metran_amd.batch import MetranBatch

    idx = pd.DatetimeIndex(g1["index_ns"].astype("datetime64[ns]"))
    raw = g1["obs"] * g1["oseries_std"] + g1["oseries_mean"]
    series = [pd.Series(raw[:, j], index=idx, name="B21B021400%d" % (j + 1)).dropna() for j in range(raw.shape[1])]
    short = [s.iloc[: len(s) // 2] for s in series]
    mb = MetranBatch([series, short], factors=g1["loadings"])
    astar = np.stack([g1["alpha_star"], g1["alpha_star"] * 1.1])
    loo = {(r, name): mb.get_loo_simulation(r, name, alpha=astar) for r, name in ((0, "B21B0214005"), (1, "B21B0214002"))}
    assert list(loo[(0, "B21B0214005")].columns) == ["mean", "lower", "upper"]
    assert loo[(0, "B21B0214005")].shape[0] == 6255 and loo[(1, "B21B0214002")].shape[0] == int(mb.batch.lengths[1])
    res = _np(mb.get_deletion_residuals(astar))
    lm, lv = _np(mb.get_loo_simulated_means(astar)), _np(mb.get_loo_simulated_variances(astar))
    obs = _np(mb.kf.obs)
    assert np.array_equal(np.isnan(res), ~np.isfinite(obs)) and np.array_equal(np.isnan(lm), ~np.isfinite(obs))
    std, mean = _np(mb._std), _np(mb._mean)
    np.testing.assert_allclose(res, (obs * std[:, None] + mean[:, None] - lm) / np.sqrt(lv), rtol=1e-12, atol=1e-12)
    for (r, name), frame in loo.items():
        j = mb._series(r, name)
        ts = np.nonzero(np.isfinite(obs[r, :, j]))[0]
        for t in (ts[0], ts[len(ts) // 2], ts[-1]):
            mask = torch.zeros((2, mb.T, mb.N), dtype=torch.uint8)
            mask[r, t, j] = 1
            mb.mask_observations(mask)
            sim = mb.get_simulation(r, name, alpha=astar)
            mb.unmask_observations()
            np.testing.assert_allclose(frame.values[t], sim.values[t], rtol=0, atol=1e-8)
    # standardised units: the same residuals
    smean = _np(mb.get_loo_simulated_means(astar, standardized=True))
    svar = _np(mb.get_loo_simulated_variances(astar, standardized=True))
    np.testing.assert_allclose(res, (obs - smean) / np.sqrt(svar), rtol=1e-10, atol=1e-10)
    assert "loo" in mb._cache


def test_hard_models_against_masking():
    """The property sweep's hard models (persistence up to 1 - 1e-9, communality up to 0.999, R > 0, x0 / P0, sparse and
    empty steps): sampled cells against mask-and-smooth with the reference algorithm, within the smoother's bar."""
    from metran_amd.engine import BatchedKalman

    rng = np.random.default_rng(7)
    for (N, K, T, B), g in hard_models.groups(per_shape=16, shapes=[s for s in SHAPES if s in hard_models.AOT_SHAPES + hard_models.JIT_SHAPES]):
        kf = BatchedKalman(0)
        kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
        r = kf.loo_predict(g["phi"], g["q"], g["x0"], g["P0"])
        gm, gv = _np(r["loo_means"]), _np(r["loo_vars"])
        seen = np.isfinite(g["obs"])
        assert np.array_equal(np.isnan(gm), ~seen)
        for b in range(0, B, 3):
            if not seen[b].any():
                continue
            ref = hard_models.oracle_model(oracle, g, b)
            tol = hard_models.smoother_tolerance(g, b, ref)
            Rb = None if g["obsvar"] is None else g["obsvar"][b]
            x0 = None if g["x0"] is None else g["x0"][b]
            P0 = None if g["P0"] is None else g["P0"][b]
            cells = loo_ref.sample_cells(g["obs"][b], rng, 2)
            bm, bv = loo_ref.loo_brute(oracle, g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b], cells, Rb, x0, P0)
            what = (N, K, T, b, g["patterns"][b])
            np.testing.assert_allclose([gm[b][c] for c in cells], bm, rtol=0, atol=tol, err_msg=str(what))
            np.testing.assert_allclose([gv[b][c] for c in cells], np.maximum(bv, 0.0), rtol=0, atol=tol, err_msg=str(what))


def test_unserved_shapes_raise():
    from metran_amd import _lib
    from metran_amd._lib import MetranHipError, Problem
    from metran_amd.engine import BatchedKalman

    d = make_dfm_batch(2, 8, 2, 16, seed=3)
    kf = BatchedKalman(0)
    kf.set_observations(d["obs"]).set_loadings(d["loadings"])
    kf.set_variant("kernel_family", "generic")
    assert not kf.loo_supported()
    with pytest.raises(MetranHipError, match="N=8, K=2"):
        kf.loo_predict(d["phi"], d["q"])
    kf.set_variant("kernel_family", "specialised")
    assert kf.loo_supported()
    # the C ABI itself: n = 64 (generic kernels serve it, mk_loo does not) fails before any launch
    L = _lib.lib()
    import torch

    buf = torch.zeros(64 * 64, dtype=torch.float64, device="cuda")
    p = ctypes.c_void_p(buf.data_ptr())
    prob = Problem(1, 1, 4, 60, 4, 0, p, p, p, p, None, None, None, 0, None, None)
    rc = L.mk_loo(kf._ctx, ctypes.byref(prob), p, 0, p, p, None)
    assert rc == -2 and b"N=60, K=4" in L.mk_last_error()
    # a workspace smaller than the call needs is refused
    kf2 = BatchedKalman(0)
    kf2.set_observations(d["obs"]).set_loadings(d["loadings"])
    phi, q = kf2._dev(d["phi"]), kf2._dev(d["q"])
    prob, keep, B = kf2._problem(phi, q, 0, None, None)
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf2._ctx, 128, ctypes.byref(small)) == 0   # an allocation of its own: its size is known exactly
    out = torch.empty((2, 16, 8), dtype=torch.float64, device="cuda")
    try:
        rc = L.mk_loo(kf2._ctx, ctypes.byref(prob), small, 0, ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(out.data_ptr()), None)
        assert rc == -1 and b"d_work" in L.mk_last_error()
    finally:
        L.mk_free(kf2._ctx, small)
