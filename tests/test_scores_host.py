"""Per-step scores on the CPU: the numpy restatement of the tangent filter (tests/score_ref.py, the yardstick of
tests/test_scores_gpu.py) pinned to the definition -- central differences of the per-step objective of an extended-precision
filter -- and to the adjoint restatement's gradient; exact zeros at empty steps; the conditioning of every input of the GPU
tier; six deliberately wrong variants far outside the bars; the host mathematics of ``metran_amd.scores`` (``cvm_sf`` against the
closed form for k = 2 and the tabulated Cramer-von Mises points for k = 1, ``nyblom`` and ``parameter_covariance`` against direct
numpy formulas); the zero mean of the score at the truth; and the accessors of ``MetranBatch`` over a stand-in engine
(tests/score_engine.py).

All comparisons of scores are relative to the output's SCALE (tests/score_ref.py)."""
import numpy as np
import pytest
import torch

import adjoint_ref
import score_ref
from batch_standin import stand_in, two_models
from metran_amd.scores import cvm_sf, nyblom, parameter_covariance
from metran_amd.synthetic import make_dfm_batch
from score_engine import ScoreEngine

LD, F64 = np.longdouble, np.float64
DEFINITION_BAR = 1e-10    # of the scale: the central differences' truncation is h^2-sized (h = 1e-6 alpha); measured 2.2e-12
CONDITIONING_BAR = 1e-12  # float64 against extended precision on every input of the GPU tier


def _model(N=4, K=2, T=60, seed=3):
    """One model, 30 % missing, one empty step in the middle and two at the start."""
    d = make_dfm_batch(1, N, K, T, seed=seed, missing=0.3)
    y = d["obs"][0].copy()
    y[7] = np.nan
    y[:2] = np.nan
    return y, d["loadings"][0], d["alpha"][0]


def _from_alpha(alpha, G, dtype):
    """(phi, q, dphi, dq) of Metran's parametrisation in ``dtype``, dt = 1."""
    a, G = np.asarray(alpha, dtype=dtype), np.asarray(G, dtype=dtype)
    phi = np.exp(-1 / a)
    c = np.concatenate([1 - (G * G).sum(1), np.ones(G.shape[1], dtype=dtype)])
    dphi = phi / (a * a)
    return phi, (1 - phi * phi) * c, dphi, -2 * phi * dphi * c


def _warmup_of(obs, t_first):
    return int(np.isfinite(obs[:t_first]).any(axis=1).sum())


def test_the_restatement_is_the_derivative_of_the_per_step_objective():
    """Central differences (h = 1e-6 alpha) of l_t from an extended-precision filter, parameter by parameter."""
    y, G, alpha = _model()
    T, n = y.shape[0], alpha.size
    phi, q, dphi, dq = _from_alpha(alpha, G, LD)
    ref = score_ref.scores(y, phi, q, G, dphi=dphi, dq=dq, t_first=1, dtype=LD)
    num = np.zeros((T, n), dtype=LD)
    for p in range(n):
        h = LD(1e-6) * LD(alpha[p])
        up, dn = np.asarray(alpha, dtype=LD).copy(), np.asarray(alpha, dtype=LD).copy()
        up[p] += h
        dn[p] -= h
        ell = [score_ref.base(y, *_from_alpha(a, G, LD)[:2], G, dtype=LD)["ell"] for a in (up, dn)]
        num[:, p] = (ell[0] - ell[1]) / (2 * h)
    err = float(np.max(np.abs(num - ref["score"]) / ref["scale"]["score"]))
    print("central differences against the restatement: %.3g of the scale (bar %.3g)" % (err, DEFINITION_BAR))
    assert err <= DEFINITION_BAR


@pytest.mark.parametrize("t_first", [0, 1, 3, 9])
def test_the_sum_over_the_counted_steps_is_the_adjoint_gradient(t_first):
    y, G, alpha = _model()
    phi, q, dphi, dq = _from_alpha(alpha, G, F64)
    ref = score_ref.scores(y, phi, q, G, dphi=dphi, dq=dq, t_first=t_first, dtype=F64)
    _, gphi, gq = adjoint_ref.gradient(y, phi, q, G, warmup=_warmup_of(y, t_first))
    err = np.max(np.abs(gphi * dphi + gq * dq - ref["grad"]) / ref["scale"]["grad"])
    assert err <= 1e-13, err
    assert ref["count"] == int(np.isfinite(y[t_first:]).any(axis=1).sum())


def test_an_empty_step_scores_exactly_zero():
    y, G, alpha = _model()
    for dtype in (F64, LD):
        phi, q, dphi, dq = _from_alpha(alpha, G, dtype)
        ref = score_ref.scores(y, phi, q, G, dphi=dphi, dq=dq, dtype=dtype)
        assert (ref["score"][[0, 1, 7]] == 0).all() and (ref["score"][[2, 3, 8]] != 0).any(axis=1).all()


def test_the_inputs_of_the_gpu_tier_are_well_conditioned():
    """On every input set of tests/test_scores_gpu.py the float64 and the extended-precision restatement agree to 1e-12 of the
    scale, and to the figures its bars are made of (an input that does not is replaced, the bar is not widened)."""
    import test_scores_gpu as ts

    worst = {cls: {key: 0.0 for key in score_ref.OUTPUTS} for cls in ("short", "long")}
    for p, dphi, dq, t_first, compared in ts.input_sets():
        cls = "short" if p["obs"].shape[1] <= ts.SHORT else "long"
        for b in compared:
            r64 = ts._reference(p, b, dphi, dq, t_first, dtype=F64)
            rld = ts._reference(p, b, dphi, dq, t_first, dtype=LD)
            assert r64["count"] == rld["count"]
            diff = score_ref.differences(r64, rld)
            for key in score_ref.OUTPUTS:
                worst[cls][key] = max(worst[cls][key], diff[key])
    print("float64 against extended precision:", worst)
    for cls, measured in (("long", ts.MEASURED), ("short", ts.MEASURED_SHORT)):
        for key in score_ref.OUTPUTS:
            assert worst[cls][key] <= CONDITIONING_BAR, (cls, key, worst[cls][key])
            assert worst[cls][key] <= 1.005 * measured[key], (cls, key, worst[cls][key], measured[key])   # the docstring's figures, to three digits


@pytest.mark.parametrize("bad", ["half", "no_v2", "filtered_t", "records", "count_before", "uncentred"])
def test_wrong_variants_are_far_outside_the_bars(bad):
    """On an input of the GPU tier ((8,2), T = 17, observation variances and initial moments given, t_first = 1, an instance of
    record 0, whose step 0 holds observations) each wrong variant is more than a thousand bars from the restatement."""
    import test_scores_gpu as ts

    N, K, T = 8, 2, 17
    p = ts._data(N, K, T, seed=100 * N + T, full=True)
    dphi, dq = ts._derivs(p, 100 * N + T)
    b = 2
    assert np.isfinite(p["obs"][0, 0]).any()
    good = ts._reference(p, b, dphi, dq, 1, dtype=F64)
    if bad == "records":
        args = list(ts._args(p, b))
        args[0], args[3], args[4] = p["obs"][1], p["loadings"][1], p["obsvar"][1]      # the record of instance b + 1
        wrong = score_ref.scores(*args, dphi=dphi[b], dq=dq[b], t_first=1, dtype=F64)
    else:
        wrong = score_ref.scores(*ts._args(p, b), dphi=dphi[b], dq=dq[b], t_first=1, dtype=F64, **{bad: True})
    diff = score_ref.differences(wrong, good)
    far = {key: diff[key] / ts.BAR[key] for key in score_ref.OUTPUTS}
    print(bad, far)
    assert max(far.values()) > 1000, (bad, far)
    if bad == "uncentred":
        assert far["cusum"] > 1000 and far["score"] == far["grad"] == far["opg"] == 0
    elif bad == "count_before":
        assert far["grad"] > 1000 and far["score"] == 0
    else:
        assert far["score"] > 1000 and far["grad"] > 1000


def test_the_stand_in_engine_notices_another_record():
    models, G = two_models()
    alpha = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    right = stand_in(ScoreEngine, models, G)
    wrong = stand_in(ScoreEngine, models, G)
    wrong.kf.shift_records = 1
    a, b = right.kf.scores_alpha(alpha), wrong.kf.scores_alpha(alpha)
    assert not torch.allclose(a["grad"], b["grad"], rtol=1e-3)


# ---------------------------------------------------------------------- host mathematics
def test_cvm_sf_k2_is_the_closed_form():
    j = np.arange(1, 200)
    for x in (0.2, 0.5, 1.0, 2.0):
        closed = 2.0 * np.sum((-1.0) ** (j - 1) * np.exp(-j * j * np.pi ** 2 * x / 2.0))
        assert abs(cvm_sf(x, 2) - closed) <= 1e-8, x


def test_cvm_sf_k1_is_the_cramer_von_mises_table():
    """The tabulated upper points (five digits: about 1e-5 in p).  A principal-branch square root returns 0.041, 0.074 and -0.016."""
    for x, p in ((0.34730, 0.10), (0.46136, 0.05), (0.74346, 0.01)):
        assert abs(cvm_sf(x, 1) - p) <= 2e-5, (x, cvm_sf(x, 1))


def test_cvm_sf_is_monotone_in_x_and_increasing_in_k():
    xs = np.linspace(0.02, 4.0, 60)
    tol = 1e-12                                       # the rounding of the numerical inversion
    table = np.stack([cvm_sf(xs, k) for k in (1, 2, 3, 4, 6, 10)])
    assert ((table >= 0) & (table <= 1)).all()
    assert (np.diff(table, axis=1) <= tol).all() and (np.diff(table, axis=0) >= -tol).all()
    assert (np.diff(table, axis=1) < 0).any(axis=1).all() and (np.diff(table, axis=0) > 0).any(axis=1).all()
    assert cvm_sf(0.0, 3) == 1.0 and cvm_sf(-1.0, 1) == 1.0 and np.isnan(cvm_sf(np.nan, 1)) and cvm_sf(40.0, 2) <= 1e-12
    got = cvm_sf(np.array([[0.3, 0.5], [1.0, np.nan]]), 1)
    assert got.shape == (2, 2) and abs(got[0, 0] - cvm_sf(0.3, 1)) <= tol and np.isnan(got[1, 1])
    with pytest.raises(ValueError):
        cvm_sf(1.0, 0)


def test_cvm_sf_costs_per_value_not_per_largest_value():
    """A batch's statistics in one call, one model with a clear break among them (a mean shift of the scores by one standard
    deviation half-way through 2000 steps gives L of about 40): the grid of a chunk follows the chunk's own values, and beyond
    ``_cvm_zero_from(k)`` no quadrature runs.  Bounded by work, not by the clock: the sizes of the temporaries that ``numpy.exp``
    is asked for."""
    from metran_amd import scores

    assert 8.0 < scores._cvm_zero_from(1) < 9.0 and 19.0 < scores._cvm_zero_from(36) < 21.0
    for k in (1, 4, 36):                                           # nothing is cut off that is not zero to rounding
        z = scores._cvm_zero_from(k)
        assert cvm_sf(0.999 * z, k) <= 1e-13 and cvm_sf(z, k) == 0.0 and cvm_sf(1e6, k) == 0.0 and cvm_sf(np.inf, k) == 0.0
    quiet = np.full(640, 0.3)
    loud = np.concatenate([quiet, [20.0, 40.0, 100.0, 1e9]])
    cells = []
    real_exp = np.exp

    def counting_exp(a, *args, **kwargs):
        cells.append(np.size(a))
        return real_exp(a, *args, **kwargs)

    scores.np.exp = counting_exp
    try:
        base = cvm_sf(quiet, 1)
        work_quiet, cells[:] = sum(cells), []
        got = cvm_sf(loud, 1)
        work_loud, peak = sum(cells), max(cells)
        cells[:] = []
        mid = cvm_sf(np.concatenate([quiet, [8.0]]), 1)             # a value just inside: a chunk of its own size, not the others'
        work_mid, peak_mid = sum(cells), max(cells)
    finally:
        scores.np.exp = real_exp
    assert (got[-4:] == 0).all() and np.array_equal(got[:640], base)
    assert work_loud == work_quiet and peak <= scores._CVM_CHUNK_CELLS
    assert mid[-1] <= 1e-13 and peak_mid <= scores._CVM_CHUNK_CELLS and work_mid <= 2 * work_quiet


def _sums(rng, R=3, T=50, n=4):
    s = rng.normal(size=(R, T, n)) * np.array([1.0, 0.1, 5.0, 2.0])
    s[:, :, 1] += 0.05                                # not centred: as at a bound
    grad = s.sum(1)
    opg = np.einsum("rtp,rtq->rpq", s, s)
    S = np.cumsum(s - grad[:, None, :] / T, axis=1)
    return s, grad, opg, np.einsum("rtp,rtq->rpq", S, S), np.full(R, T)


def test_nyblom_against_direct_formulas():
    rng = np.random.default_rng(11)
    s, grad, opg, cusum, m = _sums(rng)
    res = nyblom(cusum, opg, grad, m)
    for r in range(3):
        V = opg[r] - np.outer(grad[r], grad[r]) / m[r]
        np.testing.assert_allclose(res["L_param"][r], np.diag(cusum[r]) / (m[r] * np.diag(V)), rtol=1e-13)
        np.testing.assert_allclose(res["L"][r], np.trace(np.linalg.pinv(V) @ cusum[r]) / m[r], rtol=1e-12)
        np.testing.assert_allclose(res["pvalue_param"][r], cvm_sf(res["L_param"][r], 1), rtol=0, atol=1e-12)   # the grid follows the largest x
        assert abs(res["pvalue"][r] - cvm_sf(res["L"][r], 4)) <= 1e-12 and res["df"][r] == 4
    # a parameter the model does not have: NaN for it, the joint statistic over the other three
    exists = np.ones((3, 4), dtype=bool)
    exists[1, 3] = False
    part = nyblom(cusum, opg, grad, m, exists)
    V = (opg[1] - np.outer(grad[1], grad[1]) / m[1])[:3, :3]
    assert np.isnan(part["L_param"][1, 3]) and np.isnan(part["pvalue_param"][1, 3]) and part["df"].tolist() == [4, 3, 4]
    np.testing.assert_allclose(part["L"][1], np.trace(np.linalg.pinv(V) @ cusum[1][:3, :3]) / m[1], rtol=1e-12)
    assert abs(part["pvalue"][1] - cvm_sf(part["L"][1], 3)) <= 1e-12 and part["L"][0] == res["L"][0]
    # constant parameters: the statistic of white scores is of the size of its law's mean, 1/6 per parameter
    assert (res["L_param"] < 2.0).all() and (res["pvalue_param"] > 1e-4).all()


def test_parameter_covariance_against_direct_formulas():
    rng = np.random.default_rng(12)
    _, grad, opg, _, m = _sums(rng)
    A = rng.normal(size=(3, 4, 4))
    H = A @ A.transpose(0, 2, 1) + 4.0 * np.eye(4)
    for r in range(3):
        Hi = np.linalg.pinv(H[r])
        assert np.array_equal(parameter_covariance(opg, m, grad, H, "hessian")[r], 2.0 * Hi)          # exactly 2 pinv(H)
        np.testing.assert_allclose(parameter_covariance(opg, m, grad, kind="opg")[r], 4.0 * np.linalg.inv(opg[r]), rtol=1e-10)
        np.testing.assert_allclose(parameter_covariance(opg, m, grad, H, "robust")[r], np.linalg.inv(H[r]) @ opg[r] @ np.linalg.inv(H[r]), rtol=1e-10)
    # when the information equality holds, H = opg / 2, the three agree
    for kind in ("opg", "hessian", "robust"):
        np.testing.assert_allclose(parameter_covariance(opg, m, grad, 0.5 * opg, kind), 4.0 * np.linalg.inv(opg), rtol=1e-9)
    t = parameter_covariance(torch.from_numpy(opg), None, None, torch.from_numpy(H), "robust")
    assert isinstance(t, torch.Tensor) and np.allclose(t.numpy(), parameter_covariance(opg, hessian=H, kind="robust"), rtol=1e-12)
    with pytest.raises(ValueError):
        parameter_covariance(opg, m, grad, None, "robust")
    with pytest.raises(ValueError):
        parameter_covariance(opg, m, grad, H, "sandwich")


def test_the_score_has_zero_mean_at_the_truth():
    """200 records of a (3,1) model, T = 100, each simulated at its own true parameters from x = 0 (so x0 = 0, P0 = 0 is the
    truth too): the mean of ``grad`` over the records is within 4 of its Monte Carlo standard errors of zero, for every parameter."""
    R, N, K, T = 200, 3, 1, 100
    d = make_dfm_batch(R, N, K, T, seed=21, missing=0.2)
    n = N + K
    grads = np.empty((R, n))
    for r in range(R):
        phi, q, dphi, dq = _from_alpha(d["alpha"][r], d["loadings"][r], F64)
        grads[r] = score_ref.scores(d["obs"][r], phi, q, d["loadings"][r], None, np.zeros(n), np.zeros((n, n)), dphi=dphi, dq=dq,
                                    t_first=0, dtype=F64)["grad"]
    mean, se = grads.mean(0), grads.std(0, ddof=1) / np.sqrt(R)
    print("mean of grad in standard errors:", mean / se)
    assert (np.abs(mean) <= 4.0 * se).all(), mean / se


# ---------------------------------------------------------------------- the facade over the stand-in engine
def test_metran_batch_scores_over_a_stand_in_engine():
    """Frames, names, the numbers of the restatement, the three covariances, the stability table, NaN for the parameters of a
    padding factor, and the cache."""
    models, G = two_models()
    mb = stand_in(ScoreEngine, models, G)
    kf = mb.kf
    alpha = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    names = ["s0_sdf_alpha", "s1_sdf_alpha", "s2_sdf_alpha", "cdf1_alpha"]
    frame = mb.get_scores(1, alpha=alpha)
    L1 = int(mb.batch.lengths[1])
    assert kf.calls == 1 and L1 < mb.T
    assert list(frame.columns) == names and frame.shape == (L1, 4) and list(frame.index) == list(mb.batch.index[1])
    ref = []
    for r in range(2):
        phi, q, dphi, dq = _from_alpha(alpha[r], G[r], F64)
        ref.append(score_ref.scores(kf.obs_np[r], phi, q, G[r], dphi=dphi, dq=dq, t_first=1, dtype=F64))
    np.testing.assert_allclose(frame.values, ref[1]["score"][:L1], rtol=1e-12, atol=1e-14)
    assert (ref[1]["score"][L1:] == 0).all()                       # the padding steps are empty
    opg = mb.get_parameter_covariance("opg", alpha=alpha)
    assert kf.calls == 1                                           # the same run serves the covariance ...
    table = mb.test_parameter_stability(alpha=alpha)
    assert kf.calls == 1                                           # ... and the test
    assert set(opg) == {"pcov", "stderr", "corr"} and opg["pcov"].shape == (2, 4, 4) and opg["stderr"].shape == (2, 4)
    for r in range(2):
        np.testing.assert_allclose(opg["pcov"][r], 4.0 * np.linalg.pinv(np.asarray(ref[r]["opg"], dtype=F64)), rtol=1e-9)
        np.testing.assert_allclose(opg["stderr"][r], np.sqrt(np.diag(opg["pcov"][r])), rtol=1e-15)
        np.testing.assert_allclose(np.diag(opg["corr"][r]), 1.0, rtol=1e-14)
    assert list(table.index) == [(r, nm) for r in range(2) for nm in names + ["joint"]] and list(table.columns) == ["L", "pvalue", "n_steps"]
    for r in range(2):
        want = nyblom(ref[r]["cusum"], ref[r]["opg"], ref[r]["grad"], ref[r]["count"])
        np.testing.assert_allclose(table.loc[r]["L"].values, list(want["L_param"]) + [want["L"]], rtol=1e-10)
        assert (table.loc[r]["n_steps"] == ref[r]["count"]).all()
    assert ((table["pvalue"] >= 0) & (table["pvalue"] <= 1)).all()
    # the Hessian kinds: differenced from the stand-in's adjoint gradient, once
    log0 = len(kf.log)
    hes = mb.get_parameter_covariance("hessian", alpha=alpha)
    launches = len(kf.log) - log0
    rob = mb.get_parameter_covariance("robust", alpha=alpha)
    assert launches >= 1 and len(kf.log) - log0 == launches and kf.calls == 1
    for r in range(2):
        H = 2.0 * np.linalg.pinv(hes["pcov"][r])
        np.testing.assert_allclose(rob["pcov"][r], np.linalg.pinv(H) @ np.asarray(ref[r]["opg"], dtype=F64) @ np.linalg.pinv(H), rtol=1e-8)
        assert (np.diag(rob["pcov"][r]) > 0).all()                 # a congruence of opg; the Hessian away from an optimum need not be definite
    mb.get_scores(0, alpha=alpha, t_first=2)
    assert kf.calls == 2                                           # another t_first is another request
    mb.get_scores(0, alpha=alpha + 1.0)
    assert kf.calls == 3                                           # another parameter set replaces the kind's results
    with pytest.raises(ValueError):
        mb.get_parameter_covariance("sandwich", alpha=alpha)
    # without an adjoint gradient "opg" still works and the other two raise calibrate_batch's message
    bare = stand_in(lambda obs, load: ScoreEngine(obs, load, adjoint=False), models, G)
    assert np.isfinite(bare.get_parameter_covariance("opg", alpha=alpha)["stderr"]).all()
    with pytest.raises(ValueError, match="differences the adjoint gradient"):
        bare.get_parameter_covariance("robust", alpha=alpha)


def test_parameters_of_a_padding_factor_are_nan():
    """A model with fewer factors than the batch maximum carries a zero loading column: the parameter of that factor does not
    exist -- NaN in the covariances and in the stability table, left out of the joint statistic -- as ``solve`` treats ``stderr``."""
    models, G = two_models()
    G2 = np.concatenate([G, np.zeros((2, 3, 1))], axis=2)
    G2[0, :, 1] = [0.3, -0.2, 0.4]                                 # model 0 has two factors, model 1 one
    mb = stand_in(ScoreEngine, models, G2)
    mb.nfactors = np.array([2, 1])
    alpha = np.array([[8.0, 6.0, 9.0, 12.0, 15.0], [5.0, 7.0, 8.0, 10.0, 10.0]])
    cov = mb.get_parameter_covariance("opg", alpha=alpha)
    assert np.isfinite(cov["pcov"][0]).all() and np.isfinite(cov["stderr"][0]).all()
    assert np.isnan(cov["pcov"][1, 4]).all() and np.isnan(cov["pcov"][1, :, 4]).all() and np.isfinite(cov["pcov"][1, :4, :4]).all()
    assert np.isnan(cov["stderr"][1, 4]) and np.isfinite(cov["stderr"][1, :4]).all()
    table = mb.test_parameter_stability(alpha=alpha)
    assert len(table) == 2 * 6
    assert np.isnan(table.loc[(1, "cdf2_alpha"), "L"]) and np.isnan(table.loc[(1, "cdf2_alpha"), "pvalue"])
    assert np.isfinite(table.loc[1].drop("cdf2_alpha").values).all() and np.isfinite(table.loc[0].values).all()


def test_the_hessian_counts_the_steps_the_scores_count():
    """A record that begins with an empty step: with t_first = 1 the scores count every step that holds an observation, and so
    does the Hessian -- warm-up 0 for that record, 1 for the other -- so both halves of the sandwich are built on the same steps."""
    from metran_amd.scores import hessian_alpha

    models, G = two_models()
    mb = stand_in(ScoreEngine, models, G)
    mb.kf.obs_np[1, 0] = np.nan
    alpha = torch.tensor([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]], dtype=torch.float64)
    got = mb._run("hessian", alpha, 1)["hessian"].numpy()
    want = [hessian_alpha(mb.kf.subset([r]), alpha[r:r + 1], warmup=w)[0].numpy() for r, w in ((0, 1), (1, 0))]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    other = hessian_alpha(mb.kf.subset([1]), alpha[1:], warmup=1)[0].numpy()
    assert not np.allclose(got[1], other, rtol=1e-6)
    # ... and the gradient the scores sum is the gradient that Hessian differences
    grad = mb._run("scores", alpha, 1)["grad"].numpy()
    for r, w in ((0, 1), (1, 0)):
        _, g = mb.kf.subset([r]).loglik_grad_alpha(alpha[r:r + 1], warmup=w)
        np.testing.assert_allclose(grad[r], g[0].numpy(), rtol=1e-9, atol=1e-11)
