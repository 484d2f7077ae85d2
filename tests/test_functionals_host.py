"""Window functionals without a GPU: the kernel's recursion (tests/functional_ref.py::functional_walk, float64, from the C oracle's
records) against the DEFINITION (``functional_definition``: dense conditioning in longdouble) on every group of the GPU tier;
identities with the oracle's own projection; deliberately wrong variants shown to be far outside the bars; and the MetranBatch
accessors over a stand-in engine that answers from the recursion.

MEASURED_RATIO: the largest (float64 walk - longdouble definition) / bar over all groups, windows and contrasts below is 6.6e-6
(at (13,4), T = 17; 5.0e-6 at (60,4), T = 3) -- the lag terms cost nothing visible next to the tier's 1e-9 on S and Ps.  Four times that (the diagnostics tier's allowance for the kernels' tree-order fused sums) is far below 1,
so the bars stand as given: SMOOTH_ATOL A zeta and SMOOTH_ATOL (A zeta)^2.  ``test_walk_equals_definition`` asserts it."""
import numpy as np
import pytest

import call_forms as cf
import functional_ref as fr
from batch_standin import stand_in, two_models
from functional_engine import FunctionalEngine

F64 = np.float64
MEASURED_RATIO = 6.6e-6
WRONG_GROUPS = ((8, 2, 17), (13, 4, 17))


@pytest.mark.parametrize("shape", fr.GROUPS, ids=["%dx%d-T%d" % s for s in fr.GROUPS])
def test_walk_equals_definition(shape):
    g = fr.group(*shape)
    wins = fr.windows(shape[2])
    worst = 0.0
    seen = [0.0] * g["R"]
    for kind in ("mixed",) + (("unit",) if shape[0] <= 13 else ()):
        table = fr.contrasts(g, kind)
        for i in range(g["B"]):
            r = i % g["R"]
            dm, dv = fr.functional_definition(g, i, wins[r], table)
            for w, win in enumerate(wins[r]):
                for k, c in enumerate(fr.contrast_rows(g, i, table)):
                    m, v = fr.functional_walk(g, i, win, c)
                    if np.isnan(dm[w, k]):
                        assert np.isnan(m) and np.isnan(v) and fr.alphas(win, shape[2])[0] is None
                        continue
                    bm, bv = fr.bars(g, i, win, c)
                    if bm == 0.0:
                        assert m == 0.0 and v == 0.0 and dm[w, k] == 0.0 and dv[w, k] == 0.0
                        continue
                    worst = max(worst, abs(float(m - dm[w, k])) / bm, abs(float(v - dv[w, k])) / bv)
                    seen[r] = max(seen[r], float(dv[w, k]))
    print("(%d,%d) T=%d: float64 walk at most %.3g bars from the definition" % (shape + (worst,)))
    assert worst <= 2.0 * MEASURED_RATIO and 4.0 * worst <= 1.0
    assert min(seen) > 1e-3, "every record needs a functional with a variance above 1e-3 (a condition on the inputs)"


def test_one_step_windows_are_the_oracles_projection():
    """A one-step window with unit contrasts is sim_means / sim_vars of call_forms.reference; a two-series contrast at one step is
    z' Ps z."""
    g = fr.group(8, 2, 17)
    N = g["N"]
    for i in range(g["B"]):
        ref = cf.reference(g, i, 0, parts=("state",))
        r = ref["rec"]
        for t in (0, 5, 16):
            win = (t, t + 1, 0, 0)
            dm, dv = fr.functional_definition(g, i, [win], None)
            for j in range(N):
                m, v = fr.functional_walk(g, i, win, np.eye(N)[j])
                bm, bv = fr.bars(g, i, win, np.eye(N)[j])
                tol = cf.bar("sim_means", None, g, r)
                assert abs(m - ref["sim_means"][t, j]) <= bm and abs(v - ref["sim_vars"][t, j]) <= bv
                assert abs(float(dm[0, j]) - ref["sim_means"][t, j]) <= tol and abs(float(dv[0, j]) - ref["sim_vars"][t, j]) <= tol
            c = np.zeros(N)
            c[1], c[4] = 1.0, -1.0
            z = fr.zvector(g, i, c)
            m, v = fr.functional_walk(g, i, win, c)
            assert abs(v - z @ ref["Ps"][t] @ z) <= fr.bars(g, i, win, c)[1]
            assert abs(m - (ref["sim_means"][t, 1] - ref["sim_means"][t, 4])) <= 2 * fr.bars(g, i, win, c)[0]


def test_a_difference_is_the_combination_of_its_point_functionals():
    """The four-range functional equals sum_t alpha_t (point functional at t), its variance alpha' P alpha with P the covariance of
    the point functionals taken from the definition's posterior covariance."""
    g = fr.group(8, 2, 17)
    T, n = g["T"], g["N"] + g["K"]
    c = fr.contrasts(g, "mixed")[0, 3]
    for i in (0, 4, 8):
        mv, C = fr.posterior(g, i)
        pts = [fr.weights_vector(g, i, (t, t + 1, 0, 0), c) for t in range(T)]
        A = np.stack([p[0] for p in pts])
        pm, P = A @ mv + np.array([p[1] for p in pts]), A @ C @ A.T
        for win in ((1, 4, 8, 12), (10, 14, 3, 7), (2, 6, 6, 9), (0, 17, 0, 0)):
            al, _ = fr.alphas(win, T, dtype=fr.LD)
            m, v = fr.functional_walk(g, i, win, c)
            bm, bv = fr.bars(g, i, win, c)
            assert abs(float(m - al @ pm)) <= bm and abs(float(v - al @ P @ al)) <= bv
        # the SUM of two windows' means (second_sign) from the same covariance
        al, _ = fr.alphas((1, 4, 8, 12), T, dtype=fr.LD, wrong="second_sign")
        m, v = fr.functional_walk(g, i, (1, 4, 8, 12), c, wrong="second_sign")
        assert abs(float(v - al @ P @ al)) <= fr.bars(g, i, (1, 4, 8, 12), c)[1]


def _separates(g, r, wrong_of):
    """The largest distance in bars, over the functionals of record r's instances, between the right value and ``wrong_of(i, win, c)``
    (None = the variant does not apply to the instance)."""
    wins = fr.windows(g["T"])[r]
    table = fr.contrasts(g, "mixed")
    far = 0.0
    for i in range(r, g["B"], g["R"]):
        for win in wins:
            if fr.alphas(win, g["T"])[0] is None:
                continue
            for c in table[r]:
                bm, bv = fr.bars(g, i, win, c)
                if bm == 0.0:
                    continue
                got = wrong_of(i, win, c)
                if got is None:
                    continue
                m, v = fr.functional_walk(g, i, win, c)
                far = max(far, abs(got[0] - m) / bm, abs(got[1] - v) / bv)
    return far


@pytest.mark.parametrize("shape", WRONG_GROUPS, ids=["%dx%d-T%d" % s for s in WRONG_GROUPS])
def test_wrong_variants_are_far_outside_the_bars(shape):
    g = fr.group(*shape)
    R, S, B = g["R"], g["S"], g["B"]
    swapped = cf.variant(g, x0=g["x0"][np.arange(B) % R])       # x0 of instance i % R
    variants = {name: (lambda i, win, c, name=name: fr.functional_walk(g, i, win, c, wrong=name)) for name in fr.WRONG}
    variants["record i // S"] = lambda i, win, c: None if i // S == i % R else fr.functional_walk(g, i, win, c, rec=i // S)
    variants["x0 of instance i % R"] = lambda i, win, c: None if i < R else fr.functional_walk(swapped, i, win, c)
    for name, wrong_of in variants.items():
        for r in range(R):
            far = _separates(g, r, wrong_of)
            assert far >= cf.FACTOR, "%s: record %d is only %.3g bars from the right value" % (name, r, far)


# ------------------------------------------------------------------------------------------------------------------ facade
ALPHA = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])


def test_facade_window_means_units_and_cache():
    import pandas as pd

    models, G = two_models()
    mb = stand_in(FunctionalEngine, models, G)
    kf = mb.kf
    idx = mb.batch.index[0]
    wins = [(idx[2], idx[9]), (idx[5], idx[20]), (idx[30], idx[38])]          # the first two overlap
    frame = mb.get_window_means(wins, alpha=ALPHA)
    assert list(frame.columns) == ["mean", "sd"] and frame.index.names == ["model", "series", "window"]
    assert len(frame) == 2 * 3 * 3 and kf.calls == 1 and kf.scalings == ["set"]
    again = mb.get_window_means(wins, alpha=ALPHA)
    assert kf.calls == 1 and again.equals(frame)                               # from the cache
    std = mb.get_window_means(wins, alpha=ALPHA, standardized=True)
    assert kf.calls == 2 and kf.scalings[-1] == "none" and kf.scale is not None   # the facade's scaling is left behind
    s, m = mb._std.numpy(), mb._mean.numpy()
    for r in range(2):
        for j, name in enumerate(mb.batch.names[r]):
            a, b = frame.loc[(r, name)], std.loc[(r, name)]
            assert np.allclose(a["mean"].values, b["mean"].values * s[r, j] + m[r, j], rtol=1e-12, atol=1e-12)
            # (variances: a fully observed window has one of 0 +- rounding, whose root is not small)
            assert np.allclose(a["sd"].values ** 2, (b["sd"].values * s[r, j]) ** 2, rtol=1e-9, atol=1e-15)
    one = mb.get_window_mean(1, "s2", wins, alpha=ALPHA)
    assert one.equals(frame.loc[(1, "s2")]) and list(one.index) == [w[0] for w in wins]
    # against the recursion directly, and a one-day window against the projection of the oracle's smoother
    phi, q = kf.params_from_alpha(ALPHA, dt=mb.dt)
    g = cf.variant(dict(N=3, K=1, T=mb.T, R=2, B=2, obs=kf.obs_np, loadings=kf.load_np, obsvar=None, scale=s, offset=m, phi=phi.numpy(),
                        q=q.numpy(), x0=None, P0=None))
    mean, var = fr.functional_walk(g, 0, (5, 20, 0, 0), np.eye(3)[1])
    assert frame.loc[(0, "s1", idx[5]), "mean"] == mean and frame.loc[(0, "s1", idx[5]), "sd"] == np.sqrt(var)
    day = mb.get_window_means([(idx[7], idx[8])], alpha=ALPHA)
    ref = cf.reference(g, 0, 0, parts=("state",))
    assert abs(day.loc[(0, "s0", idx[7]), "mean"] - ref["sim_means"][7, 0]) <= 1e-8
    assert abs(day.loc[(0, "s0", idx[7]), "sd"] ** 2 - ref["sim_vars"][7, 0]) <= 1e-8
    # an offset alias: the months of the model's own index; the shorter model's padding is in no window
    months = mb.get_window_means("MS", alpha=ALPHA)
    assert set(months.index.get_level_values("window")) == {pd.Timestamp("2001-01-01"), pd.Timestamp("2001-02-01")}
    assert np.isfinite(months.values).all()
    with pytest.raises(ValueError):
        mb.get_window_means([(idx[9], idx[2])], alpha=ALPHA)
    with pytest.raises(KeyError):
        mb.get_window_mean(0, "nope", wins, alpha=ALPHA)


def test_facade_contrasts_and_changes():
    from scipy.stats import norm

    models, G = two_models()
    models[1] = [s.rename("w%d" % j) for j, s in enumerate(models[1])]      # the second model has other series
    mb = stand_in(FunctionalEngine, models, G)
    idx = mb.batch.index[0]
    a, b = (idx[3], idx[12]), (idx[20], idx[33])
    contrasts = {"gradient": {"s0": 1.0, "s2": -1.0}, "group": {"w0": 0.5, "w1": 0.5}, "absent": {"zz": 1.0}}
    frame = mb.get_window_means([a], contrasts=contrasts, alpha=ALPHA)
    assert list(frame.index) == [(0, "gradient", a[0]), (1, "group", a[0])]
    unit = mb.get_window_means([a], alpha=ALPHA)
    assert abs(frame.loc[(0, "gradient", a[0]), "mean"] - (unit.loc[(0, "s0", a[0]), "mean"] - unit.loc[(0, "s2", a[0]), "mean"])) <= 1e-10
    assert abs(frame.loc[(1, "group", a[0]), "mean"] - 0.5 * (unit.loc[(1, "w0", a[0]), "mean"] + unit.loc[(1, "w1", a[0]), "mean"])) <= 1e-10
    with pytest.raises(KeyError):
        mb.get_window_means([a], contrasts={"absent": {"zz": 1.0}}, alpha=ALPHA)
    change = mb.get_changes(a, b, alpha=ALPHA)
    assert list(change.columns) == ["estimate", "sd", "z", "pvalue"] and change.index.names == ["model", "series"] and len(change) == 6
    both = mb.get_window_means([a, b], alpha=ALPHA)
    for (r, name), row in change.iterrows():
        assert abs(row["estimate"] - (both.loc[(r, name, a[0]), "mean"] - both.loc[(r, name, b[0]), "mean"])) <= 1e-10
        assert row["z"] == row["estimate"] / row["sd"] and row["pvalue"] == 2.0 * norm.sf(abs(row["z"]))
        # var(A - B) = var A + var B - 2 cov, |cov| <= sd A sd B
        sa, sb = both.loc[(r, name, a[0]), "sd"], both.loc[(r, name, b[0]), "sd"]
        assert row["sd"] > 0.0 and abs(row["sd"] ** 2 - (sa ** 2 + sb ** 2)) <= 2.0 * sa * sb * (1 + 1e-9) + 1e-12
    back = mb.get_changes(b, a, alpha=ALPHA)
    assert np.allclose(back["estimate"].values, -change["estimate"].values, rtol=0, atol=1e-10)
    assert np.allclose(back["sd"].values, change["sd"].values, rtol=1e-9, atol=0)
    labelled = mb.get_changes(a, b, contrasts=contrasts, alpha=ALPHA)
    assert list(labelled.index) == [(0, "gradient"), (1, "group")]
    # the second model is four days shorter: a period in its padding has no step -> NaN for that model only
    late = mb.get_changes(a, (idx[37], idx[39]) , alpha=ALPHA)
    assert np.isfinite(late.loc[0].values).all() and np.isnan(late.loc[1][["estimate", "sd", "z", "pvalue"]].values).all()
    with pytest.raises(ValueError):
        mb.get_changes(a, (idx[10], idx[15]), alpha=ALPHA)
