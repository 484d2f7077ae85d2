"""Exact window means, changes and contrasts on the GPU (C ABI mk_functionals: the recording forward pass, the smoother,
functional_walk_kernel) against the DEFINITION in numpy longdouble (tests/functional_ref.py::functional_definition: dense
conditioning of the stacked states, no filter and no smoother), at the bars of tests/functional_ref.py::bars -- SMOOTH_ATOL A zeta
for the mean, SMOOTH_ATOL (A zeta)^2 for the variance; tests/test_functionals_host.py measures that the float64 recursion itself
stays 6.6e-6 of a bar from the definition, so the bars stand as given -- bit for bit across batches and numbers of windows, under
both layouts and kernel families, next to invalid models, and the refusals of the raw ABI.

Measured on the MI355X: the largest distance on any case of this file is 6.8e-6 of a bar ((8,2), T = 17; printed per case with
``-s``); the file's 31 tests take 20 s.

The models here are MILD by construction: the records come from call_forms.shared_group, which redraws until every persistence is
below 1 - 1e-3.  Persistence up to 1 - 1e-9, a communality of 0.999 and the hard missingness patterns are run through this route
by tests/test_gpu_property_fits.py (tests/test_property_fits.py on the CPU), at the conditioning-aware bars of tests/hard_models.py."""
import ctypes

import numpy as np
import pytest

import call_forms as cf
import functional_ref as fr
import status_cases as sc

pytestmark = pytest.mark.gpu

PREFILL = 0xA5A5A5A5
LAYOUTS = ("model_major", "time_major")
CASES = [(N, K, T, "specialised") for N, K, T in fr.GROUPS] + [(8, 2, 17, "generic")]


def _np(t):
    return t.detach().cpu().numpy()


def _engine(g, layout="model_major", family="specialised", packed_sym=False):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout, packed_sym=packed_sym)
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
    if g["scale"] is not None:
        kf.set_scaling(g["scale"], g["offset"])
    if family == "generic":
        kf.set_variant("kernel_family", family)
    return kf


def _call(kf, g, wins, table, **kw):
    res = kf.functionals(g["phi"], g["q"], wins, table, **cf.init(g), **kw)
    return {k: _np(res[k]).copy() for k in ("mean", "var", "status")}


def _compare(g, got, wins, table, what):
    """Every functional of every instance against the definition; returns the largest distance in bars."""
    worst = 0.0
    W = np.broadcast_to(wins, (g["R"],) + tuple(np.shape(wins)[-2:]))
    for i in range(g["B"]):
        r = i % g["R"]
        dm, dv = fr.functional_definition(g, i, W[r], table)
        rows = fr.contrast_rows(g, i, table)
        assert got["mean"][i].shape == dm.shape
        for w, win in enumerate(W[r]):
            for k, c in enumerate(rows):
                m, v = got["mean"][i, w, k], got["var"][i, w, k]
                where = "%s: instance %d, window %s, contrast %d" % (what, i, tuple(win), k)
                if np.isnan(dm[w, k]):
                    assert np.isnan(m) and np.isnan(v), where
                    continue
                assert v >= 0.0, where
                bm, bv = fr.bars(g, i, win, c)
                if bm == 0.0:      # the all-zero contrast
                    assert m == 0.0 and v == 0.0, where
                    continue
                em, ev = abs(float(m - dm[w, k])) / bm, abs(float(v - dv[w, k])) / bv
                assert em <= 1.0 and ev <= 1.0, "%s: mean %.3g bars, variance %.3g bars from the definition" % (where, em, ev)
                worst = max(worst, em, ev)
    return worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=["%dx%d-T%d-%s" % c for c in CASES])
def test_against_the_definition(case, layout):
    """B = 15 on 3 records, a different window list per record, given x0 / P0, observation variances on about half the series, a
    scale and an offset: the unit contrasts (NULL), C = 1, and a table with a two-well difference, an all-zero contrast and a group
    mean; C = 64 at (60,4)."""
    N, K, T, family = case
    g = fr.group(N, K, T)
    kf = _engine(g, layout, family)
    assert kf.functionals_supported
    wins = fr.windows(T)
    worst = 0.0
    for kind in ("unit", "one", "mixed") + (("full",) if N == 60 else ()):
        table = fr.contrasts(g, kind)
        got = _call(kf, g, wins, table)
        assert not got["status"].any()
        worst = max(worst, _compare(g, got, wins, table, "(%d,%d) T=%d %s %s %s" % (N, K, T, family, layout, kind)))
    print("(%d,%d) T=%d %s %s: at most %.3g bars from the definition" % (N, K, T, family, layout, worst))


@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17), (60, 4, 3)], ids=["8x2", "13x4", "60x4"])
def test_batch_position_independent(shape):
    """The 15-instance call equals the five 3-instance calls bit for bit, and the two layouts agree bit for bit."""
    g = fr.group(*shape)
    wins, table = fr.windows(shape[2]), fr.contrasts(g, "mixed")

    def fn(grp, layout="model_major"):
        out = _call(_engine(grp, layout), grp, wins, table)
        return {k: out[k] for k in ("mean", "var")}

    cf.check_position_independent(fn, g, "functionals (%d,%d)" % shape[:2])
    a, b = fn(g), fn(g, "time_major")
    assert np.array_equal(a["mean"], b["mean"], equal_nan=True) and np.array_equal(a["var"], b["var"], equal_nan=True)


@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17)], ids=["8x2", "13x4"])
def test_windows_one_at_a_time(shape):
    """A call with all W windows equals W one-window calls bit for bit, and the unit contrasts given as a table equal NULL."""
    g = fr.group(*shape)
    kf = _engine(g)
    wins = fr.windows(shape[2])
    whole = _call(kf, g, wins, None)
    for w in range(wins.shape[1]):
        one = _call(kf, g, wins[:, w:w + 1], None)
        assert np.array_equal(one["mean"][:, 0], whole["mean"][:, w], equal_nan=True), w
        assert np.array_equal(one["var"][:, 0], whole["var"][:, w], equal_nan=True), w
    eye = _call(kf, g, wins, np.broadcast_to(np.eye(g["N"]), (g["R"], g["N"], g["N"])).copy())
    assert np.array_equal(eye["mean"], whole["mean"], equal_nan=True) and np.array_equal(eye["var"], whole["var"], equal_nan=True)


@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17)], ids=["8x2", "13x4"])
def test_one_step_windows_are_the_projection(shape):
    """An independent kernel: one-step windows with unit contrasts are sim_means / sim_vars of the projecting smoother."""
    g = fr.group(*shape)
    T = shape[2]
    kf = _engine(g)
    wins = np.array([(t, t + 1, 0, 0) for t in range(T)], dtype=np.int64)
    got = _call(kf, g, wins, None)
    sim = kf.simulate_smoothed(g["phi"], g["q"], warmup=0, **cf.init(g))
    sm, sv = _np(sim["sim_means"]), _np(sim["sim_vars"])
    for i in range(g["B"]):
        r = i % g["R"]
        tol = cf.bar("sim_means", None, g, r) + cf.SMOOTH_ATOL * float(g["scale"][r].max()) ** 2
        assert np.abs(got["mean"][i] - sm[i]).max() <= tol and np.abs(got["var"][i] - sv[i]).max() <= tol, i


@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17)], ids=["8x2", "13x4"])
def test_fully_observed_window_without_observation_variances(shape):
    """Every cell observed, obsvar = None: the variance of a unit contrast over observed steps is exactly 0 or within the bar of
    it, never negative -- and within the bar of the definition."""
    g0 = fr.group(*shape)
    rng = np.random.default_rng(5)
    obs = np.where(np.isnan(g0["obs"]), rng.normal(size=g0["obs"].shape), g0["obs"])
    g = cf.variant(g0, obs=obs, obsvar=None)
    wins = np.array([(3, 4, 0, 0), (2, 9, 0, 0), (0, shape[2], 0, 0), (1, 3, 10, 15)], dtype=np.int64)
    got = _call(_engine(g), g, wins, None)
    assert not got["status"].any() and (got["var"] >= 0.0).all()
    _compare(g, got, wins, None, "fully observed (%d,%d)" % shape[:2])
    for i in range(g["B"]):
        for w, win in enumerate(wins):
            for j in range(g["N"]):
                assert got["var"][i, w, j] <= fr.bars(g, i, win, np.eye(g["N"])[j])[1], (i, w, j)


@pytest.mark.parametrize("shape", [(8, 2), (13, 4)], ids=["8x2", "13x4"])
def test_status(shape):
    """The zero-pivot common factor sets MK_FLAG_RANK_DEFICIENT and gives finite outputs; an instance with a negative observation
    variance gets NaN rows and its filter's bits, its neighbours' outputs are bit-identical to the same call on the clean twin.
    d_status goes in prefilled: the call WRITES the word."""
    wins = np.array([(0, sc.T, 0, 0), (1, 4, 5, sc.T), (sc.T - 1, sc.T, 0, 0), (2, 3, 0, 0)], dtype=np.int64)
    for name in ("zero_factor", "neg_once"):
        c = sc.case(shape[0], shape[1], name)
        outs = []
        for g in (c["bad"], c["twin"]):
            kf = _engine(g)
            buf = kf.alloc_functionals(g["B"], len(wins), g["N"])
            buf["status"].fill_(PREFILL - (1 << 32))
            outs.append(_call(kf, g, wins, None, buffers=buf))
        bad, twin = outs
        sc.check_flags(bad["status"], c, "rts", "functionals")
        sc.check_twin_flags(twin["status"], c, "rts", "functionals")
        sc.check_containment(bad, twin, c, "functionals")
        touched = list(c["touched"])
        if name == "zero_factor":
            assert (bad["status"][touched] == sc.FLAG_RANK_DEFICIENT).all()
            assert np.isfinite(bad["mean"]).all() and np.isfinite(bad["var"]).all()
        else:
            assert (bad["status"][touched] & sc.FLAG_NONPOSITIVE_F).all()
            assert np.isnan(bad["mean"][touched]).all() and np.isnan(bad["var"][touched]).all()
        _compare(c["twin"], twin, wins, None, "twin of %s" % name)


def test_refusals():
    """C = 65, W = 0, a NULL d_work or output, a buffer too small: MK_ERR_INVALID; N + K = 65: MK_ERR_SHAPE; a packed-symmetric
    engine: refused by the engine -- all without a launch, the outputs keep their sentinel."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import FunctionalRequest, Problem
    from metran_amd.engine import MetranHipError

    g = fr.group(8, 2, 17)
    kf = _engine(g)
    L = _lib.lib()
    assert int(L.mk_functionals_max_contrasts()) == 64
    assert int(L.mk_functionals_work_stride(61, 4)) == 0 and int(L.mk_functionals_work_stride(60, 4)) == 2 * int(L.mk_record_stride(64))
    B, W, C, N = g["B"], 3, 8, 8
    prob, keep, _ = kf._problem(kf._dev(g["phi"]), kf._dev(g["q"]), 0, None, None)
    buf = kf.alloc_functionals(B, W, C)
    buf["mean"].fill_(7.5)
    buf["var"].fill_(7.5)
    wins = torch.as_tensor(fr.windows(17)[:, :W].copy(), dtype=torch.int64, device="cuda")
    table = torch.zeros((3, 65, N), dtype=torch.float64, device="cuda")
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0   # an allocation of its own: its size is known exactly

    def call(work=buf["_work"].data_ptr(), windows=wins.data_ptr(), contrasts=0, n_windows=W, n_contrasts=C, mean=buf["mean"].data_ptr(),
             var=buf["var"].data_ptr(), problem=prob):
        c = lambda v: ctypes.c_void_p(v) if v else None   # noqa: E731
        req = FunctionalRequest()
        req.n_windows, req.n_contrasts, req.d_windows, req.d_contrasts = n_windows, n_contrasts, windows or None, contrasts or None
        return L.mk_functionals(kf._ctx, ctypes.byref(problem), c(work), 0, ctypes.byref(req), c(mean), c(var), None)

    try:
        assert call(work=0) == -1 and b"d_work" in L.mk_last_error()
        assert call(windows=0) == -1 and call(mean=0) == -1 and call(var=0) == -1 and b"required" in L.mk_last_error()
        assert call(n_windows=0) == -1 and b"n_windows" in L.mk_last_error()
        assert call(n_contrasts=65, contrasts=table.data_ptr()) == -1 and b"n_contrasts" in L.mk_last_error()
        assert call(n_contrasts=0, contrasts=table.data_ptr()) == -1 and b"n_contrasts" in L.mk_last_error()
        assert call(n_contrasts=5) == -1 and b"unit contrasts" in L.mk_last_error()          # NULL contrasts: C must be N
        assert call(work=small.value) == -1 and b"d_work" in L.mk_last_error()
        assert call(windows=small.value, n_windows=40) == -1 and b"d_windows" in L.mk_last_error()
        assert call(mean=small.value) == -1 and b"d_mean" in L.mk_last_error()
        assert call(var=small.value) == -1 and b"d_var" in L.mk_last_error()
        assert call(contrasts=small.value, n_contrasts=3) == -1 and b"d_contrasts" in L.mk_last_error()
        q = ctypes.c_void_p(buf["_work"].data_ptr())
        wide = Problem(1, 1, 4, 61, 4, 0, q, q, q, q, None, None, None, 0, None, None)
        assert call(problem=wide) == -2 and b"N=61, K=4" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    torch.cuda.synchronize()
    assert (buf["mean"] == 7.5).all() and (buf["var"] == 7.5).all()
    assert call() == 0
    torch.cuda.synchronize()
    assert not (buf["mean"] == 7.5).any()
    packed = _engine(g, packed_sym=True)
    assert not packed.functionals_supported
    with pytest.raises(MetranHipError, match="-2"):
        packed.functionals(g["phi"], g["q"], fr.windows(17))
    with pytest.raises(ValueError):
        kf.functionals(g["phi"], g["q"], np.zeros((2, 3, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        kf.functionals(g["phi"], g["q"], fr.windows(17), np.zeros((3, 65, N)))
    with pytest.raises(ValueError):
        kf.alloc_functionals(3, 0, 8)


def test_metran_batch_end_to_end():
    """Through MetranBatch: one-day windows are get_simulation's mean and band; a window mean's sd agrees with the sd of the draws'
    window means to Monte Carlo accuracy; a change is the difference of the two window means, and a contrast of two series at one
    step the difference of their simulated means."""
    import pandas as pd

    from metran_amd.batch import MetranBatch
    from metran_amd.synthetic import make_dfm_batch

    T = 90
    d = make_dfm_batch(2, 3, 1, T, seed=5, missing=0.5)
    idx = pd.date_range("2001-01-01", periods=T, freq="D")
    models = [[pd.Series(10.0 * (j + 1) + (1.0 + 0.5 * j) * d["obs"][r, :, j], index=idx, name="s%d" % j).dropna() for j in range(3)]
              for r in range(2)]
    mb = MetranBatch(models, factors=d["loadings"])
    alpha = d["alpha"]
    days = [(idx[t], idx[t + 1]) for t in (3, 40, 41)]
    frame = mb.get_window_means(days, alpha=alpha)
    sim = mb.get_simulation(0, "s1", alpha=alpha, ci=None)
    var = _np(mb.get_simulated_variances(alpha=alpha))
    i0 = mb.batch.index[0]
    for start, _ in days:
        t = i0.get_loc(start)
        row = frame.loc[(0, "s1", start)]
        assert abs(row["mean"] - sim.iloc[t]) <= 1e-8 and abs(row["sd"] ** 2 - var[0, t, 1]) <= 1e-8
    months = mb.get_window_mean(1, "s2", "MS", alpha=alpha)
    stats = mb.get_window_statistic(1, "s2", "MS", ndraws=200, alpha=alpha)
    assert len(months) == len(stats) and list(months.index) == list(stats.index)
    ok = np.isfinite(months["sd"].values)
    assert ok.sum() >= 2
    assert np.all(np.abs(months["mean"].values[ok] - stats[("mean", "mean")].values[ok]) <= 5.0 * months["sd"].values[ok] / np.sqrt(200) + 1e-9)
    assert np.all(np.abs(stats[("mean", "sd")].values[ok] / months["sd"].values[ok] - 1.0) <= 5.0 / np.sqrt(400))   # relative error 1/sqrt(2S)
    a, b = (idx[5], idx[30]), (idx[50], idx[80])
    change = mb.get_changes(a, b, alpha=alpha)
    both = mb.get_window_means([a, b], alpha=alpha)
    for r in range(2):
        for name in ("s0", "s1", "s2"):
            row = change.loc[(r, name)]
            assert abs(row["estimate"] - (both.loc[(r, name, a[0]), "mean"] - both.loc[(r, name, b[0]), "mean"])) <= 1e-9
            assert row["sd"] > 0 and abs(row["z"] - row["estimate"] / row["sd"]) <= 1e-12 and 0.0 <= row["pvalue"] <= 1.0
    grad = mb.get_window_means(days[:1], contrasts={"gradient": {"s0": 1.0, "s2": -1.0}}, alpha=alpha)
    means = _np(mb.get_simulated_means(alpha=alpha))
    t = i0.get_loc(days[0][0])
    assert abs(grad.loc[(0, "gradient", days[0][0]), "mean"] - (means[0, t, 0] - means[0, t, 2])) <= 1e-8
