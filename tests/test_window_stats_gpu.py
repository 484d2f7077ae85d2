"""Window statistics of posterior draws on the GPU (ensemble_kernels.hip behind mk_path_functionals / mk_ensemble_summary,
BatchedKalman.draw_window_statistics inside the chunk loop of draw_smoothed, MetranBatch.get_window_statistics): against the
numpy restatement (tests/ensemble_ref.py) -- the path functionals bit for bit, the summary's fixed-order statistics bit for bit
and its sd and quantiles to one rounding per summand -- invariance under chunking / sub-ranges / layout, the anchors to what
the smoother pins, the memory the call needs, and the refusals."""
import ctypes

import numpy as np
import pytest

import ensemble_ref as ref
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

TOL = 1e-9        # the tier's smoothed-moment bar


def _np(t):
    return t.detach().cpu().numpy()


def _engine(layout="model_major", **kw):
    from metran_amd.engine import BatchedKalman

    return BatchedKalman(0, layout=layout, **kw)


def _dev(a, dtype=None):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _raw_functionals(kf, paths, windows, thresholds, time_major):
    """mk_path_functionals on ``paths [S,B,T,Wd]`` as a series problem of N = Wd, K = 1."""
    import torch

    from metran_amd._lib import Problem

    S, B, T, Wd = paths.shape
    R, W = windows.shape[:2]
    flat = paths.reshape(S * B, T, Wd)
    stored = _dev(flat.transpose(1, 0, 2) if time_major else flat)
    win, thr = _dev(windows, np.int64), None if thresholds is None else _dev(thresholds)
    out = torch.full((S, B, Wd, W, 5), -777.0, dtype=torch.float64, device="cuda")
    prob = Problem(B, R, T, Wd, 1, 0, None, None, None, None, None, None, None, 0, None, None)
    rc = kf._L.mk_path_functionals(kf._ctx, ctypes.byref(prob), S, 0, int(time_major), _ptr(stored), W, _ptr(win), _ptr(thr), _ptr(out))
    assert rc == 0, kf._L.mk_last_error()
    torch.cuda.synchronize()
    return _np(out)


# 1 ------------------------------------------------------------------ the path kernel through the raw ABI
@pytest.mark.parametrize("Wd", [1, 8, 36, 73])
@pytest.mark.parametrize("T", [1, 2, 33, 200])
def test_path_functionals_equal_the_restatement_bit_for_bit(T, Wd):
    kf = _engine()
    assert kf._L.mk_path_functional_count() == 5
    for S in (1, 3):
        paths, thr = ref.synthetic_paths(S, 15, T, Wd)             # B = 15 on R = 3
        for win in ref.window_sets(T):
            for th in (None, thr):
                want = ref.path_functionals(paths, win, th)
                for tm in (False, True):
                    got = _raw_functionals(kf, paths, win, th, tm)
                    assert ref.same_bits(got, want), (S, win.shape, th is None, tm)


# 2 ------------------------------------------------------------------ the summary kernel through the raw ABI
def _raw_summary(kf, values, probs):
    import torch

    S, cells = values.shape
    probs = np.ascontiguousarray(probs, dtype=np.float64)
    out = torch.full((cells, 5 + probs.size), -777.0, dtype=torch.float64, device="cuda")
    rc = kf._L.mk_ensemble_summary(kf._ctx, S, cells, _ptr(_dev(values)), probs.size, probs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                   _ptr(out))
    assert rc == 0, kf._L.mk_last_error()
    torch.cuda.synchronize()
    return _np(out)


def _check_summary(got, values, probs, tag):
    want = ref.ensemble_summary(values, probs)
    assert ref.same_bits(got[:, [0, 1, 3, 4]], want[:, [0, 1, 3, 4]]), (tag, "count, mean, min, max")
    assert np.array_equal(np.isnan(got), np.isnan(want)), tag
    err, bar = np.abs(np.nan_to_num(got - want)), ref.summary_bar(values)
    print("summary %s: largest error over its bar %.3f" % (tag, (err / np.maximum(bar, 1e-300)[:, None]).max()))
    assert (err <= bar[:, None]).all(), tag


@pytest.mark.parametrize("S", [1, 2, 3, 5, 33, 64, 65, "cap"])
def test_ensemble_summary_matches_the_restatement(S):
    kf = _engine()
    cap = int(kf._L.mk_ensemble_max_draws())
    assert cap >= 4096
    S = cap if S == "cap" else S
    values = ref.summary_values(S)
    _check_summary(_raw_summary(kf, values, ref.PROBS), values, ref.PROBS, "S=%d" % S)


# 3 ------------------------------------------------------------------ end to end against the draws of the same engine
def _model(N, K, B, T, seed):
    d = make_dfm_batch(B, N, K, T, seed=seed, missing=0.3)
    obs = d["obs"].copy()
    obs[:, 0] = np.nan
    rng = np.random.default_rng(seed)
    return d, obs, rng.uniform(0.5, 2.0, (B, N)), rng.normal(size=(B, N))


@pytest.mark.parametrize("layout", ["model_major", "time_major"])
@pytest.mark.parametrize("shape", [(8, 2, 3, 30), (32, 4, 3, 30), (70, 3, 2, 12)], ids=["8x2_records", "32x4_tape", "70x3_generic"])
def test_statistics_equal_the_restatement_on_the_draws(shape, layout):
    N, K, B, T = shape
    S, seed = 6, 2024
    d, obs, scale, offset = _model(N, K, B, T, 5 * N + K)
    kf = _engine(layout)
    kf.set_observations(obs).set_loadings(d["loadings"]).set_scaling(scale, offset)
    if (N, K) == (32, 4):
        assert kf.tape_path()
    win = ref.window_sets(T, R=B)[1]
    rng = np.random.default_rng(7)
    for what in ("series", "states"):
        Wd = N if what == "series" else N + K
        thr = offset + 0.3 * scale * rng.standard_normal((B, N)) if what == "series" else 0.3 * rng.standard_normal((B, Wd))
        for antithetic in (False, True):
            kw = dict(seed=seed, what=what, antithetic=antithetic, first_instance=2)
            draws = kf.draw_smoothed(d["phi"], d["q"], S, **kw)
            assert int(draws["status"].abs().sum().item()) == 0
            want = ref.path_functionals(_np(draws["draws"]), win, thr)
            one = kf.draw_window_statistics(d["phi"], d["q"], S, win, thr, probs=ref.PROBS, chunk=S, return_functionals=True, **kw)
            tag = (what, antithetic)
            assert tuple(one["summary"].shape) == (B, Wd, 5, 5, 10) and tuple(one["status"].shape) == (S, B)
            assert int(one["status"].abs().sum().item()) == 0
            assert ref.same_bits(_np(one["functionals"]), want), tag
            each = kf.draw_window_statistics(d["phi"], d["q"], S, win, thr, probs=ref.PROBS, chunk=1, return_functionals=True, **kw)
            assert ref.same_bits(_np(each["functionals"]), want), (tag, "chunk = 1")
            assert ref.same_bits(_np(each["summary"]), _np(one["summary"])), (tag, "chunk = 1")
            halves = [kf.draw_window_statistics(d["phi"], d["q"], 3, win, thr, first_draw=f, return_functionals=True, **kw)
                      for f in (0, 3)]
            assert ref.same_bits(np.concatenate([_np(h["functionals"]) for h in halves]), want), (tag, "first_draw 0 and 3")
            assert "functionals" not in kf.draw_window_statistics(d["phi"], d["q"], 2, win, thr, **kw)
            _check_summary(_np(one["summary"]).reshape(-1, 10), want.reshape(S, -1), ref.PROBS, "%s %s %s" % (shape, layout, tag))


def test_a_flagged_path_is_outside_the_counts():
    """An instance with a NaN persistence: its paths are flagged, NaN in the functionals and not counted in the summary."""
    from metran_amd.engine import FLAG_NONPOSITIVE_F

    N, K, B, T, S = 8, 2, 3, 20, 4
    d, obs, scale, offset = _model(N, K, B, T, 3)
    kf = _engine("time_major")
    kf.set_observations(obs).set_loadings(d["loadings"])
    phi = d["phi"].copy()
    phi[1, 2] = np.nan
    out = kf.draw_window_statistics(phi, d["q"], S, ref.window_sets(T, R=B)[0], return_functionals=True)
    status, fun, summary = _np(out["status"]), _np(out["functionals"]), _np(out["summary"])
    assert (status[:, 1] & FLAG_NONPOSITIVE_F).all() and not status[:, [0, 2]].any()
    assert np.isnan(fun[:, 1]).all() and np.isfinite(fun[:, [0, 2], :, :, :3]).all()
    assert (summary[1, ..., 0] == 0).all() and np.isnan(summary[1, ..., 1:]).all()
    assert (summary[[0, 2], :, :, :3, 0] == S).all()


# 4 ------------------------------------------------------------------ anchors to what the smoother pins
def test_an_observed_window_has_no_spread():
    """Where a window of series j lies wholly in observed cells (no observation variance), its mean is the observed window mean
    in every draw."""
    N, K, B, T, S = 8, 2, 3, 40, 6
    d = make_dfm_batch(B, N, K, T, seed=11, missing=0.0)
    obs = d["obs"].copy()
    drop = np.random.default_rng(3).random(obs.shape) < 0.4
    drop[:, 10:25, 2] = False                                # series 2 is observed throughout steps 10..24
    obs[drop] = np.nan
    rng = np.random.default_rng(4)
    scale, offset = rng.uniform(0.5, 2.0, (B, N)), rng.normal(size=(B, N))
    kf = _engine("time_major")
    kf.set_observations(obs).set_loadings(d["loadings"]).set_scaling(scale, offset)
    win = np.array([[0, 10], [10, 25], [25, 40]], dtype=np.int64)
    out = kf.draw_window_statistics(d["phi"], d["q"], S, win, seed=8, return_functionals=True)
    fun, summary = _np(out["functionals"]), _np(out["summary"])
    want = (obs[:, 10:25, 2] * scale[:, None, 2] + offset[:, None, 2]).mean(axis=1)
    assert np.abs(fun[:, :, 2, 1, 0] - want[None]).max() <= TOL * max(1.0, np.abs(want).max())
    assert (summary[:, 2, 1, 0, 2] < TOL).all()              # the ensemble sd of the window mean
    assert (summary[:, 2, 0, 0, 2] > 1e-3).all()             # a window with gaps does spread


def test_antithetic_one_step_windows_average_to_the_smoothed_projection():
    N, K, B, T = 8, 2, 3, 24
    d, obs, scale, offset = _model(N, K, B, T, 21)
    kf = _engine("time_major")
    kf.set_observations(obs).set_loadings(d["loadings"]).set_scaling(scale, offset)
    sim = _np(kf.simulate_smoothed(d["phi"], d["q"])["sim_means"])          # [B,T,N]
    win = np.stack([np.arange(T), np.arange(T) + 1], axis=1).astype(np.int64)
    out = kf.draw_window_statistics(d["phi"], d["q"], 2, win, seed=5, antithetic=True)
    mean = _np(out["summary"])[:, :, :, 0, 1]                                # [B,N,W] ensemble mean of the window mean
    assert np.abs(mean.transpose(0, 2, 1) - sim).max() <= TOL * max(1.0, np.abs(sim).max())


# 5 ------------------------------------------------------------------ memory: the ensemble is never held
def test_the_ensemble_is_never_allocated():
    import torch

    N, K, B, T, S = 8, 2, 16, 512, 256
    d, obs, scale, offset = _model(N, K, B, T, 1)
    kf = _engine("time_major")
    kf.set_observations(obs).set_loadings(d["loadings"]).set_scaling(scale, offset)
    win = np.array([[0, 128], [128, 256], [256, 384], [384, 512]], dtype=np.int64)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = kf.draw_window_statistics(d["phi"], d["q"], S, win, thresholds=offset, chunk=4)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    ensemble = 8 * S * B * T * N
    print("window statistics of %d draws: peak %.1f MB against %.1f MB for the ensemble" % (S, peak / 1e6, ensemble / 1e6))
    assert (_np(out["summary"])[..., 0] == S).all()
    assert peak < 0.5 * ensemble


# 6 ------------------------------------------------------------------ the facade
def test_metran_batch_window_statistics():
    import pandas as pd

    from metran_amd.batch import MetranBatch

    N, K, S = 4, 1, 5
    d = make_dfm_batch(2, N, K, 150, seed=9, missing=0.25)
    names = ["well%d" % j for j in range(N)]
    frames = [pd.DataFrame(d["obs"][0], index=pd.date_range("2010-01-20", periods=150, freq="D"), columns=names),
              pd.DataFrame(d["obs"][1][:95] * 2.0 + 3.0, index=pd.date_range("2010-02-10", periods=95, freq="D"), columns=names)]
    mb = MetranBatch(frames, factors=d["loadings"])
    alpha = np.full((2, N + K), 12.0)
    levels = {"well0": 0.1, "well2": 2.5}
    frame = mb.get_window_statistics("MS", thresholds=levels, ndraws=S, probs=(0.1, 0.5), seed=4, alpha=alpha)
    draws = _np(mb.get_simulation_draws(S, seed=4, alpha=alpha))            # [S,R,T,N], original units
    from metran_amd.windows import step_windows

    steps, starts = step_windows(mb.batch.index, "MS", mb.T)
    W = steps.shape[1]
    assert W == len(starts[0]) >= 5 and 3 <= len(starts[1]) < W          # about six months against about four: pads in model 1
    thr = np.array([[levels.get(name, np.nan) for name in names]] * 2)
    fun = ref.path_functionals(draws, steps, thr)
    want = ref.ensemble_summary(fun.reshape(S, -1), (0.1, 0.5)).reshape(2, N, W, 5, 7)
    assert list(frame.index.names) == ["model", "series", "window"] and len(frame) == N * (len(starts[0]) + len(starts[1]))
    assert list(frame.columns.get_level_values(0).unique()) == list(ref.FUNCTIONALS)
    assert list(frame["mean"].columns) == ["count", "mean", "sd", "min", "max", "q0.1", "q0.5"]
    bar = ref.summary_bar(fun.reshape(S, -1)).reshape(2, N, W, 5)
    for r in range(2):
        for j, name in enumerate(names):
            rows = frame.loc[(r, name)]
            assert list(rows.index) == list(starts[r])
            got = rows.values.reshape(len(starts[r]), 5, 7)
            w = want[r, j, : len(starts[r])]
            assert np.array_equal(np.isnan(got), np.isnan(w))
            assert ref.same_bits(got[..., [0, 1, 3, 4]], w[..., [0, 1, 3, 4]])
            assert (np.abs(np.nan_to_num(got - w)) <= bar[r, j, : len(starts[r]), :, None]).all()
            assert np.isnan(got[:, 3:, 1:]).all() == (name not in levels)
    one = mb.get_window_statistic(1, "well2", "MS", thresholds=levels, ndraws=S, probs=(0.1, 0.5), seed=4, alpha=alpha)
    assert one.equals(frame.loc[(1, "well2")])
    with pytest.raises(KeyError):
        mb.get_window_statistic(1, "nowhere", "MS", alpha=alpha)


# 7 ------------------------------------------------------------------ refusals
def test_refusals():
    import torch

    from metran_amd._lib import MetranHipError, Problem

    N, K, B, T = 8, 2, 2, 16
    d, obs, scale, offset = _model(N, K, B, T, 3)
    kf = _engine()
    kf.set_observations(obs).set_loadings(d["loadings"])
    L = kf._L
    for bad in ([[0, 8], [6, 12]], [[8, 12], [0, 4]], [[0, 17]], [[5, 3]], [[-1, 3]]):
        with pytest.raises(ValueError):
            kf.draw_window_statistics(d["phi"], d["q"], 2, np.array(bad, dtype=np.int64))
    cap = int(L.mk_ensemble_max_draws())
    with pytest.raises(ValueError):
        kf.draw_window_statistics(d["phi"], d["q"], cap + 1, np.array([[0, 16]]))
    with pytest.raises(ValueError):
        kf.draw_window_statistics(d["phi"], d["q"], 2, np.array([[0, 16]]), probs=(0.5, 1.5))
    with pytest.raises(ValueError):
        kf.draw_window_statistics(d["phi"], d["q"], 2, np.array([[0, 16]]), probs=np.linspace(0, 1, 17))
    with pytest.raises(ValueError):
        kf.draw_window_statistics(d["phi"], d["q"], 2, np.array([[0, 16]]), what="other")
    packed = _engine(packed_sym=True)
    packed.set_observations(obs).set_loadings(d["loadings"])
    with pytest.raises(MetranHipError):
        packed.draw_window_statistics(d["phi"], d["q"], 2, np.array([[0, 16]]))
    # the raw ABI: every refusal is MK_ERR_INVALID with a message, the outputs untouched
    buf = torch.full((4096,), -777.0, dtype=torch.float64, device="cuda")
    p = _ptr(buf)
    dp = ctypes.POINTER(ctypes.c_double)
    probs = (ctypes.c_double * 17)(*np.linspace(0.0, 1.0, 17))
    assert L.mk_ensemble_summary(kf._ctx, cap + 1, 1, p, 1, ctypes.cast(probs, dp), p) == -1 and b"mk_ensemble_max_draws" in L.mk_last_error()
    assert L.mk_ensemble_summary(kf._ctx, 0, 1, p, 1, ctypes.cast(probs, dp), p) == -1
    assert L.mk_ensemble_summary(kf._ctx, 4, 2, p, 17, ctypes.cast(probs, dp), p) == -1 and b"nprobs" in L.mk_last_error()
    for wrong in (1.5, -0.1, float("nan")):
        one = (ctypes.c_double * 2)(0.5, wrong)
        assert L.mk_ensemble_summary(kf._ctx, 4, 2, p, 2, ctypes.cast(one, dp), p) == -1 and b"probs[1]" in L.mk_last_error()
    assert L.mk_ensemble_summary(kf._ctx, 4, 2, None, 1, ctypes.cast(probs, dp), p) == -1 and b"d_values" in L.mk_last_error()
    assert L.mk_ensemble_summary(kf._ctx, 4, 2, p, 1, None, p) == -1
    prob = Problem(2, 2, 8, 4, 1, 0, None, None, None, None, None, None, None, 0, None, None)
    win = _dev(np.array([[[0, 8]], [[0, 8]]]), np.int64)
    assert L.mk_path_functionals(kf._ctx, ctypes.byref(prob), 1, 0, 0, p, 0, _ptr(win), None, p) == -1 and b"W >= 1" in L.mk_last_error()
    assert L.mk_path_functionals(kf._ctx, ctypes.byref(prob), 0, 0, 0, p, 1, _ptr(win), None, p) == -1
    assert L.mk_path_functionals(kf._ctx, ctypes.byref(prob), 1, 2, 0, p, 1, _ptr(win), None, p) == -1 and b"what" in L.mk_last_error()
    assert L.mk_path_functionals(kf._ctx, ctypes.byref(prob), 1, 0, 0, None, 1, _ptr(win), None, p) == -1 and b"d_paths" in L.mk_last_error()
    assert L.mk_path_functionals(kf._ctx, ctypes.byref(prob), 1, 0, 0, p, 1, None, None, p) == -1
    assert L.mk_path_functionals(kf._ctx, ctypes.byref(prob), 1, 0, 0, p, 1, _ptr(win), None, None) == -1
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0
    try:
        assert L.mk_path_functionals(kf._ctx, ctypes.byref(prob), 1, 0, 0, p, 1, _ptr(win), None, small) == -1
        assert b"d_functionals" in L.mk_last_error()
        assert L.mk_ensemble_summary(kf._ctx, 4, 8, small, 1, ctypes.cast(probs, dp), p) == -1 and b"d_values" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    torch.cuda.synchronize()
    assert bool((buf == -777.0).all())
