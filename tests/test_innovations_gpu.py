"""One-step-ahead innovations and their whiteness statistics on the GPU (C ABI mk_innovations: the recording forward pass +
innov_step_kernel; mk_innovation_stats: innov_stats_kernel) against the extended-precision numpy restatement
(tests/innov_ref.py, pinned to the oracle by tests/test_innovations_host.py), end to end through MetranBatch, on the hard
models of the property sweep, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

import hard_models
import innov_ref
import oracle
from metran_amd.synthetic import make_dfm_batch
from shape_matrix import MATRIX

pytestmark = pytest.mark.gpu

N64 = [s for s in MATRIX if s[0] + s[1] == 64][0]
SHAPES = [(8, 2), (12, 4), (13, 4), (19, 2), (32, 4), (33, 4), N64]   # n = 10, 16, 17, 21, 36, 37, 64: every W of the kernel from both sides
OUT = ("v", "f", "pred_mean", "pred_var")


def _np(t):
    return t.detach().cpu().numpy()


def _data(N, K, T, R, B, seed, full):
    """Records [R,T,N] with an empty first step (record 0), an empty step, a step with one series and a full one; ``full``:
    observation variances, initial moments and scaling given."""
    d = make_dfm_batch(B, N, K, T, seed=seed, missing=0.3)
    obs = d["obs"][:R].copy()
    obs[0, 0] = np.nan
    if T > 8:
        obs[:, 3] = np.nan
        obs[1 % R, 5, 1:] = np.nan
        obs[1 % R, 5, 0] = 0.25
        obs[2 % R, 7] = np.where(np.isfinite(obs[2 % R, 7]), obs[2 % R, 7], -0.5)
    rng = np.random.default_rng(seed)
    n = N + K
    p = dict(obs=obs, loadings=d["loadings"][:R], phi=d["phi"], q=d["q"], obsvar=None, x0=None, P0=None, scale=None, offset=None)
    if full:
        p["obsvar"] = rng.uniform(0.05, 0.4, (R, N)) * (rng.random((R, N)) < 0.6)
        p["x0"] = rng.normal(size=(B, n))
        A = rng.normal(size=(B, n, n))
        p["P0"] = A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
        p["scale"] = rng.uniform(0.5, 3.0, (R, N))
        p["offset"] = rng.normal(size=(R, N))
    return p


def _engine(p, layout="model_major"):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(p["obs"]).set_loadings(p["loadings"], p["obsvar"]).set_scaling(p["scale"], p["offset"])
    return kf


def _ref(p, b):
    r = b % p["obs"].shape[0]
    pick = lambda a, i: None if a is None else a[i]   # noqa: E731
    return innov_ref.innovations(p["obs"][r], p["phi"][b], p["q"][b], p["loadings"][r], pick(p["obsvar"], r), pick(p["x0"], b),
                                 pick(p["P0"], b), pick(p["scale"], r), pick(p["offset"], r))


def _check(p, got, instances=None, what=OUT):
    """The bars of tests/test_loo_gpu.py against its same-algorithm reference: atol 1e-12 max(1, max|y|) on v and pred_mean,
    1e-12 relative on f and pred_var; NaN exactly where a cell is not observed."""
    B = p["phi"].shape[0]
    R = p["obs"].shape[0]
    for b in (range(B) if instances is None else instances):
        ref = _ref(p, b)
        y = p["obs"][b % R]
        seen = np.isfinite(y)
        big = max(1.0, np.nanmax(np.abs(y))) if seen.any() else 1.0
        for k in what:
            g, w = got[k][b], ref[k].astype(np.float64)
            if k in ("v", "f"):
                assert np.array_equal(np.isnan(g), ~seen), (k, b)
                g, w = g[seen], w[seen]
            if k == "v":
                np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * big, err_msg="v of instance %d" % b)
            elif k == "pred_mean":   # in the units of the output: max|y| is that of the scaled record
                sc = 1.0 if p["scale"] is None else p["scale"][b % R]
                of = 0.0 if p["offset"] is None else p["offset"][b % R]
                bigo = max(1.0, np.nanmax(np.abs(y * sc + of))) if seen.any() else 1.0
                np.testing.assert_allclose(g, w, rtol=0, atol=1e-12 * bigo, err_msg="pred_mean of instance %d" % b)
            else:
                np.testing.assert_allclose(g, w, rtol=1e-12, atol=0, err_msg="%s of instance %d" % (k, b))


@pytest.mark.parametrize("T", [1, 2, 17])
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_step_kernel_against_restatement(shape, T):
    """B = 6 instances on R = 3 records; t = 0 reads x0 / P0 (given for T = 17, with observation variances and scaling; the
    defaults otherwise).  The per-step sums of v, f reproduce mk_filter's sigmas / detfs of the same call."""
    N, K = shape
    p = _data(N, K, T, 3, 6, seed=100 * N + K + T, full=(T == 17))
    kf = _engine(p)
    assert kf.innovations_supported
    r = kf.innovations(p["phi"], p["q"], p["x0"], p["P0"])
    assert int(r["status"].abs().sum().item()) == 0
    got = {k: _np(r[k]) for k in OUT}
    _check(p, got, instances=range(6) if N + K <= 21 else (0, 4))
    # the invariant: sigma_t = sum_j v^2 / f, detf_t = sum_j log f (compressed indexing).  The filter may be another kernel
    # (another order of the same sums), so v and f agree with ITS v and f within the bars above, 1e-12 big on v and 1e-12 relative
    # on f; propagated through v^2 / f and log f that is the bound used here.
    fl = kf.filter(p["phi"], p["q"], warmup=0, x0=p["x0"], P0=p["P0"], outputs=())
    sig, det, sc = _np(fl["sigmas"]), _np(fl["detfs"]), _np(fl["sigmacount"])
    for b in range(6):
        y = p["obs"][b % 3]
        big = max(1.0, np.nanmax(np.abs(y))) if np.isfinite(y).any() else 1.0
        v, f = got["v"][b], got["f"][b]
        steps = [t for t in range(T) if np.isfinite(v[t]).any()]
        assert len(steps) == sc[b]
        for i, t in enumerate(steps):
            js = np.isfinite(v[t])
            s = np.sum(v[t, js] ** 2 / f[t, js])
            tol = np.sum(2 * np.abs(v[t, js]) * 1e-12 * big / f[t, js] + 2e-12 * v[t, js] ** 2 / f[t, js]) + 4e-16 * N * s
            assert abs(s - sig[b, i]) <= tol, (b, t, s, sig[b, i])
            assert abs(np.sum(np.log(f[t, js])) - det[b, i]) <= 1e-12 * js.sum() + 1e-13, (b, t)


def test_partial_last_workgroup():
    """B = 5, T = 7: 35 pairs, 16 per workgroup of the 16-lane kernel -- the last workgroup is partial; nothing past the
    arrays is written (guard cells around the outputs keep their value)."""
    import torch

    p = _data(8, 2, 7, 5, 5, seed=5, full=False)
    kf = _engine(p)
    buf = kf.alloc_innovations(5)
    guard = {}
    for k in OUT:   # the output in the middle of a larger allocation
        whole = torch.full((5 * 7 * 8 + 64,), 777.0, dtype=torch.float64, device="cuda")
        guard[k] = whole
        buf[k] = whole[32:32 + 5 * 7 * 8].view(5, 7, 8)
    r = kf.innovations(p["phi"], p["q"], buffers=buf)
    _check(p, {k: _np(r[k]) for k in OUT})
    for k in OUT:
        g = _np(guard[k])
        assert (g[:32] == 777.0).all() and (g[-32:] == 777.0).all(), k


@pytest.mark.parametrize("shape", [(8, 2), (19, 2)], ids=["8x2", "19x2"])
@pytest.mark.parametrize("time_major", [0, 1])
@pytest.mark.parametrize("obs_time_major", [0, 1])
def test_layouts_crossed(shape, time_major, obs_time_major):
    """The C ABI itself: the outputs' and the work buffer's layout (time_major) crossed with the observations' (obs_time_major)."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem

    N, K = shape
    B, R, T = 6, 3, 9
    p = _data(N, K, T, R, B, seed=N + 7, full=True)
    kf = _engine(p)   # holds the context and ensures the shape's kernels
    L = _lib.lib()
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    obs = dev(p["obs"].transpose(1, 0, 2) if obs_time_major else p["obs"])
    t = {k: dev(p[k]) for k in ("phi", "q", "loadings", "obsvar", "x0", "P0", "scale", "offset")}
    prob = Problem(B, R, T, N, K, 0, ptr(obs), ptr(t["phi"]), ptr(t["q"]), ptr(t["loadings"]), ptr(t["obsvar"]), ptr(t["x0"]),
                   ptr(t["P0"]), obs_time_major, ptr(t["scale"]), ptr(t["offset"]))
    ws = int(L.mk_innovations_work_stride(N, K))
    assert ws == int(L.mk_record_stride(N + K))
    work = torch.empty(B * T * ws, dtype=torch.float64, device="cuda")
    outs = {k: torch.empty((T, B, N) if time_major else (B, T, N), dtype=torch.float64, device="cuda") for k in OUT}
    status = torch.ones(B, dtype=torch.int32, device="cuda")
    kf._bind_stream()
    rc = L.mk_innovations(kf._ctx, ctypes.byref(prob), ptr(work), time_major, ptr(outs["v"]), ptr(outs["f"]), ptr(outs["pred_mean"]),
                          ptr(outs["pred_var"]), ptr(status))
    assert rc == 0, L.mk_last_error()
    torch.cuda.synchronize()
    assert int(status.abs().sum().item()) == 0
    _check(p, {k: _np(outs[k].transpose(0, 1) if time_major else outs[k]) for k in OUT})


def test_engine_time_major_and_generic_family():
    """The engine's time-major layout, and the size-generic kernel family's recording pass (row-major records: the transpose of
    the specialised kernels' image)."""
    p = _data(8, 2, 17, 3, 6, seed=31, full=True)
    kf = _engine(p, "time_major")
    r = kf.innovations(p["phi"], p["q"], p["x0"], p["P0"])
    _check(p, {k: _np(r[k]) for k in OUT})
    kg = _engine(p)
    kg.set_variant("kernel_family", "generic")
    assert kg.innovations_supported
    rg = kg.innovations(p["phi"], p["q"], p["x0"], p["P0"])
    _check(p, {k: _np(rg[k]) for k in OUT})


def test_null_outputs():
    """Each output left out in turn, and the forecast alone (no updates run): what is written is bit-identical to the full call."""
    p = _data(13, 4, 9, 3, 6, seed=77, full=True)
    kf = _engine(p)
    full = {k: _np(t) for k, t in kf.innovations(p["phi"], p["q"], p["x0"], p["P0"]).items() if k in OUT}
    for outputs in [tuple(k for k in OUT if k != drop) for drop in OUT] + [("pred_mean", "pred_var"), ("v",), ("pred_var",)]:
        r = kf.innovations(p["phi"], p["q"], p["x0"], p["P0"], outputs=outputs)
        assert set(r) == set(outputs) | {"_work", "status"}
        for k in outputs:
            assert np.array_equal(_np(r[k]), full[k], equal_nan=True), (outputs, k)


def test_invalid_model_shares_a_wavefront():
    """One instance with a negative observation variance among valid ones (16-lane groups: four pairs per wavefront): its status
    bit is set and its rows are NaN; the neighbours' outputs are bit-identical to the call without it."""
    from metran_amd.engine import FLAG_NONPOSITIVE_F

    p = _data(8, 2, 9, 8, 8, seed=3, full=True)
    good = {k: _np(t) for k, t in _engine(p).innovations(p["phi"], p["q"], p["x0"], p["P0"]).items() if k in OUT}
    bad = dict(p)
    bad["obsvar"] = p["obsvar"].copy()
    bad["obsvar"][2] = -5.0
    r = _engine(bad).innovations(p["phi"], p["q"], p["x0"], p["P0"])
    status = _np(r["status"])
    assert status[2] & FLAG_NONPOSITIVE_F and not np.delete(status, 2).any()
    for k in OUT:
        g = _np(r[k])
        assert np.isnan(g[2]).all(), k
        assert np.array_equal(np.delete(g, 2, axis=0), np.delete(good[k], 2, axis=0), equal_nan=True), k


def test_hard_models():
    """The property sweep's hard models (persistence up to 1 - 1e-9, communality up to 0.999, R > 0, x0 / P0, sparse and empty
    steps) within tests/hard_models.py's own conditioning-aware bar on the moments."""
    from metran_amd.engine import BatchedKalman

    for (N, K, T, B), g in hard_models.groups(per_shape=16, shapes=[(8, 2), (32, 4)]):
        kf = BatchedKalman(0)
        kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
        r = kf.innovations(g["phi"], g["q"], g["x0"], g["P0"])
        assert int(r["status"].abs().sum().item()) == 0
        got = {k: _np(r[k]) for k in OUT}
        for b in range(0, B, 3):
            ref = hard_models.oracle_model(oracle, g, b, smooth=False)
            _, tol = hard_models.filter_tolerances(g, b, ref)
            want = innov_ref.innovations(g["obs"][b], g["phi"][b], g["q"][b], g["loadings"][b],
                                         None if g["obsvar"] is None else g["obsvar"][b], None if g["x0"] is None else g["x0"][b],
                                         None if g["P0"] is None else g["P0"][b])
            seen = np.isfinite(g["obs"][b])
            what = str((N, K, T, b, g["patterns"][b]))
            for k in OUT:
                gk, wk = got[k][b], want[k].astype(np.float64)
                if k in ("v", "f"):
                    assert np.array_equal(np.isnan(gk), ~seen), what
                    gk, wk = gk[seen], wk[seen]
                np.testing.assert_allclose(gk, wk, rtol=0, atol=tol, err_msg=k + " " + what)


def test_refusals():
    """An unserved shape, a missing work buffer, no output at all, a work buffer that is too small: refused before any launch."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem

    d = make_dfm_batch(2, 8, 2, 16, seed=3)
    p = dict(obs=d["obs"], loadings=d["loadings"], phi=d["phi"], q=d["q"], obsvar=None, x0=None, P0=None, scale=None, offset=None)
    kf = _engine(p)
    L = _lib.lib()
    assert int(L.mk_innovations_work_stride(70, 2)) == 0 and int(L.mk_innovations_work_stride(60, 4)) == int(L.mk_record_stride(64))
    buf = torch.zeros(72 * 72, dtype=torch.float64, device="cuda")
    q = ctypes.c_void_p(buf.data_ptr())
    prob = Problem(1, 1, 4, 70, 2, 0, q, q, q, q, None, None, None, 0, None, None)
    assert L.mk_innovations(kf._ctx, ctypes.byref(prob), q, 0, q, q, q, q, None) == -2 and b"N=70, K=2" in L.mk_last_error()
    prob, keep, B = kf._problem(kf._dev(d["phi"]), kf._dev(d["q"]), 0, None, None)
    out = torch.empty((2, 16, 8), dtype=torch.float64, device="cuda")
    o = ctypes.c_void_p(out.data_ptr())
    work = kf.alloc_innovations(2)["_work"]
    w = ctypes.c_void_p(work.data_ptr())
    assert L.mk_innovations(kf._ctx, ctypes.byref(prob), None, 0, o, o, o, o, None) == -1 and b"d_work" in L.mk_last_error()
    assert L.mk_innovations(kf._ctx, ctypes.byref(prob), w, 0, None, None, None, None, None) == -1
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0   # an allocation of its own: its size is known exactly
    try:
        assert L.mk_innovations(kf._ctx, ctypes.byref(prob), small, 0, o, o, o, o, None) == -1 and b"d_work" in L.mk_last_error()
        assert L.mk_innovations(kf._ctx, ctypes.byref(prob), w, 0, small, o, o, o, None) == -1 and b"d_v" in L.mk_last_error()
        assert L.mk_innovation_stats(kf._ctx, 2, 16, 8, 0, 0, 4, o, o, small) == -1 and b"d_stats" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    assert L.mk_innovation_stats(kf._ctx, 2, 16, 8, 0, 0, 33, o, o, o) == -1
    assert L.mk_innovation_stats(kf._ctx, 2, 16, 8, 0, -1, 4, o, o, o) == -1
    with pytest.raises(ValueError):
        kf.innovation_stats(out, out, nlags=0)


# ------------------------------------------------------------------------------------------------------------ statistics
TILE = 64   # innov_stats_kernel's time tile (held to the source by tests/test_innovations_host.py)


@functools.lru_cache(maxsize=None)
def _stats_engine(layout="model_major"):
    from metran_amd.engine import BatchedKalman

    return BatchedKalman(0, layout=layout)


def _stats(v, f, L, t_first, layout="model_major"):
    kf = _stats_engine(layout)
    tv, tf = kf._layout(kf._dev(v)), kf._layout(kf._dev(f))
    return _np(kf.innovation_stats(tv, tf, nlags=L, t_first=t_first))


def _check_stats(got, v, f, L, t_first):
    """1e-10 relative, the count exact, NaN where the restatement has NaN."""
    for b in range(v.shape[0]):
        want = innov_ref.stats(v[b], f[b], L, t_first).astype(np.float64)
        assert np.array_equal(got[b][:, 0], want[:, 0]), b
        assert np.array_equal(np.isnan(got[b]), np.isnan(want)), b
        ok = np.isfinite(want)
        np.testing.assert_allclose(got[b][ok], want[ok], rtol=1e-10, atol=0, err_msg="instance %d" % b)


def _cells(B, T, N, seed, missing=0.3):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(B, T, N))
    f = rng.uniform(0.5, 2.0, (B, T, N))
    v[rng.random((B, T, N)) < missing] = np.nan
    return v, f


@pytest.mark.parametrize("T", [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
@pytest.mark.parametrize("L", [1, 32])
def test_stats_lengths_lags_offsets(T, L):
    v, f = _cells(4, T, 3, seed=T + L)
    for t_first in (0, 1, T):
        _check_stats(_stats(v, f, L, t_first), v, f, L, t_first)
    _check_stats(_stats(v, f, L, 1, "time_major"), v, f, L, 1)


@pytest.mark.parametrize("L", [1, 32])
def test_stats_cell_counts(L):
    """m = 0, 1, L, L + 1, L + 2 valid cells, scattered over more than two tiles."""
    T = 2 * TILE + 1
    ms = [0, 1, L, L + 1, L + 2]
    rng = np.random.default_rng(L)
    v = np.full((1, T, len(ms)), np.nan)
    for j, m in enumerate(ms):
        v[0, np.sort(rng.choice(T, size=m, replace=False)), j] = rng.normal(size=m)
    f = np.ones_like(v)
    got = _stats(v, f, L, 0)
    assert list(got[0][:, 0]) == ms
    assert np.isnan(got[0][:3, 3:]).all() and np.isfinite(got[0][3:]).all()
    _check_stats(got, v, f, L, 0)


def test_stats_special_inputs():
    T = TILE + 9
    for N in (1, 33):
        v, f = _cells(2, T, N, seed=N)
        v[0, :, 0] = 0.5
        f[0, :, 0] = 0.25                 # a constant series: e = 1 exactly, c_0 = 0
        f[1, ::5, 0] = np.nan             # cells without a variance are skipped
        f[1, 1::7, 0] = -1.0              # ... and cells with a non-positive one
        got = _stats(v, f, 5, 0)
        assert got[0, 0, 0] == T and got[0, 0, 1] == 1.0 and got[0, 0, 2] == 0.0 and np.isnan(got[0, 0, 3:]).all()
        _check_stats(got, v, f, 5, 0)
    # the alternating series of even length m, with gaps: r_1 = -(m - 1) / m
    m = 40
    v = np.full((1, 3 * m, 1), np.nan)
    v[0, ::3, 0] = [(-1.0) ** i for i in range(m)]
    got = _stats(v, np.ones_like(v), 2, 0)
    assert got[0, 0, 0] == m and got[0, 0, 1] == 0.0 and got[0, 0, 2] == 1.0 and abs(got[0, 0, 4] + (m - 1) / m) <= 1e-15


def test_stats_do_not_depend_on_the_batch():
    """The same model at batch positions 0 and B - 1, and alone: bit-identical statistics."""
    v, f = _cells(7, 2 * TILE + 1, 5, seed=9)
    v[6], f[6] = v[0], f[0]
    for layout in ("model_major", "time_major"):
        got = _stats(v, f, 10, 1, layout)
        alone = _stats(v[:1], f[:1], 10, 1, layout)
        assert np.array_equal(got[0], got[6], equal_nan=True) and np.array_equal(got[0], alone[0], equal_nan=True)


# ---------------------------------------------------------------------------------------------------------------- facade
def test_metran_batch_facade(g1):
    """get_innovations, get_prediction and test_whiteness of two models of different lengths (the g1 records, cut short)
    against the restatement fed the same standardised records and parameters."""
    import pandas as pd
    from scipy.stats import chi2, norm

    from metran_amd.batch import MetranBatch

    idx = pd.DatetimeIndex(g1["index_ns"].astype("datetime64[ns]"))
    raw = g1["obs"] * g1["oseries_std"] + g1["oseries_mean"]
    series = [pd.Series(raw[:, j], index=idx, name="B21B021400%d" % (j + 1)).dropna() for j in range(raw.shape[1])]
    mb = MetranBatch([[s.iloc[: len(s) // 2] for s in series], [s.iloc[: len(s) // 3] for s in series]], factors=g1["loadings"])
    astar = np.stack([g1["alpha_star"], g1["alpha_star"] * 1.1])
    phi, q = (_np(t) for t in mb.kf.params_from_alpha(mb._alpha(astar), dt=mb.dt))
    obs, std, mean = _np(mb.kf.obs), _np(mb._std), _np(mb._mean)
    ref = [innov_ref.innovations(obs[r], phi[r], q[r], g1["loadings"], None, None, None, std[r], mean[r]) for r in range(2)]
    e = _np(mb.get_innovations(astar))
    v, f = (_np(t) for t in mb.get_innovations(astar, standardized=False))
    nlags = 10
    white = mb.test_whiteness(astar, nlags=nlags)
    assert list(white.columns) == ["nobs", "mean", "var", "Q", "pvalue"] + ["r%d" % l for l in range(1, nlags + 1)]
    assert white.index.names == ["model", "series"] and len(white) == 2 * mb.N
    for r in range(2):
        seen = np.isfinite(obs[r])
        big = max(1.0, np.nanmax(np.abs(obs[r])))
        assert np.array_equal(np.isnan(e[r]), ~seen)
        wv, wf = ref[r]["v"].astype(np.float64), ref[r]["f"].astype(np.float64)
        np.testing.assert_allclose(v[r][seen], wv[seen], rtol=0, atol=1e-12 * big)
        np.testing.assert_allclose(f[r][seen], wf[seen], rtol=1e-12, atol=0)
        we = (wv / np.sqrt(wf))[seen]   # the bars on v and f carried through v / sqrt(f)
        assert (np.abs(e[r][seen] - we) <= 1e-12 * big / np.sqrt(wf[seen]) + 1e-12 * np.abs(we)).all()
        want = innov_ref.stats(ref[r]["v"], ref[r]["f"], nlags, 1).astype(np.float64)
        rows = white.loc[r]
        assert list(rows.index) == list(mb.batch.names[r]) and list(rows["nobs"]) == list(want[:, 0])
        got = rows[["mean", "var", "Q"] + ["r%d" % l for l in range(1, nlags + 1)]].values
        assert np.array_equal(np.isnan(got), np.isnan(want[:, 1:]))
        ok = np.isfinite(want[:, 1:])
        np.testing.assert_allclose(got[ok], want[:, 1:][ok], rtol=1e-10, atol=0)
        okq = np.isfinite(want[:, 3])
        np.testing.assert_allclose(rows["pvalue"].values[okq], chi2.sf(want[okq, 3], nlags), rtol=1e-8, atol=1e-300)
        # the one-step-ahead forecast of one series: mean and band in original units, defined at every step
        name = mb.batch.names[r][4 - r]
        j = mb._series(r, name)
        frame = mb.get_prediction(r, name, alpha=astar)
        Lr = int(mb.batch.lengths[r])
        assert list(frame.columns) == ["mean", "lower", "upper"] and frame.shape[0] == Lr
        pm, pv = ref[r]["pred_mean"].astype(np.float64)[:Lr, j], ref[r]["pred_var"].astype(np.float64)[:Lr, j]
        bigm = max(1.0, np.abs(pm).max())
        np.testing.assert_allclose(frame["mean"].values, pm, rtol=0, atol=1e-12 * bigm)
        iv = norm.ppf(0.975) * np.sqrt(pv)
        np.testing.assert_allclose(frame["upper"].values - frame["lower"].values, 2 * iv, rtol=1e-11, atol=0)
        std_frame = mb.get_prediction(r, name, alpha=astar, standardized=True, ci=None)
        np.testing.assert_allclose(std_frame.values, (pm - mean[r, j]) / std[r, j], rtol=0, atol=1e-12 * bigm / std[r, j])
    assert "innov" in mb._cache
