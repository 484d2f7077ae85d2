"""Multi-step-ahead forecasts and the forecast skill by horizon on the GPU (C ABI mk_forecast: the recording forward pass +
forecast_path_kernel / forecast_skill_kernel) against the extended-precision numpy restatement (tests/forecast_ref.py, pinned
to the oracle by tests/test_forecast_host.py), against the existing kernels without any new reference, bit for bit across
batches and subsets of outputs, under both kernel families, next to an invalid model, the refusals of the raw ABI, and end to
end through MetranBatch.

Bars (derived in tests/test_forecast_host.py): atol 1e-12 max(1, max |y|) on a mean (in the units of the output), rtol 1e-12 on a
variance, ``forecast_ref.sum_bars`` -- those two carried through e^2, e^2 / s and log s over the pairs -- on the sums; the pair
count and the hits exact (no pair of the inputs sits within 1e-6 z^2 of the threshold: asserted on the reference)."""
import ctypes

import numpy as np
import pytest

import forecast_ref
from metran_amd.synthetic import make_dfm_batch
from shape_matrix import MATRIX

pytestmark = pytest.mark.gpu

CHUNK = 32   # kForecastChunk (held to the source by tests/test_forecast_host.py)
N64 = [s for s in MATRIX if s[0] + s[1] == 64][0]
# lane groups of 8 (N <= 8), 16 (N <= 16), 32 (N <= 32) and 64 lanes, each width from both sides: N = 8 | 9, 16 | 17, 32 | 33
SHAPES = [(2, 1), (8, 2), (9, 2), (12, 4), (13, 4), (16, 2), (17, 3), (32, 4), (33, 4), N64]
LENGTHS = [1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 1]
ATOL_MEAN, RTOL_VAR = 1e-12, 1e-12
FAN, TRACK = ("fan_mean", "fan_var"), ("track_mean", "track_var")
ALL = ("fan", "track", "skill")


def _np(t):
    return t.detach().cpu().numpy()


def _z(coverage):
    from scipy.stats import norm

    return float(norm.ppf(0.5 + 0.5 * coverage))


def _data(N, K, T, R, B, seed, full):
    """Records [R,T,N] with an empty first step (record 0), an empty run, a step with one series, a full one and a series
    that is never observed (the last of record 1); ``full``: observation variances, initial moments and scaling given."""
    d = make_dfm_batch(B, N, K, T, seed=seed, missing=0.3)
    obs = d["obs"][:R].copy()
    obs[0, 0] = np.nan
    if T > 8:
        obs[:, 3:5] = np.nan
        obs[1 % R, 6, 1:] = np.nan
        obs[1 % R, 6, 0] = 0.25
        obs[2 % R, 7] = np.where(np.isfinite(obs[2 % R, 7]), obs[2 % R, 7], -0.5)
    obs[1 % R, :, N - 1] = np.nan
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


def _engine(p, layout="model_major", family="specialised"):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(p["obs"]).set_loadings(p["loadings"], p["obsvar"]).set_scaling(p["scale"], p["offset"])
    if family != "specialised":
        kf.set_variant("kernel_family", family)
    return kf


def _pick(a, i):
    return None if a is None else a[i]


def _table(p, b, hmax):
    r = b % p["obs"].shape[0]
    return forecast_ref.table(p["obs"][r], p["phi"][b], p["q"][b], p["loadings"][r], _pick(p["obsvar"], r), _pick(p["x0"], b),
                              _pick(p["P0"], b), hmax)


def _ref(p, b, tab, H, origin, th, t_first, z):
    r = b % p["obs"].shape[0]
    return forecast_ref.forecast(p["obs"][r], p["phi"][b], p["q"][b], p["loadings"][r], _pick(p["obsvar"], r), _pick(p["x0"], b),
                                 _pick(p["P0"], b), _pick(p["scale"], r), _pick(p["offset"], r), horizon=H, origin=origin,
                                 track_horizon=th, t_first=t_first, z=z, tab=tab)


def _check(p, got, b, ref, t_first, z, what):
    """One instance's outputs against the restatement, at the bars of the module docstring."""
    R = p["obs"].shape[0]
    y = p["obs"][b % R]
    seen = np.isfinite(y)
    big = max(1.0, np.nanmax(np.abs(y))) if seen.any() else 1.0
    sc = 1.0 if p["scale"] is None else p["scale"][b % R]
    of = 0.0 if p["offset"] is None else p["offset"][b % R]
    bigo = max(1.0, np.nanmax(np.abs(y * sc + of))) if seen.any() else 1.0
    for k in FAN + TRACK:
        if k in got:
            w = ref[k].astype(np.float64)
            if k.endswith("mean"):
                np.testing.assert_allclose(got[k][b], w, rtol=0, atol=ATOL_MEAN * max(bigo, np.abs(w).max()), err_msg="%s of instance %d, %s" % (k, b, what))
            else:
                np.testing.assert_allclose(got[k][b], w, rtol=RTOL_VAR, atol=0, err_msg="%s of instance %d, %s" % (k, b, what))
    if "skill" in got:
        H = got["skill"].shape[2]
        ratio = ref["ratio"][np.isfinite(ref["ratio"])].astype(np.float64)
        assert ratio.size == 0 or np.min(np.abs(ratio - z * z)) >= 1e-6 * z * z, "a pair sits on the coverage threshold: another seed"
        bars = forecast_ref.sum_bars(y, ref["M"], ref["S"], H, t_first, ATOL_MEAN * big, RTOL_VAR)
        g, w = got["skill"][b], ref["skill"].astype(np.float64)
        assert np.array_equal(g[:, :, 0], w[:, :, 0]) and np.array_equal(g[:, :, 5], w[:, :, 5]), (b, what)
        assert (np.abs(g - w) <= bars).all(), (b, what, float(np.max(np.abs(g - w) - bars)))
        assert (g[w[:, :, 0] == 0] == 0).all(), (b, what)   # no pairs: six exact zeros
        if b % R == 1 % R:
            assert (g[y.shape[1] - 1] == 0).all()           # the never-observed series


def _origins(kind, T, R):
    return {"last": None, "initial": [-1] * R, "first": [0] * R, "differ": [(T - 1 - r) if T - 1 - r >= -1 else -1 for r in range(R)]}[kind]


# per length: (H, t_first, fan origins, track_horizon, layout, full) -- every H in {1, 2, 9, 32} and H >= T, every t_first in
# {0, 1, T - 1, T}, every kind of origin, track horizons 1, 2 and T (T = 1, 2, CHUNK - 1), both layouts, with and without R / x0 / P0 / scaling
PLAN = {1: (2, 0, "initial", 1, "model_major", False),
        2: (32, 1, "first", 2, "time_major", True),
        CHUNK - 1: (9, CHUNK - 2, "differ", CHUNK - 1, "model_major", True),
        CHUNK: (1, CHUNK, "last", 1, "time_major", False),
        CHUNK + 1: (32, 1, "differ", 2, "model_major", True),
        2 * CHUNK + 1: (9, 0, "last", 2, "time_major", True)}


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("shape", SHAPES, ids=["%dx%d" % s for s in SHAPES])
def test_against_restatement(shape, T):
    """B = 6 instances on R = 3 records, all three outputs in one call; the wide shapes are compared on two instances, the
    widest on one (the restatement's extended-precision loops are what takes the time) and at H = 9 where the plan says 32 and T > 2."""
    N, K = shape
    H, t_first, okind, th, layout, full = PLAN[T]
    wide = N + K > 17
    if wide and H == 32 and T > 2:
        H = 9
    p = _data(N, K, T, 3, 6, seed=1000 * N + 10 * K + T, full=full)
    kf = _engine(p, layout)
    assert kf.forecast_supported
    origins = _origins(okind, T, 3)
    r = kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], horizon=H, outputs=ALL, origins=origins, track_horizon=th, t_first=t_first,
                    coverage=0.9)
    assert int(r["status"].abs().sum().item()) == 0
    got = {k: _np(r[k]) for k in FAN + TRACK + ("skill",)}
    assert got["fan_mean"].shape == (6, H, N) and got["track_var"].shape == (6, T, N) and got["skill"].shape == (6, N, H, 6)
    z = _z(0.9)
    for b in ((4,) if N + K == 64 else (1, 5) if wide else range(6)):
        ref = _ref(p, b, _table(p, b, max(H, th)), H, None if origins is None else origins[b % 3], th, t_first, z)
        _check(p, got, b, ref, t_first, z, "T=%d" % T)


def test_horizons_and_first_origins_crossed():
    """(8, 2) at T = CHUNK + 1: H in {1, 2, 9, 32} x t_first in {0, 1, T - 1, T}, the skill alone, one table of the restatement."""
    T = CHUNK + 1
    p = _data(8, 2, T, 3, 6, seed=77, full=True)
    kf = _engine(p)
    tabs = {b: _table(p, b, 32) for b in (0, 4)}
    z = _z(0.95)
    for H in (1, 2, 9, 32):
        for t_first in (0, 1, T - 1, T):
            r = kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], horizon=H, outputs=("skill",), t_first=t_first)
            got = {"skill": _np(r["skill"])}
            for b in (0, 4):
                _check(p, got, b, _ref(p, b, tabs[b], H, None, 1, t_first, z), t_first, z, "H=%d t_first=%d" % (H, t_first))


@pytest.mark.parametrize("shape", [(32, 4), (33, 4), N64], ids=["32x4", "33x4", "n64"])
def test_every_horizon_block_of_the_wide_groups(shape):
    """The 32- and 64-lane instantiations at H = 32 with pairs at every horizon (T = CHUNK + 3: two chunks, all four blocks of
    eight horizons), the skill alone, one instance against the restatement."""
    N, K = shape
    T, H, t_first = CHUNK + 3, 32, 1
    p = _data(N, K, T, 3, 6, seed=9 * N + K, full=True)
    r = _engine(p).forecast(p["phi"], p["q"], p["x0"], p["P0"], horizon=H, outputs=("skill",), t_first=t_first)
    assert int(r["status"].abs().sum().item()) == 0
    got = {"skill": _np(r["skill"])}
    assert (got["skill"][4, 0, :, 0] > 0).all()   # a pair at every horizon
    z = _z(0.95)
    _check(p, got, 4, _ref(p, 4, _table(p, 4, H), H, None, 1, t_first, z), t_first, z, "H=32")


def test_partial_last_workgroup_and_guards():
    """B = 5, T = 7: the last workgroup of either kernel is partial; nothing past the arrays is written."""
    import torch

    p = _data(8, 2, 7, 5, 5, seed=5, full=False)
    kf = _engine(p)
    buf = kf.alloc_forecast(5, 3, ALL)
    guard = {}
    for k in FAN + TRACK + ("skill",):
        size = buf[k].numel()
        whole = torch.full((size + 64,), 777.0, dtype=torch.float64, device="cuda")
        guard[k] = whole
        buf[k] = whole[32:32 + size].view(buf[k].shape)
    r = kf.forecast(p["phi"], p["q"], horizon=3, outputs=ALL, track_horizon=2, t_first=0, buffers=buf)
    got = {k: _np(r[k]) for k in FAN + TRACK + ("skill",)}
    z = _z(0.95)
    for b in range(5):
        _check(p, got, b, _ref(p, b, _table(p, b, 3), 3, None, 2, 0, z), 0, z, "guards")
    for k, g in guard.items():
        g = _np(g)
        assert (g[:32] == 777.0).all() and (g[-32:] == 777.0).all(), k


# ------------------------------------------------------------------------------------- against the existing kernels
def test_track_of_horizon_one_is_the_innovations_forecast():
    """The same multiply-adds in the same order: bit for bit, under either layout and kernel family."""
    for shape, layout, family in (((8, 2), "model_major", "specialised"), ((13, 4), "time_major", "specialised"),
                                  ((33, 4), "model_major", "specialised"), ((8, 2), "model_major", "generic")):
        p = _data(shape[0], shape[1], CHUNK + 1, 3, 6, seed=sum(shape), full=True)
        kf = _engine(p, layout, family)
        i = kf.innovations(p["phi"], p["q"], p["x0"], p["P0"], outputs=("pred_mean", "pred_var"))
        want = (_np(i["pred_mean"]).copy(), _np(i["pred_var"]).copy())
        r = kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], outputs=("track",), track_horizon=1)
        assert np.array_equal(_np(r["track_mean"]), want[0]) and np.array_equal(_np(r["track_var"]), want[1]), (shape, layout, family)


def test_fan_is_the_filters_prediction_on_the_truncated_record():
    """The fan from origin o against mk_filter's predicted moments of steps o + 1 .. o + H on the record whose steps after o are
    missing, through mk_simulate's projection (+ the observation variance).  Each side is held to the bars above against the same
    truth, so they differ by at most twice the bars."""
    N, K, T, H, o = 13, 4, 40, 9, 22
    p = _data(N, K, T, 3, 6, seed=8, full=True)
    p["scale"] = p["offset"] = None
    fan = _engine(p).forecast(p["phi"], p["q"], p["x0"], p["P0"], horizon=H, outputs=("fan",), origins=[o] * 3)
    cut = dict(p, obs=p["obs"].copy())
    cut["obs"][:, o + 1:] = np.nan
    kt = _engine(cut)
    f = kt.filter(p["phi"], p["q"], warmup=0, x0=p["x0"], P0=p["P0"], outputs=("Xp", "Pp"))
    Z = np.concatenate([np.broadcast_to(np.eye(N), (3, N, N)), p["loadings"]], axis=2)
    sm, sv = kt.simulate(Z, f["Xp"], f["Pp"])
    sm, sv = _np(sm)[:, o + 1:o + 1 + H], _np(sv)[:, o + 1:o + 1 + H] + p["obsvar"][np.arange(6) % 3][:, None, :]
    big = max(1.0, np.nanmax(np.abs(p["obs"])))
    np.testing.assert_allclose(_np(fan["fan_mean"]), sm, rtol=0, atol=2 * ATOL_MEAN * big)
    np.testing.assert_allclose(_np(fan["fan_var"]), sv, rtol=2 * RTOL_VAR, atol=0)


def test_skill_sums_are_the_sums_of_the_tracks():
    """The reduction against the per-cell path: H track calls give (m, s) of every pair -- the skill kernel's own numbers -- and the
    sums are formed on the host.  Only the order of the additions and the logarithm differ: mu terms added in float64 on either
    side are within (mu - 1) eps sum |term| of the exact sum each -- the bar is 2 (mu + 4) eps sum |term|; count and hits are
    exact.  sum log s: the kernel forms log(product of the mantissas) + ln 2 (sum of the exponents) per chunk -- every factor
    costs eps / 2 relative on the product, that is eps / 2 ABSOLUTE on its logarithm, and the two parts it adds are each at most
    sum |log s| + 0.7 mu large -- so its bar is 2 (mu + 4) eps (sum |log s| + mu)."""
    N, K, T, H, t_first = 8, 2, 2 * CHUNK + 1, 9, 1
    p = _data(N, K, T, 3, 6, seed=12, full=True)
    p["scale"] = p["offset"] = None
    kf = _engine(p)
    z = _z(0.95)
    got = _np(kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], horizon=H, outputs=("skill",), t_first=t_first)["skill"])
    eps = np.finfo(float).eps
    for h in range(1, H + 1):
        r = kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], outputs=("track",), track_horizon=h)
        m, s = _np(r["track_mean"]), _np(r["track_var"])
        for b in range(6):
            y = p["obs"][b % 3]
            ok = np.isfinite(y) & (np.arange(T) >= t_first + h)[:, None]
            e = np.where(ok, y - m[b], 0.0)
            sb = np.where(ok, s[b], 1.0)
            terms = np.stack([ok * 1.0, e, e * e, e * e / sb, np.log(sb), (ok & (e * e <= z * z * sb)) * 1.0], axis=2)   # [T,N,6]
            want, mag, mu = terms.sum(0), np.abs(terms).sum(0), ok.sum(0)[:, None]
            g = got[b, :, h - 1]
            assert np.array_equal(g[:, (0, 5)], want[:, (0, 5)]), (h, b)
            mag[:, 4] += mu[:, 0]
            assert (np.abs(g - want) <= 2 * (mu + 4) * eps * mag).all(), (h, b)


# ------------------------------------------------------------------------------------------------ batch invariance
def test_outputs_do_not_depend_on_the_batch_or_on_the_subset():
    """Each instance alone (its own record, B = R = 1) equals its rows of the 6-instance call bit for bit; so does a call that
    asks for one output against the call that asks for all three.  T spans three chunks."""
    T, H = 2 * CHUNK + 1, 9
    for shape, layout in (((8, 2), "model_major"), ((33, 4), "time_major")):
        N, K = shape
        p = _data(N, K, T, 3, 6, seed=N, full=True)
        origins = [T - 1, 5, -1]
        kw = dict(horizon=H, track_horizon=3, t_first=1, coverage=0.8)
        keys = FAN + TRACK + ("skill",)
        kf = _engine(p, layout)
        full = {k: _np(t).copy() for k, t in kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], outputs=ALL, origins=origins, **kw).items() if k in keys}
        for out in ALL:
            r = kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], outputs=(out,), origins=origins, **kw)
            for k in keys:
                if k.startswith(out):
                    assert np.array_equal(_np(r[k]), full[k]), (shape, out, k)
        for b in range(6):
            rec = b % 3
            one = dict(p, obs=p["obs"][rec:rec + 1], loadings=p["loadings"][rec:rec + 1], obsvar=p["obsvar"][rec:rec + 1],
                       scale=p["scale"][rec:rec + 1], offset=p["offset"][rec:rec + 1])
            r = _engine(one, layout).forecast(p["phi"][b:b + 1], p["q"][b:b + 1], p["x0"][b:b + 1], p["P0"][b:b + 1], outputs=ALL,
                                              origins=origins[rec:rec + 1], **kw)
            for k in keys:
                assert np.array_equal(_np(r[k])[0], full[k][b]), (shape, b, k)


# ------------------------------------------------------------------------------------------------ both kernel families
@pytest.mark.parametrize("shape", [(8, 2), (33, 4)], ids=["8x2", "33x4"])
def test_generic_family(shape):
    """The size-generic recording pass writes the transpose of the specialised image; the forecast kernels read the same
    positions under either family (the two images agree to rounding) and must meet the same bars."""
    N, K = shape
    T, H, th, t_first = CHUNK + 1, 9, 2, 1
    p = _data(N, K, T, 3, 6, seed=N + K, full=True)
    kf = _engine(p, family="generic")
    assert kf.forecast_supported
    r = kf.forecast(p["phi"], p["q"], p["x0"], p["P0"], horizon=H, outputs=ALL, track_horizon=th, t_first=t_first)
    assert int(r["status"].abs().sum().item()) == 0
    got = {k: _np(r[k]) for k in FAN + TRACK + ("skill",)}
    z = _z(0.95)
    for b in (0, 4):
        _check(p, got, b, _ref(p, b, _table(p, b, H), H, None, th, t_first, z), t_first, z, "generic family")


# ---------------------------------------------------------------------------------------------------------------- status
def test_invalid_model_shares_a_group():
    """tests/status_cases.py's negative observation variance (record 1: instances 1, 4, 7 of 9, eight instances per wavefront of
    the 8-lane kernels): the flag, NaN rows at the engine level, the neighbours bit-identical to the clean twin's."""
    import status_cases as sc

    c = sc.case(8, 2, "neg_once")
    res = {}
    for which in ("bad", "twin"):
        g = c[which]
        kf = _engine(dict(obs=g["obs"], loadings=g["loadings"], obsvar=g["obsvar"], scale=g["scale"], offset=g["offset"]))
        res[which] = kf.forecast(g["phi"], g["q"], g["x0"], g["P0"], horizon=5, outputs=ALL, track_horizon=2, t_first=0)
    sc.check_flags(res["bad"]["status"], c, "filter", "forecast")
    sc.check_twin_flags(res["twin"]["status"], c, "filter", "forecast")
    sc.check_containment(res["bad"], res["twin"], c, "forecast")
    for k in FAN + TRACK + ("skill",):
        g = _np(res["bad"][k])
        for i in c["touched"]:
            assert np.isnan(g[i]).all(), (k, i)
        assert np.isfinite(np.delete(g, list(c["touched"]), axis=0)).all(), k


# -------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_through_the_raw_abi():
    """Every MK_ERR_INVALID / MK_ERR_SHAPE case: refused before any launch -- the prefilled outputs and the status keep their
    values."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import ForecastRequest, Problem

    B, N, K, T, H = 2, 8, 2, 16, 4
    d = make_dfm_batch(B, N, K, T, seed=3)
    p = dict(obs=d["obs"], loadings=d["loadings"], phi=d["phi"], q=d["q"], obsvar=None, x0=None, P0=None, scale=None, offset=None)
    kf = _engine(p)
    L = _lib.lib()
    assert int(L.mk_forecast_max_horizon()) == 32
    assert int(L.mk_forecast_work_stride(70, 2)) == 0 and int(L.mk_forecast_work_stride(61, 4)) == 0
    assert int(L.mk_forecast_work_stride(60, 4)) > int(L.mk_record_stride(64))
    prob, keep, _ = kf._problem(kf._dev(d["phi"]), kf._dev(d["q"]), 0, None, None)
    bufs = kf.alloc_forecast(B, H, ALL)
    outs = [bufs[k] for k in FAN + TRACK + ("skill",)]
    status = torch.full((B,), 99, dtype=torch.int32, device="cuda")
    for t in outs:
        t.fill_(777.0)
    org = torch.tensor([T - 1, 0], dtype=torch.int64, device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()   # noqa: E731

    def request(**kw):
        r = ForecastRequest()
        r.horizon, r.t_first, r.track_horizon, r.coverage_z = H, 1, 2, 1.96
        r.d_fan_origins = ptr(org)
        r.d_fan_means, r.d_fan_vars, r.d_track_means, r.d_track_vars, r.d_skill = (ptr(t) for t in outs)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    def call(req, prob=prob, work=bufs["_work"]):
        kf._bind_stream()
        rc = L.mk_forecast(kf._ctx, ctypes.byref(prob), None if work is None else ctypes.c_void_p(work.data_ptr()), 0,
                           None if req is None else ctypes.byref(req), ctypes.c_void_p(status.data_ptr()))
        torch.cuda.synchronize()
        return rc, L.mk_last_error() or b""

    none = dict(d_fan_means=None, d_fan_vars=None, d_track_means=None, d_track_vars=None, d_skill=None)
    raw = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(raw)) == 0   # an allocation of its own: its size is known exactly

    class small:   # what call() and ptr() ask of a tensor
        data_ptr = staticmethod(lambda: raw.value)

    cases = [("all outputs NULL", request(**none), {}, b"nothing to write"),
             ("no work buffer", request(), dict(work=None), b"d_work"),
             ("horizon 0", request(horizon=0), {}, b"horizon"),
             ("horizon 33", request(horizon=33), {}, b"horizon"),
             ("track_horizon 0", request(track_horizon=0), {}, b"track_horizon"),
             ("track_horizon T + 1", request(track_horizon=T + 1), {}, b"track_horizon"),
             ("t_first -1", request(t_first=-1), {}, b"t_first"),
             ("coverage_z 0", request(coverage_z=0.0), {}, b"coverage_z"),
             ("coverage_z inf", request(coverage_z=float("inf")), {}, b"coverage_z"),
             ("coverage_z nan", request(coverage_z=float("nan")), {}, b"coverage_z"),
             ("origin T", request(d_fan_origins=ptr(torch.tensor([T, 0], dtype=torch.int64, device="cuda"))), {}, b"d_fan_origins"),
             ("origin -2", request(d_fan_origins=ptr(torch.tensor([0, -2], dtype=torch.int64, device="cuda"))), {}, b"d_fan_origins"),
             ("small work", request(), dict(work=small), b"d_work"),
             ("small skill", request(d_skill=ptr(small)), {}, b"d_skill"),
             ("small fan", request(d_fan_vars=ptr(small)), {}, b"d_fan_vars"),
             ("small track", request(d_track_means=ptr(small)), {}, b"d_track_means")]
    bufs["_work"].fill_(777.0)

    def untouched(name):   # no launch: neither the forward pass (work buffer, status) nor a forecast kernel wrote anything
        for t in outs + [bufs["_work"]]:
            assert bool((t == 777.0).all().item()), name
        assert bool((status == 99).all().item()), name

    try:
        for name, req, kw, word in cases:
            rc, msg = call(req, **kw)
            assert rc == -1 and word in msg, (name, rc, msg)
            untouched(name)
    finally:
        L.mk_free(kf._ctx, raw)
    # track_horizon is read only when a track output is set
    rc, msg = call(request(track_horizon=0, d_track_means=None, d_track_vars=None))
    assert rc == 0, msg
    assert not bool((status == 99).any().item()) and not bool((bufs["skill"] == 777.0).any().item())   # ... and that call did run
    for t in outs + [bufs["_work"]]:
        t.fill_(777.0)
    status.fill_(99)
    # MK_ERR_SHAPE: N + K > 64
    big = torch.zeros(72 * 72, dtype=torch.float64, device="cuda")
    q = ctypes.c_void_p(big.data_ptr())
    wide = Problem(1, 1, 4, 61, 4, 0, q, q, q, q, None, None, None, 0, None, None)
    rc, msg = call(request(), prob=wide)
    assert rc == -2 and b"N=61, K=4" in msg
    untouched("N + K > 64")
    # the engine's own argument checks
    for kw in (dict(horizon=0), dict(horizon=33), dict(outputs=()), dict(outputs=("fan", "nope")), dict(outputs=("track",), track_horizon=T + 1),
               dict(t_first=-1), dict(coverage=1.0), dict(origins=[0])):
        with pytest.raises(ValueError):
            kf.forecast(d["phi"], d["q"], **kw)


# ---------------------------------------------------------------------------------------------------------------- facade
def test_metran_batch_facade():
    """get_forecast, get_prediction_at and forecast_skill of two ingested models of different lengths (120 and 100 days, three
    series with gaps) against the restatement fed the same standardised records and parameters."""
    import pandas as pd
    from scipy.stats import norm

    from metran_amd.batch import MetranBatch

    rng = np.random.default_rng(4)
    idx = pd.date_range("2001-01-01", periods=120, freq="D")
    models = []
    for r in range(2):
        cols = []
        for j in range(3):
            s = pd.Series(10.0 * (j + 1) + (2.0 + j) * np.cumsum(rng.normal(size=120)) / 3.0, index=idx, name="s%d" % j)
            cols.append(s[rng.random(120) > 0.3])
        models.append(cols if r == 0 else [c[c.index < idx[100]] for c in cols])
    G = np.broadcast_to(np.array([[0.6], [0.5], [-0.4]]), (2, 3, 1)).copy()
    mb = MetranBatch(models, factors=G)
    assert mb.T <= 150 and int(mb.batch.lengths[1]) < int(mb.batch.lengths[0])
    astar = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    phi, q = (_np(t) for t in mb.kf.params_from_alpha(mb._alpha(astar), dt=mb.dt))
    obs, std, mean = _np(mb.kf.obs), _np(mb._std), _np(mb._mean)
    H, th, z = 7, 3, _z(0.9)
    Ls = [int(v) for v in mb.batch.lengths]
    ref = [forecast_ref.forecast(obs[r], phi[r], q[r], G[r], None, None, None, std[r], mean[r], horizon=H, origin=Ls[r] - 1,
                                 track_horizon=th, t_first=1, z=z) for r in range(2)]
    sk = mb.forecast_skill(horizon=H, alpha=astar, t_first=1, coverage=0.9)
    assert len(sk) == 2 * mb.N * H
    for r in range(2):
        name = mb.batch.names[r][1 + r]
        j = mb._series(r, name)
        bigm = max(1.0, np.nanmax(np.abs(obs[r] * std[r] + mean[r])))
        frame = mb.get_forecast(r, name, steps=H, alpha=astar)
        assert frame.index[0] == mb.batch.index[r][-1] + pd.Timedelta(days=1) and frame.shape == (H, 3)
        fm, fv = ref[r]["fan_mean"].astype(np.float64)[:, j], ref[r]["fan_var"].astype(np.float64)[:, j]
        np.testing.assert_allclose(frame["mean"].values, fm, rtol=0, atol=ATOL_MEAN * bigm)
        np.testing.assert_allclose((frame["upper"] - frame["lower"]).values, 2 * norm.ppf(0.975) * np.sqrt(fv), rtol=1e-11, atol=0)
        tr = mb.get_prediction_at(r, name, th, alpha=astar)
        assert tr.shape[0] == Ls[r] and tr.index.equals(mb.batch.index[r])
        tm, tv = ref[r]["track_mean"].astype(np.float64)[:Ls[r], j], ref[r]["track_var"].astype(np.float64)[:Ls[r], j]
        np.testing.assert_allclose(tr["mean"].values, tm, rtol=0, atol=ATOL_MEAN * bigm)
        np.testing.assert_allclose((tr["upper"] - tr["lower"]).values, 2 * norm.ppf(0.975) * np.sqrt(tv), rtol=1e-11, atol=0)
        # the skill table from the restatement's sums, the bars of the sums carried through the divisions by the count
        big = max(1.0, np.nanmax(np.abs(obs[r])))
        bars = forecast_ref.sum_bars(obs[r], ref[r]["M"], ref[r]["S"], H, 1, ATOL_MEAN * big, RTOL_VAR)
        w = ref[r]["skill"].astype(np.float64)
        for jj, nm in enumerate(mb.batch.names[r]):
            for h in range(1, H + 1):
                row, s, bar = sk.loc[(r, nm, h)], w[jj, h - 1], bars[jj, h - 1]
                m = s[0]
                assert row["nobs"] == m
                if m == 0:
                    continue
                assert abs(row["bias"] - s[1] / m * std[r, jj]) <= bar[1] / m * std[r, jj] * 1.01 + 1e-15
                assert abs(row["rmse"] ** 2 - s[2] / m * std[r, jj] ** 2) <= (bar[2] / m * 1.01 + 4e-16 * s[2] / m) * std[r, jj] ** 2
                assert abs(row["msse"] - s[3] / m) <= bar[3] / m * 1.01 + 4e-16 * s[3] / m
                assert abs(row["logscore"] + 0.5 * (np.log(2 * np.pi) + s[4] / m + s[3] / m)) <= 0.5 * (bar[4] + bar[3]) / m * 1.01 + 1e-14
                assert row["coverage"] == s[5] / m and row["nominal"] == 0.9
    assert "forecast" in mb._cache
