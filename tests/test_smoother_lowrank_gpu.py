"""GPU: the rank-K covariance step of the record smoother (smoother_record_kernel LR) -- taken, per model,
at the steps where the model observed all N series, for n <= 10, full-square records and no observation variances.

Shapes (1,1), (4,1), (8,2), (7,3), and (12,2) where the path does not exist; T = 1, 2, 3, 17; B = 1 (one model), 4 (a full
wavefront), 5 (a partial one with replicated surplus groups); no gap, one missing cell at t = 0 / T-2 / T-1 / two steps in a
row, every second step, one model of the wavefront with gaps (mixed wavefronts), every model with gaps; both layouts, both
record forms, the three entry points.  Every case four ways:

(a) against the oracle at 1e-9;
(b) bit-equal between a model inside a mixed batch and the same model alone (the path is chosen per model);
(c) against the general-only variant of the same build (``set_variant("smoother16", "record_general")``) at
    ``hard_models.smoother_tolerance``;
(d) with ``obsvar`` given as an array of zeros, bit-equal to the general-only variant: the guard is the NULL pointer.

Largest difference measured in (c) on an MI355X: see LARGEST_MEASURED below (printed by the last test of the module)."""
import numpy as np
import pytest

import hard_models as hm
import oracle
from metran_amd.params import observation_matrix
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

SMOOTH_ATOL = 1e-9
SHAPES = [(1, 1), (4, 1), (8, 2), (7, 3), (12, 2)]
PATTERNS = ("none", "cell_first", "cell_penultimate", "cell_last", "two_in_a_row", "every_second", "one_model", "all_models")
LARGEST_MEASURED = 7.8e-16   # (c) over the whole module, MI355X (17 820 full model-steps at n <= 10); the bar is >= 1e-9
_ENGINES, _CASES, _SEEN = {}, {}, {"c": 0.0, "lowrank_steps": 0}


def _np(t):
    return t.detach().cpu().numpy()


def _engine(layout, sym, variant):
    from metran_amd.engine import BatchedKalman

    key = (layout, sym, variant)
    if key not in _ENGINES:
        # "stepwise": a model run alone (one record) goes through the batched filter_kernel too, not the single-record walker,
        # whose filtered moments may differ in the last bit -- (b) compares the same kernels on the same model
        _ENGINES[key] = BatchedKalman(0, layout=layout, packed_sym=sym).set_variant("smoother16", variant).set_variant("single_record", "stepwise")
    return _ENGINES[key]


def _like(got, full):
    if got.ndim == full.ndim:
        return full
    iu = np.triu_indices(full.shape[-1])
    return full[..., iu[0], iu[1]]


def _gaps(obs, pattern, seed):
    """``obs`` [B,T,N] without gaps -> the pattern's gaps, or None where the pattern needs more steps / models than there are."""
    B, T, N = obs.shape
    y = obs.copy()
    rng = np.random.default_rng(seed)
    if pattern == "cell_first":
        y[:, 0, N - 1] = np.nan
    elif pattern == "cell_penultimate":
        if T < 2:
            return None
        y[:, T - 2, 0] = np.nan
    elif pattern == "cell_last":
        y[:, T - 1, 0] = np.nan
    elif pattern == "two_in_a_row":
        if T < 2:
            return None
        y[:, T // 2 - 1:T // 2 + 1, N // 2] = np.nan
    elif pattern == "every_second":
        y[:, ::2, N - 1] = np.nan
    elif pattern == "one_model":
        if B < 2:
            return None
        y[1][rng.random((T, N)) < 0.3] = np.nan
        y[1, T // 2, 0] = np.nan
    elif pattern == "all_models":
        y[rng.random((B, T, N)) < 0.3] = np.nan
        y[np.arange(B), np.arange(B) % T, 0] = np.nan
    return y


def _case(N, K, T, B, pattern):
    """Seeded inputs, the oracle's moments (computed once) and per-model bars of (c)."""
    key = (N, K, T, B, pattern)
    if key not in _CASES:
        d = make_dfm_batch(B, N, K, T, seed=5000 + 100 * N + 10 * K + T, missing=0.0)
        obs = _gaps(d["obs"], pattern, 7 * T + B)
        if obs is None:
            _CASES[key] = None
            return None
        d = dict(d, obs=obs)
        ref = oracle.dfm_batch(d["obs"], d["phi"], d["q"], d["loadings"])
        assert np.isfinite(ref["S"]).all() and np.isfinite(ref["Ps"]).all()
        bars = np.array([hm.smoother_tolerance(d, b, {"Pp": ref["Pp"][b], "F": ref["F"][b]}) for b in range(B)])
        Z = np.concatenate([np.broadcast_to(np.eye(N), (B, N, N)), d["loadings"]], axis=2)
        want = {"S": ref["S"], "Ps": ref["Ps"], "sim_means": np.einsum("bjn,btn->btj", Z, ref["S"]),
                "sim_vars": np.maximum(np.einsum("bjn,btnm,bjm->btj", Z, ref["Ps"], Z), 0.0), "var": np.diagonal(ref["Ps"], axis1=2, axis2=3)}
        for a in list(d.values()) + list(want.values()):
            a.setflags(write=False)
        full = np.isfinite(d["obs"]).all(axis=2)[:, :-1]       # the steps at which a model may take the rank-K form
        _CASES[key] = d, want, bars, int(full.sum())
    return _CASES[key]


ROUTES = (("filter_smooth", ("S", "Ps")), ("simulate_smoothed", ("sim_means", "sim_vars")), ("smooth_state_variances", ("S", "var")))


def _run(kf, d, route, obsvar=None, rows=slice(None)):
    kf.set_observations(np.ascontiguousarray(d["obs"][rows])).set_loadings(np.ascontiguousarray(d["loadings"][rows]),
                                                                           obsvar=None if obsvar is None else obsvar[rows])
    r = getattr(kf, route)(np.ascontiguousarray(d["phi"][rows]), np.ascontiguousarray(d["q"][rows]))
    assert not r.get("_tape")
    out = {k: _np(r[k]) for k in dict(ROUTES)[route]}
    assert not _np(r["status"]).any(), route
    return out


def _four_ways(N, K, T, B, pattern, layout, sym):
    case = _case(N, K, T, B, pattern)
    if case is None:
        return 0
    d, want, bars, nfull = case
    kf, kg = _engine(layout, sym, "record"), _engine(layout, sym, "record_general")
    what = (N, K, T, B, pattern, layout, sym)
    for route, keys in ROUTES:
        got, gen = _run(kf, d, route), _run(kg, d, route)
        zeros = _run(kf, d, route, obsvar=np.zeros((B, N)))
        for k in keys:
            ref = _like(got[k], want[k]) if k == "Ps" else want[k]
            np.testing.assert_allclose(got[k], ref, rtol=0, atol=SMOOTH_ATOL, err_msg="(a) %s %s %s" % (route, k, what))       # (a)
            diff = np.abs(got[k] - gen[k]).reshape(B, -1).max(axis=1)
            _SEEN["c"] = max(_SEEN["c"], float(diff.max()))
            assert (diff <= bars).all(), ("(c)", route, k, what, diff, bars)                                                    # (c)
            np.testing.assert_array_equal(zeros[k], gen[k], err_msg="(d) %s %s %s" % (route, k, what))                         # (d)
        if B > 1 and pattern in ("one_model", "all_models"):                                                                    # (b)
            for i in sorted({0, 1, B - 1}):
                alone = _run(kf, d, route, rows=slice(i, i + 1))
                for k in keys:
                    np.testing.assert_array_equal(got[k][i:i + 1], alone[k], err_msg="(b) %s %s model %d %s" % (route, k, i, what))
    return nfull


@pytest.mark.parametrize("T", [1, 2, 3, 17])
@pytest.mark.parametrize("N,K", SHAPES)
def test_four_ways(N, K, T):
    steps = 0
    for B in (1, 4, 5):
        for pattern in PATTERNS:
            for layout in ("model_major", "time_major"):
                for sym in (False, True):
                    steps += _four_ways(N, K, T, B, pattern, layout, sym)
    assert steps > 0 or T == 1
    if N + K <= 10:
        _SEEN["lowrank_steps"] += steps


@pytest.mark.parametrize("layout", ["model_major", "time_major"])
@pytest.mark.parametrize("N,K", [(8, 2), (4, 1)])
def test_the_rank_k_products_are_what_ran(N, K, layout):
    """The four checks above also hold where the launcher falls back to the parent's kernel.  At shapes that keep their occupancy
    with the step ((8,2): 206 VGPRs for 206, (4,1): 104 for 102) and with every step full, the default MUST have taken it: the two
    forms sum in another order, so Ps differs from the general-only variant's in the last bits -- and S, which the step does not
    touch, only through Ps of later steps (never at T - 2, T - 1)."""
    d, want, bars, nfull = _case(N, K, 17, 4, "none")
    assert nfull == 4 * 16
    got = _run(_engine(layout, False, "record"), d, "filter_smooth")
    gen = _run(_engine(layout, False, "record_general"), d, "filter_smooth")
    diff = np.abs(got["Ps"] - gen["Ps"]).reshape(4, -1).max(axis=1)
    assert (diff > 0.0).all(), diff                      # every model took the other form somewhere ...
    assert (diff <= bars).all(), (diff, bars)            # ... and it is the same quantity
    np.testing.assert_array_equal(got["Ps"][:, -1], gen["Ps"][:, -1])   # the last step is the filtered one in both
    np.testing.assert_array_equal(got["S"], gen["S"])    # J and the mean sweep are untouched


def _singular_reference(d, P0):
    B, T, N = d["obs"].shape
    n = d["phi"].shape[1]
    S, Ps = np.empty((B, T, n)), np.empty((B, T, n, n))
    for b in range(B):
        o, oi, oc = oracle.set_observations(d["obs"][b])
        Phi, Q, Z = np.diag(d["phi"][b]), np.diag(d["q"][b]), observation_matrix(d["loadings"][b])
        f = oracle.seqkalmanfilter(o, Phi, Q, Z, np.zeros(N), oi, oc, np.zeros(n), P0[b])
        S[b], Ps[b] = oracle.kalmansmoother(f[3], f[4], f[5], f[6], Phi)
    return S, Ps


@pytest.mark.parametrize("N,K,r", [(8, 2, 4), (4, 1, 0)])
def test_cold_path_model_among_full_steps(N, K, r):
    """A model whose state r is identically zero (q_r = 0, row and column r of P0 zero: pivot r of every step is exactly 0.0)
    re-factorises its whole wavefront at every step; every step of every model is full, so the redo is followed by the rank-K
    products.  The healthy neighbours must be bit-equal to the same models run without it."""
    from metran_amd.engine import FLAG_RANK_DEFICIENT

    B, at = 7, 2
    d = {k: a.copy() for k, a in make_dfm_batch(B, N, K, 17, seed=5900 + N, missing=0.0).items()}
    P0 = np.tile(np.eye(N + K), (B, 1, 1))
    d["q"][at, r] = 0.0
    P0[at, r, :] = 0.0
    P0[at, :, r] = 0.0
    S, Ps = _singular_reference(d, P0)
    assert np.isfinite(S).all() and np.isfinite(Ps).all()
    others = np.array([b for b in range(B) if b != at])
    for layout in ("model_major", "time_major"):
        kf = _engine(layout, False, "record")
        kf.set_observations(d["obs"]).set_loadings(d["loadings"])
        res = kf.filter_smooth(d["phi"], d["q"], P0=P0)
        st = _np(res["status"])
        assert st[at] == FLAG_RANK_DEFICIENT and not st[others].any(), (layout, st)
        np.testing.assert_allclose(_np(res["S"]), S, rtol=0, atol=SMOOTH_ATOL)
        np.testing.assert_allclose(_np(res["Ps"]), Ps, rtol=0, atol=SMOOTH_ATOL)
        got_S, got_Ps = _np(res["S"])[others], _np(res["Ps"])[others]
        sub = {k: np.ascontiguousarray(a[others]) for k, a in d.items()}
        kf.set_observations(sub["obs"]).set_loadings(sub["loadings"])
        alone = kf.filter_smooth(sub["phi"], sub["q"], P0=np.ascontiguousarray(P0[others]))
        assert not _np(alone["status"]).any()
        np.testing.assert_array_equal(got_S, _np(alone["S"]))
        np.testing.assert_array_equal(got_Ps, _np(alone["Ps"]))


def test_largest_difference_to_the_general_products():
    """Runs last in the module: what (c) measured over every case above."""
    print("largest |default - general-only| over the module: %.3e (recorded: %.1e); full steps walked at n <= 10: %d"
          % (_SEEN["c"], LARGEST_MEASURED, _SEEN["lowrank_steps"]))
    assert _SEEN["c"] <= SMOOTH_ATOL
