"""The residual diagnostics on the GPU (C ABI mk_residual_series: resid_series_kernel; mk_residual_cross: resid_cross_kernel)
against the longdouble restatement at its worst-case bars (tests/resid_ref.py, pinned by tests/test_residuals_host.py): the
kernels' tile, workgroup and lag-block boundaries, both layouts, bit-identity whatever the batch, end to end through MetranBatch
on the filter's own innovations, and the refusals."""
import ctypes
import functools

import numpy as np
import pytest

import innov_ref
import resid_ref as R
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

LAYOUTS = ("model_major", "time_major")
SERIES_CASES = R.check_decisive(R.series_cases())
CROSS_CASES = R.cross_cases()


def _np(t):
    return t.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def _engine(layout="model_major"):
    from metran_amd.engine import BatchedKalman

    return BatchedKalman(0, layout=layout)


def _run(v, f, t_first, layout, nlags=None):
    """(stats [B,N,12], counts, sums) of the two kernels (the cross sums only with ``nlags``)."""
    kf = _engine(layout)
    tv, tf = kf._layout(kf._dev(v)), kf._layout(kf._dev(f))
    stats = kf.residual_series(tv, tf, t_first=t_first)
    if nlags is None:
        return _np(stats), None, None
    counts, sums = kf.residual_cross(tv, tf, stats, nlags=nlags, t_first=t_first)
    return _np(stats), _np(counts), _np(sums)


@pytest.mark.parametrize("case", range(len(SERIES_CASES)), ids=[c[0] for c in SERIES_CASES])
def test_series_kernel_against_restatement(case):
    """Every case at t_first = 0, 1, T, T + 1 (the long records also shortly before and after step 1024) in both layouts: counts and h exact, the sums inside the bars, the steps of the
    excursions exact (every series of every case is decisive: tests/resid_ref.py)."""
    name, v, f = SERIES_CASES[case]
    for t_first in R.t_firsts(v.shape[1]):
        for layout in LAYOUTS:
            got = _run(v, f, t_first, layout)[0]
            assert got.shape == v.shape[:1] + (v.shape[2], 12)
            for b in range(v.shape[0]):
                R.check_series(got[b], v[b], f[b], t_first, (name, b, t_first, layout))


def test_series_special_rows():
    """What the special model's rows hold: the empty series' row, h of the short ones, the constant series' raw sums."""
    v, f = R.special_model()
    got = _run(v, f, 0, "model_major")[0][0]
    assert got[0, 0] == 0 and got[0, 5] == 0 and np.isnan(got[0, [1, 2, 3, 4, 6, 7, 8, 9, 10, 11]]).all()
    assert list(got[1:6, 0]) == [1, 2, 3, 4, 5] and list(got[1:6, 5]) == [0, 1, 1, 1, 2]
    assert got[1, 2] == 0 and got[1, 6] == 0 and got[1, 8] == 0                 # one cell: d = 0, no thirds
    assert got[6, 0] == 130 and got[6, 1] == 1.0 and (got[6, [2, 3, 4, 8, 10]] == 0).all() and got[6, 9] == 0 and got[6, 11] == 0
    assert got[7, 0] == 2 and got[7, 9] >= 128                                   # the last tile's two cells
    ok = R.valid_cells(v[0], f[0], 0)
    assert got[8, 0] == ok[:, 8].sum() < 110


@pytest.mark.parametrize("case", range(len(CROSS_CASES)), ids=[c[0] for c in CROSS_CASES])
def test_cross_kernel_against_restatement(case):
    name, v, f, L = CROSS_CASES[case]
    T = v.shape[1]
    for t_first, layout in ((0, "model_major"), (1, "time_major"), (min(T, 40), "model_major")):
        stats, counts, sums = _run(v, f, t_first, layout, nlags=L)
        assert counts.shape == sums.shape == (v.shape[0], L + 1, v.shape[2], v.shape[2]) and counts.dtype == np.int64
        for b in range(v.shape[0]):
            R.check_series(stats[b], v[b], f[b], t_first, (name, b, t_first, layout))
            R.check_cross(counts[b], sums[b], v[b], f[b], L, t_first, (name, b, t_first, layout))


def test_cross_special_pairs():
    """The even/odd pair never overlaps at lag 0 and does at lag 1; a pair with a dead series has n = 0 and s = NaN; lags beyond
    the record have n = 0 and s = 0."""
    v, f = R.even_odd_model(97, 5, 3)
    _, counts, sums = _run(v, f, 0, "model_major", nlags=3)
    assert counts[0, 0, 0, 1] == 0 == counts[0, 0, 1, 0] and sums[0, 0, 0, 1] == 0.0
    assert counts[0, 1, 0, 1] == 48 and counts[0, 1, 1, 0] == 48 and counts[0, 2, 0, 1] == 0 and counts[0, 2, 0, 0] == 48
    name, v, f, L = [c for c in CROSS_CASES if c[0] == "dead_series"][0]
    _, counts, sums = _run(v, f, 0, "time_major", nlags=L)
    dead = np.zeros((4, 4), dtype=bool)
    dead[2:, :] = dead[:, 2:] = True
    assert (counts[0][:, dead] == 0).all() and np.isnan(sums[0][:, dead]).all() and np.isfinite(sums[0][:, ~dead]).all()
    assert abs(sums[0, 0, 0, 0] - counts[0, 0, 0, 0]) < 1e-9                      # sum of e~^2 = m
    v, f = R._cells(1, 5, 3, 1, 0.0)
    _, counts, sums = _run(v, f, 0, "model_major", nlags=32)
    assert (counts[0, 5:] == 0).all() and (sums[0, 5:] == 0).all() and (counts[0, 4] == 1).all()


@pytest.mark.parametrize("T", [130, 1100])
def test_results_do_not_depend_on_the_batch_or_the_layout(T):
    """One instance alone, at positions 0, 4 and 8 of a batch of nine with other neighbours, and in the other layout:
    bit-identical statistics, counts and sums.  T = 1100: the late model (tests/resid_ref.py), past the steps the series kernel
    keeps in registers."""
    N, L = 5, 10
    v, f = R._cells(9, T, N, seed=21, missing=0.3)
    one_v, one_f = R._cells(1, T, N, seed=22, missing=0.4) if T == 130 else R.late_model(T)
    for p in (0, 4, 8):
        v[p], f[p] = one_v[0], one_f[0]
    alone = _run(one_v, one_f, 1, "model_major", nlags=L)
    assert np.isfinite(alone[0]).all() and np.isfinite(alone[2]).all()
    for layout in LAYOUTS:
        batch = _run(v, f, 1, layout, nlags=L)
        solo = _run(one_v, one_f, 1, layout, nlags=L)
        for k in range(3):
            assert np.array_equal(solo[k][0], alone[k][0], equal_nan=True), (layout, k)
            for p in (0, 4, 8):
                assert np.array_equal(batch[k][p], alone[k][0], equal_nan=True), (layout, k, p)


# ---------------------------------------------------------------------------------------------------------- end to end
def test_metran_batch_end_to_end():
    """Three (5,2) models on 130 days: the three accessors on the filter's own innovations against the frames the restatement
    computes from tests/innov_ref.py's longdouble innovations.  The raw sums at their bar plus what the innovations' own
    tolerance (tests/test_innovations_gpu.py: 1e-12 max(1, max|y|) on v, 1e-12 relative on f) moves them by, first order; the
    statistics and p-values at rtol 1e-6."""
    import pandas as pd

    from metran_amd.batch import MetranBatch

    Rn, N, K, T = 3, 5, 2, 130
    d = make_dfm_batch(Rn, N, K, T, seed=41, missing=0.3)
    idx = pd.date_range("2010-01-01", periods=T, freq="D")
    models = [[pd.Series(10.0 + 2.0 * d["obs"][r, :, j], index=idx, name="w%d" % j).dropna() for j in range(N)] for r in range(Rn)]
    mb = MetranBatch(models, factors=d["loadings"])
    alpha = np.full((Rn, N + K), 12.0) + np.arange(N + K)[None, :]
    _end_to_end(mb, alpha, _np(mb.kf.obs), d["loadings"])


def _end_to_end(mb, alpha, obs, loadings):
    Rn, N = mb.R, mb.N
    phi, q = (_np(t) for t in mb.kf.params_from_alpha(mb._alpha(alpha), dt=mb.dt))
    norm, het, cross = mb.test_normality(alpha), mb.test_heteroskedasticity(alpha), mb.test_cross_correlation(alpha, nlags=3, min_pairs=20)
    stats = _np(mb._residual_stats(alpha, 1)[1])
    counts, sums = mb._residual_cross(alpha, 1, 3)
    for r in range(Rn):
        ref = innov_ref.innovations(obs[r], phi[r], q[r], loadings[r], None, None, None)
        rv, rf = ref["v"], ref["f"]
        T = rv.shape[0]
        want, bars, dec = R.series(rv, rf, 1, detail=True)
        wc, ws, cbars = R.cross(rv, rf, 3, 1, detail=True)
        assert np.array_equal(counts[r], wc)
        big = max(1.0, np.nanmax(np.abs(obs[r])))
        ok = R.valid_cells(rv, rf, 1)
        A, D = np.zeros((T, N), dtype=R.LD), np.zeros((T, N), dtype=R.LD)   # |e~| and how far the tolerances move e~
        for j in range(N):
            o = ok[:, j]
            e = (rv[o, j] / np.sqrt(rf[o, j]))
            de = 1e-12 * big / np.sqrt(rf[o, j]) + 1e-12 * np.abs(e)          # |de_i| from the tolerances on v and f
            dd = de + de.mean()                                               # d_i = e_i - mean
            ad = np.abs(e - want[j, R.MEAN])
            tol = np.zeros(12, dtype=R.LD)
            tol[R.MEAN], tol[R.S2], tol[R.S3], tol[R.S4] = de.mean(), (2 * ad * dd).sum(), (3 * ad ** 2 * dd).sum(), (4 * ad ** 3 * dd).sum()
            tol[R.SS_FIRST] = tol[R.SS_LAST] = (2 * np.abs(e) * de).sum()
            tol[R.CUSUM], tol[R.CUSQ] = dd.sum(), 2 * (2 * ad * dd).sum()
            sd = np.sqrt(want[j, R.S2] / want[j, R.M])
            A[o, j] = ad / sd
            D[o, j] = dd / sd + A[o, j] * tol[R.S2] / (2 * want[j, R.S2])     # e~ = d / sd, sd = sqrt(S2 / m)
            for c in (R.MEAN, R.S2, R.S3, R.S4, R.SS_FIRST, R.SS_LAST, R.CUSUM, R.CUSQ):
                err = abs(R.LD(stats[r, j, c]) - want[j, c])
                print("model %d series %d column %d: error %.3e, bar %.3e + tolerance %.3e" % (r, j, c, err, bars[j, c], tol[c]))
                assert err <= bars[j, c] + tol[c], (r, j, c)
            assert stats[r, j, R.M] == want[j, R.M] and stats[r, j, R.H] == want[j, R.H]
            name = mb.batch.names[r][j]
            np.testing.assert_allclose(norm.loc[(r, name)].values.astype(float), R.normality(want[j]), rtol=1e-6)
            hw = R.heteroskedasticity(want[j])
            row = het.loc[(r, name)]
            np.testing.assert_allclose(row[["nobs", "h", "H", "pvalue", "cusum", "cusum_pvalue", "cusumsq", "cusumsq_pvalue"]].values.astype(float),
                                       [hw[i] for i in (0, 1, 2, 3, 4, 6, 7, 9)], rtol=1e-6)
            # the excursions of the fixed seed are decisive by more than the bar AND the innovations' tolerance
            C, Q = np.cumsum(e - want[j, R.MEAN]), np.cumsum((e - want[j, R.MEAN]) ** 2)
            for x, c in ((np.abs(C), R.CUSUM), (np.abs(Q - np.arange(1, len(e) + 1) / R.LD(len(e)) * want[j, R.S2]), R.CUSQ)):
                top = np.sort(x)[-2:]
                assert top[1] - top[0] > 2 * (bars[j, c] + tol[c]), (r, j, c)
            assert row["cusum_time"] == mb.batch.index[r][hw[5]] and row["cusumsq_time"] == mb.batch.index[r][hw[8]]
        for l in range(4):
            ctol = A[l:].T @ D[:T - l] + D[l:].T @ A[:T - l]
            err = np.abs(sums[r, l].astype(R.LD) - ws[l])
            print("model %d lag %d: largest error / (bar + tolerance) %.3f" % (r, l, float(np.max(err / (cbars[l] + ctol)))))
            assert (err <= cbars[l] + ctol).all(), (r, l)
        qw = R.cross_test(wc, ws, 20)
        np.testing.assert_allclose(cross.loc[r, ["Q", "df", "pvalue"]].values.astype(float), qw[:3], rtol=1e-6)
        assert abs(qw[3][4]) - qw[4] > 1e-6                                    # the worst pair is decisive
        names = mb.batch.names[r]
        assert (cross.loc[r, "series_a"], cross.loc[r, "series_b"], cross.loc[r, "lag"]) == (names[qw[3][0]], names[qw[3][1]], qw[3][2])
        np.testing.assert_allclose([cross.loc[r, "r"], cross.loc[r, "z"]], qw[3][3:], rtol=1e-6)
    screen = mb.screen_residuals(alpha, nlags=3)
    assert len(screen) == Rn * N and list(screen.columns)[-1] == "flag"


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals():
    """N = 65, nlags = 33 and -1, a NULL d_stats and an output one element short: MK_ERR_INVALID with the argument named, and no
    launch -- the outputs keep their sentinel."""
    import torch

    from metran_amd import _lib

    kf = _engine()
    L = _lib.lib()
    B, T, N, nl = 2, 16, 8, 4
    big = torch.full((B * 5 * 65 * 65,), 777.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((B * 5 * 65 * 65,), 777, dtype=torch.int64, device="cuda")
    cells = torch.ones(B * T * 65, dtype=torch.float64, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())   # noqa: E731
    kf._bind_stream()

    def refused(rc, word):
        torch.cuda.synchronize()
        assert rc == -1 and word in L.mk_last_error(), (rc, L.mk_last_error())
        assert bool((big == 777.0).all()) and bool((cnt == 777).all())

    refused(L.mk_residual_cross(kf._ctx, B, T, 65, 0, 0, nl, p(cells), p(cells), p(big), p(cnt), p(big)), b"N <= 64")
    refused(L.mk_residual_cross(kf._ctx, B, T, N, 0, 0, 33, p(cells), p(cells), p(big), p(cnt), p(big)), b"nlags")
    refused(L.mk_residual_cross(kf._ctx, B, T, N, 0, 0, -1, p(cells), p(cells), p(big), p(cnt), p(big)), b"nlags")
    # a missing pointer: the message names that argument and no other
    for k, word in ((6, b"d_v"), (7, b"d_f"), (8, b"d_stats")):
        args = [kf._ctx, B, T, N, 0, 0, p(cells), p(cells), p(big)]
        args[k] = None
        refused(L.mk_residual_series(*args), word + b" is required")
    for k, word in ((7, b"d_v"), (8, b"d_f"), (9, b"d_stats"), (10, b"d_counts"), (11, b"d_sums")):
        args = [kf._ctx, B, T, N, 0, 0, nl, p(cells), p(cells), p(big), p(cnt), p(big)]
        args[k] = None
        refused(L.mk_residual_cross(*args), word + b" is required")
    refused(L.mk_residual_series(kf._ctx, B, T, N, 0, -1, p(cells), p(cells), p(big)), b"t_first")
    pairs = B * (nl + 1) * N * N
    short = {}
    try:
        for name, doubles in (("stats", B * N * 12 - 1), ("counts", pairs - 1), ("sums", pairs - 1)):
            ptr = ctypes.c_void_p()
            assert L.mk_malloc(kf._ctx, doubles * 8, ctypes.byref(ptr)) == 0   # an allocation of its own: its size is known exactly
            short[name] = ptr
        refused(L.mk_residual_series(kf._ctx, B, T, N, 0, 0, p(cells), p(cells), short["stats"]), b"d_stats")
        refused(L.mk_residual_cross(kf._ctx, B, T, N, 0, 0, nl, p(cells), p(cells), short["stats"], p(cnt), p(big)), b"d_stats")
        refused(L.mk_residual_cross(kf._ctx, B, T, N, 0, 0, nl, p(cells), p(cells), p(big), short["counts"], p(big)), b"d_counts")
        refused(L.mk_residual_cross(kf._ctx, B, T, N, 0, 0, nl, p(cells), p(cells), p(big), p(cnt), short["sums"]), b"d_sums")
    finally:
        for ptr in short.values():
            L.mk_free(kf._ctx, ptr)
    v = torch.ones((B, T, N), dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        kf.residual_cross(v, v, kf.residual_series(v, v), nlags=33)
    with pytest.raises(ValueError):
        kf.residual_cross(v, v, torch.ones((B, N, 11), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        kf.residual_series(v, v.float())
