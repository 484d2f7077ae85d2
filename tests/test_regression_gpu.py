"""Intervention effects by GLS on the GPU (C ABI mk_regression: the recording forward pass, the gain tape written by
innov_step_kernel, regress_replay_kernel; mk_regression_adjust) against the extended-precision numpy restatement
(tests/regress_ref.py, pinned to dense conditioning, the oracle and the leave-one-out restatement by
tests/test_regression_host.py), against independent kernels (the filter's objective and sigmas, the leave-one-out predictions),
bit for bit across batches, layouts and sets of effects, under both kernel families and on a shape without specialised kernels,
next to an invalid model, the refusals of the raw ABI, and end to end through MetranBatch.

The bars are measured, not chosen (scripts/measure_regression_bar.py prints them): on the inputs of ``test_against_restatement``
(every shape, length, instance and effect list below) the largest difference between the float64 and the extended-precision
restatement is, for the normal matrix A entrywise relative to sqrt(A_pp A_qq), MEASURED_A = 1.31e-14 (at (32,4), T = 2), and for
beta, cov and gain -- which carry the conditioning of S -- relative to max(1, |value|), MEASURED_S = 1.07e-13 (at (14,2), T = 17).
Times 16 -- the kernel's tree-order sums differ from numpy's left-to-right order, the factor of tests/test_weights_gpu.py -- with
the project's floor of 1e-13: BAR_A = 2.1e-13, BAR_S = 1.7e-12.  The condition number of the unit-diagonal S of the effects kept is
at most 1e4 on every input (tests/test_regression_host.py checks the cap; the largest here is 4.6e2).

Counting convention of the checks against the filter: mk_regression counts the cells of the steps t >= t_first, the filter's
warm-up (get_mle, metran/kalmanfilter.py:550-567) skips the first ``warmup`` steps THAT HOLD AN OBSERVATION.  The two name the same
cells when warmup = the number of non-empty steps before t_first (``_warmup_of``), which is what the comparisons use: the
records of the data pattern begin with empty steps.

The models here are MILD by construction (``test_weights_gpu._data``: 40 % missing cells, ordinary persistence, P0 near the
identity; effect lists whose unit-diagonal condition number stays below 1e4).  Persistence up to 1 - 1e-9, a communality of 0.999,
records with one observation or a never-observed series and nearly collinear effects are run through this route by
tests/test_gpu_property_fits.py (tests/test_property_fits.py on the CPU), at the conditioning-aware bars of tests/hard_models.py."""
import ctypes

import numpy as np
import pytest

import regress_ref
import weights_ref
from test_weights_gpu import _data, _engine, _np, _plan, _sub

pytestmark = pytest.mark.gpu

MEASURED_A = 1.31e-14
MEASURED_S = 1.07e-13
BAR_A = max(16 * MEASURED_A, 1e-13)
BAR_S = max(16 * MEASURED_S, 1e-13)
B_, R_ = 5, 2
# 16-lane groups up to n = 16 ((14,2) the last), one wavefront from n = 17 ((15,2) the first)
SHAPES = [(3, 1), (8, 2), (14, 2), (15, 2), (20, 2), (32, 4)]
LENGTHS = [1, 2, 17, 40]
CASES = [(N, K, "specialised") for N, K in SHAPES] + [(3, 1, "generic")]
UNSPECIALISED = (7, 7)   # no ahead-of-time or prebuilt module: the size-generic filter records for it
LEVEL, RAMP = regress_ref.LEVEL, regress_ref.RAMP
UNUSED = (-1, 0, 0, 1)
OUTPUTS = ("beta", "cov", "gain", "normal", "support", "dropped")


def _effects(N, T, M):
    """[R,M,4], the same list for both records.  M = 16 from T = 17 on: a pulse at the observed cell (7, 0) and one at the
    missing cell (7, 1) (support 0), a shift on the last series (never observed on record 1: support 0 there), a permanent shift
    (t1 = T) and its exact duplicate further down (the later one dropped), a whole-record ramp and a whole-record level
    (t0 = 0, t1 = T) on one series, temporary offsets, ramps that hold, a pulse at the last step, an unused slot.  T = 1, 2: a pulse
    at the observed cell (0, 0), its exact duplicate and one at the missing cell (0, 1), a whole-record level on the last series and
    a whole-record ramp on series 2 (the same series for N = 3: proportional where one step is observed), a pulse at the last
    step, unused slots -- effects on different series, or exactly collinear ones, never nearly collinear ones.
    M = 3 and M = 1 are sub-lists of it."""
    if T >= 17:
        full = [(0, LEVEL, 7, 8), (1, LEVEL, 7, 8), (N - 1, LEVEL, 3, T), (1, LEVEL, 9, T), (2, RAMP, 0, T), (0, LEVEL, 0, 4), UNUSED,
                (1, LEVEL, 9, T), (2, LEVEL, 10, 14), (0, RAMP, 10, 15), (1, LEVEL, T - 1, T), (0, LEVEL, 12, T), (2, LEVEL, 0, T),
                (1, RAMP, 2, 9), (0, LEVEL, 8, 10), (2, LEVEL, 15, 17)]
        pick = {16: range(16), 3: (0, 3, 4), 1: (4,)}[M]
    else:
        full = [(0, LEVEL, 0, 1), (1, LEVEL, 0, 1), (N - 1, LEVEL, 0, T), (2, RAMP, 0, T), UNUSED, (0, LEVEL, 0, 1), (1, LEVEL, T - 1, T)] + [UNUSED] * 9
        pick = {16: range(16), 3: (0, 3, 6), 1: (3,)}[M]
    ef = np.array([full[i] for i in pick], dtype=np.int64)
    return np.broadcast_to(ef, (R_,) + ef.shape).copy()


def input_sets():
    """Every (problem, effects [R,M,4], t_first) that the tests of this file estimate effects on, for the conditioning cap of
    tests/test_regression_host.py.  (The pulses of ``test_pulses_are_the_deletion_residuals`` are estimated one at a time: S is
    1 x 1.)"""
    cases = [(c, si) for si, c in enumerate(CASES)] + [(UNSPECIALISED + ("unspecialised",), len(CASES))]
    for (N, K, _), si in cases:
        for ti, T in enumerate(LENGTHS):
            p = _data(N, K, T, 100 * N + T, _plan(si, ti)[1])
            for M in (16, 3, 1):
                yield p, _effects(N, T, M), _t_first(si, ti)
    for N, K in ((8, 2), (20, 2)):
        yield _data(N, K, 17, seed=17 + N, full=True), _effects(N, 17, 16), 1          # test_dropped_effects_leave_the_others_unchanged
        yield _data(N, K, 17, seed=9, full=True), _effects(N, 17, 16), 1               # test_batch_independence
    for N, K in ((8, 2), (32, 4)):
        for t_first in (0, 1):
            yield _data(N, K, 40, seed=61 + N, full=True, B=4), _effects(N, 40, 16), t_first   # test_gain_is_the_drop_of_the_filters_objective
    yield _data(8, 2, 17, seed=13, full=True, B=4), _effects(8, 17, 16), 1             # test_invalid_model_in_the_batch


def _t_first(si, ti):
    """0 and 1 in turn: every shape sees both, and so does every length."""
    return (si + ti // 2) % 2


def _warmup_of(obs, t_first):
    """The filter's warm-up that names the cells of the steps t >= t_first of a record: the non-empty steps before t_first."""
    return int(np.isfinite(obs[:t_first]).any(axis=1).sum())


def _raw(kf, p, effects, t_first, time_major=False):
    """mk_regression through the raw ABI (any B >= R): dict of numpy arrays."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem, RegressionRequest

    L = _lib.lib()
    R, T, N = p["obs"].shape
    K = p["loadings"].shape[2]
    B, M = p["phi"].shape[0], effects.shape[1]
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    t = {k: dev(p[k]) for k in ("obs", "phi", "q", "loadings", "obsvar", "x0", "P0")}
    prob = Problem(B, R, T, N, K, 0, ptr(t["obs"]), ptr(t["phi"]), ptr(t["q"]), ptr(t["loadings"]), ptr(t["obsvar"]), ptr(t["x0"]),
                   ptr(t["P0"]), 0, None, None)
    ws = int(L.mk_regression_work_stride(N, K))
    assert ws == int(L.mk_weights_work_stride(N, K)) == int(L.mk_record_stride(N + K)) + N * ((N + K + 3) & ~1)
    work = torch.empty(B * T * ws, dtype=torch.float64, device="cuda")
    ef = torch.as_tensor(np.ascontiguousarray(effects), dtype=torch.int64, device="cuda")
    out = {"beta": torch.full((B, M), 7.5, dtype=torch.float64, device="cuda"), "cov": torch.full((B, M, M), 7.5, dtype=torch.float64, device="cuda"),
           "gain": torch.full((B,), 7.5, dtype=torch.float64, device="cuda"),
           "normal": torch.full((B, M + 1, M + 1), 7.5, dtype=torch.float64, device="cuda"),
           "support": torch.full((B, M), -3, dtype=torch.int64, device="cuda"), "dropped": torch.full((B,), -3, dtype=torch.int32, device="cuda")}
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    req = RegressionRequest()
    req.n_effects, req.t_first, req.d_effects = M, t_first, ef.data_ptr()
    for key in OUTPUTS:
        setattr(req, "d_" + key, out[key].data_ptr())
    kf._bind_stream()
    rc = L.mk_regression(kf._ctx, ctypes.byref(prob), ptr(work), 1 if time_major else 0, ctypes.byref(req), ptr(status))
    assert rc == 0, L.mk_last_error()
    torch.cuda.synchronize()
    res = {k: _np(v) for k, v in out.items()}
    res["status"] = _np(status)
    return res


def _args(p, b):
    r = b % p["obs"].shape[0]
    pick = lambda a, i: None if a is None else a[i]   # noqa: E731
    return (p["obs"][r], p["phi"][b], p["q"][b], p["loadings"][r], pick(p["obsvar"], r), pick(p["x0"], b), pick(p["P0"], b))


def _reference(p, b, effects, t_first, gain=None, dtype=np.longdouble):
    args = _args(p, b)
    gain = gain if gain is not None else weights_ref.gains(*args, dtype=dtype)
    return regress_ref.regression(*args, effects=effects[b % p["obs"].shape[0]], t_first=t_first, dtype=dtype, gain=gain), gain


def _mask(dropped):
    return sum(1 << m for m, gone in enumerate(dropped) if gone)


def differences(got, ref):
    """(largest difference of A relative to sqrt(A_pp A_qq), largest difference of beta, cov and gain relative to max(1, |value|))
    between two results of one instance; the NaN patterns must agree."""
    A, Ar = np.asarray(got["normal"], dtype=np.longdouble), np.asarray(ref["normal"], dtype=np.longdouble)
    dg = np.sqrt(np.abs(np.diag(Ar)).astype(np.float64))
    scale = np.outer(dg, dg)
    scale[scale == 0] = 1.0
    da = float(np.max(np.abs(A - Ar).astype(np.float64) / scale))
    ds = 0.0
    for key in ("beta", "cov", "gain"):
        g, r = np.atleast_1d(np.asarray(got[key], dtype=np.longdouble)), np.atleast_1d(np.asarray(ref[key], dtype=np.longdouble))
        assert np.array_equal(np.isnan(g), np.isnan(r)), key
        ok = ~np.isnan(r)
        if ok.any():
            ds = max(ds, float(np.max((np.abs(g - r)[ok] / np.maximum(1, np.abs(r[ok]))).astype(np.float64))))
    return da, ds


def _check_case(N, K, T, family, time_major, full, seed, t_first):
    p = _data(N, K, T, seed, full)
    kf = _engine(p, family)
    if family == "unspecialised":
        assert not kf.specialised() and kf.regression_supported
    gains = {}
    for M in (16, 3, 1):
        ef = _effects(N, T, M)
        got = _raw(kf, p, ef, t_first, time_major)
        assert not got["status"].any()
        for b in range(B_):
            ref, gains[b] = _reference(p, b, ef, t_first, gains.get(b))
            mine = {k: got[k][b] for k in OUTPUTS}
            what = "instance %d, M = %d" % (b, M)
            assert int(mine["dropped"]) == _mask(ref["dropped"]), (what, int(mine["dropped"]), ref["dropped"])
            assert np.array_equal(mine["support"], ref["support"]), what
            da, ds = differences(mine, ref)
            print("(%d,%d) %s T=%d t_first=%d %s: A %.3g of %.3g, solve %.3g of %.3g" % (N, K, family, T, t_first, what, da, BAR_A, ds, BAR_S))
            assert da <= BAR_A and ds <= BAR_S, (what, da, ds)


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%s" % c for c in CASES])
def test_against_restatement(case, T):
    """B = 5 instances on R = 2 records, M = 16, 3 and 1 effects, through the raw ABI (the engine wants B a multiple of R)."""
    N, K, family = case
    si, ti = CASES.index(case), LENGTHS.index(T)
    time_major, full = _plan(si, ti)
    _check_case(N, K, T, family, time_major, full, seed=100 * N + T, t_first=_t_first(si, ti))


@pytest.fixture
def no_jit(monkeypatch, tmp_path):
    """A machine without hipcc and without prebuilt modules: a shape outside the ahead-of-time list runs the size-generic filter."""
    monkeypatch.setenv("METRAN_HIP_JIT", "0")
    monkeypatch.setenv("METRAN_HIP_CACHE", str(tmp_path))
    from metran_amd import jit

    monkeypatch.setattr(jit, "PREBUILT_DIR", str(tmp_path / "no_prebuilt_modules"))


@pytest.mark.parametrize("T", LENGTHS)
def test_a_shape_without_specialised_kernels(no_jit, T):
    N, K = UNSPECIALISED
    si, ti = len(CASES), LENGTHS.index(T)
    time_major, full = _plan(si, ti)
    _check_case(N, K, T, "unspecialised", time_major, full, seed=100 * N + T, t_first=_t_first(si, ti))


@pytest.mark.parametrize("shape", [(8, 2), (15, 2)], ids=["8x2", "15x2"])
def test_nothing_counted_when_t_first_is_T(shape):
    """t_first = T: no cell is counted -- A is zero, every effect is dropped, the gain is 0."""
    N, K = shape
    T = 17
    p = _data(N, K, T, seed=7 + N, full=True)
    got = _raw(_engine(p), p, _effects(N, T, 3), T)
    assert (got["normal"] == 0).all() and (got["support"] == 0).all() and (got["dropped"] == 7).all() and (got["gain"] == 0).all()
    assert np.isnan(got["beta"]).all() and np.isnan(got["cov"]).all()


@pytest.mark.parametrize("shape", [(8, 2), (20, 2)], ids=["8x2", "20x2"])
def test_dropped_effects_leave_the_others_unchanged(shape):
    """The pulse at the missing cell, the effect on the never-observed series, the duplicate and the unused slot: the other
    effects' estimates are bit-identical to a call without them."""
    N, K = shape
    T = 17
    p = _data(N, K, T, seed=17 + N, full=True)
    kf = _engine(p)
    ef = _effects(N, T, 16)
    full = _raw(kf, p, ef, 1)
    for b in range(B_):
        gone = [m for m in range(16) if (int(full["dropped"][b]) >> m) & 1]
        assert set(gone) >= {1, 6, 7} and (2 in gone) == (b % R_ == 1), (b, gone)
    rec1 = [b for b in range(B_) if b % R_ == 1]
    keep = [m for m in range(16) if m not in (1, 2, 6, 7)]
    rest = _raw(kf, p, ef[:, keep], 1)
    assert np.array_equal(rest["beta"][rec1], full["beta"][rec1][:, keep], equal_nan=True)
    assert np.array_equal(rest["cov"][rec1], full["cov"][rec1][:, keep][:, :, keep], equal_nan=True)
    assert np.array_equal(rest["gain"][rec1], full["gain"][rec1]) and np.array_equal(rest["support"][rec1], full["support"][rec1][:, keep])


def _filter_sums(kf, p, warmup):
    """(-2 log L, sum of the filter's sigmas from its warm-up on) per instance, through the engine."""
    res = kf.filter(p["phi"], p["q"], warmup=warmup, x0=p["x0"], P0=p["P0"], outputs=())
    sg = _np(res["sigmas"])
    return _np(res["mle"]), np.array([sg[b, warmup:].sum() for b in range(sg.shape[0])])


@pytest.mark.parametrize("t_first", [0, 1])
@pytest.mark.parametrize("shape", [(8, 2), (32, 4)], ids=["8x2", "32x4"])
def test_gain_is_the_drop_of_the_filters_objective(shape, t_first):
    """Independent kernels: A[0,0] is the filter's sum of sigmas, and -2 log L of the ADJUSTED records (adjust_observations, then
    the filter's own objective) is -2 log L of the records as they are minus the gain; unadjust_observations brings the
    observations back bit for bit.  Through the engine, B = 4 on R = 2; each record at the warm-up that names its cells."""
    N, K = shape
    T = 40
    p = _data(N, K, T, seed=61 + N, full=True, B=4)
    kf = _engine(p)
    ef = _effects(N, T, 16)
    res = kf.regression(p["phi"], p["q"], ef, t_first=t_first, x0=p["x0"], P0=p["P0"])
    assert set(res) == {"_work", "status"} | set(OUTPUTS) and not _np(res["status"]).any()
    raw = _raw(kf, p, ef, t_first, time_major=False)
    for key in OUTPUTS:
        assert np.array_equal(_np(res[key]), raw[key], equal_nan=True), key
    A, gain, beta = _np(res["normal"]), _np(res["gain"]), _np(res["beta"])
    before = _np(kf.obs).copy()
    base = {w: _filter_sums(kf, p, w) for w in {_warmup_of(p["obs"][r], t_first) for r in range(R_)}}
    # the instances of a record share the adjustment: one instance per record at a time
    for s in range(2):
        kf.adjust_observations(ef, beta[s * R_:(s + 1) * R_])
        assert not np.array_equal(_np(kf.obs), before, equal_nan=True)
        for r in range(R_):
            b, w = s * R_ + r, _warmup_of(p["obs"][r], t_first)
            mle, _ = _filter_sums(kf, p, w)
            nobs = np.isfinite(p["obs"][r][t_first:]).sum()
            bar = BAR_S * max(1.0, abs(gain[b])) + 1e-13 * (abs(base[w][0][b]) + nobs * np.log(2 * np.pi))
            assert abs((base[w][0][b] - mle[b]) - gain[b]) <= bar, (b, base[w][0][b] - mle[b], gain[b], bar)
            assert abs(A[b, 0, 0] - base[w][1][b]) <= BAR_A * A[b, 0, 0] + 1e-13 * base[w][1][b], (b, A[b, 0, 0], base[w][1][b])
    kf.unadjust_observations()
    assert np.array_equal(_np(kf.obs), before, equal_nan=True)


def test_adjust_and_unadjust_with_a_mask():
    """The adjustment against the restatement, with and without a mask: applied to the masked records and to the kept unmasked
    copy; unadjust restores both bit for bit; a second adjustment starts from the originals."""
    N, K, T = 8, 2, 17
    p = _data(N, K, T, seed=71, full=False, B=2)
    kf = _engine(p)
    ef = _effects(N, T, 16)
    beta = np.random.default_rng(3).normal(size=(R_, 16))
    beta[:, 5] = np.nan
    want = np.stack([regress_ref.adjusted(p["obs"][r], ef[r], beta[r]) for r in range(R_)])
    before = _np(kf.obs).copy()
    kf.adjust_observations(ef, beta)
    np.testing.assert_allclose(_np(kf.obs), want, rtol=0, atol=4 * np.finfo(float).eps * (1 + np.nanmax(np.abs(want))), equal_nan=True)
    once = _np(kf.obs).copy()
    kf.adjust_observations(ef, beta)
    assert np.array_equal(_np(kf.obs), once, equal_nan=True)
    kf.unadjust_observations()
    assert np.array_equal(_np(kf.obs), before, equal_nan=True)
    mask = np.zeros((R_, T, N), dtype=bool)
    mask[:, 8:11, 0] = True
    kf.mask_observations(mask)
    masked = _np(kf.obs).copy()
    kf.adjust_observations(ef, beta)
    assert np.array_equal(_np(kf.obs), np.where(mask, np.nan, once), equal_nan=True)
    kf.unmask_observations()
    assert np.array_equal(_np(kf.obs), once, equal_nan=True)            # adjusted, unmasked
    kf.unadjust_observations()
    assert np.array_equal(_np(kf.obs), masked, equal_nan=True)          # as before the adjustment: masked
    kf.unmask_observations()
    assert np.array_equal(_np(kf.obs), before, equal_nan=True)


@pytest.mark.parametrize("shape", [(8, 2), (32, 4)], ids=["8x2", "32x4"])
def test_pulses_are_the_deletion_residuals(shape):
    """A pulse at an observed cell with t_first = 0: the estimate is the observation minus its leave-one-out prediction and its
    variance the deletion variance (loo_predict's, plus the observation variance) -- an independent kernel."""
    N, K = shape
    T = 40
    p = _data(N, K, T, seed=81 + N, full=True, B=4)
    kf = _engine(p)
    assert kf.loo_supported()
    seen = np.isfinite(p["obs"])
    cells = [(t, j) for t in (7, 0, 2, T - 1, 20, 21, 33) for j in (0, 1, 2) if seen[:, t, j].all()][:8]
    assert len(cells) >= 4 and (7, 0) in cells
    ef = np.broadcast_to(np.array([(j, LEVEL, t, t + 1) for t, j in cells], dtype=np.int64), (R_, len(cells), 4)).copy()
    loo = kf.loo_predict(p["phi"], p["q"], x0=p["x0"], P0=p["P0"])
    lm, lv = _np(loo["loo_means"]), _np(loo["loo_vars"])
    for m, (t, j) in enumerate(cells):       # one pulse per call: together they would be estimated jointly
        res = kf.regression(p["phi"], p["q"], ef[:, m:m + 1], t_first=0, x0=p["x0"], P0=p["P0"])
        beta, cov = _np(res["beta"])[:, 0], _np(res["cov"])[:, 0, 0]
        assert not _np(res["dropped"]).any() and (_np(res["support"]) == 1).all()
        for b in range(4):
            r = b % R_
            resid, var = p["obs"][r, t, j] - lm[b, t, j], lv[b, t, j] + p["obsvar"][r, j]
            assert abs(beta[b] - resid) <= 1e-9 * max(1.0, abs(resid)) and abs(cov[b] - var) <= 1e-9 * max(1.0, var), (b, t, j)


@pytest.mark.parametrize("shape", [(8, 2), (20, 2)], ids=["8x2", "20x2"])
def test_batch_independence(shape):
    """An instance's outputs are bit-identical alone and inside the batch of five, in either layout of the work buffer; the block
    of A of a subset of the effects does not depend on the other effects of the call."""
    N, K = shape
    T = 17
    p = _data(N, K, T, seed=9, full=True)
    kf = _engine(p)
    ef = _effects(N, T, 16)
    full = _raw(kf, p, ef, 1)
    other = _raw(kf, p, ef, 1, time_major=True)
    for key in OUTPUTS:
        assert np.array_equal(full[key], other[key], equal_nan=True), key
    for b in (0, 3, 4):
        sub, rec = _sub(p, [b])
        alone = _raw(_engine(sub), sub, ef[rec], 1)
        for key in OUTPUTS:
            assert np.array_equal(alone[key][0], full[key][b], equal_nan=True), (key, b)
    for pick in ([3], [0, 4, 9], [2, 3, 5, 8, 10, 11, 12, 13, 15]):     # 1, 3 and 9 columns: every width of the kernel but the full one
        part = _raw(kf, p, ef[:, pick], 1)
        rows = [0] + [m + 1 for m in pick]
        assert np.array_equal(part["normal"], full["normal"][:, rows][:, :, rows]), pick
        assert np.array_equal(part["support"], full["support"][:, pick]), pick


def test_invalid_model_in_the_batch():
    """A model with a negative observation variance among the records: its instances carry the status bit and NaN rows; the
    instances of the other record are bit-identical to the same call without it."""
    from metran_amd.engine import FLAG_NONPOSITIVE_F

    p = _data(8, 2, 17, seed=13, full=True, B=4)
    ef = _effects(8, 17, 16)
    good = _engine(p).regression(p["phi"], p["q"], ef, x0=p["x0"], P0=p["P0"])
    good = {k: _np(good[k]) for k in OUTPUTS + ("status",)}
    assert not good["status"].any()
    q = dict(p, obsvar=p["obsvar"].copy())
    q["obsvar"][1, :] = -50.0
    bad = _engine(q).regression(p["phi"], p["q"], ef, x0=p["x0"], P0=p["P0"])
    bad = {k: _np(bad[k]) for k in OUTPUTS + ("status",)}
    assert (bad["status"][[1, 3]] & FLAG_NONPOSITIVE_F).all() and not bad["status"][[0, 2]].any()
    for key in ("beta", "cov", "gain", "normal"):
        assert np.isnan(bad[key][[1, 3]]).all(), key
    for key in OUTPUTS:
        assert np.array_equal(bad[key][[0, 2]], good[key][[0, 2]], equal_nan=True), key


def test_refusals():
    """Every MK_ERR_INVALID case and MK_ERR_SHAPE at N + K = 65: refused before any launch -- the outputs keep their sentinel."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem, RegressionRequest

    p = _data(8, 2, 17, seed=3, full=False, B=2, R=2)
    kf = _engine(p)
    L = _lib.lib()
    assert int(L.mk_regression_max_effects()) == 16
    assert int(L.mk_regression_work_stride(61, 4)) == 0 and int(L.mk_regression_work_stride(60, 4)) == int(L.mk_record_stride(64)) + 60 * 66
    assert kf.regression_supported
    B, T, N, M = 2, 17, 8, 3
    prob, keep, _ = kf._problem(kf._dev(p["phi"]), kf._dev(p["q"]), 0, None, None)
    buf = kf.alloc_regression(B, M)
    for key in ("beta", "cov", "gain", "normal"):
        buf[key].fill_(7.5)
    ef0 = np.broadcast_to(np.array([(0, LEVEL, 7, 8), (1, RAMP, 0, T), UNUSED], dtype=np.int64), (2, M, 4)).copy()
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0   # an allocation of its own: its size is known exactly
    held = []

    def table(slot=None):
        ef = ef0.copy()
        if slot is not None:
            ef[1, 1] = slot
        held.append(torch.as_tensor(ef, dtype=torch.int64, device="cuda"))
        return held[-1].data_ptr()

    def call(work=buf["_work"].data_ptr(), effects=None, n_effects=M, t_first=1, problem=prob, **ptrs):
        req = RegressionRequest()
        req.n_effects, req.t_first, req.d_effects = n_effects, t_first, table() if effects is None else (effects or None)
        for key in OUTPUTS:
            setattr(req, "d_" + key, ptrs.get(key, buf[key].data_ptr()) or None)
        return L.mk_regression(kf._ctx, ctypes.byref(problem), ctypes.c_void_p(work) if work else None, 0, ctypes.byref(req), None)

    def adjust(n_effects=M, effects=None, beta=buf["beta"].data_ptr(), obs_in=kf.obs.data_ptr(), obs_out=buf["_work"].data_ptr(), R=2):
        c = lambda v: ctypes.c_void_p(v) if v else None   # noqa: E731
        return L.mk_regression_adjust(kf._ctx, R, T, N, 0, n_effects, c(table() if effects is None else effects), c(beta), c(obs_in),
                                      c(obs_out))

    try:
        assert call(work=None) == -1 and b"d_work" in L.mk_last_error()
        assert call(effects=0) == -1 and b"d_effects" in L.mk_last_error()
        for key in OUTPUTS:
            assert call(**{key: 0}) == -1 and b"required" in L.mk_last_error(), key
        assert call(n_effects=0) == -1 and call(n_effects=17) == -1 and b"n_effects" in L.mk_last_error()
        assert call(t_first=-1) == -1 and b"t_first" in L.mk_last_error()
        assert call(work=small.value) == -1 and b"d_work" in L.mk_last_error()
        assert call(effects=small.value, n_effects=9) == -1 and b"d_effects" in L.mk_last_error()
        assert call(beta=small.value, n_effects=16) == -1
        assert call(cov=small.value) == -1 and b"d_cov" in L.mk_last_error()
        assert call(normal=small.value) == -1 and b"d_normal" in L.mk_last_error()
        assert call(support=small.value, n_effects=16) == -1
        for slot, word in (((N, LEVEL, 0, 3), b"series"), ((0, 2, 0, 3), b"kind"), ((0, -1, 0, 3), b"kind"), ((0, LEVEL, -1, 3), b"t0"),
                           ((0, LEVEL, 3, 3), b"t0"), ((0, RAMP, 5, 4), b"t0"), ((0, LEVEL, 3, T + 1), b"t1")):
            assert call(effects=table(slot)) == -1 and word in L.mk_last_error() and b"d_effects[1, 1]" in L.mk_last_error(), slot
            assert adjust(effects=table(slot)) == -1 and word in L.mk_last_error(), slot
        q = ctypes.c_void_p(buf["_work"].data_ptr())
        wide = Problem(1, 1, 4, 61, 4, 0, q, q, q, q, None, None, None, 0, None, None)
        assert call(problem=wide) == -2 and b"N=61, K=4" in L.mk_last_error()
        assert adjust(n_effects=0) == -1 and adjust(n_effects=17) == -1 and b"n_effects" in L.mk_last_error()
        assert adjust(beta=0) == -1 and adjust(obs_in=0) == -1 and adjust(obs_out=0) == -1 and b"required" in L.mk_last_error()
        assert adjust(R=0) == -1
        assert adjust(obs_out=small.value) == -1 and b"d_obs_out" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    torch.cuda.synchronize()
    assert all((buf[key] == 7.5).all() for key in ("beta", "cov", "gain", "normal"))
    assert call(effects=table((-1, 9, 99, -5))) == 0                   # an unused slot is not read further ... and the call runs
    torch.cuda.synchronize()
    assert not (buf["normal"] == 7.5).any()
    with pytest.raises(ValueError):
        kf.regression(p["phi"], p["q"], np.zeros((3, 2, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        kf.regression(p["phi"], p["q"], np.zeros((2, 17, 4), dtype=np.int64))
    with pytest.raises(ValueError):
        kf.regression(p["phi"], p["q"], ef0, t_first=-1)
    with pytest.raises(ValueError):
        kf.alloc_regression(2, 0)


def test_metran_batch_end_to_end():
    """Through MetranBatch: synthesised records, a known shift of 0.8 standard deviations added to one series from a mid-record
    step on.  The estimate is within three of its own standard errors of the shift; the gain is the difference of ``get_mle``
    before and after ``adjust_observations``; ``unadjust_observations`` brings ``get_mle`` back exactly."""
    import pandas as pd

    from metran_amd.batch import MetranBatch

    from metran_amd.synthetic import make_dfm_batch

    T = 160
    d = make_dfm_batch(2, 3, 1, T, seed=5, missing=0.2)            # records drawn from the model whose parameters are used below
    idx = pd.date_range("2001-01-01", periods=T, freq="D")
    models, shift = [], {}
    for r in range(2):
        cols = [pd.Series(10.0 * (j + 1) + (1.0 + 0.5 * j) * d["obs"][r, :, j], index=idx, name="s%d" % j).dropna() for j in range(3)]
        models.append(cols if r == 0 else [c[c.index < idx[150]] for c in cols])
    G = d["loadings"]
    std0 = _np(MetranBatch(models, factors=G)._std)
    for r, j, when in ((0, 1, idx[60]), (1, 2, idx[45])):
        shift[r] = 0.8 * std0[r, j]
        s = models[r][j].copy()
        s[s.index >= when] += shift[r]
        models[r][j] = s
    mb = MetranBatch(models, factors=G)
    astar = d["alpha"]
    frame = mb.fit_interventions([(0, "s1", "level", idx[60]), (1, "s2", "level", idx[45], None), (1, "s0", "ramp", 20, 30)], alpha=astar)
    assert list(frame.index) == [(0, 0), (1, 0), (1, 1)] and not frame["dropped"].any()
    for r in range(2):
        row = frame.loc[(r, 0)]
        assert abs(row["estimate"] - shift[r]) <= 3.0 * row["stderr"], (r, row["estimate"], shift[r], row["stderr"])
        assert 0.0 <= row["pvalue"] <= 1.0 and row["n_obs"] > 20
    per_model = frame.attrs["models"]
    before = _np(mb.get_mle(astar))
    obs0 = _np(mb.kf.obs).copy()
    mb.adjust_observations()
    after = _np(mb.get_mle(astar))
    gain = per_model["gain"].values
    assert np.all(gain > 0) and np.all(np.abs((before - after) - gain) <= BAR_S * np.maximum(1.0, gain) + 1e-13 * np.abs(before))
    assert np.all(np.abs(per_model["obj"].values - before) <= 1e-13 * np.abs(before))
    assert np.allclose(per_model["obj_adjusted"].values, after, rtol=1e-12, atol=0)
    mb.unadjust_observations()
    assert np.array_equal(_np(mb.get_mle(astar)), before) and np.array_equal(_np(mb.kf.obs), obs0, equal_nan=True)
