"""Per-step scores by the tangent filter on the GPU (C ABI mk_scores: the recording forward pass, the gain tape and the innovations
written by innov_step_kernel, score_tangent_kernel, score_stats_kernel) against the extended-precision numpy restatement
(tests/score_ref.py, pinned to central differences of the per-step objective and to the adjoint gradient by
tests/test_scores_host.py), against independent kernels (the adjoint gradient), bit for bit across batches and layouts, under
both kernel families, on shapes without specialised kernels up to the 64-state limit, next to an invalid model, the refusals of
the raw ABI, and end to end through MetranBatch.

Every comparison is relative to the SCALE of the output (tests/score_ref.py: the output's expression with every term replaced by
its absolute value; for ``score`` the scale of the (instance, parameter) pair's largest step).  The bars are measured, not
chosen (scripts/measure_scores_bar.py prints them): 16 times the largest difference between the float64 and the extended-precision
restatement on the inputs of ``input_sets`` (the kernel's tree-order sums differ from numpy's order: the factor of
tests/test_weights_gpu.py), with the project's floor of 1e-13 -- separately for the records of 17 and 40 steps and for those of
one and two steps, so that the short records do not set the bars of the long ones:
    T >= 17   MEASURED        score 2.11e-14, grad 4.96e-15, opg 8.78e-15 (all at (32,4), T = 40), cusum 1.01e-16
              bars            3.37e-13, 1e-13, 1.41e-13, 1e-13
    T <= 2    MEASURED_SHORT  score 1.16e-14 (at (15,2), T = 1), grad 8.75e-14 (at (32,4), T = 2), opg 9.88e-14 and cusum 2.78e-16
              (both at (20,2), T = 2);   bars 1.86e-13, 1.4e-12, 1.58e-12, 1e-13
The larger figures of grad and opg at T = 2 are not a matter of the initial moments (they occur with the default x0 = 0, P0 = I and
with given ones alike, on every shape, at the instances of record 1, whose only counted step is the second one): there the sum
has ONE step, so its scale is that step's own, and what the tangent carries into the step from the one before is rounded at the
size of the carried state, not of the step's terms -- the effect for which ``score`` takes the pair's largest step as its scale.
Over 17 and 40 steps the same errors are 5e-15 of the sum's scale.

Counting convention of the checks against the adjoint gradient: mk_scores counts the steps t >= t_first that hold an observation,
the filter's warm-up skips the first ``warmup`` steps that hold one.  The two name the same steps when warmup = the number of
non-empty steps before t_first (``_warmup_of``, as in tests/test_regression_gpu.py).

The models here are MILD by construction (``test_weights_gpu._data``: 40 % missing cells, ordinary persistence, P0 near the
identity), which is what the flat bars above are for.  Persistence up to 1 - 1e-9, a communality of 0.999 and the hard missingness
patterns are run through this route, with Metran's own chain rule for (dphi, dq), by tests/test_gpu_property_fits.py
(tests/test_property_fits.py on the CPU), at the conditioning-aware bars of tests/hard_models.py."""
import ctypes

import numpy as np
import pytest

import score_ref
from test_weights_gpu import _data, _engine, _np, _plan, _sub

pytestmark = pytest.mark.gpu

MEASURED = {"score": 2.11e-14, "grad": 4.96e-15, "opg": 8.78e-15, "cusum": 1.01e-16}           # T >= 17
MEASURED_SHORT = {"score": 1.16e-14, "grad": 8.75e-14, "opg": 9.88e-14, "cusum": 2.78e-16}     # T <= 2
BAR = {key: max(16 * val, 1e-13) for key, val in MEASURED.items()}
BAR_SHORT = {key: max(16 * val, 1e-13) for key, val in MEASURED_SHORT.items()}
B_, R_ = 5, 2
# 16-lane groups up to n = 16 ((14,2) the last), one wavefront from n = 17 ((15,2) the first)
SHAPES = [(3, 1), (8, 2), (14, 2), (15, 2), (20, 2), (32, 4)]
LENGTHS = [1, 2, 17, 40]
CASES = [(N, K, "specialised") for N, K in SHAPES] + [(3, 1, "generic")]
UNSPECIALISED = (7, 7)   # no ahead-of-time or prebuilt module: the size-generic filter records for it
LIMIT = (60, 4)          # n = 64, the most the kernels serve; T = 17 only
SHORT = 2                # records of up to two steps have bars of their own
OUTPUTS = ("score", "grad", "count", "opg", "cusum")


def _derivs(p, seed):
    """(dphi, dq) [B,n]: of the size of Metran's own (phi dt / alpha^2 is below 0.4), both signs."""
    rng = np.random.default_rng(1000 + seed)
    return rng.uniform(-0.4, 0.4, p["phi"].shape), rng.uniform(-0.8, 0.8, p["phi"].shape)


def _bars(T):
    return BAR_SHORT if T <= SHORT else BAR


def _t_first(si, ti):
    """0 and 1 in turn: every shape sees both, and so does every length."""
    return (si + ti // 2) % 2


def _compared(N, K):
    """The instances compared with the restatement: all five up to n = 16; above, one of each record and the last one (0, 3 and 4:
    the tail of the grid) -- time is the reason, the restatement's extended-precision arrays are [n,n,n] per cell, and the other two
    are held to the same numbers by ``test_batch_independence``; at n = 64, where one instance takes five seconds, instance 3."""
    return list(range(B_)) if N + K <= 16 else ([0, 3, 4] if N + K < 64 else [3])


def _case_input(N, K, si, ti):
    T = LENGTHS[ti]
    seed = 100 * N + T
    time_major, full = _plan(si, ti)
    p = _data(N, K, T, seed, full)
    return p, _derivs(p, seed), _t_first(si, ti), time_major


def input_sets():
    """Every (problem, dphi, dq, t_first, instances compared) that ``test_against_restatement`` and its two companions run, for the
    conditioning check of tests/test_scores_host.py and for scripts/measure_scores_bar.py."""
    cases = [(c, si) for si, c in enumerate(CASES)] + [(UNSPECIALISED + ("unspecialised",), len(CASES))]
    for (N, K, _), si in cases:
        for ti in range(len(LENGTHS)):
            p, (dphi, dq), t_first, _ = _case_input(N, K, si, ti)
            yield p, dphi, dq, t_first, _compared(N, K)
    p, (dphi, dq), t_first, _ = _case_input(*LIMIT, len(CASES) + 1, LENGTHS.index(17))
    yield p, dphi, dq, t_first, _compared(*LIMIT)


def _warmup_of(obs, t_first):
    """The filter's warm-up that names the steps t >= t_first of a record: the non-empty steps before t_first."""
    return int(np.isfinite(obs[:t_first]).any(axis=1).sum())


def _raw(kf, p, dphi, dq, t_first, time_major=False):
    """mk_scores through the raw ABI (any B >= R): dict of numpy arrays, ``score`` as [B,T,n] in either layout."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem, ScoresRequest

    L = _lib.lib()
    R, T, N = p["obs"].shape
    K = p["loadings"].shape[2]
    B, n = p["phi"].shape[0], N + K
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    t = {k: dev(p[k]) for k in ("obs", "phi", "q", "loadings", "obsvar", "x0", "P0")}
    d1, d2 = dev(dphi), dev(dq)
    prob = Problem(B, R, T, N, K, 0, ptr(t["obs"]), ptr(t["phi"]), ptr(t["q"]), ptr(t["loadings"]), ptr(t["obsvar"]), ptr(t["x0"]),
                   ptr(t["P0"]), 0, None, None)
    ws = int(L.mk_scores_work_stride(N, K))
    assert ws == int(L.mk_weights_work_stride(N, K)) + N == int(L.mk_record_stride(n)) + N * ((n + 3) & ~1) + N
    work = torch.empty(B * T * ws, dtype=torch.float64, device="cuda")
    fill = lambda *shape: torch.full(shape, 7.5, dtype=torch.float64, device="cuda")   # noqa: E731
    out = {"score": fill(T, B, n) if time_major else fill(B, T, n), "grad": fill(B, n), "opg": fill(B, n, n), "cusum": fill(B, n, n),
           "count": torch.full((B,), -3, dtype=torch.int64, device="cuda")}
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    req = ScoresRequest()
    req.d_dphi, req.d_dq, req.t_first = d1.data_ptr(), d2.data_ptr(), t_first
    for key in OUTPUTS:
        setattr(req, "d_" + key, out[key].data_ptr())
    kf._bind_stream()
    rc = L.mk_scores(kf._ctx, ctypes.byref(prob), ptr(work), 1 if time_major else 0, ctypes.byref(req), ptr(status))
    assert rc == 0, L.mk_last_error()
    torch.cuda.synchronize()
    res = {k: _np(v) for k, v in out.items()}
    if time_major:
        res["score"] = np.ascontiguousarray(res["score"].transpose(1, 0, 2))
    res["status"] = _np(status)
    return res


def _args(p, b):
    r = b % p["obs"].shape[0]
    pick = lambda a, i: None if a is None else a[i]   # noqa: E731
    return (p["obs"][r], p["phi"][b], p["q"][b], p["loadings"][r], pick(p["obsvar"], r), pick(p["x0"], b), pick(p["P0"], b))


def _reference(p, b, dphi, dq, t_first, dtype=np.longdouble):
    return score_ref.scores(*_args(p, b), dphi=dphi[b], dq=dq[b], t_first=t_first, dtype=dtype)


def _check_case(N, K, si, ti, family):
    p, (dphi, dq), t_first, time_major = _case_input(N, K, si, ti)
    kf = _engine(p, family)
    if family == "unspecialised":
        assert not kf.specialised() and kf.scores_supported
    got = _raw(kf, p, dphi, dq, t_first, time_major)
    assert not got["status"].any()
    for b in _compared(N, K):
        ref = _reference(p, b, dphi, dq, t_first)
        assert int(got["count"][b]) == ref["count"], (b, int(got["count"][b]), ref["count"])
        empty = ~np.isfinite(p["obs"][b % R_]).any(axis=1)
        assert (got["score"][b][empty] == 0).all(), b
        diff, bar = score_ref.differences({k: got[k][b] for k in score_ref.OUTPUTS}, ref), _bars(LENGTHS[ti])
        print("(%d,%d) %s T=%d t_first=%d instance %d: %s" % (N, K, family, LENGTHS[ti], t_first, b,
                                                            ", ".join("%s %.3g of %.3g" % (k, diff[k], bar[k]) for k in score_ref.OUTPUTS)))
        for key in score_ref.OUTPUTS:
            assert diff[key] <= bar[key], (b, key, diff[key])


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%s" % c for c in CASES])
def test_against_restatement(case, T):
    """B = 5 instances on R = 2 records through the raw ABI (the engine wants B a multiple of R)."""
    N, K, family = case
    _check_case(N, K, CASES.index(case), LENGTHS.index(T), family)


@pytest.fixture
def no_jit(monkeypatch, tmp_path):
    """A machine without hipcc and without prebuilt modules: a shape outside the ahead-of-time list runs the size-generic filter."""
    monkeypatch.setenv("METRAN_HIP_JIT", "0")
    monkeypatch.setenv("METRAN_HIP_CACHE", str(tmp_path))
    from metran_amd import jit

    monkeypatch.setattr(jit, "PREBUILT_DIR", str(tmp_path / "no_prebuilt_modules"))


@pytest.mark.parametrize("T", LENGTHS)
def test_a_shape_without_specialised_kernels(no_jit, T):
    _check_case(*UNSPECIALISED, len(CASES), LENGTHS.index(T), "unspecialised")


def test_the_limit_of_64_states(no_jit):
    """(60,4): every lane of the wavefront a state, 32 KB of tangent covariance per group, the size-generic recording pass
    (selected by the kernel family: a shape module of another test may be registered in the process)."""
    _check_case(*LIMIT, len(CASES) + 1, LENGTHS.index(17), "generic")


@pytest.mark.parametrize("t_first", [0, 1])
@pytest.mark.parametrize("shape", [(8, 2), (20, 2)], ids=["8x2", "20x2"])
def test_grad_is_the_adjoint_gradient(shape, t_first):
    """Independent kernels: with (dphi, dq) = (1, 0) ``grad`` is loglik_grad's ``gphi``, with (0, 1) its ``gq``, and
    ``scores_alpha``'s is ``loglik_grad_alpha``'s -- each record at the warm-up that names its steps; twice the bar, two float64
    kernels being compared.  Through the engine, B = 4 on R = 2, default observation variances and initial moments (what
    ``loglik_grad_alpha`` runs on)."""
    N, K = shape
    T = 40
    p = _data(N, K, T, seed=61 + N, full=False, B=4)
    kf = _engine(p)
    assert kf.has_adjoint() and kf.scores_supported
    one, zero = np.ones_like(p["phi"]), np.zeros_like(p["phi"])
    alpha = -1.0 / np.log(p["phi"])
    runs = {"gphi": kf.scores(p["phi"], p["q"], one, zero, t_first=t_first), "gq": kf.scores(p["phi"], p["q"], zero, one, t_first=t_first),
            "galpha": kf.scores_alpha(alpha, t_first=t_first)}
    assert set(runs["gphi"]) == {"_work", "status"} | set(OUTPUTS)
    grads = {k: _np(v["grad"]) for k, v in runs.items()}
    c = np.concatenate([1.0 - (p["loadings"] ** 2).sum(2), np.ones((R_, K))], axis=1)[np.arange(4) % R_]
    dphi_a = p["phi"] / alpha ** 2
    derivs = {"gphi": (one, zero), "gq": (zero, one), "galpha": (dphi_a, -2.0 * p["phi"] * dphi_a * c)}
    scale = {k: np.stack([score_ref.scores(*_args(p, b), dphi=d1[b], dq=d2[b], t_first=t_first, dtype=np.float64)["scale"]["grad"] for b in range(4)])
             for k, (d1, d2) in derivs.items()}
    for s in scale.values():
        s[s == 0] = 1.0      # the state of a series that is never observed: every term of its gradient is zero
    for r in range(R_):
        w = _warmup_of(p["obs"][r], t_first)
        _, gphi, gq = kf.loglik_grad(p["phi"], p["q"], warmup=w)
        _, galpha = kf.loglik_grad_alpha(alpha, warmup=w)
        for key, want in (("gphi", _np(gphi)), ("gq", _np(gq)), ("galpha", _np(galpha))):
            for b in range(r, 4, R_):
                diff = float(np.max(np.abs(grads[key][b] - want[b]) / scale[key][b]))
                print("(%d,%d) t_first=%d %s instance %d: %.3g of %.3g" % (N, K, t_first, key, b, diff, 2 * BAR["grad"]))
                assert diff <= 2 * BAR["grad"], (key, b, diff)


@pytest.mark.parametrize("shape", [(8, 2), (20, 2)], ids=["8x2", "20x2"])
def test_batch_independence(shape):
    """An instance's outputs are bit-identical alone and inside the batch of five, in either layout of the work buffer, and with
    B = R as with B > R."""
    N, K = shape
    T = 17
    p = _data(N, K, T, seed=9, full=True)
    dphi, dq = _derivs(p, 9)
    kf = _engine(p)
    full = _raw(kf, p, dphi, dq, 1)
    other = _raw(kf, p, dphi, dq, 1, time_major=True)
    for key in OUTPUTS:
        assert np.array_equal(full[key], other[key]), key
    for b in (0, 3, 4):
        sub, _ = _sub(p, [b])
        alone = _raw(_engine(sub), sub, dphi[[b]], dq[[b]], 1)
        for key in OUTPUTS:
            assert np.array_equal(alone[key][0], full[key][b]), (key, b)
    pair = dict(p, phi=p["phi"][:R_], q=p["q"][:R_], x0=p["x0"][:R_], P0=p["P0"][:R_])   # B = R: each record once
    two = _raw(kf, pair, dphi[:R_], dq[:R_], 1)
    for key in OUTPUTS:
        assert np.array_equal(two[key], full[key][:R_]), key


def test_invalid_model_in_the_batch():
    """A model with a negative observation variance among the records: its instances carry the status bit and NaN rows; the
    instances of the other record are bit-identical to the same call without it."""
    from metran_amd.engine import FLAG_NONPOSITIVE_F

    p = _data(8, 2, 17, seed=13, full=True, B=4)
    dphi, dq = _derivs(p, 13)
    keys = OUTPUTS + ("status",)
    good = _engine(p).scores(p["phi"], p["q"], dphi, dq, x0=p["x0"], P0=p["P0"])
    good = {k: _np(good[k]) for k in keys}
    assert not good["status"].any()
    q = dict(p, obsvar=p["obsvar"].copy())
    q["obsvar"][1, :] = -50.0
    bad = _engine(q).scores(p["phi"], p["q"], dphi, dq, x0=p["x0"], P0=p["P0"])
    bad = {k: _np(bad[k]) for k in keys}
    assert (bad["status"][[1, 3]] & FLAG_NONPOSITIVE_F).all() and not bad["status"][[0, 2]].any()
    for key in score_ref.OUTPUTS:
        assert np.isnan(bad[key][[1, 3]]).all(), key
    for key in OUTPUTS:
        assert np.array_equal(bad[key][[0, 2]], good[key][[0, 2]]), key


def test_refusals():
    """Every MK_ERR_INVALID case and MK_ERR_SHAPE at N + K = 65: refused before any launch -- the outputs keep their sentinel; a
    packed-symmetric engine is refused."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import MetranHipError, Problem, ScoresRequest
    from metran_amd.engine import BatchedKalman

    p = _data(8, 2, 17, seed=3, full=False, B=2, R=2)
    kf = _engine(p)
    L = _lib.lib()
    assert int(L.mk_scores_max_states()) == 64
    assert int(L.mk_scores_work_stride(61, 4)) == 0 and int(L.mk_scores_work_stride(60, 4)) == int(L.mk_record_stride(64)) + 60 * 66 + 60
    assert kf.scores_supported
    B = 2
    prob, keep, _ = kf._problem(kf._dev(p["phi"]), kf._dev(p["q"]), 0, None, None)
    buf = kf.alloc_scores(B)
    for key in score_ref.OUTPUTS:
        buf[key].fill_(7.5)
    d1 = torch.ones((B, 10), dtype=torch.float64, device="cuda")
    inputs = {"dphi": d1.data_ptr(), "dq": d1.data_ptr()}
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0   # an allocation of its own: its size is known exactly

    def call(work=buf["_work"].data_ptr(), t_first=1, problem=prob, request=True, **ptrs):
        req = ScoresRequest()
        req.t_first = t_first
        for key in ("dphi", "dq"):
            setattr(req, "d_" + key, ptrs.get(key, inputs[key]) or None)
        for key in OUTPUTS:
            setattr(req, "d_" + key, ptrs.get(key, buf[key].data_ptr()) or None)
        return L.mk_scores(kf._ctx, ctypes.byref(problem), ctypes.c_void_p(work) if work else None, 0, ctypes.byref(req) if request else None, None)

    try:
        assert call(request=False) == -1 and b"null mk_scores_request" in L.mk_last_error()
        assert call(work=None) == -1 and b"d_work" in L.mk_last_error()
        for key in ("dphi", "dq") + OUTPUTS:
            assert call(**{key: 0}) == -1 and b"required" in L.mk_last_error(), key
        assert call(t_first=-1) == -1 and b"t_first" in L.mk_last_error()
        assert call(work=small.value) == -1 and b"d_work" in L.mk_last_error()
        assert call(score=small.value) == -1 and b"d_score" in L.mk_last_error()
        assert call(opg=small.value) == -1 and b"d_opg" in L.mk_last_error()
        assert call(cusum=small.value) == -1 and b"d_cusum" in L.mk_last_error()
        assert call(dphi=small.value) == -1 and b"d_dphi" in L.mk_last_error()
        q = ctypes.c_void_p(buf["_work"].data_ptr())
        wide = Problem(1, 1, 4, 61, 4, 0, q, q, q, q, None, None, None, 0, None, None)
        assert call(problem=wide) == -2 and b"N=61, K=4" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    torch.cuda.synchronize()
    assert all((buf[key] == 7.5).all() for key in score_ref.OUTPUTS)
    assert call() == 0
    torch.cuda.synchronize()
    assert not (buf["opg"] == 7.5).any()
    with pytest.raises(ValueError):
        kf.scores(p["phi"], p["q"], np.ones((2, 10)), np.ones((2, 10)), t_first=-1)
    with pytest.raises(ValueError):
        kf.scores(p["phi"], p["q"], np.ones((2, 9)), np.ones((2, 10)))
    packed = BatchedKalman(0, packed_sym=True)
    packed.set_observations(p["obs"]).set_loadings(p["loadings"])
    assert not packed.scores_supported
    with pytest.raises(MetranHipError, match="MK_ERR_SHAPE"):
        packed.scores(p["phi"], p["q"], np.ones((2, 10)), np.ones((2, 10)))


def test_metran_batch_end_to_end():
    """Three small models through MetranBatch: solve(stderr=True), then the three covariances and the stability test.
    ``"hessian"`` is twice ``fit["pcov"]`` (the same differencing: equal to rounding); ``"opg"`` and ``"robust"`` are symmetric with
    a positive diagonal; the stability table has n + 1 rows per model and p-values in [0, 1]."""
    import pandas as pd

    from metran_amd.batch import MetranBatch
    from metran_amd.synthetic import make_dfm_batch

    T, N, K, R = 160, 3, 1, 3
    d = make_dfm_batch(R, N, K, T, seed=5, missing=0.2)
    idx = pd.date_range("2001-01-01", periods=T, freq="D")
    models = [[pd.Series(10.0 * (j + 1) + (1.0 + 0.5 * j) * d["obs"][r, :, j], index=idx, name="s%d" % j).dropna() for j in range(N)]
              for r in range(R)]
    mb = MetranBatch(models, factors=d["loadings"])
    fit = mb.solve(stderr=True)
    n = N + K
    cov = {kind: mb.get_parameter_covariance(kind) for kind in ("hessian", "opg", "robust")}
    pc = _np(fit["pcov"]) if hasattr(fit["pcov"], "detach") else np.asarray(fit["pcov"])
    assert cov["hessian"]["pcov"].shape == (R, n, n)
    assert np.all(np.abs(cov["hessian"]["pcov"] - 2.0 * pc) <= 1e-12 * np.abs(2.0 * pc).max(axis=(1, 2), keepdims=True))
    for kind in ("opg", "robust"):
        m = cov[kind]["pcov"]
        assert np.all(np.abs(m - m.transpose(0, 2, 1)) <= 1e-12 * np.abs(m).max(axis=(1, 2), keepdims=True)), kind
        assert (np.diagonal(m, axis1=1, axis2=2) > 0).all() and np.isfinite(cov[kind]["stderr"]).all(), kind
        assert np.allclose(np.diagonal(cov[kind]["corr"], axis1=1, axis2=2), 1.0)
    table = mb.test_parameter_stability()
    assert len(table) == R * (n + 1)
    assert ((table["pvalue"] >= 0) & (table["pvalue"] <= 1)).all() and (table["L"] >= 0).all() and (table["n_steps"] > 100).all()
    frame = mb.get_scores(1)
    assert frame.shape == (T, n) and list(frame.index) == list(idx)
