"""Observation weights of smoothed series and states on the GPU (C ABI mk_observation_weights: the recording forward pass, the
gain tape written by innov_step_kernel, weights_walk_kernel) against the extended-precision numpy restatement
(tests/weights_ref.py, pinned to dense conditioning, the oracle and the reference by tests/test_weights_host.py), against an
independent kernel through the reconstruction identity, bit for bit across batches and numbers of targets, under both kernel
families and on a shape without specialised kernels, next to an invalid model, and the refusals of the raw ABI.

The bar is measured, not chosen: the largest difference between the float64 and the extended-precision restatement on the
inputs of ``test_against_restatement`` (every shape, length and target below, weights and intercepts), relative to
max(1, max |w|) of the target, is MEASURED = 4.04e-15 (scripts/measure_weights_bar.py prints it; at (7,7), T = 40); times 16 --
the kernel's tree-order sums differ from numpy's left-to-right order -- that is 6.5e-14, below the floor of 1e-13: BAR = 1e-13."""
import ctypes
import math

import numpy as np
import pytest

import weights_ref
from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

MEASURED = 4.04e-15
BAR = max(16 * MEASURED, 1e-13)
assert BAR == 1e-13
B_, R_ = 5, 2
# 16-lane groups up to n = 16 ((14,2) the last), one wavefront from n = 17 ((15,2) the first)
SHAPES = [(3, 1), (8, 2), (14, 2), (15, 2), (20, 2), (32, 4)]
LENGTHS = [1, 2, 17, 40]
CASES = [(N, K, "specialised") for N, K in SHAPES] + [(3, 1, "generic")]
UNSPECIALISED = (7, 7)   # no ahead-of-time or prebuilt module: the size-generic filter records for it


def _np(t):
    return t.detach().cpu().numpy()


def _plan(si, ti):
    """(time_major work buffer, observation variances and initial moments given) of shape number si at length number ti: every
    shape sees both settings of both, and so does every length."""
    return (si + ti) % 2 == 1, (si // 2 + ti) % 2 == 0


def _data(N, K, T, seed, full, B=B_, R=R_):
    """B instances on R records, 40 % missing.  From T = 17 on: step 5 empty, step 7 partly observed with (7, 0) observed and
    (7, 1) missing, on record 1 two leading empty steps and the last series never observed.  T = 1, 2: (0, 0) observed and
    (0, 1) missing, the last step of record 0 empty when T = 2, the last series of record 1 never observed."""
    d = make_dfm_batch(B, N, K, T, seed=seed, missing=0.4)
    obs = d["obs"][:R].copy()
    rng = np.random.default_rng(seed)
    n = N + K
    if T >= 17:
        obs[:, 5] = np.nan
        obs[:, 7, 0], obs[:, 7, 1] = 0.3, np.nan
        obs[:, T - 1, 1] = -0.45
        obs[1 % R, :2] = np.nan
    else:
        obs[:, 0, 0], obs[:, 0, 1] = 0.3, np.nan
        if T == 2:
            obs[0, 1] = np.nan
    obs[1 % R, :, N - 1] = np.nan
    p = dict(obs=obs, loadings=d["loadings"][:R], phi=d["phi"], q=d["q"], obsvar=None, x0=None, P0=None)
    if full:
        p["obsvar"] = rng.uniform(0.05, 0.4, (R, N)) * (rng.random((R, N)) < 0.6)
        p["x0"] = rng.normal(size=(B, n))
        A = rng.normal(size=(B, n, n))
        p["P0"] = A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n)
    return p


def _targets(p, what):
    """[R,M,2]: series -- an observed cell, a missing cell of a partly observed step, a cell of the empty step, t* = 0, t* = T - 1,
    the never-observed series (on record 1), an unused slot (step -1) and a column out of range; states -- a common factor, a
    specific state, an unused slot, a column out of range and a step out of range.  The last valid one sits at the end so that
    the groups of a wavefront differ in where their forward walk starts."""
    R, T, N = p["obs"].shape
    n = N + p["loadings"].shape[2]
    if what == "series":
        if T >= 17:
            tg = [(7, 0), (7, 1), (5, 2), (0, 0), (T - 1, 1), (9, N - 1), (-1, 0), (3, N), (T - 2, N - 1)]
        else:
            tg = [(0, 0), (0, 1), (T - 1, 2), (0, 0), (T - 1, 1), (0, N - 1), (-1, 0), (0, N), (T - 1, N - 1)]
    else:
        tm = T // 2
        tg = [(tm, N), (tm, 1), (-3, 0), (tm, n), (T, 0), (T - 1, n - 1)]
    return np.broadcast_to(np.array(tg, dtype=np.int64), (R, len(tg), 2)).copy()


def _engine(p, family="specialised"):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0)
    kf.set_observations(p["obs"]).set_loadings(p["loadings"], p["obsvar"])
    if family == "generic":
        kf.set_variant("kernel_family", family)
    return kf


def _sub(p, instances):
    """The problem of some instances alone, each on its own record."""
    R = p["obs"].shape[0]
    rec = [b % R for b in instances]
    pick = lambda a, i: None if a is None else a[i]   # noqa: E731
    return dict(obs=p["obs"][rec], loadings=p["loadings"][rec], obsvar=pick(p["obsvar"], rec), phi=p["phi"][instances], q=p["q"][instances],
                x0=pick(p["x0"], instances), P0=pick(p["P0"], instances)), rec


def _raw(kf, p, targets, what, time_major=False, intercept=True):
    """mk_observation_weights through the raw ABI (any B >= R): dict of numpy ``weights [B,M,T,N]``, ``intercept [B,M]``, ``status``."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem, WeightsRequest

    L = _lib.lib()
    R, T, N = p["obs"].shape
    K = p["loadings"].shape[2]
    B, M = p["phi"].shape[0], targets.shape[1]
    dev = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device="cuda")   # noqa: E731
    ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())   # noqa: E731
    t = {k: dev(p[k]) for k in ("obs", "phi", "q", "loadings", "obsvar", "x0", "P0")}
    prob = Problem(B, R, T, N, K, 0, ptr(t["obs"]), ptr(t["phi"]), ptr(t["q"]), ptr(t["loadings"]), ptr(t["obsvar"]), ptr(t["x0"]),
                   ptr(t["P0"]), 0, None, None)
    ws = int(L.mk_weights_work_stride(N, K))
    assert ws == int(L.mk_record_stride(N + K)) + N * ((N + K + 3) & ~1)
    work = torch.empty(B * T * ws, dtype=torch.float64, device="cuda")
    tg = torch.as_tensor(np.ascontiguousarray(targets), dtype=torch.int64, device="cuda")
    out = torch.full((B, M, T, N), 7.5, dtype=torch.float64, device="cuda")
    ic = torch.full((B, M), 7.5, dtype=torch.float64, device="cuda")
    status = torch.zeros(B, dtype=torch.int32, device="cuda")
    req = WeightsRequest()
    req.n_targets, req.what = M, {"series": 0, "states": 1}[what]
    req.d_targets, req.d_weights, req.d_intercept = tg.data_ptr(), out.data_ptr(), ic.data_ptr() if intercept else None
    kf._bind_stream()
    rc = L.mk_observation_weights(kf._ctx, ctypes.byref(prob), ptr(work), 1 if time_major else 0, ctypes.byref(req), ptr(status))
    assert rc == 0, L.mk_last_error()
    torch.cuda.synchronize()
    return {"weights": _np(out), "intercept": _np(ic), "status": _np(status)}


def _reference(p, b, targets, what, gain=None, dtype=np.longdouble):
    R = p["obs"].shape[0]
    r = b % R
    pick = lambda a, i: None if a is None else a[i]   # noqa: E731
    args = (p["obs"][r], p["phi"][b], p["q"][b], p["loadings"][r], pick(p["obsvar"], r), pick(p["x0"], b), pick(p["P0"], b))
    gain = gain if gain is not None else weights_ref.gains(*args, dtype=dtype)
    return weights_ref.weights(*args, targets=targets[r], what=what, dtype=dtype, gain=gain), gain


def _compared(N, K):
    return list(range(B_)) if N + K <= 16 else [0, 3]   # the restatement's extended-precision loops are what takes the time


def _check_case(N, K, T, family, time_major, full, seed):
    p = _data(N, K, T, seed, full)
    kf = _engine(p, family)
    if family == "unspecialised":
        assert not kf.specialised() and kf.observation_weights_supported
    gains = {}
    for what in ("series", "states"):
        tg = _targets(p, what)
        got = _raw(kf, p, tg, what, time_major)
        assert not got["status"].any()
        for b in _compared(N, K):
            (w, ic), gains[b] = _reference(p, b, tg, what, gains.get(b))
            seen = np.isfinite(p["obs"][b % R_])
            for m in range(tg.shape[1]):
                g, what_m = got["weights"][b, m], "%s target %s of instance %d" % (what, tuple(tg[b % R_, m]), b)
                if np.isnan(ic[m]):   # an unused slot, a column or a step out of range
                    assert np.isnan(g).all() and np.isnan(got["intercept"][b, m]), what_m
                    continue
                assert np.array_equal(np.isnan(g), ~seen), what_m             # NaN exactly at the cells that are not observed
                wm = w[m].astype(np.float64)
                bar = BAR * max(1.0, np.nanmax(np.abs(wm))) if seen.any() else BAR
                assert seen.sum() == 0 or np.nanmax(np.abs(g - wm)) <= bar, (what_m, float(np.nanmax(np.abs(g - wm))), bar)
                assert abs(got["intercept"][b, m] - float(ic[m])) <= bar, (what_m, got["intercept"][b, m], float(ic[m]))


@pytest.mark.parametrize("T", LENGTHS)
@pytest.mark.parametrize("case", CASES, ids=["%dx%d-%s" % c for c in CASES])
def test_against_restatement(case, T):
    """B = 5 instances on R = 2 records, series and state targets in one call each, through the raw ABI (the engine wants B a
    multiple of R)."""
    N, K, family = case
    si, ti = CASES.index(case), LENGTHS.index(T)
    time_major, full = _plan(si, ti)
    _check_case(N, K, T, family, time_major, full, seed=100 * N + T)


PER_RECORD_SHAPES = [(8, 2), (15, 2)]   # the 16-lane groups and the one-wavefront walk
PER_RECORD_T = 17


def _per_record_case(N, K):
    """B = 5 on R = 2 with target lists that differ between the two records in every slot: (problem, {what: targets [2,M,2]})."""
    T = PER_RECORD_T
    p = _data(N, K, T, seed=23 + N, full=True)
    n = N + K
    tg = {"series": np.array([[(7, 0), (5, 2), (0, 0), (T - 1, 1)], [(9, 3), (2, 1), (T - 1, 0), (3, 2)]], dtype=np.int64),
          "states": np.array([[(8, N), (8, 1)], [(3, n - 1), (12, 0)]], dtype=np.int64)}
    return p, tg


def _other_records_list(p, b, tg, what):
    """What instance b would get from the OTHER record's target list (on its own record and parameters): a kernel that reads
    one list for every record returns this for the instances of one of the two."""
    return _reference(p, b, tg[::-1], what)[0]


@pytest.mark.parametrize("shape", PER_RECORD_SHAPES, ids=["%dx%d" % s for s in PER_RECORD_SHAPES])
def test_every_record_has_its_own_target_list(shape):
    """weights_walk_kernel reads targets[(rec * M + m) * 2]: the other tests hand it ONE list broadcast to the records.  Here the
    two records' lists differ, every instance is compared at BAR with the restatement on ITS record's list, and is more than
    1000 BAR from what the other record's list gives (tests/test_weights_host.py shows that of the restatement itself)."""
    N, K = shape
    p, tgs = _per_record_case(N, K)
    kf = _engine(p)
    for what, tg in tgs.items():
        got = _raw(kf, p, tg, what, time_major=(what == "states"))
        assert not got["status"].any()
        for b in range(B_):
            (w, ic), _ = _reference(p, b, tg, what)
            wo, io = _other_records_list(p, b, tg, what)
            seen = np.isfinite(p["obs"][b % R_])
            for m in range(tg.shape[1]):
                g, what_m = got["weights"][b, m], "%s target %s of instance %d" % (what, tuple(tg[b % R_, m]), b)
                assert np.array_equal(np.isnan(g), ~seen), what_m
                wm = w[m].astype(np.float64)
                bar = BAR * max(1.0, np.nanmax(np.abs(wm)))
                assert np.nanmax(np.abs(g - wm)) <= bar and abs(got["intercept"][b, m] - float(ic[m])) <= bar, what_m
                assert np.nanmax(np.abs(g - wo[m].astype(np.float64))) > 1000 * bar, what_m


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
    time_major, full = _plan(len(CASES), LENGTHS.index(T))
    _check_case(N, K, T, "unspecialised", time_major, full, seed=100 * N + T)


@pytest.mark.parametrize("shape", [(8, 2), (32, 4)], ids=["8x2-records", "32x4-tape"])
def test_identity_against_the_projecting_smoother(shape):
    """sum w y + intercept, summed on the host with math.fsum, is simulate_smoothed's unscaled mean at the target -- an independent
    kernel (the record route at (8,2), the tape route at (32,4)); through the engine, B = 4 on R = 2."""
    N, K = shape
    T = 40
    p = _data(N, K, T, seed=41 + N, full=True, B=4)
    kf = _engine(p)
    assert bool(kf.tape_path()) == (shape == (32, 4))
    tg = _targets(p, "series")
    sim = _np(kf.simulate_smoothed(p["phi"], p["q"], x0=p["x0"], P0=p["P0"])["sim_means"])
    res = kf.observation_weights(p["phi"], p["q"], tg, "series", x0=p["x0"], P0=p["P0"])
    assert set(res) == {"_work", "weights", "intercept", "status"} and not _np(res["status"]).any()
    w, ic = _np(res["weights"]), _np(res["intercept"])
    raw = _raw(kf, p, tg, "series")
    assert np.array_equal(raw["weights"], w, equal_nan=True) and np.array_equal(raw["intercept"], ic, equal_nan=True)
    for b in range(4):
        y = p["obs"][b % R_]
        seen = np.isfinite(y)
        for m, (ts, col) in enumerate(tg[b % R_]):
            if not (0 <= ts < T and 0 <= col < N):
                continue
            terms = (w[b, m][seen] * y[seen]).tolist()
            total = math.fsum(terms + [ic[b, m]])
            bar = BAR * max(1.0, np.abs(w[b, m][seen]).max()) + 1e-12 * math.fsum(abs(v) for v in terms)
            assert abs(total - sim[b, ts, col]) <= bar, (b, m, total, sim[b, ts, col], bar)


@pytest.mark.parametrize("shape", [(3, 1), (15, 2)], ids=["3x1", "15x2"])
def test_an_observed_cell_without_observation_noise_is_its_own_observation(shape):
    """R = 0: the smoothed projection at an observed cell is the observation -- its own weight 1, every other weight and the
    intercept 0."""
    N, K = shape
    p = _data(N, K, 17, seed=5, full=True)
    p["obsvar"] = None
    tg = np.broadcast_to(np.array([(7, 0), (16, 1), (0, 0)], dtype=np.int64), (R_, 3, 2)).copy()
    p["obs"][:, 0, 0] = 0.8
    got = _raw(_engine(p), p, tg, "series", time_major=True)
    for b in range(B_):
        for m, (ts, col) in enumerate(tg[b % R_]):
            want = np.where(np.isfinite(p["obs"][b % R_]), 0.0, np.nan)
            want[ts, col] = 1.0
            np.testing.assert_allclose(got["weights"][b, m], want, rtol=0, atol=BAR, equal_nan=True)
            assert abs(got["intercept"][b, m]) <= BAR


@pytest.mark.parametrize("shape", [(8, 2), (20, 2)], ids=["8x2", "20x2"])
def test_batch_independence(shape):
    """An instance's weights are bit-identical alone and inside the batch of five, and with M = 1 and inside M = 7."""
    N, K = shape
    p = _data(N, K, 17, seed=9, full=True)
    kf = _engine(p)
    for what in ("series", "states"):
        tg = _targets(p, what)
        tg = np.concatenate([tg, tg], axis=1)[:, :7]   # M = 7: the unused slot among them (series), a repeated target (states)
        full = _raw(kf, p, tg, what)
        for b in (0, 3, 4):
            sub, rec = _sub(p, [b])
            alone = _raw(_engine(sub), sub, tg[rec], what)
            assert np.array_equal(alone["weights"][0], full["weights"][b], equal_nan=True), (what, b)
            assert np.array_equal(alone["intercept"][0], full["intercept"][b], equal_nan=True), (what, b)
        for m in (0, 4, 6):
            one = _raw(kf, p, tg[:, m:m + 1], what, time_major=True)
            assert np.array_equal(one["weights"][:, 0], full["weights"][:, m], equal_nan=True), (what, m)
            assert np.array_equal(one["intercept"][:, 0], full["intercept"][:, m], equal_nan=True), (what, m)
    # without the intercept: the weights are the same
    none = _raw(kf, p, tg, what, intercept=False)
    assert np.array_equal(none["weights"], full["weights"], equal_nan=True) and (none["intercept"] == 7.5).all()


def test_invalid_model_in_the_batch():
    """One instance with negative q among five (16-lane groups: its targets share wavefronts with its neighbours'): its status
    bit is set and its rows are NaN; the neighbours are bit-identical to the same call without it."""
    from metran_amd.engine import FLAG_NONPOSITIVE_F

    p = _data(8, 2, 17, seed=13, full=True, B=5, R=1)
    tg = _targets(p, "series")
    kf = _engine(p)
    good = kf.observation_weights(p["phi"], p["q"], tg, "series", x0=p["x0"], P0=p["P0"])
    good = {k: _np(good[k]) for k in ("weights", "intercept", "status")}
    assert not good["status"].any()
    q = p["q"].copy()
    q[2] = -5.0
    bad = kf.observation_weights(p["phi"], q, tg, "series", x0=p["x0"], P0=p["P0"])
    bad = {k: _np(bad[k]) for k in ("weights", "intercept", "status")}
    assert bad["status"][2] & FLAG_NONPOSITIVE_F and not np.delete(bad["status"], 2).any()
    assert np.isnan(bad["weights"][2]).all() and np.isnan(bad["intercept"][2]).all()
    for k in ("weights", "intercept"):
        assert np.array_equal(np.delete(bad[k], 2, axis=0), np.delete(good[k], 2, axis=0), equal_nan=True), k


def test_refusals():
    """Every MK_ERR_INVALID case and MK_ERR_SHAPE at N + K = 65: refused before any launch -- the outputs keep their sentinel."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem, WeightsRequest

    p = _data(8, 2, 17, seed=3, full=False, B=2, R=2)
    kf = _engine(p)
    L = _lib.lib()
    assert int(L.mk_weights_work_stride(61, 4)) == 0 and int(L.mk_weights_work_stride(60, 4)) == int(L.mk_record_stride(64)) + 60 * 66
    assert kf.observation_weights_supported
    B, T, N, M = 2, 17, 8, 3
    prob, keep, _ = kf._problem(kf._dev(p["phi"]), kf._dev(p["q"]), 0, None, None)
    buf = kf.alloc_observation_weights(B, M)
    buf["weights"].fill_(7.5)
    buf["intercept"].fill_(7.5)
    tg = torch.zeros((2, M, 2), dtype=torch.int64, device="cuda")
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0   # an allocation of its own: its size is known exactly

    def call(work=buf["_work"].data_ptr(), targets=tg.data_ptr(), weights=buf["weights"].data_ptr(), intercept=buf["intercept"].data_ptr(),
             n_targets=M, what=0, problem=prob):
        req = WeightsRequest()
        req.n_targets, req.what, req.d_targets, req.d_weights, req.d_intercept = n_targets, what, targets, weights, intercept
        return L.mk_observation_weights(kf._ctx, ctypes.byref(problem), ctypes.c_void_p(work) if work else None, 0, ctypes.byref(req), None)

    try:
        assert call(work=None) == -1 and b"d_work" in L.mk_last_error()
        assert call(targets=None) == -1 and b"d_targets" in L.mk_last_error()
        assert call(weights=None) == -1 and b"d_weights" in L.mk_last_error()
        assert call(n_targets=0) == -1 and b"n_targets" in L.mk_last_error()
        assert call(what=2) == -1 and call(what=-1) == -1 and b"MK_DRAW_SERIES" in L.mk_last_error()
        assert call(work=small.value) == -1 and b"d_work" in L.mk_last_error()
        assert call(targets=small.value, n_targets=9) == -1 and b"d_targets" in L.mk_last_error()
        assert call(weights=small.value) == -1 and b"d_weights" in L.mk_last_error()
        assert call(intercept=small.value, n_targets=17) == -1   # 2 * 17 doubles do not fit into 128 bytes (nor do the other buffers)
        q = ctypes.c_void_p(buf["_work"].data_ptr())
        wide = Problem(1, 1, 4, 61, 4, 0, q, q, q, q, None, None, None, 0, None, None)
        assert call(problem=wide) == -2 and b"N=61, K=4" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    torch.cuda.synchronize()
    assert (buf["weights"] == 7.5).all() and (buf["intercept"] == 7.5).all()
    assert call() == 0                                           # ... and the same call, complete, runs
    torch.cuda.synchronize()
    assert not (buf["weights"] == 7.5).any()
    with pytest.raises(ValueError):
        kf.observation_weights(p["phi"], p["q"], tg, "level")
    with pytest.raises(ValueError):
        kf.observation_weights(p["phi"], p["q"], np.zeros((3, 2, 2), dtype=np.int64))
    with pytest.raises(ValueError):
        kf.alloc_observation_weights(2, 0)


def test_metran_batch_end_to_end():
    """Through MetranBatch (the weights of one model run on a sub-engine of that model): the weights of a gap-filled value, in
    original units, rebuild ``get_simulation``'s mean there from the observations -- an independent kernel, the projecting
    smoother with its scaling -- and the shares of a time add up to 1."""
    import pandas as pd

    from metran_amd.batch import MetranBatch

    rng = np.random.default_rng(4)
    idx = pd.date_range("2001-01-01", periods=60, freq="D")
    models = []
    for r in range(2):
        cols = []
        for j in range(3):
            s = pd.Series(10.0 * (j + 1) + (2.0 + j) * np.cumsum(rng.normal(size=60)) / 3.0, index=idx, name="s%d" % j)
            cols.append(s[rng.random(60) > 0.3])
        models.append(cols if r == 0 else [c[c.index < idx[50]] for c in cols])
    G = np.broadcast_to(np.array([[0.6], [0.5], [-0.4]]), (2, 3, 1)).copy()
    mb = MetranBatch(models, factors=G)
    astar = np.array([[8.0, 6.0, 9.0, 12.0], [5.0, 7.0, 8.0, 10.0]])
    obs, std, mean = _np(mb.kf.obs), _np(mb._std), _np(mb._mean)
    for r, name in ((1, "s2"), (0, "s0")):
        j = mb._series(r, name)
        L = int(mb.batch.lengths[r])
        index = mb.batch.index[r]
        gap = int(np.nonzero(~np.isfinite(obs[r, 5:L, j]))[0][0]) + 5
        sim = mb.get_simulation(r, name, alpha=astar, ci=None)
        frames = mb.get_observation_weights(r, name, [index[gap], L - 1], alpha=astar)
        y = obs[r, :L] * std[r] + mean[r]
        for s in (gap, L - 1):
            f = frames[index[s]]
            assert f.shape == (L, 3) and np.array_equal(np.isnan(f.values), ~np.isfinite(obs[r, :L]))
            seen = np.isfinite(y)
            terms = (f.values[seen] * (y[seen] - np.broadcast_to(mean[r], y.shape)[seen])).tolist()
            total = math.fsum(terms + [mean[r, j], f.attrs["intercept"]])
            bar = (BAR * max(1.0, np.abs(f.values[seen]).max()) + 1e-12 * math.fsum(abs(v) for v in terms)) * max(1.0, std[r].max() / std[r].min())
            assert abs(total - sim.iloc[s]) <= bar + 1e-12 * abs(sim.iloc[s]), (r, s, total, sim.iloc[s], bar)
        sh = mb.get_weight_shares(r, name, [index[gap]], alpha=astar)
        assert abs(sh["share"].sum() - 1.0) <= 1e-14 and (sh["first"] <= index[gap]).all() and (sh["last"] >= index[gap]).all()
        sw = mb.get_state_weights(r, 3, [gap], alpha=astar)[index[gap]]
        assert sw.shape == (L, 3) and np.isfinite(sw.values[np.isfinite(obs[r, :L])]).all()
