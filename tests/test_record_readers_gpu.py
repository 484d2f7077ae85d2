"""The plumbing the record readers share (C ABI mk_loo, mk_disturbances, mk_innovations, mk_forecast, mk_observation_weights,
mk_regression, mk_scores, mk_functionals: the recording forward pass into a workspace, then kernels that read its filtered
records), per entry point: a buffer smaller than the call needs is refused by name before any launch, a refusal writes nothing, a
second call into the same buffers (``buffers=``) gives the first call's outputs bit for bit, and the engine refuses a caller's
buffer of the wrong dtype, device or shape, or a missing one, by its key before anything is launched.  What the outputs ARE is the
business of each entry point's own test file.

Shape: (N, K) = (2, 1), B = R = 2, T = 4 -- the work buffer needs at least 2 * 4 * 16 doubles, an output of the series 2 * 4 * 2
doubles = 128 bytes.  The undersized work buffer is an allocation of 128 bytes; the undersized output one of 64 bytes, because
128 bytes is what a [2,4,2] output needs exactly -- and with M = 1 target, M = 5 effects and W = 3 windows of the N unit contrasts
the first outputs of the four request-struct readers need 128, 80, 192 and 96 bytes.  Both are allocations of their own
(mk_malloc): their sizes are known exactly."""
import ctypes

import numpy as np
import pytest

from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

B, N, K, T, H = 2, 2, 1, 4, 8
SENTINEL, STATUS_SENTINEL = 777.0, 99
TARGETS = [[1, 0]]                                                                          # M = 1: (step, series)
EFFECTS = [[0, 0, 1, 2], [1, 0, 2, 3], [0, 1, 1, 4], [1, 0, 0, 1], [0, 0, 3, 4]]            # M = 5: (series, kind, t0, t1)
WINDOWS = [[0, 2, 2, 2], [1, 2, 2, 2], [0, 2, 2, 4]]                                        # W = 3: (t0, t1, t2, t3)
TANGENT = np.ones((B, N + K))

# entry point -> (allocator, its arguments after B, method, its keyword arguments, the output buffers in the order of the C
# arguments or of the request struct's fields)
READERS = {
    "mk_loo": ("alloc_loo", {}, "loo_predict", {}, ("loo_means", "loo_vars")),
    "mk_disturbances": ("alloc_disturbances", {}, "disturbances", {}, ("r", "ninfo")),
    "mk_innovations": ("alloc_innovations", {}, "innovations", {}, ("v", "f", "pred_mean", "pred_var")),
    "mk_forecast": ("alloc_forecast", dict(horizon=H, outputs=("fan", "track", "skill")), "forecast",
                    dict(horizon=H, outputs=("fan", "track", "skill")), ("fan_mean", "fan_var", "track_mean", "track_var", "skill")),
    "mk_observation_weights": ("alloc_observation_weights", dict(M=len(TARGETS)), "observation_weights", dict(targets=TARGETS),
                               ("weights", "intercept")),
    "mk_regression": ("alloc_regression", dict(M=len(EFFECTS)), "regression", dict(effects=EFFECTS),
                      ("beta", "cov", "gain", "normal", "support", "dropped")),
    "mk_scores": ("alloc_scores", {}, "scores", dict(dphi=TANGENT, dq=TANGENT), ("score", "grad", "count", "opg", "cusum")),
    "mk_functionals": ("alloc_functionals", dict(W=len(WINDOWS), C=N), "functionals", dict(windows=WINDOWS), ("mean", "var")),
}
# the name under which mk_last_error() reports the first output buffer
FIRST_OUTPUT = {"mk_loo": b"d_loo_means", "mk_disturbances": b"d_r", "mk_innovations": b"d_v", "mk_forecast": b"d_fan_means",
                "mk_observation_weights": b"d_weights", "mk_regression": b"d_beta", "mk_scores": b"d_score", "mk_functionals": b"d_mean"}


@pytest.fixture(scope="module")
def engine():
    from metran_amd.engine import BatchedKalman

    d = make_dfm_batch(B, N, K, T, seed=11, missing=0.2)
    kf = BatchedKalman(0)
    kf.set_observations(d["obs"]).set_loadings(d["loadings"], None)
    return kf, d


def _raw_call(kf, entry, prob, work, outs, status):
    """The entry point through the raw ABI on device addresses: (return code, mk_last_error())."""
    import torch

    from metran_amd import _lib

    L = _lib.lib()
    kf._bind_stream()

    def table(rows, dtype=torch.int64):   # one table per record, on the device
        return torch.as_tensor(np.asarray(rows), dtype=dtype)[None].repeat(B, 1, 1).cuda()

    specific, keep = list(outs), None
    if entry == "mk_forecast":
        req = _lib.ForecastRequest()
        req.horizon, req.t_first, req.track_horizon, req.coverage_z = H, 1, 1, 1.96
        req.d_fan_origins = None
        req.d_fan_means, req.d_fan_vars, req.d_track_means, req.d_track_vars, req.d_skill = outs
        specific = [ctypes.byref(req)]
    elif entry == "mk_observation_weights":
        req, keep = _lib.WeightsRequest(), table(TARGETS)
        req.n_targets, req.what, req.d_targets = len(TARGETS), 0, keep.data_ptr()
        req.d_weights, req.d_intercept = outs
        specific = [ctypes.byref(req)]
    elif entry == "mk_regression":
        req, keep = _lib.RegressionRequest(), table(EFFECTS)
        req.n_effects, req.t_first, req.d_effects = len(EFFECTS), 1, keep.data_ptr()
        req.d_beta, req.d_cov, req.d_gain, req.d_normal, req.d_support, req.d_dropped = outs
        specific = [ctypes.byref(req)]
    elif entry == "mk_scores":
        req, keep = _lib.ScoresRequest(), torch.as_tensor(TANGENT).cuda()
        req.d_dphi, req.d_dq, req.t_first = keep.data_ptr(), keep.data_ptr(), 1
        req.d_score, req.d_grad, req.d_count, req.d_opg, req.d_cusum = outs
        specific = [ctypes.byref(req)]
    elif entry == "mk_functionals":
        req, keep = _lib.FunctionalRequest(), table(WINDOWS)
        req.n_windows, req.n_contrasts, req.d_windows, req.d_contrasts = len(WINDOWS), N, keep.data_ptr(), None
        specific = [ctypes.byref(req)] + list(outs)
    rc = getattr(L, entry)(kf._ctx, ctypes.byref(prob), work, 0, *specific, status)
    torch.cuda.synchronize()
    return rc, L.mk_last_error() or b""


@pytest.mark.parametrize("entry", sorted(READERS))
def test_undersized_buffers_are_refused_by_name_and_nothing_is_written(engine, entry):
    import torch

    from metran_amd import _lib

    kf, d = engine
    L = _lib.lib()
    alloc, akw, _, _, keys = READERS[entry]
    bufs = getattr(kf, alloc)(B, **akw)
    prob, keep, _ = kf._problem(kf._dev(d["phi"]), kf._dev(d["q"]), 0, None, None)
    status = torch.full((B,), STATUS_SENTINEL, dtype=torch.int32, device="cuda")
    tensors = [bufs[k] for k in keys + ("_work",)]
    for t in tensors:
        t.fill_(SENTINEL)
    assert bufs["_work"].numel() * 8 > 128 and bufs[keys[0]].numel() * 8 > 64   # the two small allocations ARE too small
    outs = [bufs[k].data_ptr() for k in keys]

    def untouched(what):
        for t in tensors:
            assert bool((t == SENTINEL).all().item()), what
        assert bool((status == STATUS_SENTINEL).all().item()), what

    small_work, small_out = ctypes.c_void_p(), ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small_work)) == 0
    assert L.mk_malloc(kf._ctx, 64, ctypes.byref(small_out)) == 0
    try:
        rc, msg = _raw_call(kf, entry, prob, small_work.value, outs, status.data_ptr())
        assert rc == -1 and b"d_work" in msg and entry.encode() in msg, (rc, msg)   # MK_ERR_INVALID
        untouched("undersized work buffer")
        rc, msg = _raw_call(kf, entry, prob, bufs["_work"].data_ptr(), [small_out.value] + outs[1:], status.data_ptr())
        assert rc == -1 and FIRST_OUTPUT[entry] in msg and entry.encode() in msg, (rc, msg)
        untouched("undersized first output")
    finally:
        L.mk_free(kf._ctx, small_work)
        L.mk_free(kf._ctx, small_out)


@pytest.mark.parametrize("entry", sorted(READERS))
def test_a_second_call_into_the_same_buffers_is_bit_equal(engine, entry):
    kf, d = engine
    _, _, method, kw, keys = READERS[entry]
    first = getattr(kf, method)(d["phi"], d["q"], **kw)
    want = {k: first[k].detach().cpu().numpy().copy() for k in keys + ("status",)}
    assert all(np.isfinite(want[k]).any() for k in keys)   # the call computed something
    again = getattr(kf, method)(d["phi"], d["q"], buffers=first, **kw)
    assert again is first
    for k in keys:
        got = np.ascontiguousarray(again[k].detach().cpu().numpy())
        assert np.array_equal(got.view(np.int64), want[k].view(np.int64)), (entry, k)
    assert np.array_equal(again["status"].cpu().numpy(), want["status"]), entry


@pytest.mark.parametrize("entry", sorted(READERS))
def test_a_wrong_buffer_is_refused_by_its_key_and_nothing_is_written(engine, entry):
    """A caller's buffer of the wrong dtype or on the wrong device, a ``status`` of the wrong shape and a missing ``status``: each
    is a ValueError that names the key and the allocator, raised before the stream is bound or anything is launched."""
    import torch

    kf, d = engine
    alloc, akw, method, kw, keys = READERS[entry]

    def spoil(bufs, case):
        t = bufs[keys[0]]
        if case == "float32":
            bufs[keys[0]] = torch.empty_like(t, dtype=torch.float32)
        elif case == "on the CPU":
            bufs[keys[0]] = torch.empty(tuple(t.shape), dtype=torch.float64)
        elif case == "status of the wrong shape":
            bufs["status"] = torch.zeros(B + 1, dtype=torch.int32, device="cuda")
        else:
            del bufs["status"]
        return keys[0] if case in ("float32", "on the CPU") else "status"

    for case in ("float32", "on the CPU", "status of the wrong shape", "no status"):
        bufs = getattr(kf, alloc)(B, **akw)
        for t in bufs.values():
            t.fill_(SENTINEL)
        key = spoil(bufs, case)
        others = [t for k, t in bufs.items() if k != key]
        with pytest.raises(ValueError) as err:
            getattr(kf, method)(d["phi"], d["q"], buffers=bufs, **kw)
        assert repr(key) in str(err.value) and alloc in str(err.value), (entry, case, str(err.value))
        torch.cuda.synchronize()
        for t in others:
            assert bool((t == SENTINEL).all().item()), (entry, case)
