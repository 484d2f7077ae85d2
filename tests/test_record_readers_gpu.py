"""The plumbing the record readers share (C ABI mk_loo, mk_disturbances, mk_innovations, mk_forecast: the recording forward
pass into a workspace, then one kernel that reads its filtered records), per entry point: a buffer smaller than the call needs
is refused by name before any launch, a refusal writes nothing, and a second call into the same buffers (``buffers=``) gives the
first call's outputs bit for bit.  What the outputs ARE is the business of each entry point's own test file.

Shape: (N, K) = (2, 1), B = R = 2, T = 4 -- the work buffer needs 2 * 4 * 16 doubles, an output of the series 2 * 4 * 2 doubles =
128 bytes.  The undersized work buffer is an allocation of 128 bytes; the undersized output one of 64 bytes, because 128 bytes is
what a [2,4,2] output needs exactly.  Both are allocations of their own (mk_malloc): their sizes are known exactly."""
import ctypes

import numpy as np
import pytest

from metran_amd.synthetic import make_dfm_batch

pytestmark = pytest.mark.gpu

B, N, K, T, H = 2, 2, 1, 4, 8
SENTINEL, STATUS_SENTINEL = 777.0, 99

# entry point -> (allocator, method, keyword arguments of both, the output buffers in the order of the C arguments)
READERS = {
    "mk_loo": ("alloc_loo", "loo_predict", {}, ("loo_means", "loo_vars")),
    "mk_disturbances": ("alloc_disturbances", "disturbances", {}, ("r", "ninfo")),
    "mk_innovations": ("alloc_innovations", "innovations", {}, ("v", "f", "pred_mean", "pred_var")),
    "mk_forecast": ("alloc_forecast", "forecast", dict(horizon=H, outputs=("fan", "track", "skill")),
                    ("fan_mean", "fan_var", "track_mean", "track_var", "skill")),
}
# the name under which mk_last_error() reports the first output buffer
FIRST_OUTPUT = {"mk_loo": b"d_loo_means", "mk_disturbances": b"d_r", "mk_innovations": b"d_v", "mk_forecast": b"d_fan_means"}


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
    from metran_amd._lib import ForecastRequest

    L = _lib.lib()
    kf._bind_stream()
    if entry == "mk_forecast":
        req = ForecastRequest()
        req.horizon, req.t_first, req.track_horizon, req.coverage_z = H, 1, 1, 1.96
        req.d_fan_origins = None
        req.d_fan_means, req.d_fan_vars, req.d_track_means, req.d_track_vars, req.d_skill = outs
        rc = L.mk_forecast(kf._ctx, ctypes.byref(prob), work, 0, ctypes.byref(req), status)
    else:
        rc = getattr(L, entry)(kf._ctx, ctypes.byref(prob), work, 0, *outs, status)
    torch.cuda.synchronize()
    return rc, L.mk_last_error() or b""


@pytest.mark.parametrize("entry", sorted(READERS))
def test_undersized_buffers_are_refused_by_name_and_nothing_is_written(engine, entry):
    import torch

    from metran_amd import _lib

    kf, d = engine
    L = _lib.lib()
    alloc, _, kw, keys = READERS[entry]
    bufs = getattr(kf, alloc)(B, **kw)
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
    _, method, kw, keys = READERS[entry]
    first = getattr(kf, method)(d["phi"], d["q"], **kw)
    want = {k: first[k].detach().cpu().numpy().copy() for k in keys + ("status",)}
    assert all(np.isfinite(want[k]).any() for k in keys)   # the call computed something
    again = getattr(kf, method)(d["phi"], d["q"], buffers=first, **kw)
    assert again is first
    for k in keys:
        got = np.ascontiguousarray(again[k].detach().cpu().numpy())
        assert np.array_equal(got.view(np.int64), want[k].view(np.int64)), (entry, k)
    assert np.array_equal(again["status"].cpu().numpy(), want["status"]), entry
