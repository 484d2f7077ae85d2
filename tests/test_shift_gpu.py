"""The level-shift scan on the GPU (C ABI mk_level_shifts: the recording forward pass, the gain tape and the innovations written
by innov_step_kernel, shift_scan_kernel) against the DEFINITION in extended precision (tests/shift_ref.py: the dense precision of
the record's data vector; pinned to the restatement and to the regression by tests/test_shift_host.py), against independent
kernels (regression with one level effect, loo_predict at the last observed cell of a series), bit for bit across batches, layouts
and slots of a wavefront, under both kernel families, next to an invalid model, into prefilled buffers, the refusals of the raw
ABI, and ``MetranBatch.detect_level_shifts`` end to end on the planted-shift batch of the host tier.

The bar against the definition (shift_ref.bars): 4 * MU * eps * scale + 1e-12, scale = |x|'|u| for A and |x|'|M||x| for D, and
MU = shift_ref.MU the largest (float64 restatement - definition) / (eps * scale) over every group, instance and candidate of this
tier, measured on the CPU by tests/test_shift_host.py::test_restatement_against_definition: mu = 1288 ((8,2), T = 2), MU = 1300;
the two groups this tier adds at T = 5 measure 4263 and have MU = 4300 of their own.  Every test prints the kernel's largest
distance in units of the bar; on an MI355X it is 0.0092 of the bar among the groups at MU = 1300 ((8,2), T = 3; 0.0057 at (8,2),
T = 2, 0.0039 at (5,1), T = 70 and (13,4), T = 17, below 0.0031 elsewhere; the same under both layouts), 0.129 at (60,4), T = 5 and
0.017 at (15,1), T = 5 with their own MU, 0.037 at the (13,4) twin of the status case; against the level regression at most
0.022 of that tier's bar."""
import ctypes

import numpy as np
import pytest

import call_forms as cf
import shift_ref as sr
import status_cases as sc

pytestmark = pytest.mark.gpu

LAYOUTS = ("model_major", "time_major")
CASES = [(N, K, T, "specialised") for N, K, T in sr.GROUPS] + [(8, 2, 17, "generic")]
IDS = ["%dx%d-T%d-%s" % c for c in CASES]
OUTPUTS = ("num", "den")
SENTINEL = 7.5
LEVEL = 0


def _np(t):
    return t.detach().cpu().numpy()


def _engine(g, layout="model_major", family="specialised"):
    from metran_amd.engine import BatchedKalman

    kf = BatchedKalman(0, layout=layout)
    kf.set_observations(g["obs"]).set_loadings(g["loadings"], g["obsvar"])
    if g["scale"] is not None:
        kf.set_scaling(g["scale"], g["offset"])
    if family == "generic":
        kf.set_variant("kernel_family", family)
    return kf


def _call(kf, g, **kw):
    res = kf.level_shifts(g["phi"], g["q"], **cf.init(g), **kw)
    return {k: _np(res[k]).copy() for k in OUTPUTS + ("status",)}


def _compare(g, got, what, instances=None):
    """Every instance against the definition; returns the largest distance in bars."""
    worst = 0.0
    for i in (range(g["B"]) if instances is None else instances):
        d = sr.distance({k: got[k][i] for k in OUTPUTS}, sr.definition(g, i))
        assert d <= 1.0, "%s: instance %d is %.3g bars from the definition" % (what, i, d)
        worst = max(worst, d)
    return worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_definition(case, layout):
    N, K, T, family = case
    g = sr.group(N, K, T)
    kf = _engine(g, layout, family)
    assert kf.level_shifts_supported
    got = _call(kf, g)
    assert not got["status"].any()
    worst = _compare(g, got, "(%d,%d) T=%d %s %s" % (N, K, T, family, layout))
    print("(%d,%d) T=%d %s %s: %.3g of the bar" % (N, K, T, family, layout, worst))


def _candidates(g, r, count=4):
    """A handful of observed cells (t, j) of record r: the first and the last of the record and cells spread between them."""
    cells = np.argwhere(np.isfinite(g["obs"][r]))
    if len(cells) == 0:
        return []
    pick = sorted({int(round(x)) for x in np.linspace(0, len(cells) - 1, count)})
    return [tuple(int(v) for v in cells[p]) for p in pick]


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "specialised"], ids=lambda c: "%dx%d-T%d" % c[:3])
def test_against_level_regression(case):
    """Independent kernels: regression with the single effect (j, level, tau, T) and t_first = 0 gives beta = A / D, cov = 1 / D
    and gain = A^2 / D, for a handful of candidates per record, at the regression tier's bar."""
    from test_regression_gpu import BAR_S

    N, K, T, _ = case
    g = sr.group(N, K, T)
    kf = _engine(g)
    got = _call(kf, g)
    picks = [_candidates(g, r) for r in range(g["R"])]
    worst, seen = 0.0, 0
    for c in range(max(len(p) for p in picks)):
        ef = np.full((g["R"], 1, 4), -1, dtype=np.int64)
        ef[:, :, 1:] = (0, 0, 1)
        for r, p in enumerate(picks):
            if c < len(p):
                ef[r, 0] = (p[c][1], LEVEL, p[c][0], T)
        reg = kf.regression(g["phi"], g["q"], ef, t_first=0, **cf.init(g))
        beta, cov, gain = _np(reg["beta"]), _np(reg["cov"]), _np(reg["gain"])
        for i in range(g["B"]):
            r = i % g["R"]
            if c >= len(picks[r]):
                continue
            t, j = picks[r][c]
            A, D = got["num"][i, t, j], got["den"][i, t, j]
            pairs = ((A / D, beta[i, 0]), (1 / D, cov[i, 0, 0]), (A * A / D, gain[i]))
            dist = max(abs(a - b) / max(1.0, abs(b)) for a, b in pairs) / BAR_S
            assert dist <= 1.0, (i, t, j, pairs)
            worst, seen = max(worst, dist), seen + 1
    assert seen >= g["S"]
    print("(%d,%d) T=%d: %.3g of the bar against the level regression" % (N, K, T, worst))


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "specialised" and cf.has_loo(c[0], c[1])], ids=lambda c: "%dx%d-T%d" % c[:3])
def test_last_cell_is_loo(case):
    """Independent kernels: at the LAST observed cell s of a series the regressor is a pulse, A = u_s and D = M_ss, and
    y_s - E[y_s | the rest] = u_s / M_ss, Var[y_s | the rest] = 1 / M_ss: A / D is the observation MINUS the leave-one-out mean
    (positive where the series reads above its prediction) and 1 / D the leave-one-out variance plus the observation variance,
    in the units the filter runs on.  The bar: the LOO tier's own (1e-12 * big, 1e-12 * big^2, caller's units) plus the scan's bar
    carried through A / D and 1 / D."""
    N, K, T, _ = case
    g = sr.group(N, K, T)
    kf = _engine(g)
    got = _call(kf, g)
    loo = kf.loo_predict(g["phi"], g["q"], **cf.init(g))
    lm, lv = _np(loo["loo_means"]), _np(loo["loo_vars"])
    seen = 0
    for i in range(g["B"]):
        r = i % g["R"]
        ref = sr.definition(g, i)
        bar = sr.bars(ref)
        big = max(1.0, float(np.nanmax(np.abs(lm[i])))) if np.isfinite(lm[i]).any() else 1.0
        for j in range(N):
            steps = np.nonzero(np.isfinite(g["obs"][r, :, j]))[0]
            if len(steps) == 0:
                continue
            t = int(steps[-1])
            A, D = got["num"][i, t, j], got["den"][i, t, j]
            s_, of, Rv = g["scale"][r, j], g["offset"][r, j], g["obsvar"][r, j]
            slack_e = (bar["num"][t, j] + abs(A) / D * bar["den"][t, j]) / D
            slack_v = bar["den"][t, j] / (D * D)
            resid = (g["obs"][r, t, j] * s_ + of - lm[i, t, j]) / s_        # observation minus leave-one-out mean, filter's units
            assert abs(A / D - resid) <= cf.LOO_TOL * big / s_ + slack_e, (i, t, j, A / D, resid)
            if lv[i, t, j] > 0:                                            # a variance that rounding took below zero is stored as 0
                assert abs(1 / D - (lv[i, t, j] / s_ ** 2 + Rv)) <= cf.LOO_TOL * big * big / s_ ** 2 + slack_v, (i, t, j)
            seen += 1
    assert seen >= g["S"]


def _moved(g):
    """The group with its parameter sets rotated by one: instance i at position (i + R) % B, another slot of its wavefront
    (R = 3 against groups of four and of one instance per wavefront), on the same record."""
    perm = (np.arange(g["B"]) - g["R"]) % g["B"]
    return cf.variant(g, **{k: g[k][perm] for k in ("phi", "q", "x0", "P0")}), perm


@pytest.mark.parametrize("case", [(8, 2, 17, "specialised"), (15, 1, 5, "specialised"), (13, 4, 17, "specialised"), (60, 4, 5, "specialised"),
                                  (8, 2, 33, "specialised"), (8, 2, 17, "generic")], ids=lambda c: "%dx%d-T%d-%s" % c)
def test_bit_for_bit(case):
    """The 15-instance call equals the five 3-instance calls; both layouts agree; an instance moved to another slot of its
    wavefront keeps its numbers."""
    N, K, T, family = case
    g = sr.group(N, K, T)
    engines = {}

    def fn(grp):
        key = grp["B"]
        if key not in engines:
            engines[key] = _engine(grp, "model_major", family)
        out = _call(engines[key], grp)
        return {k: out[k] for k in OUTPUTS}

    cf.check_position_independent(fn, g, "level_shifts")
    whole = fn(g)
    other = _call(_engine(g, "time_major", family), g)
    moved, perm = _moved(g)
    shifted = fn(moved)
    for k in OUTPUTS:
        assert np.array_equal(whole[k], other[k], equal_nan=True), k
        assert np.array_equal(shifted[k], whole[k][perm], equal_nan=True), k


def _raw(kf, prob, work, num, den, status=None, time_major=0):
    from metran_amd import _lib

    req = _lib.ShiftRequest()
    req.d_num, req.d_den = num or None, den or None
    return _lib.lib().mk_level_shifts(kf._ctx, ctypes.byref(prob), ctypes.c_void_p(work) if work else None, time_major, ctypes.byref(req),
                                      status)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("shape", [(8, 2, 17), (13, 4, 17)], ids=["8x2", "13x4"])
def test_prefilled_buffers(shape, layout):
    """Every (t, j) of the outputs is written, with a number where the cell is observed and NaN where it is not; the words around
    [B,T,N] keep their pattern (the raw ABI on the inside of a larger allocation)."""
    import torch

    g = sr.group(*shape)
    kf = _engine(g, layout)
    buf = kf.alloc_level_shifts(g["B"])
    for k in OUTPUTS:
        buf[k].fill_(SENTINEL)
    got = _call(kf, g, buffers=buf)
    seen = np.isfinite(g["obs"])[np.arange(g["B"]) % g["R"]]
    for k in OUTPUTS:
        assert np.array_equal(np.isfinite(got[k]), seen) and np.isnan(got[k][~seen]).all() and not (got[k] == SENTINEL).any(), k
    B, T, N = g["B"], g["T"], g["N"]
    size, pad = B * T * N, 96
    wide = {k: torch.full((size + 2 * pad,), SENTINEL, dtype=torch.float64, device="cuda") for k in OUTPUTS}
    prob, keep, _ = kf._problem(kf._dev(g["phi"]), kf._dev(g["q"]), 0, kf._dev(g["x0"]), kf._dev(g["P0"]))
    assert _raw(kf, prob, buf["_work"].data_ptr(), wide["num"][pad:].data_ptr(), wide["den"][pad:].data_ptr(),
                time_major=1 if layout == "time_major" else 0) == 0
    torch.cuda.synchronize()
    for k in OUTPUTS:
        w = _np(wide[k])
        assert (w[:pad] == SENTINEL).all() and (w[pad + size:] == SENTINEL).all(), k
        inner = w[pad:pad + size].reshape((T, B, N) if layout == "time_major" else (B, T, N))
        inner = inner.transpose(1, 0, 2) if layout == "time_major" else inner
        assert np.array_equal(inner, got[k], equal_nan=True), k


@pytest.mark.parametrize("shape", [(8, 2), (13, 4)], ids=["8x2", "13x4"])
def test_status(shape):
    """An instance with a negative observation variance gets NaN rows and its filter's bits, its neighbours' outputs -- (8,2):
    in the same wavefront -- are bit-identical to the same call on the clean twin.  d_status goes in prefilled: the call WRITES
    the words."""
    c = sc.case(shape[0], shape[1], "neg_once")
    outs = []
    for g in (c["bad"], c["twin"]):
        kf = _engine(g)
        buf = kf.alloc_level_shifts(g["B"])
        buf["status"].fill_(0xA5A5A5A5 - (1 << 32))
        outs.append(_call(kf, g, buffers=buf))
    bad, twin = outs
    sc.check_flags(bad["status"], c, "filter", "level_shifts")
    sc.check_twin_flags(twin["status"], c, "filter", "level_shifts")
    sc.check_containment(bad, twin, c, "level_shifts")
    touched = list(c["touched"])
    assert (bad["status"][touched] & sc.FLAG_NONPOSITIVE_F).all()
    for k in OUTPUTS:
        assert np.isnan(bad[k][touched]).all(), k
    assert not twin["status"].any()
    worst = _compare(c["twin"], twin, "twin of neg_once")
    print("(%d,%d) twin: %.3g of the bar" % (shape + (worst,)))


def test_refusals():
    """A NULL d_num or d_den, a short d_work, a shape with 65 states: refused before any launch -- the outputs keep their
    sentinel."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import Problem

    g = sr.group(8, 2, 17)
    kf = _engine(g)
    L = _lib.lib()
    assert int(L.mk_shift_work_stride(61, 4)) == 0 and int(L.mk_shift_work_stride(60, 4)) == int(L.mk_block_work_stride(60, 4)) > 0
    assert int(L.mk_shift_work_stride(8, 2)) == int(L.mk_block_work_stride(8, 2)) == kf._reader_stride("shifts")
    prob, keep, _ = kf._problem(kf._dev(g["phi"]), kf._dev(g["q"]), 0, None, None)
    buf = kf.alloc_level_shifts(g["B"])
    for k in OUTPUTS:
        buf[k].fill_(SENTINEL)
    work, num, den = (buf[k].data_ptr() for k in ("_work", "num", "den"))
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0
    try:
        assert _raw(kf, prob, None, num, den) == -1 and b"d_work" in L.mk_last_error()
        assert _raw(kf, prob, work, None, den) == -1 and b"required" in L.mk_last_error()
        assert _raw(kf, prob, work, num, None) == -1 and b"required" in L.mk_last_error()
        assert _raw(kf, prob, small.value, num, den) == -1 and b"d_work" in L.mk_last_error()
        assert _raw(kf, prob, work, small.value, den) == -1 and b"d_num" in L.mk_last_error()
        assert _raw(kf, prob, work, num, small.value) == -1 and b"d_den" in L.mk_last_error()
        q = ctypes.c_void_p(work)
        wide = Problem(1, 1, 4, 61, 4, 0, q, q, q, q, None, None, None, 0, None, None)
        assert _raw(kf, wide, work, num, den) == -2 and b"N=61, K=4" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    torch.cuda.synchronize()
    assert all((buf[k] == SENTINEL).all() for k in OUTPUTS)
    assert _raw(kf, prob, work, num, den) == 0                          # ... and the same call with everything in place runs
    torch.cuda.synchronize()
    assert not any((buf[k] == SENTINEL).any() for k in OUTPUTS)


def test_metran_batch_end_to_end():
    """``MetranBatch.detect_level_shifts`` on the device finds the three planted shifts of the host tier's batch and nothing in the
    untouched models, and leaves the records as they were, bit for bit."""
    from metran_amd.engine import BatchedKalman
    from shift_engine import raw_facade
    from test_shift_host import check_planted, planted_models

    models, loadings, alpha, idx = planted_models()
    mb = raw_facade(lambda obs, G: BatchedKalman(0, layout="time_major").set_observations(obs).set_loadings(G), models, loadings)
    before = mb.kf.obs
    kept = _np(before).copy()
    frame = check_planted(mb, alpha, idx)
    assert mb.kf.obs is before and np.array_equal(_np(mb.kf.obs), kept, equal_nan=True) and not mb.kf.observations_adjusted
    screen = mb.screen_level_shifts(alpha=alpha, min_segment=sr.PLANT_MIN_SEGMENT)
    for r, j, t in sr.PLANTED:
        assert screen.loc[(r, "s%d" % j), "time"] == idx[t]
    print(frame[["series", "start", "estimate", "stderr", "t"]].to_string())
