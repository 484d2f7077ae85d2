"""Leave-block-out predictions on the GPU (C ABI mk_block_predict: the recording forward pass, the gain tape and the innovations
written by innov_step_kernel, block_checkpoint_kernel, block_walk_kernel) against the DEFINITION in extended precision
(tests/block_ref.py: dense conditioning of the record's data vector; pinned to the oracle and the leave-one-out restatement by
tests/test_block_host.py), against independent kernels (loo_predict for one-cell blocks, simulate_smoothed on a copy of the record
with the block masked, regression with one pulse per block cell), bit for bit across batches, layouts and block lists, under both
kernel families, next to an invalid model and a degenerate block, and the refusals of the raw ABI.

The bar against the definition (block_ref.bars): the LOO tier's flat bar, 1e-12 * big for the means and * big^2 for the variances
(quad and log det V relative to max(1, m)), plus 4 * MU * kappa * eps * scale, kappa the condition number of the unit-diagonal
M_II in the reference and MU = block_ref.MU the largest (float64 restatement - definition) / (kappa * eps * scale) over every
group, record and block of this tier, measured on the CPU by tests/test_block_host.py::test_restatement_against_definition:
mu = 1016 ((5,1), T = 70, the quad of a one-cell block with kappa = 1 and a large quad), MU = 1100.  Every test prints the
kernel's largest distance in units of the bar; on an MI355X it is 0.11 of the bar ((5,1), T = 70), 0.034 at (8,2), T = 3 and
0.010 at (13,4), T = 17, below 0.01 elsewhere."""
import ctypes

import numpy as np
import pytest

import block_ref as br
import call_forms as cf
import status_cases as sc

pytestmark = pytest.mark.gpu

PREFILL = 0xA5A5A5A5
LAYOUTS = ("model_major", "time_major")
CASES = [(N, K, T, "specialised") for N, K, T in br.GROUPS] + [(8, 2, 17, "generic")]
IDS = ["%dx%d-T%d-%s" % c for c in CASES]
OUTPUTS = ("means", "vars", "summary", "flags")
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


def _call(kf, g, blocks, **kw):
    res = kf.block_predict(g["phi"], g["q"], blocks, **cf.init(g), **kw)
    return {k: _np(res[k]).copy() for k in OUTPUTS + ("status",)}


def _row(got, i, w, L):
    s = got["summary"][i, w]
    return dict(means=got["means"][i, w, :L], vars=got["vars"][i, w, :L], m=(-1 if np.isnan(s[0]) else int(s[0])), quad=s[1], logdet=s[2],
                ovo=s[3])


def _compare(g, got, blocks, what):
    """Every instance and block against the definition; returns the largest distance in bars."""
    worst = 0.0
    Lmax = got["means"].shape[2]
    for i in range(g["B"]):
        for w, blk in enumerate(blocks[i % g["R"]]):
            ref = br.definition(g, i, blk)
            if ref is None:
                assert np.isnan(got["means"][i, w]).all() and np.isnan(got["vars"][i, w]).all() and np.isnan(got["summary"][i, w]).all()
                assert got["flags"][i, w] == 0
                continue
            L = int(blk[2] - blk[1])
            assert np.isnan(got["means"][i, w, L:]).all() and np.isnan(got["vars"][i, w, L:]).all(), (what, i, w)
            assert got["flags"][i, w] == 0, (what, i, w)
            d = br.distance(_row(got, i, w, L), ref, br.bars(g, i, blk, ref))
            assert d <= 1.0, "%s: instance %d, block %d %s (m = %d, kappa = %.3g) is %.3g bars from the definition" % (
                what, i, w, tuple(blk), ref["m"], ref["kappa"], d)
            worst = max(worst, d)
    assert Lmax >= 1
    return worst


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_definition(case, layout):
    N, K, T, family = case
    g = br.group(N, K, T)
    blocks = br.blocks(g)
    got = _call(_engine(g, layout, family), g, blocks)
    assert not got["status"].any()
    worst = _compare(g, got, blocks, "(%d,%d) T=%d %s %s" % (N, K, T, family, layout))
    print("(%d,%d) T=%d %s %s: %.3g of the bar" % (N, K, T, family, layout, worst))


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "specialised" and cf.has_loo(c[0], c[1])], ids=lambda c: "%dx%d-T%d" % c[:3])
def test_one_cell_blocks_are_loo(case):
    """Independent kernels: a block of one cell is loo_predict's cell, at the LOO tier's bar."""
    N, K, T, _ = case
    g = br.group(N, K, T)
    blocks = br.blocks(g)
    kf = _engine(g)
    got = _call(kf, g, blocks)
    loo = kf.loo_predict(g["phi"], g["q"], **cf.init(g))
    lm, lv = _np(loo["loo_means"]), _np(loo["loo_vars"])
    seen = 0
    for i in range(g["B"]):
        for w, (js, t0, t1) in enumerate(blocks[i % g["R"]]):
            if js < 0 or t1 - t0 != 1:
                continue
            a, b = got["means"][i, w, 0], lm[i, t0, js]
            assert np.isnan(a) == np.isnan(b), (i, w)
            if np.isnan(a):
                continue
            seen += 1
            big = max(1.0, float(np.nanmax(np.abs(lm[i]))))
            assert abs(a - b) <= cf.LOO_TOL * big and abs(got["vars"][i, w, 0] - lv[i, t0, js]) <= cf.LOO_TOL * big * big, (i, w, a, b)
    assert seen >= g["S"]


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "specialised"], ids=lambda c: "%dx%d-T%d" % c[:3])
def test_against_the_masked_smoother(case):
    """Independent kernels: simulate_smoothed on a copy of the record with the block masked gives the block's means and variances,
    at the bars tests/test_loo_gpu.py uses for this comparison (1e-9 * big, 1e-9 * big^2)."""
    N, K, T, _ = case
    g = br.group(N, K, T)
    blocks = br.blocks(g)
    kf = _engine(g)
    got = _call(kf, g, blocks)
    worst = 0.0
    for w in range(blocks.shape[1]):
        mask = np.zeros(g["obs"].shape, dtype=bool)
        for r in range(g["R"]):
            js, t0, t1 = blocks[r, w]
            if js >= 0:
                mask[r, t0:t1, js] = True
        kf.mask_observations(mask)
        sm = kf.simulate_smoothed(g["phi"], g["q"], **cf.init(g))
        mean, var = _np(sm["sim_means"]).copy(), _np(sm["sim_vars"]).copy()
        kf.unmask_observations()
        for i in range(g["B"]):
            js, t0, t1 = blocks[i % g["R"], w]
            if js < 0:
                continue
            have = np.isfinite(got["means"][i, w, :t1 - t0])
            assert np.array_equal(have, np.isfinite(g["obs"][i % g["R"], t0:t1, js])), (i, w)
            if not have.any():
                continue
            big = max(1.0, float(np.abs(mean[i]).max()))
            dm = np.abs(got["means"][i, w, :t1 - t0] - mean[i, t0:t1, js])[have].max() / (1e-9 * big)
            dv = np.abs(got["vars"][i, w, :t1 - t0] - var[i, t0:t1, js])[have].max() / (1e-9 * big * big)
            assert dm <= 1.0 and dv <= 1.0, (i, w, dm, dv)
            worst = max(worst, dm, dv)
    print("(%d,%d) T=%d: %.3g of the bar against the masked smoother" % (N, K, T, worst))


@pytest.mark.parametrize("case", [c for c in CASES if c[3] == "specialised"], ids=lambda c: "%dx%d-T%d" % c[:3])
def test_against_pulse_regression(case):
    """Independent kernels: regression with one pulse per block cell and t_first = 0, for the blocks of at most 16 steps:
    beta = observed - predicted, cov = V, gain = quad, at the regression tier's bar."""
    from test_regression_gpu import BAR_S

    N, K, T, _ = case
    g = br.group(N, K, T)
    blocks = br.blocks(g)
    kf = _engine(g)
    got = _call(kf, g, blocks)
    Rv = g["obsvar"]
    worst, seen = 0.0, 0
    for w in range(blocks.shape[1]):
        if (blocks[:, w, 2] - blocks[:, w, 1]).max() > 16:
            continue
        ef = np.full((g["R"], 16, 4), -1, dtype=np.int64)
        ef[:, :, 3] = 1
        ef[:, :, 1:3] = 0
        for r in range(g["R"]):
            js, t0, t1 = blocks[r, w]
            for c in range(t1 - t0 if js >= 0 else 0):
                ef[r, c] = (js, LEVEL, t0 + c, t0 + c + 1)
        if (ef[:, :, 0] < 0).all():
            continue
        reg = kf.regression(g["phi"], g["q"], ef, t_first=0, **cf.init(g))
        beta, cov, gain = _np(reg["beta"]), _np(reg["cov"]), _np(reg["gain"])
        for i in range(g["B"]):
            r = i % g["R"]
            js, t0, t1 = blocks[r, w]
            if js < 0 or got["summary"][i, w, 0] < 1:
                continue
            sc_, of = g["scale"][r, js], g["offset"][r, js]
            have = np.isfinite(got["means"][i, w, :t1 - t0])
            assert np.array_equal(have, np.isfinite(beta[i, :t1 - t0])), (i, w)
            resid = (g["obs"][r, t0:t1, js] * sc_ + of - got["means"][i, w, :t1 - t0])[have] / sc_
            d = [np.abs(resid - beta[i, :t1 - t0][have]) / np.maximum(1.0, np.abs(resid))]
            vd = np.diag(cov[i])[:t1 - t0][have]
            mine = got["vars"][i, w, :t1 - t0][have] / sc_ ** 2 + Rv[r, js]
            clipped = got["vars"][i, w, :t1 - t0][have] == 0
            d.append(np.where(clipped, 0.0, np.abs(mine - vd) / np.maximum(1.0, vd)))
            idx = np.nonzero(have)[0]
            ovo = cov[i][np.ix_(idx, idx)].sum() / len(idx) ** 2
            d.append([abs(got["summary"][i, w, 3] / sc_ ** 2 - ovo) / max(1.0, ovo), abs(got["summary"][i, w, 1] - gain[i]) / max(1.0, gain[i])])
            dist = max(float(np.max(x)) for x in d) / BAR_S
            assert dist <= 1.0, (i, w, dist)
            worst, seen = max(worst, dist), seen + 1
    assert seen >= g["B"]
    print("(%d,%d) T=%d: %.3g of the bar against the pulse regression" % (N, K, T, worst))


@pytest.mark.parametrize("case", [(8, 2, 17, "specialised"), (13, 4, 17, "specialised"), (32, 4, 3, "specialised"), (5, 1, 70, "specialised"),
                                  (8, 2, 17, "generic")], ids=lambda c: "%dx%d-T%d-%s" % c)
def test_bit_for_bit(case):
    """The 15-instance call equals the five 3-instance calls; both layouts agree; W blocks equal W one-block calls; permuting the
    block list permutes the rows."""
    N, K, T, family = case
    g = br.group(N, K, T)
    blocks = br.blocks(g)
    engines = {}

    def fn(grp):
        key = grp["B"]
        if key not in engines:
            engines[key] = _engine(grp, "model_major", family)
        out = _call(engines[key], grp, blocks)
        return {k: out[k] for k in OUTPUTS}

    cf.check_position_independent(fn, g, "block_predict")
    kf = engines[g["B"]]
    whole = _call(kf, g, blocks)
    other = _call(_engine(g, "time_major", family), g, blocks)
    for k in OUTPUTS:
        assert np.array_equal(whole[k], other[k], equal_nan=True), k
    L = whole["means"].shape[2]
    for w in range(blocks.shape[1]):
        one = _call(kf, g, blocks[:, w:w + 1])
        Lw = one["means"].shape[2]
        assert np.array_equal(one["means"][:, 0], whole["means"][:, w, :Lw], equal_nan=True), w
        assert np.array_equal(one["vars"][:, 0], whole["vars"][:, w, :Lw], equal_nan=True), w
        assert np.isnan(whole["means"][:, w, Lw:]).all()
        assert np.array_equal(one["summary"][:, 0], whole["summary"][:, w], equal_nan=True) and np.array_equal(one["flags"][:, 0], whole["flags"][:, w])
    perm = np.random.default_rng(5).permutation(blocks.shape[1])
    shuffled = _call(kf, g, blocks[:, perm])
    for k in OUTPUTS:
        assert np.array_equal(shuffled[k], whole[k][:, perm], equal_nan=True), k
    assert L >= 1


@pytest.mark.parametrize("shape", [(8, 2), (13, 4)], ids=["8x2", "13x4"])
def test_status(shape):
    """An instance with a negative observation variance gets NaN rows and its filter's bits, its neighbours' outputs are
    bit-identical to the same call on the clean twin.  d_status and d_flags go in prefilled: the call WRITES the words."""
    T = sc.T
    blocks = np.array([(0, 0, T), (1, 2, 6), (0, sc.STEP_A, sc.STEP_A + 1), (2, T - 2, T), (-1, 0, 0)], dtype=np.int64)
    c = sc.case(shape[0], shape[1], "neg_once")
    outs = []
    for g in (c["bad"], c["twin"]):
        kf = _engine(g)
        buf = kf.alloc_block_predict(g["B"], len(blocks), T)
        buf["status"].fill_(PREFILL - (1 << 32))
        buf["flags"].fill_(PREFILL - (1 << 32))
        outs.append(_call(kf, g, blocks, buffers=buf))
    bad, twin = outs
    sc.check_flags(bad["status"], c, "filter", "block_predict")
    sc.check_twin_flags(twin["status"], c, "filter", "block_predict")
    sc.check_containment(bad, twin, c, "block_predict")
    touched = list(c["touched"])
    assert (bad["status"][touched] & sc.FLAG_NONPOSITIVE_F).all()
    for k in ("means", "vars", "summary"):
        assert np.isnan(bad[k][touched]).all(), k
    assert not twin["flags"].any() and not twin["status"].any()
    g = c["twin"]
    worst = _compare(g, twin, np.broadcast_to(blocks, (g["R"],) + blocks.shape), "twin of neg_once")
    print("(%d,%d) twin: %.3g of the bar" % (shape + (worst,)))


def test_degenerate_block():
    """A block whose second cell is fixed by its first one given the rest (block_ref.degenerate_group; shown degenerate on the CPU by
    tests/test_block_host.py): bit 0 of its flag, NaN outputs beside m, no status bit; the other blocks of the instance are
    bit-identical to a call without it, and the same block of the ordinary instance beside it is fine."""
    g = br.degenerate_group()
    blocks = br.DEGENERATE_BLOCKS
    kf = _engine(g)
    got = _call(kf, g, blocks)
    assert not got["status"].any()
    assert got["flags"].tolist() == [[1, 0, 0, 0], [0, 0, 0, 0]]
    assert got["summary"][0, 0, 0] == 2 and np.isnan(got["summary"][0, 0, 1:]).all()
    assert np.isnan(got["means"][0, 0]).all() and np.isnan(got["vars"][0, 0]).all()
    rest = _call(kf, g, blocks[:, 1:])
    Lr = rest["means"].shape[2]
    assert np.array_equal(rest["means"], got["means"][:, 1:, :Lr], equal_nan=True) and np.array_equal(rest["vars"], got["vars"][:, 1:, :Lr], equal_nan=True)
    assert np.array_equal(rest["summary"], got["summary"][:, 1:], equal_nan=True) and not rest["flags"].any()
    worst = 0.0
    # against the definition: the ordinary instance (the data vector of instance 0 is singular to sixteen digits, so that its dense
    # conditioning is no reference even in extended precision)
    for i, w in ((1, 0), (1, 1), (1, 2), (1, 3)):
        ref = br.definition(g, i, blocks[0, w])
        L = int(blocks[0, w, 2] - blocks[0, w, 1])
        d = br.distance(_row(got, i, w, L), ref, br.bars(g, i, blocks[0, w], ref))
        assert d <= 1.0, (i, w, d)
        worst = max(worst, d)
    assert np.isfinite(got["summary"][0, 1:]).all()
    print("beside the degenerate block: %.3g of the bar" % worst)


def test_refusals():
    """L = 65, t1 - t0 > L, t0 >= t1, series >= N, NULL pointers, an undersized buffer: MK_ERR_INVALID before any launch -- the
    outputs keep their sentinel; a shape with 65 states: MK_ERR_SHAPE."""
    import torch

    from metran_amd import _lib
    from metran_amd._lib import BlockRequest, Problem

    g = br.group(8, 2, 17)
    kf = _engine(g)
    L = _lib.lib()
    assert int(L.mk_block_max_cells()) == 64 == kf.block_max_cells and kf.block_predict_supported
    assert int(L.mk_block_work_stride(61, 4)) == 0 and int(L.mk_block_work_stride(60, 4)) == int(L.mk_scores_work_stride(60, 4)) > 0
    assert int(L.mk_block_work_stride(8, 2)) == int(L.mk_record_stride(10)) + 8 * ((10 + 3) & ~1) + 8
    B, T, N, W, Lc = g["B"], 17, 8, 3, 6
    prob, keep, _ = kf._problem(kf._dev(g["phi"]), kf._dev(g["q"]), 0, None, None)
    buf = kf.alloc_block_predict(B, W, Lc)
    for key in ("means", "vars", "summary"):
        buf[key].fill_(7.5)
    buf["flags"].fill_(-3)
    bl0 = np.broadcast_to(np.array([(0, 0, 6), (1, 5, 9), (-1, 0, 0)], dtype=np.int64), (3, W, 3)).copy()
    small = ctypes.c_void_p()
    assert L.mk_malloc(kf._ctx, 128, ctypes.byref(small)) == 0
    held = []

    def table(slot=None):
        bl = bl0.copy()
        if slot is not None:
            bl[1, 1] = slot
        held.append(torch.as_tensor(bl, dtype=torch.int64, device="cuda"))
        return held[-1].data_ptr()

    def call(work=buf["_work"].data_ptr(), blocks=None, n_blocks=W, n_cells=Lc, problem=prob, **ptrs):
        req = BlockRequest()
        req.n_blocks, req.n_cells, req.d_blocks = n_blocks, n_cells, table() if blocks is None else (blocks or None)
        req.d_checkpoints = ptrs.get("checkpoints", buf["_checkpoints"].data_ptr()) or None
        for key in OUTPUTS:
            setattr(req, "d_" + key, ptrs.get(key, buf[key].data_ptr()) or None)
        return L.mk_block_predict(kf._ctx, ctypes.byref(problem), ctypes.c_void_p(work) if work else None, 0, ctypes.byref(req), None)

    try:
        assert call(work=None) == -1 and b"d_work" in L.mk_last_error()
        assert call(blocks=0) == -1 and b"d_blocks" in L.mk_last_error()
        for key in OUTPUTS + ("checkpoints",):
            assert call(**{key: 0}) == -1 and b"required" in L.mk_last_error(), key
        assert call(n_blocks=0) == -1 and b"n_blocks" in L.mk_last_error()
        assert call(n_cells=0) == -1 and call(n_cells=65) == -1 and b"n_cells" in L.mk_last_error()
        assert call(work=small.value) == -1 and b"d_work" in L.mk_last_error()
        assert call(blocks=small.value, n_blocks=9) == -1 and b"d_blocks" in L.mk_last_error()
        assert call(means=small.value) == -1 and b"d_means" in L.mk_last_error()
        assert call(vars=small.value) == -1 and b"d_vars" in L.mk_last_error()
        assert call(summary=small.value) == -1 and b"d_summary" in L.mk_last_error()
        assert call(checkpoints=small.value) == -1 and b"d_checkpoints" in L.mk_last_error()
        assert call(flags=small.value, n_blocks=64) == -1
        for slot, word in (((N, 0, 3), b"series"), ((0, -1, 3), b"t0"), ((0, 3, 3), b"t0"), ((0, 5, 4), b"t0"), ((0, 12, T + 1), b"t1"),
                           ((0, 2, 9), b"n_cells")):
            assert call(blocks=table(slot)) == -1 and word in L.mk_last_error() and b"d_blocks[1, 1]" in L.mk_last_error(), slot
        q = ctypes.c_void_p(buf["_work"].data_ptr())
        wide = Problem(1, 1, 4, 61, 4, 0, q, q, q, q, None, None, None, 0, None, None)
        assert call(problem=wide) == -2 and b"N=61, K=4" in L.mk_last_error()
    finally:
        L.mk_free(kf._ctx, small)
    torch.cuda.synchronize()
    assert all((buf[key] == 7.5).all() for key in ("means", "vars", "summary")) and (buf["flags"] == -3).all()
    assert call(blocks=table((-1, 9, 99))) == 0                      # an unused slot is not read further ... and the call runs
    torch.cuda.synchronize()
    assert not (buf["summary"] == 7.5).any() and not (buf["means"] == 7.5).any() and not (buf["flags"] == -3).any()
    with pytest.raises(ValueError):
        kf.block_predict(g["phi"], g["q"], np.zeros((2, 2, 3), dtype=np.int64))
    with pytest.raises(ValueError):
        kf.block_predict(g["phi"], g["q"], np.array([[0, 0, 18]]))
    with pytest.raises(ValueError):
        kf.alloc_block_predict(B, 1, 65)
    g70 = br.group(5, 1, 70)
    with pytest.raises(ValueError, match="64"):
        _engine(g70).block_predict(g70["phi"], g70["q"], np.array([[0, 0, 65]]))


def test_metran_batch_end_to_end():
    """Through MetranBatch: the predictions of a gap are what masking the gap and ``get_simulation`` give there; the skill table
    is the same whether the models go in one call or one at a time; its length-1 rows are the leave-one-out errors."""
    import pandas as pd

    from metran_amd.batch import MetranBatch
    from metran_amd.synthetic import make_dfm_batch

    T = 90
    d = make_dfm_batch(3, 3, 1, T, seed=11, missing=0.2)
    idx = pd.date_range("2001-01-01", periods=T, freq="D")
    models = []
    for r in range(3):
        cols = [pd.Series(10.0 * (j + 1) + (1.0 + 0.5 * j) * d["obs"][r, :, j], index=idx, name="s%d" % j).dropna() for j in range(3)]
        models.append(cols if r != 1 else [c[c.index < idx[80]] for c in cols])
    mb = MetranBatch(models, factors=d["loadings"])
    alpha = d["alpha"]
    gaps = [(0, "s1", idx[20], idx[50]), (1, "s2", 40, 47), (2, "s0", idx[60], None), (0, "s0", 5, 6)]
    frame = mb.get_gap_predictions(gaps, alpha=alpha)
    info = frame.attrs["gaps"]
    assert len(frame) == info["n_obs"].sum() > 30 and not info["degenerate"].any()
    for model, name, start, end in gaps:
        r, j = model, int(name[1])
        t0, t1 = mb._effect_step(r, start), mb._effect_step(r, end, end=True)
        mask = np.zeros((3, mb.T, 3), dtype=bool)
        mask[r, t0:t1, j] = True
        mb.mask_observations(mask)
        sim = mb.get_simulation(r, name, alpha=alpha, ci=0.05)
        var = _np(mb.get_simulated_variances(alpha=alpha))[r, :, j]
        mb.unmask_observations()
        rows = frame.xs((model, name), level=("model", "series")).droplevel("gap")
        big = max(1.0, float(np.abs(sim["mean"]).max()))
        assert np.abs(rows["predicted"].values - sim["mean"].loc[rows.index].values).max() <= 1e-9 * big
        steps = [list(mb.batch.index[r]).index(t) for t in rows.index]
        assert np.abs(rows["stderr"].values ** 2 - var[steps]).max() <= 1e-9 * big * big
    table = mb.gap_fill_skill(lengths=(1, 7, 30), alpha=alpha)
    assert len(table) == 27 and (table["n_blocks"] > 0).all()
    # a budget that holds one model's workspace, checkpoints and outputs at length 7 and two at length 30, not all three
    small = mb.gap_fill_skill(lengths=(1, 7, 30), alpha=alpha, budget=8.0 * 1.8 * (mb.T * mb.kf._reader_stride("blocks") + 1600))
    assert np.array_equal(small.values, table.values, equal_nan=True)
    ones = table.xs(1, level="length")
    assert np.allclose(ones["rmse"].values, ones["rmse_loo"].values, rtol=1e-12, atol=0)
    month = table.xs(30, level="length")
    assert (month["rmse"].values > month["rmse_loo"].values).all()           # leave-one-out flatters the filling of a month
    assert (table["msse"] > 0).all() and np.isfinite(table["log_score"]).all() and ((table["coverage"] >= 0) & (table["coverage"] <= 1)).all()
