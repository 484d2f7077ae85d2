"""Leave-one-out predictions, CPU tier: the numpy restatements of tests/loo_ref.py against masking one cell and smoothing
with the reference algorithm (oracle/), the adjoint form against the tape form, the reference's own masked example, and the
C ABI's new entry points (no compute calls)."""
import os
import re

import numpy as np
import pytest

import loo_ref
import oracle
from conftest import ROOT, golden_models

TOL = 1e-9


def _models():
    """(name, obs, phi, q, loadings, obsvar) of the fixtures the check samples; one model gets R != 0."""
    out = []
    for f in ("c2_small.npz", "c4_missing.npz", "n17_k3.npz"):
        for i, m in golden_models(f):
            out.append(("%s[%d]" % (f, i), m["obs"], m["phi"], m["q"], m["loadings"], None))
    name, obs, phi, q, G, _ = out[1]
    R = np.random.default_rng(5).uniform(0.05, 0.5, obs.shape[1])
    out.append((name + "+R", obs, phi, q, G, R))
    # no fixture has a step with a single observed series: c4_missing[0] with one such step and one empty step
    name, obs, phi, q, G, _ = out[3]
    obs = obs.copy()
    keep = np.nonzero(np.isfinite(obs[5]))[0][0]
    obs[5, np.arange(obs.shape[1]) != keep] = np.nan
    obs[9] = np.nan
    out.append((name + "+single", obs, phi, q, G, None))
    return out


MODELS = _models()


@pytest.mark.parametrize("case", MODELS, ids=[m[0] for m in MODELS])
def test_restatement_matches_masking_and_smoothing(case):
    name, obs, phi, q, G, R = case
    means, variances = loo_ref.loo_tape(obs, phi, q, G, R)
    seen = np.isfinite(obs)
    assert np.array_equal(np.isnan(means), ~seen) and np.array_equal(np.isnan(variances), ~seen)
    cells = loo_ref.sample_cells(obs, np.random.default_rng(len(name)))
    cnt = seen.sum(1)
    ts = {t for t, _ in cells}
    rows = np.nonzero(cnt)[0]
    assert rows[0] in ts and rows[-1] in ts
    if (cnt == 1).any():
        assert any(cnt[t] == 1 for t in ts)
    if (cnt == obs.shape[1]).any():
        assert any(cnt[t] == obs.shape[1] for t in ts)
    bm, bv = loo_ref.loo_brute(oracle, obs, phi, q, G, cells, R)
    got_m = np.array([means[c] for c in cells])
    got_v = np.array([variances[c] for c in cells])
    np.testing.assert_allclose(got_m, bm, rtol=0, atol=TOL * max(1.0, np.abs(bm).max()))
    np.testing.assert_allclose(got_v, bv, rtol=0, atol=TOL * max(1.0, np.abs(bv).max()))


def test_sample_covers_the_edge_steps():
    """Across the sampled fixtures there is a step with one observed series and a fully observed step."""
    one = full = False
    for _, obs, *_ in MODELS:
        cnt = np.isfinite(obs).sum(1)
        one |= bool((cnt == 1).any())
        full |= bool((cnt == obs.shape[1]).any())
    assert one and full


@pytest.mark.parametrize("case", MODELS, ids=[m[0] for m in MODELS])
def test_adjoint_form_equals_tape_form(case):
    """The (a, c) form of the narrow kernel's walk -- xb = -2 r, Pb = N - r r' with unit weights -- gives the tape form's values."""
    name, obs, phi, q, G, R = case
    m1, v1 = loo_ref.loo_tape(obs, phi, q, G, R)
    m2, v2 = loo_ref.loo_adjoint(obs, phi, q, G, R)
    assert np.array_equal(np.isnan(m1), np.isnan(m2))
    np.testing.assert_allclose(m2, m1, rtol=0, atol=TOL * max(1.0, np.nanmax(np.abs(m1))))
    np.testing.assert_allclose(v2, v1, rtol=0, atol=TOL * max(1.0, np.nanmax(np.abs(v1))))


def test_adjoint_form_with_initial_moments():
    rng = np.random.default_rng(11)
    _, obs, phi, q, G, _ = MODELS[0]
    n = phi.size
    x0 = rng.normal(size=n)
    A = rng.normal(size=(n, n))
    P0 = A @ A.T / n + 0.5 * np.eye(n)
    m1, v1 = loo_ref.loo_tape(obs, phi, q, G, None, x0, P0)
    m2, v2 = loo_ref.loo_adjoint(obs, phi, q, G, None, x0, P0)
    np.testing.assert_allclose(m2, m1, rtol=0, atol=1e-10)
    np.testing.assert_allclose(v2, v1, rtol=0, atol=1e-10)
    cells = loo_ref.sample_cells(obs, rng, 4)
    bm, bv = loo_ref.loo_brute(oracle, obs, phi, q, G, cells, None, x0, P0)
    np.testing.assert_allclose([m1[c] for c in cells], bm, rtol=0, atol=1e-9)
    np.testing.assert_allclose([v1[c] for c in cells], bv, rtol=0, atol=1e-9)


def test_reference_masked_example(g1):
    """The reference's worked example masks (mask_t, series 4) and re-smooths: its get_simulation at that cell is the
    leave-one-out mean in original units."""
    t = int(g1["mask_t"])
    means, _ = loo_ref.loo_tape(g1["obs"], g1["phi"], g1["q"], g1["loadings"])
    got = means[t, 4] * g1["oseries_std"][4] + g1["oseries_mean"][4]
    want = float(g1["masked_sim_005"].ravel()[t])
    assert abs(got - want) <= 1e-9 * abs(want), (got, want)


# ---- C ABI (no compute calls) ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from metran_amd import _lib

    if not os.path.exists(_lib.library_path()):
        g.build()
    return _lib.lib()


def test_loo_entry_points_declared_and_exported(lib):
    src = open(os.path.join(ROOT, "include", "metran_hip.h")).read()
    declared = re.findall(r"MK_API\s+[\w\s\*]+?\b(mk_\w+)\s*\(", src)
    assert "mk_loo" in declared and "mk_loo_work_stride" in declared
    assert hasattr(lib, "mk_loo") and hasattr(lib, "mk_loo_work_stride")


def test_loo_work_stride(lib):
    for N, K in ((8, 2), (5, 1), (32, 4)):
        assert lib.mk_loo_work_stride(N, K) > 0, (N, K)
    assert lib.mk_loo_work_stride(8, 2) == lib.mk_record_stride(10)
    assert lib.mk_loo_work_stride(32, 4) == lib.mk_tape_stride(32, 4)
    for N, K in ((7, 7), (60, 4), (100, 4)):
        assert lib.mk_loo_work_stride(N, K) == 0, (N, K)
