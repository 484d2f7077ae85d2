"""Posterior draws (simulation smoother), CPU tier: the numpy restatement of tests/draw_ref.py -- the generator's known
answers, the exact identities of a draw, the joint law against dense Gaussian conditioning -- the C ABI's new entry points
(no compute calls) and the MetranBatch accessors over a stand-in engine."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import draw_ref
import oracle
from conftest import ROOT, golden_models

TOL = 1e-9   # the tier's smoothed-moment bar


# ---- the generator ----
KAT = [((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
       ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
       ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1))]


@pytest.mark.parametrize("counter,key,want", KAT, ids=["zeros", "ones", "pi"])
def test_philox_known_answers(counter, key, want):
    got = draw_ref.philox4x32_10(tuple(np.array([c]) for c in counter), key)
    assert tuple(int(w[0]) for w in got) == want


def test_mantissas_and_uniforms_are_strictly_inside():
    m1, m2 = draw_ref.mantissas(12345678901234567, np.arange(50)[:, None, None], np.arange(9)[None, :, None], np.arange(7)[None, None, :], 3)
    for m in (m1, m2):
        assert m.dtype == np.uint64 and int(m.max()) < 2 ** 52
        u = draw_ref.uniforms(m)
        assert (u > 0).all() and (u < 1).all()
    ends = draw_ref.uniforms(np.array([0, 2 ** 52 - 1], dtype=np.uint64))
    assert ends[0] == 2.0 ** -53 and ends[1] == 1.0 - 2.0 ** -53 and 0.0 < ends[0] and ends[1] < 1.0
    z = draw_ref.normal_block(7, 0, 3, 0, 4, False, 20, 9)
    assert z.shape == (4, 3, 21, 9) and np.isfinite(z).all() and np.abs(z).max() < 8.6
    # a value depends on its counter only: a sub-block is the same numbers
    sub = draw_ref.normal_block(7, 1, 2, 2, 2, False, 20, 9)
    assert np.array_equal(sub, z[2:4, 1:3])
    anti = draw_ref.normal_block(7, 0, 3, 0, 4, True, 20, 9)
    assert np.array_equal(anti[0], z[0]) and np.array_equal(anti[1], -z[0]) and np.array_equal(anti[3], -z[1])


# ---- the exact identities of a draw ----
def _fixed_model():
    _, m = next(golden_models("c4_missing.npz"))
    rng = np.random.default_rng(3)
    N = m["obs"].shape[1]
    return m["obs"], m["phi"], m["q"], m["loadings"], rng.uniform(0.5, 3.0, N), rng.normal(size=N)


def test_series_draw_returns_the_observation_where_observed():
    obs, phi, q, G, scale, offset = _fixed_model()
    draws = draw_ref.draw_model(oracle, obs, phi, q, G, 3, seed=11, instance=5, scale=scale, offset=offset)
    seen = np.isfinite(obs)
    assert seen.any() and (~seen).any()
    want = obs * scale + offset
    for d in draws:
        assert np.abs(d[seen] - want[seen]).max() <= TOL * max(1.0, np.abs(want[seen]).max())
    assert np.abs(draws[0] - draws[1])[~seen].max() > 1e-3     # ... and is a draw where it is not


@pytest.mark.parametrize("with_r", [False, True], ids=["R0", "R"])
def test_antithetic_pair_averages_to_the_smoothed_mean(with_r):
    obs, phi, q, G, scale, offset = _fixed_model()
    N = obs.shape[1]
    R = np.random.default_rng(8).uniform(0.05, 0.4, N) if with_r else None
    Z = np.concatenate([np.eye(N), G], axis=1)
    S, Ps = draw_ref.smooth(oracle, obs, phi, q, G, R)
    st = draw_ref.draw_model(oracle, obs, phi, q, G, 4, seed=2, what="states", obsvar=R, antithetic=True)
    se = draw_ref.draw_model(oracle, obs, phi, q, G, 4, seed=2, what="series", obsvar=R, antithetic=True, scale=scale, offset=offset)
    sm, _ = oracle.simulate(Z * scale[:, None], S, Ps)
    for k in (0, 2):
        assert np.abs(0.5 * (st[k] + st[k + 1]) - S).max() <= TOL * max(1.0, np.abs(S).max())
        assert np.abs(0.5 * (se[k] + se[k + 1]) - (sm + offset)).max() <= TOL * max(1.0, np.abs(sm + offset).max())
    assert np.abs(st[0] - st[2]).max() > 1e-3


# ---- the joint law ----
JOINT_S, JOINT_SEED, JOINT_ALPHA = 4000, 20021, 1e-6 / 4   # two cases x two statistics share a false-alarm probability of 1e-6


def _tiny(case):
    rng = np.random.default_rng(99)
    N, K, T = 3, 1, 12
    phi = np.array([0.8, 0.5, 0.9, 0.7])
    G = np.array([[0.6], [-0.5], [0.7]])
    q = 1.0 - phi ** 2
    q[:N] *= 1.0 - (G ** 2).sum(1)
    x = rng.standard_normal(N + K)
    y = np.empty((T, N))
    for t in range(T):
        x = phi * x + np.sqrt(q) * rng.standard_normal(N + K)
        y[t] = x[:N] + G @ x[N:]
    y[rng.random((T, N)) < 0.4] = np.nan
    if case == "defaults":
        return y, phi, q, G, None, None, None
    A = rng.normal(size=(N + K, N + K))
    return y, phi, q, G, np.array([0.2, 0.05, 0.3]), rng.normal(size=N + K), A @ A.T / (N + K) + 0.5 * np.eye(N + K)


@pytest.mark.parametrize("case", ["defaults", "x0_P0_R"])
def test_joint_law_against_dense_conditioning(case):
    """S draws of the projected series at ALL missing cells, whitened with the exact posterior (dense Gaussian conditioning):
    their sum of squares is chi-square with S * C degrees of freedom and the largest |column mean| * sqrt(S) is the maximum of
    C standard normals in magnitude -- limits from those laws, not from the draws."""
    from scipy import stats

    y, phi, q, G, R, x0, P0 = _tiny(case)
    miss = ~np.isfinite(y).ravel()
    C = int(miss.sum())
    assert 8 <= C <= 22 and C == int((~np.isfinite(y)).sum())
    mean, cov = draw_ref.posterior_dense(y, phi, q, G, R, x0, P0)
    m, Sig = mean[miss], cov[np.ix_(miss, miss)]
    draws = draw_ref.draw_model(oracle, y, phi, q, G, JOINT_S, seed=JOINT_SEED, what="series", obsvar=R, x0=x0, P0=P0)
    d = draws.reshape(JOINT_S, -1)[:, miss]
    # the posterior mean itself: the smoother's, to the tier's bar
    S, _ = draw_ref.smooth(oracle, y, phi, q, G, R, x0, P0)
    Z = np.concatenate([np.eye(3), G], axis=1)
    assert np.abs((S @ Z.T).ravel()[miss] - m).max() <= TOL
    w = np.linalg.solve(np.linalg.cholesky(Sig), (d - m).T).T          # [S, C] iid N(0, 1) under the law
    ss = float((w * w).sum())
    lo, hi = stats.chi2.ppf(JOINT_ALPHA / 2, JOINT_S * C), stats.chi2.isf(JOINT_ALPHA / 2, JOINT_S * C)
    worst = float(np.abs(w.mean(0)).max() * np.sqrt(JOINT_S))
    limit = stats.norm.isf((1.0 - (1.0 - JOINT_ALPHA) ** (1.0 / C)) / 2.0)
    print("case %s: C = %d, sum of squares %.1f in [%.1f, %.1f], max |mean| sqrt(S) %.3f <= %.3f" % (case, C, ss, lo, hi, worst, limit))
    assert lo <= ss <= hi
    assert worst <= limit


# ---- C ABI (no compute calls) ----
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from metran_amd import _lib

    if not os.path.exists(_lib.library_path()):
        g.build()
    return _lib.lib()


NEW = ("mk_draw_perturb", "mk_draw_combine", "mk_draw_normals")


def test_draw_entry_points_declared_and_exported(lib):
    from metran_amd import _lib

    src = open(os.path.join(ROOT, "include", "metran_hip.h")).read()
    declared = re.findall(r"MK_API\s+[\w\s\*]+?\b(mk_\w+)\s*\(", src)
    for name in NEW:
        assert name in declared and name in _lib.API and hasattr(lib, name)
    assert lib.mk_abi_version() == 7


def test_draw_calls_without_a_context_fail_with_a_message(lib):
    """No context (what a machine without a GPU has: mk_create fails there): a status and a message, no crash."""
    from metran_amd._lib import Problem

    prob = Problem(1, 1, 4, 8, 2, 0, None, None, None, None, None, None, None, 0, None, None)
    assert lib.mk_draw_perturb(None, ctypes.byref(prob), 1, 0, 0, 1, 0, None, None, None, None) == -1
    assert b"context" in lib.mk_last_error()
    assert lib.mk_draw_combine(None, ctypes.byref(prob), 1, 0, 0, None, None) == -1
    assert b"context" in lib.mk_last_error()
    assert lib.mk_draw_normals(None, 1, 0, 1, 0, 1, 0, 4, 10, 0, None) == -1
    assert b"context" in lib.mk_last_error()


def test_draw_kernels_use_no_scratch(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc is needed to inspect the kernels' resource usage")
    out = tmp_path / "draw_kernels.s"
    csrc = os.path.join(ROOT, "metran_amd", "csrc")
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + csrc,
                           "--cuda-device-only", "-S", os.path.join(csrc, "draw_kernels.hip"), "-o", str(out)],
                          stderr=subprocess.DEVNULL)
    text = out.read_text()
    names = re.findall(r"^\s+\.name:\s+(\S*draw_\w+_kernel\S*)", text, re.M)
    assert len(names) == 3, names
    assert re.findall(r"^\s+\.private_segment_fixed_size:\s+(\d+)", text, re.M) == ["0"] * 3
    assert "scratch_" not in text


# ---- MetranBatch over a stand-in engine ----
def _stand_in(models, loadings):
    """A MetranBatch whose engine answers from the oracle and the restatement (the constructor itself needs a GPU)."""
    import torch

    from batch_standin import stand_in
    from oracle_engine import OracleEngine

    class DrawEngine(OracleEngine):
        scale = offset = None
        status_bits = 0

        def set_scaling(self, scale=None, offset=None):
            self.scale, self.offset = scale, offset
            return self

        def draw_smoothed(self, phi, q, ndraws, seed=0, what="series", x0=None, P0=None, antithetic=False, first_draw=0,
                          first_instance=0, chunk=None):
            phi, q = self._dev(phi).numpy(), self._dev(q).numpy()
            out = []
            for i, r in enumerate(self._records(phi.shape[0])):
                sc = None if self.scale is None else self.scale[r].numpy()
                of = None if self.offset is None else self.offset[r].numpy()
                out.append(draw_ref.draw_model(oracle, self.obs_np[r], phi[i], q[i], self.load_np[r], ndraws, seed, first_instance + i,
                                               what, scale=sc, offset=of, antithetic=antithetic, first_draw=first_draw))
            status = torch.full((ndraws, phi.shape[0]), self.status_bits, dtype=torch.int32)
            return {"draws": torch.from_numpy(np.stack(out, axis=1)), "status": status}

    return stand_in(DrawEngine, models, loadings)


def test_metran_batch_accessors_over_a_stand_in_engine():
    from batch_standin import two_models
    from metran_amd._lib import MetranHipError

    models, G = two_models()
    mb = _stand_in(models, G)
    alpha = np.full((2, 4), 8.0)
    S = 3
    d = mb.get_simulation_draws(S, seed=5, alpha=alpha)
    assert tuple(d.shape) == (S, 2, mb.T, 3)
    ds = mb.get_simulation_draws(S, seed=5, alpha=alpha, standardized=True)
    np.testing.assert_allclose(ds.numpy() * mb._std.numpy()[None, :, None, :] + mb._mean.numpy()[None, :, None, :], d.numpy(), rtol=0, atol=1e-12)
    obs = mb.kf.obs_np
    seen = np.isfinite(obs)
    for s in range(S):
        assert np.abs(ds.numpy()[s][seen] - obs[seen]).max() <= TOL           # standardised draws return the standardised records
    x = mb.get_state_draws(S, seed=5, alpha=alpha)
    assert tuple(x.shape) == (S, 2, mb.T, 4)
    # the series draw is the projection of the state draw of the same counters
    Z = np.concatenate([np.broadcast_to(np.eye(3), (2, 3, 3)), G], axis=2)
    np.testing.assert_allclose(np.einsum("rjn,srtn->srtj", Z, x.numpy()), ds.numpy(), rtol=0, atol=1e-9)
    frame = mb.get_simulation_draw(1, "s2", S, seed=5, alpha=alpha)
    L = int(mb.batch.lengths[1])
    assert frame.shape == (L, S) and list(frame.columns) == ["draw0", "draw1", "draw2"] and frame.index.equals(mb.batch.index[1])
    np.testing.assert_array_equal(frame.values, d.numpy()[:, 1, :L, 2].T)
    with pytest.raises(KeyError, match="Unknown name"):
        mb.get_simulation_draw(0, "nope", S, alpha=alpha)
    # a sharded batch numbers its instances from the rank's offset
    mb.shard = (7, 9)
    d7 = mb.get_simulation_draws(1, seed=5, alpha=alpha)
    want = draw_ref.draw_model(oracle, obs[1], *[a[1] for a in _phi_q(alpha, G)], G[1], 1, 5, 8, "series",
                               scale=mb._std.numpy()[1], offset=mb._mean.numpy()[1])
    np.testing.assert_allclose(d7.numpy()[0, 1], want[0], rtol=0, atol=1e-12)
    mb.shard = (0, 2)
    mb.kf.status_bits = 1   # FLAG_NONPOSITIVE_F
    with pytest.raises(MetranHipError, match="innovation variance"):
        mb.get_state_draws(1, alpha=alpha)


def _phi_q(alpha, G):
    from metran_amd.params import phi_q_from_alpha

    return phi_q_from_alpha(np.asarray(alpha, float), G, 1.0)
