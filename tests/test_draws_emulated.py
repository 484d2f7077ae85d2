"""Posterior draws, CPU tier: the kernels of draw_kernels.hip themselves, compiled for the host (tests/draw_host_emulation.py:
a workgroup as 256 threads and a barrier), against the numpy restatement -- the generator bit for bit, the unconditional
paths and perturbed records in both layouts across several tiles of steps, the combine step."""
import numpy as np
import pytest

import draw_ref
from draw_host_emulation import build, ptr
from metran_amd.synthetic import make_dfm_batch


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    return build(tmp_path_factory.mktemp("draw_emulation"))


def test_generator_bit_for_bit(emu):
    seed = 0x9E3779B97F4A7C15
    out = np.full((3, 4, 26, 17), np.nan)
    assert emu.run_normals(seed, 3, 4, 2, 3, 25, 17, 0, 1, ptr(out)) == 0
    assert np.array_equal(out, draw_ref.normal_block(seed, 3, 4, 2, 3, False, 25, 17, raw=True))
    for anti in (0, 1):
        out = np.full((5, 6, 41, 13), np.nan)
        assert emu.run_normals(77, 5, 6, 3, 5, 40, 13, anti, 0, ptr(out)) == 0
        assert np.abs(out - draw_ref.normal_block(77, 5, 6, 3, 5, bool(anti), 40, 13)).max() <= 1e-13


# (8,2): 16 paths per block; (11,6): factors beyond the four kept in registers; (32,4): one wavefront per path; (70,3): two
@pytest.mark.parametrize("shape", [(8, 2, 5), (11, 6, 3), (32, 4, 3), (70, 3, 1)], ids=lambda s: "%dx%d_B%d" % s)
@pytest.mark.parametrize("full", [False, True], ids=["defaults", "P0_R"])
def test_perturb_kernel_matches_the_restatement(emu, shape, full):
    N, K, B = shape
    n = N + K
    T, S, seed, fi, fd = 37, 3, 4242, 4, 3              # 38 steps with the initial one: more than one tile of at most 32
    d = make_dfm_batch(B, N, K, T, seed=n, missing=0.3)
    obs = d["obs"].copy()
    obs[:, 0] = np.nan
    obs[B - 1, :, N - 1] = np.nan
    rng = np.random.default_rng(1)
    R = rng.uniform(0.05, 0.4, (B, N)) if full else None
    A = rng.normal(size=(B, n, n))
    L0 = np.ascontiguousarray(np.linalg.cholesky(A @ A.transpose(0, 2, 1) / n + 0.5 * np.eye(n))) if full else None
    phi, q, G = (np.ascontiguousarray(d[k]) for k in ("phi", "q", "loadings"))
    results = []
    for tm in (0, 1):
        for anti in (0, 1):
            om = np.ascontiguousarray(obs.transpose(1, 0, 2)) if tm else np.ascontiguousarray(obs)
            ys, zx, xp = (np.full((T, S * B, w) if tm else (S * B, T, w), 7.0) for w in (N, N, n))
            assert emu.run_perturb(B, B, T, N, K, S, tm, seed, fi, fd, anti, ptr(om), ptr(phi), ptr(q), ptr(G), ptr(R), ptr(L0),
                                   ptr(ys), ptr(zx), ptr(xp)) == 0
            if tm:
                ys, zx, xp = (a.transpose(1, 0, 2) for a in (ys, zx, xp))
            ys, zx, xp = (a.reshape(S, B, T, -1) for a in (ys, zx, xp))
            z = draw_ref.normal_block(seed, fi, B, fd, S, bool(anti), T, n + (N if full else 0))
            for s in range(S):
                for i in range(B):
                    rx, rzx, _, rys = draw_ref.unconditional(obs[i], phi[i], q[i], G[i], z[s, i], None if R is None else R[i],
                                                            None if L0 is None else L0[i])
                    seen = np.isfinite(obs[i])
                    assert np.array_equal(np.isnan(ys[s, i]), ~seen)
                    assert np.abs(xp[s, i] - rx).max() <= 1e-11 and np.abs(zx[s, i] - rzx).max() <= 1e-11
                    assert np.abs(ys[s, i][seen] - rys[seen]).max() <= 1e-11
            results.append((anti, ys, zx, xp))
    for (a0, *m), (a1, *t) in zip(results[:2], results[2:]):     # model-major against time-major: the same numbers
        assert a0 == a1 and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(m, t))


def test_combine_kernel(emu):
    SB, B, R, T, W = 6, 3, 3, 5, 4
    rng = np.random.default_rng(0)
    for tm in (0, 1):
        plus = rng.normal(size=(T, SB, W) if tm else (SB, T, W))
        io = rng.normal(size=plus.shape)
        sc = rng.uniform(1, 2, (R, W))
        rows = sc[(np.arange(SB) % B) % R]
        want = io + (rows[None] if tm else rows[:, None]) * plus
        assert emu.run_combine(SB, B, R, T, W, tm, ptr(sc), ptr(plus), ptr(io)) == 0
        assert np.abs(io - want).max() <= 1e-15
        io2 = io.copy()
        assert emu.run_combine(SB, B, R, T, W, tm, None, ptr(plus), ptr(io2)) == 0     # states: no scale
        assert np.array_equal(io2, io + plus)
