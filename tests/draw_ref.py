"""numpy restatement of the SIMULATION SMOOTHER by mean correction (test infrastructure; Durbin & Koopman 2002): the
counter-based normals (Philox4x32-10 in uint64 arithmetic, 52-bit uniforms, Box-Muller), the unconditional path x+, the
perturbed record y* and the draws, smoothing with the reference algorithm (oracle/), as tests/loo_ref.py does for its feature.

Model (seqkalmanfilter, kalmanfilter.py:315-333): x_{-1} ~ N(x0, P0), x_t = phi o x_{t-1} + w_t, y_t = [I | Gamma] x_t + e_t.
Draw s of instance i:
    x+_{-1} = L0 z_init,  x+_t = phi o x+_{t-1} + sqrt(q) o z_t[0:n],  y+_t = [I | Gamma] x+_t + sqrt(R) o z_t[n:n+N]
    y* = y - y+ where observed, NaN elsewhere;   states: x+ + E[x | y*];   series: scale o ([I | Gamma] x+) + sim_means(y*)
Normals: key (seed & 0xffffffff, seed >> 32), counter (t + 1, c >> 1, first_instance + i, d); t + 1 = 0 is the initial state.
"""
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four broadcastable integer arrays (words 0..3), key: two ints -> four uint64 arrays holding 32-bit words."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & MASK for c in np.broadcast_arrays(*counter))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2                      # 32 x 32 -> 64 bits: exact in uint64
        c0, c1, c2, c3 = (p1 >> S32) ^ c1 ^ np.uint64(k0), p1 & MASK, (p0 >> S32) ^ c3 ^ np.uint64(k1), p0 & MASK
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


def mantissas(seed, step1, pair, inst, d):
    """The two 52-bit integers (m1, m2) of a counter (uint64 arrays)."""
    seed = int(seed)
    w0, w1, w2, w3 = philox4x32_10((step1, pair, inst, d), (seed & 0xFFFFFFFF, seed >> 32))
    six, s26 = np.uint64(6), np.uint64(26)
    return ((w0 >> six) << s26) + (w1 >> six), ((w2 >> six) << s26) + (w3 >> six)


def uniforms(m):
    return (m.astype(np.float64) + 0.5) * 2.0 ** -52


def normal_block(seed, first_instance, ninstances, first_draw, ndraws, antithetic, T, ncomp, raw=False):
    """[ndraws, ninstances, T + 1, ncomp]: the normals of a block of counters (time index 0 = the initial state); raw: the
    integers m1 (even c) / m2 (odd c) as doubles."""
    s = first_draw + np.arange(ndraws)[:, None, None, None]
    i = first_instance + np.arange(ninstances)[None, :, None, None]
    tt = np.arange(T + 1)[None, None, :, None]
    c = np.arange(ncomp)[None, None, None, :]
    d = s >> 1 if antithetic else s
    m1, m2 = mantissas(seed, tt, c >> 1, i, d)
    even = np.broadcast_to(c % 2 == 0, m1.shape)
    if raw:
        return np.where(even, m1, m2).astype(np.float64)
    rho = np.sqrt(-2.0 * np.log(uniforms(m1)))
    ang = (2.0 * np.pi) * uniforms(m2)
    z = rho * np.where(even, np.cos(ang), np.sin(ang))
    if antithetic:
        z = z * np.where(s % 2 == 1, -1.0, 1.0)
    return z


def unconditional(obs, phi, q, loadings, z, obsvar=None, L0=None):
    """One path.  obs [T,N] (NaN = missing), z [T + 1, ncomp] its normals -> (xplus [T,n], zxplus [T,N], yplus [T,N], ystar [T,N])."""
    T, N = obs.shape
    n = phi.size
    Z = np.concatenate([np.eye(N), loadings], axis=1)
    x = z[0, :n].copy() if L0 is None else np.tril(L0) @ z[0, :n]
    xp, zx, yp = np.empty((T, n)), np.empty((T, N)), np.empty((T, N))
    for t in range(T):
        x = phi * x + np.sqrt(q) * z[t + 1, :n]
        xp[t] = x
        zx[t] = Z @ x
        yp[t] = zx[t] + (np.sqrt(obsvar) * z[t + 1, n:n + N] if obsvar is not None else 0.0)
    ystar = np.where(np.isfinite(obs), obs - yp, np.nan)
    return xp, zx, yp, ystar


def smooth(oracle, obs, phi, q, loadings, obsvar=None, x0=None, P0=None):
    """Smoothed state means / covariances of one model with the reference algorithm."""
    N, K = loadings.shape
    n = N + K
    Z = np.concatenate([np.eye(N), loadings], axis=1)
    R = np.zeros(N) if obsvar is None else np.asarray(obsvar, float)
    o, oi, oc = oracle.set_observations(np.array(obs, float))
    xi = np.zeros(n) if x0 is None else np.asarray(x0, float)
    Pi = np.eye(n) if P0 is None else np.asarray(P0, float)
    _, _, _, F, Pf, Xp, Pp = oracle.seqkalmanfilter(o, np.diag(phi), np.diag(q), Z, R, oi, oc, xi, Pi)
    return oracle.kalmansmoother(F, Pf, Xp, Pp, np.diag(phi))


def draw_model(oracle, obs, phi, q, loadings, ndraws, seed=0, instance=0, what="series", obsvar=None, x0=None, P0=None,
               scale=None, offset=None, antithetic=False, first_draw=0, parts=False):
    """Draws of ONE instance (global instance number ``instance``): [ndraws,T,N] (series) or [ndraws,T,n] (states).
    parts: also the list of (xplus, zxplus, yplus, ystar) per draw."""
    T, N = obs.shape
    n = phi.size
    Z = np.concatenate([np.eye(N), loadings], axis=1)
    ncomp = n + (N if obsvar is not None else 0)
    L0 = None if P0 is None else np.linalg.cholesky(P0)
    z = normal_block(seed, instance, 1, first_draw, ndraws, antithetic, T, ncomp)[:, 0]
    sc = np.ones(N) if scale is None else np.asarray(scale, float)
    of = np.zeros(N) if offset is None else np.asarray(offset, float)
    out, kept = [], []
    for s in range(ndraws):
        xp, zx, yp, ystar = unconditional(obs, phi, q, loadings, z[s], obsvar, L0)
        S, _ = smooth(oracle, ystar, phi, q, loadings, obsvar, x0, P0)
        out.append(xp + S if what == "states" else sc * zx + (sc * (S @ Z.T) + of))
        kept.append((xp, zx, yp, ystar))
    out = np.array(out)
    return (out, kept) if parts else out


def posterior_dense(obs, phi, q, loadings, obsvar=None, x0=None, P0=None):
    """Exact posterior mean and covariance of the stacked projected series Z x_t (all T * N cells, row-major (t, j)) given the
    observed cells, by dense Gaussian conditioning: the joint law of all states is built explicitly."""
    T, N = obs.shape
    n = phi.size
    Z = np.concatenate([np.eye(N), loadings], axis=1)
    R = np.zeros(N) if obsvar is None else np.asarray(obsvar, float)
    m = np.zeros(n) if x0 is None else np.asarray(x0, float)
    P = np.eye(n) if P0 is None else np.asarray(P0, float)
    Phi = np.diag(phi)
    means, covs = [], []
    for t in range(T):
        m = Phi @ m
        P = Phi @ P @ Phi.T + np.diag(q)
        means.append(m)
        covs.append(P)
    C = np.zeros((T * n, T * n))                      # Cov(x_t, x_u) = Phi^(t-u) Cov(x_u) for t >= u
    for u in range(T):
        blk = covs[u]
        for t in range(u, T):
            C[t * n:(t + 1) * n, u * n:(u + 1) * n] = blk
            C[u * n:(u + 1) * n, t * n:(t + 1) * n] = blk.T
            blk = Phi @ blk
    ZZ = np.kron(np.eye(T), Z)                        # projected series of every step
    mu = ZZ @ np.concatenate(means)
    Cs = ZZ @ C @ ZZ.T                                # Cov of Z x
    seen = np.isfinite(obs).ravel()
    y = obs.ravel()[seen]
    Syy = Cs[np.ix_(seen, seen)] + np.diag(np.tile(R, T)[seen])
    Ksy = Cs[:, seen]
    sol = np.linalg.solve(Syy, np.concatenate([(y - mu[seen])[:, None], Ksy.T], axis=1))
    return mu + Ksy @ sol[:, 0], Cs - Ksy @ sol[:, 1:]
