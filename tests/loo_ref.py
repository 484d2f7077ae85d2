"""numpy restatement of the LEAVE-ONE-OUT predictions (test infrastructure): for every observed cell (t, j) the prediction of
y_tj from every other observation, parameters held fixed -- what Metran's worked example gets by masking the cell
(mask_observations, metran.py:464-506), re-running the smoother and reading get_simulation (metran.py:831-883) at that cell.

de Jong's deletion result for the sequential filter's scalar update (t, j) -- innovation v, variance f, gain k, and the
Durbin-Koopman backward quantities r, N as they stand just after that update (zero behind the last step):
    u = v/f - k.r,   D = 1/f + k'N k,   E[y_tj | others] = y_tj - u/D,   Var[z_j x_t | others] = 1/D - R_j
Two restatements of it, one per backward walk of the library:
  loo_tape      the tape walk of tests/dk_ref.py (mk_dk.hip): beta = kt.r and alpha = kt'N kt are formed there anyway
                (observable basis; kt = T k leaves both scalars unchanged), entry (s0, s1, s2) = (v/f, 1/f, y)
  loo_adjoint   the adjoint walk of tests/adjoint_ref.py (mk_kernels.hip::adjoint_kernel) with unit weights on every step:
                xb = -2 r and Pb = N - r r', so with a = xb.d and c = d'Pb d (d = P z_j' = f k)
                E = y - f (v + a/2) / (f + c + a^2/4),   Var = f^2 / (f + c + a^2/4) - R_j
and the brute force they are checked against: mask the one cell, run the reference algorithm with smoothing (oracle/) and
project the smoothed moments of step t on z_j.
"""
import numpy as np

import dk_ref


def loo_tape(obs, phi, q, loadings, obsvar=None, x0=None, P0=None):
    """One model, obs [T,N] (NaN = missing).  -> (means [T,N], variances [T,N]) of the deletion predictions, NaN where the
    cell is not observed (unscaled)."""
    tape = dk_ref.filter_tape(obs, phi, q, loadings, obsvar, x0, P0)
    Tn, N, ES = tape.shape
    n = ES - 4
    R = np.zeros(N) if obsvar is None else np.asarray(obsvar, float)
    Pht = dk_ref.transition(phi, loadings)
    r = np.zeros(n)
    Nm = np.zeros((n, n))
    means, variances = np.full((Tn, N), np.nan), np.full((Tn, N), np.nan)
    for t in range(Tn - 1, -1, -1):
        seen = ~np.isnan(tape[t, :, n + 2])
        for j in np.nonzero(seen)[0][::-1]:
            e = tape[t, j]
            k = e[:n]
            w = Nm @ k
            beta = k @ r
            alpha = k @ w
            D = e[n + 1] + alpha
            means[t, j] = e[n + 2] - (e[n] - beta) / D
            variances[t, j] = 1.0 / D - R[j]
            r[j] += e[n] - beta
            col = Nm[:, j] - w
            col[j] = Nm[j, j] - 2.0 * w[j] + alpha + e[n + 1]
            Nm[:, j] = col
            Nm[j, :] = col
        r = Pht.T @ r
        Nm = Pht.T @ Nm @ Pht
    return means, variances


def loo_adjoint(obs, phi, q, loadings, obsvar=None, x0=None, P0=None):
    """The same predictions through the adjoint walk (unit weights, no warm-up): the forward recursion of
    tests/adjoint_ref.py, then its backward pass with the deletion pair read off each update's (a, c)."""
    Tn, N = obs.shape
    K = loadings.shape[1]
    n = N + K
    R = np.zeros(N) if obsvar is None else np.asarray(obsvar, float)
    xi = np.zeros(n) if x0 is None else np.array(x0, float)
    Pi = np.eye(n) if P0 is None else np.array(P0, float)
    Z = np.concatenate([np.eye(N), loadings], axis=1)
    F, Pf = np.zeros((Tn, n)), np.zeros((Tn, n, n))
    x, P = xi.copy(), Pi.copy()
    for t in range(Tn):
        x = phi * x
        P = np.outer(phi, phi) * P + np.diag(q)
        for j in np.nonzero(np.isfinite(obs[t]))[0]:
            z = Z[j]
            v = obs[t, j] - z @ x
            d = P @ z
            f = z @ d + R[j]
            x = x + d * v / f
            P = P - np.outer(d, d) / f
        F[t], Pf[t] = x, P
    means, variances = np.full((Tn, N), np.nan), np.full((Tn, N), np.nan)
    xb, Pb = np.zeros(n), np.zeros((n, n))
    for t in range(Tn - 1, -1, -1):
        x = phi * (F[t - 1] if t > 0 else xi)
        P = np.outer(phi, phi) * (Pf[t - 1] if t > 0 else Pi) + np.diag(q)
        st = []
        for j in np.nonzero(np.isfinite(obs[t]))[0]:
            z = Z[j]
            v = obs[t, j] - z @ x
            d = P @ z
            f = z @ d + R[j]
            st.append((j, z, v, d, f))
            x = x + d * v / f
            P = P - np.outer(d, d) / f
        for j, z, v, d, f in reversed(st):
            rf = 1.0 / f
            a, b = xb @ d, Pb @ d
            c = d @ b
            den = f + c + 0.25 * a * a
            means[t, j] = obs[t, j] - f * (v + 0.5 * a) / den
            variances[t, j] = f * f / den - R[j]
            vbar = (2 * v + a) * rf
            fbar = ((1 - v * v * rf) - a * v * rf + c * rf) * rf
            dbar = xb * v * rf - 2 * b * rf + fbar * z
            xb = xb - vbar * z
            Pb = Pb + 0.5 * (np.outer(dbar, z) + np.outer(z, dbar))
        Pb = np.outer(phi, phi) * Pb
        xb = phi * xb
    return means, variances


def loo_brute(oracle, obs, phi, q, loadings, cells, obsvar=None, x0=None, P0=None):
    """Mask each cell (t, j) of ``cells`` alone, smooth with the reference algorithm and project: -> (means, variances) [len(cells)].
    oracle.dfm_batch where the initial moments are the defaults, the seqkalmanfilter / kalmansmoother pair otherwise."""
    N, K = loadings.shape
    n = N + K
    Z = np.concatenate([np.eye(N), loadings], axis=1)
    R = np.zeros(N) if obsvar is None else np.asarray(obsvar, float)
    out_m, out_v = [], []
    for t, j in cells:
        y = np.array(obs, float)
        y[t, j] = np.nan
        if x0 is None and P0 is None:
            res = oracle.dfm_batch(y[None], phi[None], q[None], loadings[None], None if obsvar is None else R[None], smooth=True)
            S, Ps = res["S"][0], res["Ps"][0]
        else:
            o, oi, oc = oracle.set_observations(y)
            xi = np.zeros(n) if x0 is None else x0
            Pi = np.eye(n) if P0 is None else P0
            _, _, _, F, Pf, Xp, Pp = oracle.seqkalmanfilter(o, np.diag(phi), np.diag(q), Z, R, oi, oc, xi, Pi)
            S, Ps = oracle.kalmansmoother(F, Pf, Xp, Pp, np.diag(phi))
        out_m.append(Z[j] @ S[t])
        out_v.append(Z[j] @ Ps[t] @ Z[j])
    return np.array(out_m), np.array(out_v)


def sample_cells(obs, rng, count=12):
    """Observed cells to check: the first and last observed steps, a step with one observed series, a fully observed step,
    and ``count`` more at random."""
    obs = np.asarray(obs)
    seen = np.isfinite(obs)
    rows = np.nonzero(seen.any(1))[0]
    cells = []

    def add_row(t):
        js = np.nonzero(seen[t])[0]
        cells.append((int(t), int(js[rng.integers(js.size)])))

    add_row(rows[0])
    add_row(rows[-1])
    cnt = seen.sum(1)
    for want in (1, obs.shape[1]):
        hit = np.nonzero(cnt == want)[0]
        if hit.size:
            add_row(hit[rng.integers(hit.size)])
    allc = np.argwhere(seen)
    for i in rng.choice(len(allc), size=min(count, len(allc)), replace=False):
        cells.append((int(allc[i][0]), int(allc[i][1])))
    return list(dict.fromkeys(cells))
