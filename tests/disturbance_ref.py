"""numpy restatements of the SMOOTHED STATE DISTURBANCES (test infrastructure): for the state equation of the filter
    x_init ~ N(x0, P0),   x_t = phi o x_{t-1} + eta_t,  eta_t ~ N(0, diag q)   (x_{-1} = x_init),   y_t = Z x_t + eps_t
the Durbin-Koopman backward pair (r_t, N_t) of every step, from which
    E[eta_t,i | Y] = q_i r_t,i      Var[eta_t,i | Y] = q_i - q_i^2 N_t,ii      u_t,i = r_t,i / sqrt(N_t,ii)
(u: the auxiliary residual of Harvey & Koopman 1992).  Three restatements, each by another route:
  dist_adjoint     the kernel's walk: tests/loo_ref.py::loo_adjoint (unit weights on every step) with the read-out added --
                   r_t = -xb/2 and N_t = Pb + r_t r_t' once the updates of step t are pulled back, before the pull-back through Phi
  dist_definition  from the oracle's filtered / predicted / smoothed moments: mean S_t - phi o S_{t-1}, variance through the
                   lag-one covariance C = J_{t-1} Ps_t, J_{t-1} = Pf_{t-1} Phi Pp_t^-1; t >= 1 (row 0 is NaN)
  dist_joint       the dense joint Gaussian of (x_init, eta_0 .. eta_{T-1}) conditioned on the observed cells (small T and n);
                   the only one that covers t = 0 and the caller's x0 / P0 directly
"""
import numpy as np


def dist_adjoint(obs, phi, q, loadings, obsvar=None, x0=None, P0=None, variant=None, dtype=np.float64):
    """One model, obs [T,N] (NaN = missing).  -> (r [T,n], ninfo [T,n]) = (r_t, diag N_t), as the kernels store them (a
    negative diagonal from rounding is 0).  ``variant``: a deliberately WRONG read-out, for the tests that show the right one
    can be told from it -- "after_phi" (read after the pull-back through Phi), "before_updates" (read before the step's
    updates are pulled back), "no_rr" (Pb's diagonal without the r^2 term), "shifted" (outputs one step late).  ``dtype``: the
    arithmetic of both passes -- ``np.float64`` (the default) or ``np.longdouble``, the yardstick of the property sweep."""
    obs = np.asarray(obs, float)
    Tn, N = obs.shape
    K = loadings.shape[1]
    n = N + K
    phi, q = np.asarray(phi, dtype=dtype), np.asarray(q, dtype=dtype)
    R = np.zeros(N, dtype=dtype) if obsvar is None else np.asarray(obsvar, dtype=dtype)
    xi = np.zeros(n, dtype=dtype) if x0 is None else np.array(x0, dtype=dtype)
    Pi = np.eye(n, dtype=dtype) if P0 is None else np.array(P0, dtype=dtype)
    Z = np.concatenate([np.eye(N), loadings], axis=1).astype(dtype)
    F, Pf = np.zeros((Tn, n), dtype=dtype), np.zeros((Tn, n, n), dtype=dtype)
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
    rr, nn = np.zeros((Tn, n), dtype=dtype), np.zeros((Tn, n), dtype=dtype)

    def read(t, xb, Pb):
        r = -0.5 * xb
        rr[t] = r
        nn[t] = np.diag(Pb) + (0.0 if variant == "no_rr" else r * r)

    xb, Pb = np.zeros(n, dtype=dtype), np.zeros((n, n), dtype=dtype)
    for t in range(Tn - 1, -1, -1):
        x = phi * (F[t - 1] if t > 0 else xi)
        P = np.outer(phi, phi) * (Pf[t - 1] if t > 0 else Pi) + np.diag(q)
        st = []
        for j in np.nonzero(np.isfinite(obs[t]))[0]:
            z = Z[j]
            v = obs[t, j] - z @ x
            d = P @ z
            f = z @ d + R[j]
            st.append((z, v, d, f))
            x = x + d * v / f
            P = P - np.outer(d, d) / f
        if variant == "before_updates":
            read(t, xb, Pb)
        for z, v, d, f in reversed(st):
            rf = 1.0 / f
            a, b = xb @ d, Pb @ d
            c = d @ b
            vbar = (2 * v + a) * rf
            fbar = ((1 - v * v * rf) - a * v * rf + c * rf) * rf
            dbar = xb * v * rf - 2 * b * rf + fbar * z
            xb = xb - vbar * z
            Pb = Pb + 0.5 * (np.outer(dbar, z) + np.outer(z, dbar))
        if variant in (None, "no_rr", "shifted"):
            read(t, xb, Pb)
        Pb = np.outer(phi, phi) * Pb
        xb = phi * xb
        if variant == "after_phi":
            read(t, xb, Pb)
    if variant == "shifted":
        rr, nn = np.roll(rr, 1, axis=0), np.roll(nn, 1, axis=0)
    return rr, np.where(nn < 0.0, 0.0, nn)


def moments(q, r, ninfo):
    """(E[eta | Y], Var[eta | Y]) from the raw pair."""
    return q * r, q - q * q * ninfo


def dist_definition(phi, q, F, Pf, Xp, Pp, S, Ps):
    """From the filter's and the smoother's moments of one model ([T,n] / [T,n,n], as the oracle returns them): -> (mean, var)
    [T,n] of eta_t given all data for t >= 1, row 0 NaN.  With J = Pf_{t-1} Phi Pp_t^-1 and C = Cov(x_{t-1}, x_t | Y) = J Ps_t:
    Var[x_t - Phi x_{t-1} | Y] = Ps_t + Phi Ps_{t-1} Phi - Phi C - C' Phi."""
    Tn, n = S.shape
    Ph = np.diag(phi)
    mean, var = np.full((Tn, n), np.nan), np.full((Tn, n), np.nan)
    for t in range(1, Tn):
        J = np.linalg.solve(Pp[t].T, (Pf[t - 1] @ Ph).T).T
        C = J @ Ps[t]
        V = Ps[t] + Ph @ Ps[t - 1] @ Ph - Ph @ C - C.T @ Ph
        mean[t] = S[t] - phi * S[t - 1]
        var[t] = np.diag(V)
    return mean, var


def dist_joint(obs, phi, q, loadings, obsvar=None, x0=None, P0=None):
    """The dense joint Gaussian: w = (x_init - x0, eta_0 .. eta_{T-1}) ~ N(0, blockdiag(P0, Q, .., Q)), every observed cell a
    linear function of w plus noise; -> (mean, var) [T,n] of eta_t given the observed cells, t = 0 included."""
    obs = np.asarray(obs, float)
    Tn, N = obs.shape
    K = loadings.shape[1]
    n = N + K
    assert Tn <= 6 and n <= 6, "the dense reference is for small models"
    R = np.zeros(N) if obsvar is None else np.asarray(obsvar, float)
    xi = np.zeros(n) if x0 is None else np.asarray(x0, float)
    Pi = np.eye(n) if P0 is None else np.asarray(P0, float)
    Z = np.concatenate([np.eye(N), loadings], axis=1)
    m = n * (Tn + 1)
    W = np.zeros((m, m))
    W[:n, :n] = Pi
    for t in range(Tn):
        W[n * (t + 1):n * (t + 2), n * (t + 1):n * (t + 2)] = np.diag(q)
    # x_t = A_t w + phi^(t+1) x0
    A = np.zeros((Tn, n, m))
    c = np.zeros((Tn, n))
    prevA, prevc = np.concatenate([np.eye(n), np.zeros((n, m - n))], axis=1), xi.copy()
    for t in range(Tn):
        At = phi[:, None] * prevA
        At[:, n * (t + 1):n * (t + 2)] += np.eye(n)
        A[t], c[t] = At, phi * prevc
        prevA, prevc = At, c[t]
    rows, resid, noise = [], [], []
    for t in range(Tn):
        for j in np.nonzero(np.isfinite(obs[t]))[0]:
            rows.append(Z[j] @ A[t])
            resid.append(obs[t, j] - Z[j] @ c[t])
            noise.append(R[j])
    mean, var = np.zeros((Tn, n)), np.tile(q, (Tn, 1)).astype(float)
    if rows:
        H = np.array(rows)
        Sy = H @ W @ H.T + np.diag(noise)
        G = np.linalg.solve(Sy, H @ W).T          # W H' Sy^-1
        wm = G @ np.array(resid)
        Wc = W - G @ H @ W
        for t in range(Tn):
            mean[t] = wm[n * (t + 1):n * (t + 2)]
            var[t] = np.diag(Wc)[n * (t + 1):n * (t + 2)]
    return mean, var
