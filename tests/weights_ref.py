"""numpy restatement of the observation weights of smoothed series and states (C ABI mk_observation_weights; the recursions of
include/metran_hip.h, after Koopman & Harvey 2003): for fixed parameters the smoother is linear in the data, so a projected
smoothed mean c' x_{t*|T} is  sum w_{t,j} y_{t,j} + intercept  over the observed cells of the record.

``gains`` is a plain filter loop (prediction first, then the observed series of the step in ascending order, Z = [I | G]) that
keeps d = P z_j' and 1 / f of every scalar update and the predicted covariance of every step; ``weights`` walks forward from the
target's step and backward over the whole record.  Plain loops, sums left to right, in ``dtype`` arithmetic (``np.longdouble``
the default: the yardstick of the GPU tests; ``np.float64`` for the bar).  Three deliberately WRONG variants exist so that the
tests can show they would notice: ``stop_at_target`` (the forward walk ends with the target's step: the weights of the FILTERED
estimate), ``no_c`` (the backward walk forgets to add c at the target's step) and ``descending`` (the series of a step taken in
descending order by both walks, on the gains of the ascending filter)."""
import numpy as np


def _Z(G, dtype):
    N, K = G.shape
    Z = np.zeros((N, N + K), dtype=dtype)
    Z[:, :N] = np.eye(N, dtype=dtype)
    Z[:, N:] = G
    return Z


def _dot(a, b, dtype, cols=None):
    s = dtype(0)
    for c in (range(len(a)) if cols is None else cols):
        s = s + a[c] * b[c]
    return s


def _cols(N, n):
    return [[j] + list(range(N, n)) for j in range(N)]   # the non-zero entries of z_j, in column order


def gains(y, phi, q, G, R=None, x0=None, P0=None, dtype=np.longdouble):
    """dict of one model: ``d [T,N,n]`` = P z_j' and ``rf [T,N]`` = 1 / f of every scalar update (zeros at a cell that is not
    observed), ``Pp [T,n,n]`` the predicted covariance of every step."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    phi, q = np.asarray(phi, dtype=dtype), np.asarray(q, dtype=dtype)
    Z = _Z(np.asarray(G, dtype=dtype), dtype)
    R = np.zeros(N, dtype=dtype) if R is None else np.asarray(R, dtype=dtype)
    P = np.eye(n, dtype=dtype) if P0 is None else np.asarray(P0, dtype=dtype)
    d = np.zeros((T, N, n), dtype=dtype)
    rf = np.zeros((T, N), dtype=dtype)
    Pp = np.empty((T, n, n), dtype=dtype)
    cols = _cols(N, n)
    for t in range(T):
        P = (phi[:, None] * P) * phi[None, :] + np.diag(q)
        Pp[t] = P
        for j in range(N):
            if not np.isfinite(y[t, j]):
                continue
            dj = np.zeros(n, dtype=dtype)
            for c in cols[j]:
                dj = dj + P[:, c] * Z[j, c]
            f = R[j] + _dot(Z[j], dj, dtype, cols[j])
            d[t, j], rf[t, j] = dj, dtype(1) / f
            k = dj * rf[t, j]
            P = P - k[:, None] * dj[None, :]
    return {"d": d, "rf": rf, "Pp": Pp}


def weights(y, phi, q, G, R=None, x0=None, P0=None, targets=(), what="series", dtype=np.longdouble, gain=None,
            stop_at_target=False, no_c=False, descending=False):
    """(w [M,T,N], intercept [M]) of one model for the targets ``(step, column)``: column = series j* (``what="series"``, c = z_j*)
    or state i (``what="states"``, c = e_i).  NaN at every cell that is not observed; a target with its step outside [0, T) or its
    column outside [0, N) / [0, n) has an all-NaN row and a NaN intercept.  ``gain``: the dict of ``gains`` computed before."""
    if what not in ("series", "states"):
        raise ValueError("what must be 'series' or 'states'")
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    g_ = gain if gain is not None else gains(y, phi, q, G, R, x0, P0, dtype)
    d, rf, Pp = g_["d"], g_["rf"], g_["Pp"]
    phi = np.asarray(phi, dtype=dtype)
    Z = _Z(np.asarray(G, dtype=dtype), dtype)
    a0 = np.zeros(n, dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype)
    targets = np.asarray(targets, dtype=np.int64).reshape(-1, 2)
    M = targets.shape[0]
    w = np.full((M, T, N), np.nan, dtype=dtype)
    icpt = np.full(M, np.nan, dtype=dtype)
    seen = np.isfinite(y)
    cols = _cols(N, n)
    up = range(N - 1, -1, -1) if descending else range(N)          # WRONG on purpose when descending
    down = range(N) if descending else range(N - 1, -1, -1)
    for m in range(M):
        ts, col = int(targets[m, 0]), int(targets[m, 1])
        if not (0 <= ts < T and 0 <= col < (N if what == "series" else n)):
            continue
        c = Z[col].copy() if what == "series" else np.eye(n, dtype=dtype)[col]
        g = np.zeros((T, N), dtype=dtype)
        p = np.zeros(n, dtype=dtype)
        for cc in range(n):
            p = p + Pp[ts][:, cc] * c[cc]
        for t in range(ts, ts + 1 if stop_at_target else T):      # WRONG on purpose when it stops at the target
            if t > ts:
                p = phi * p
            for j in up:
                g[t, j] = _dot(Z[j], p, dtype, cols[j]) * rf[t, j]
                p = p - d[t, j] * g[t, j]
        h = np.zeros(n, dtype=dtype)
        for t in range(T - 1, -1, -1):
            for j in down:
                wj = g[t, j] + _dot(h, d[t, j], dtype) * rf[t, j]
                w[m, t, j] = wj
                h = h - wj * Z[j]
            if t == ts and not no_c:                              # WRONG on purpose without c
                h = h + c
            h = phi * h
        icpt[m] = _dot(h, a0, dtype)
        w[m][~seen] = np.nan
    return w, icpt


def dense(y, phi, q, G, R=None, x0=None, P0=None, targets=(), what="series"):
    """The same (w, intercept) by dense Gaussian conditioning in float64: the joint covariance of all states and all observed
    cells, one solve.  For small T only."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    Z = _Z(np.asarray(G, float), np.float64)
    R = np.zeros(N) if R is None else np.asarray(R, float)
    a = np.zeros(n) if x0 is None else np.asarray(x0, float)
    P = np.eye(n) if P0 is None else np.asarray(P0, float)
    Phi = np.diag(np.asarray(phi, float))
    mu = np.empty((T, n))
    V = np.zeros((T, n, T, n))                 # Cov(x_t, x_s)
    for t in range(T):
        a = Phi @ a
        P = Phi @ P @ Phi.T + np.diag(np.asarray(q, float))
        mu[t] = a
        V[t, :, t, :] = P
        for s in range(t):
            V[t, :, s, :] = Phi @ V[t - 1, :, s, :]
            V[s, :, t, :] = V[t, :, s, :].T
    cells = [(t, j) for t in range(T) for j in range(N) if np.isfinite(y[t, j])]
    A = np.zeros((len(cells), T * n))          # y_obs = A x + e
    for i, (t, j) in enumerate(cells):
        A[i, t * n:(t + 1) * n] = Z[j]
    Vx = V.reshape(T * n, T * n)
    Sy = A @ Vx @ A.T + np.diag([R[j] for (_, j) in cells])
    my = A @ mu.reshape(-1)
    targets = np.asarray(targets, dtype=np.int64).reshape(-1, 2)
    w = np.full((targets.shape[0], T, N), np.nan)
    icpt = np.full(targets.shape[0], np.nan)
    for m, (ts, col) in enumerate(targets):
        c = np.zeros(T * n)
        c[ts * n:(ts + 1) * n] = Z[col] if what == "series" else np.eye(n)[col]
        sol = np.linalg.solve(Sy, A @ Vx @ c)
        for i, (t, j) in enumerate(cells):
            w[m, t, j] = sol[i]
        icpt[m] = c @ mu.reshape(-1) - sol @ my
    return w, icpt
