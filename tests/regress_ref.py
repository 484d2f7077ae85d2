"""numpy restatement of the intervention effects by GLS (C ABI mk_regression; the recursions of include/metran_hip.h, de Jong's
augmented filter): level shifts, outliers and trends of single series as known regressors of the observation equation,
y_t = X_t beta + Z x_t + e_t, estimated for fixed parameters.

``weights_ref.gains`` is the plain filter loop that keeps d = P z_j' and 1 / f of every scalar update (zeros at a cell that is not
observed); ``normal`` replays the mean recursion over those gains for y and for the M regressor columns and sums the augmented
normal matrix A over the cells of the steps t >= t_first; ``solve`` scales S = A[1:,1:] to unit diagonal, runs Cholesky in effect
order, drops an effect with support 0 or a pivot below 1e-12 and solves the rest.  Plain loops, sums left to right, in ``dtype``
arithmetic (``np.longdouble`` the default: the yardstick of the GPU tests; ``np.float64`` for the bar).  Five deliberately WRONG
variants exist so that the tests can show they would notice: ``descending`` (the series of a step in descending order, on the
gains of the ascending filter), ``inclusive`` (t1 taken as inclusive), ``ramp_from_zero`` (a ramp that starts at 0 instead of 1),
``late_sums`` (the sums started at t_first + 1) and ``skip_before`` (the steps before t_first left out of the replay)."""
import numpy as np

import weights_ref

LEVEL, RAMP = 0, 1
MIN_PIVOT = 1e-12


def regressors(T, N, effects, inclusive=False, ramp_from_zero=False):
    """X [M,T,N] float64 of one record's effects ``[M,4]`` = (series, kind, t0, t1); an unused slot (series < 0) is all zero."""
    effects = np.asarray(effects, dtype=np.int64).reshape(-1, 4)
    X = np.zeros((effects.shape[0], T, N))
    for m, (j, kind, t0, t1) in enumerate(effects):
        if j < 0:
            continue
        if inclusive:                                              # WRONG on purpose
            t1 = t1 + 1
        for t in range(t0, T):
            if kind == LEVEL:
                X[m, t, j] = 1.0 if t < t1 else 0.0
            else:
                X[m, t, j] = min(t, t1 - 1) - t0 + (0 if ramp_from_zero else 1)   # WRONG on purpose from zero
    return X


def normal(y, phi, G, gain, effects, t_first=1, x0=None, dtype=np.longdouble, descending=False, inclusive=False,
           ramp_from_zero=False, late_sums=False, skip_before=False):
    """(A [M+1,M+1], support [M]) of one model: the replay of the mean recursion for y and the regressors over ``gain`` (the dict
    of ``weights_ref.gains`` in the same dtype)."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    d, rf = gain["d"], gain["rf"]
    phi = np.asarray(phi, dtype=dtype)
    Z = weights_ref._Z(np.asarray(G, dtype=dtype), dtype)
    cols = weights_ref._cols(N, n)
    X = regressors(T, N, effects, inclusive, ramp_from_zero)
    M = X.shape[0]
    seen = np.isfinite(y)
    a = np.zeros((M + 1, n), dtype=dtype)
    if x0 is not None:
        a[0] = np.asarray(x0, dtype=dtype)
    A = np.zeros((M + 1, M + 1), dtype=dtype)
    support = np.zeros(M, dtype=np.int64)
    first = t_first + 1 if late_sums else t_first                  # WRONG on purpose when late
    Xd = X.astype(dtype)
    lower = np.tril(np.ones((M + 1, M + 1), dtype=bool))
    for t in range(t_first if skip_before else 0, T):              # WRONG on purpose when the steps before are skipped
        a = a * phi[None, :]
        for j in (range(N - 1, -1, -1) if descending else range(N)):   # WRONG on purpose when descending
            za = np.zeros(M + 1, dtype=dtype)                      # z_j a of every column, the sum left to right
            for c in cols[j]:
                za = za + Z[j, c] * a[:, c]
            V = np.concatenate([[dtype(y[t, j]) if seen[t, j] else dtype(0)], Xd[:, t, j]]) - za
            kr = d[t, j] * rf[t, j]
            a = a + V[:, None] * kr[None, :]
            if t >= first:
                A = A + np.where(lower, (V * rf[t, j])[:, None] * V[None, :], dtype(0))   # A[p,q] += (V_p / f) V_q, q <= p
                if seen[t, j]:
                    support += X[:, t, j] != 0
    for p in range(M + 1):
        for q in range(p):
            A[q, p] = A[p, q]
    return A, support


def solve(A, support, used=None, dtype=np.longdouble, pivots=None):
    """(beta [M], cov [M,M], gain, dropped [M] bool) from the augmented normal matrix: S = A[1:,1:] to unit diagonal, Cholesky in
    effect order, an effect with support 0 (or not ``used``) or a pivot below MIN_PIVOT dropped, the rest solved without it.
    ``pivots``: a list that receives the M unit-diagonal pivots as they are met (NaN for an effect that is out before its pivot is
    looked at: unused, no support or a zero diagonal)."""
    A = np.asarray(A, dtype=dtype)
    M = A.shape[0] - 1
    used = np.ones(M, dtype=bool) if used is None else np.asarray(used, dtype=bool)
    one, zero = dtype(1), dtype(0)
    s, S = A[1:, 0], A[1:, 1:]
    sd = np.array([np.sqrt(S[i, i]) if S[i, i] > 0 else one for i in range(M)], dtype=dtype)
    keep = np.array([bool(used[i] and S[i, i] > 0 and support[i] > 0) for i in range(M)])
    U = np.zeros((M, M), dtype=dtype)
    for i in range(M):
        for j in range(i + 1):
            U[i, j] = S[i, j] / (sd[i] * sd[j])
    ss = np.array([s[i] / sd[i] for i in range(M)], dtype=dtype)
    for k in range(M):                                             # right-looking, row by row below the pivot
        piv = U[k, k]
        if pivots is not None:
            pivots.append(float(piv) if keep[k] else float("nan"))
        keep[k] = bool(keep[k] and piv >= MIN_PIVOT)
        lk = np.sqrt(piv) if keep[k] else one
        U[k, k] = lk
        for i in range(k + 1, M):
            U[i, k] = U[i, k] / lk if keep[k] else zero
        for i in range(k + 1, M):
            for j in range(k + 1, i + 1):
                U[i, j] = U[i, j] - U[i, k] * U[j, k]
    Li = np.zeros((M, M), dtype=dtype)                             # L^-1, column by column
    for l in range(M):
        if not keep[l]:
            continue
        for i in range(l, M):
            if not keep[i]:
                continue
            if i == l:
                Li[i, l] = one / U[i, i]
            else:
                acc = zero
                for k in range(l, i):
                    acc = acc + U[i, k] * Li[k, l]
                Li[i, l] = -acc / U[i, i]
    w = np.zeros(M, dtype=dtype)
    for k in range(M):
        if keep[k]:
            for j in range(k + 1):
                if keep[j]:
                    w[k] = w[k] + Li[k, j] * ss[j]
    beta = np.full(M, np.nan, dtype=dtype)
    cov = np.full((M, M), np.nan, dtype=dtype)
    gain = zero
    for k in range(M):
        gain = gain + w[k] * w[k]
    for i in range(M):
        if not keep[i]:
            continue
        acc = zero
        for k in range(i, M):
            acc = acc + Li[k, i] * w[k]
        beta[i] = acc / sd[i]
        for j in range(M):
            if not keep[j]:
                continue
            acc = zero
            for k in range(max(i, j), M):
                acc = acc + Li[k, i] * Li[k, j]
            cov[i, j] = acc / (sd[i] * sd[j])
    return beta, cov, gain, ~keep


def regression(y, phi, q, G, R=None, x0=None, P0=None, effects=(), t_first=1, dtype=np.longdouble, gain=None, **wrong):
    """dict of one model: ``beta, cov, gain, normal, support, dropped`` (dropped as a bool array [M]) and ``pivots`` (``solve``).
    ``gain``: the dict of ``weights_ref.gains`` computed before, in the same dtype."""
    effects = np.asarray(effects, dtype=np.int64).reshape(-1, 4)
    g_ = gain if gain is not None else weights_ref.gains(y, phi, q, G, R, x0, P0, dtype)
    A, support = normal(y, phi, G, g_, effects, t_first, x0, dtype, **wrong)
    pivots = []
    beta, cov, gn, dropped = solve(A, support, effects[:, 0] >= 0, dtype, pivots)
    return {"beta": beta, "cov": cov, "gain": gn, "normal": A, "support": support, "dropped": dropped, "pivots": np.array(pivots)}


def adjusted(y, effects, beta):
    """y - sum_m beta_m x_m for one record (a NaN beta counts as 0)."""
    y = np.asarray(y, dtype=np.float64)
    X = regressors(y.shape[0], y.shape[1], effects)
    out = y.copy()
    for m in range(X.shape[0]):
        b = float(beta[m])
        out = out - (b if b == b else 0.0) * X[m]
    return out


def unit_condition(A, dropped):
    """Condition number of the unit-diagonal S of the effects that were kept."""
    S = np.asarray(A, dtype=np.float64)[1:, 1:]
    kept = np.nonzero(~np.asarray(dropped))[0]
    if kept.size == 0:
        return 1.0
    S = S[np.ix_(kept, kept)]
    sd = np.sqrt(np.diag(S))
    return float(np.linalg.cond(S / np.outer(sd, sd)))
