"""numpy restatement of the one-step-ahead innovations (C ABI mk_innovations / mk_innovation_stats): the prediction and the
sequential scalar updates of seqkalmanfilter (metran/kalmanfilter.py:318-378) with the innovation v and its variance f of every
update kept, the marginal one-step-ahead forecast of every series, and the portmanteau statistics of e = v / sqrt(f).

Plain loops, every sum taken left to right in the order of the reference's own loops (oracle/kalman_oracle.c restates the
same), in ``dtype`` arithmetic: ``np.longdouble`` (the default: the yardstick of the GPU tests) or ``np.float64`` (the same
operations as the oracle, for tests/test_innovations_host.py).  Three deliberately WRONG variants exist so that the tests can
show they would notice: ``descending`` (updates in descending series order), ``record_of_step`` (step t predicted from the
filtered moments of step t instead of t - 1) and, for the statistics, ``calendar`` (lags in calendar steps)."""
import numpy as np


def _dot(a, b, cols, dtype):
    s = dtype(0)
    for c in cols:
        s = s + a[c] * b[c]
    return s


def step(x, P, y, phi, q, G, R, dtype=np.longdouble, descending=False):
    """One step from the filtered moments (x, P) of the step before: (v [N], f [N], pm [N], pv [N], x', P') -- v / f NaN where
    y is not finite, pm / pv the unscaled marginal forecast z_j x, z_j P z_j' + R_j of every series, (x', P') this step's filtered
    moments."""
    N, K = G.shape
    n = N + K
    x = phi * x
    P = (phi[:, None] * P) * phi[None, :] + np.diag(q)
    v = np.full(N, np.nan, dtype=dtype)
    f = np.full(N, np.nan, dtype=dtype)
    pm = np.empty(N, dtype=dtype)
    pv = np.empty(N, dtype=dtype)
    Z = np.zeros((N, n), dtype=dtype)
    Z[:, :N] = np.eye(N, dtype=dtype)
    Z[:, N:] = G
    cols = [[j] + list(range(N, n)) for j in range(N)]   # the non-zero entries of z_j, in column order
    for j in range(N):
        d = np.zeros(n, dtype=dtype)
        for c in cols[j]:
            d = d + P[:, c] * Z[j, c]
        pm[j] = _dot(Z[j], x, cols[j], dtype)
        pv[j] = R[j] + _dot(Z[j], d, cols[j], dtype)
    for j in (range(N - 1, -1, -1) if descending else range(N)):
        if not np.isfinite(y[j]):
            continue
        z = Z[j]
        v[j] = dtype(y[j]) - _dot(z, x, cols[j], dtype)
        d = np.zeros(n, dtype=dtype)
        for c in cols[j]:
            d = d + P[:, c] * z[c]
        f[j] = R[j] + _dot(z, d, cols[j], dtype)
        k = d / f[j]
        P = P + (-k[:, None] * k[None, :]) * f[j]
        x = x + k * v[j]
    return v, f, pm, pv, x, P


def innovations(y, phi, q, G, R=None, x0=None, P0=None, scale=None, offset=None, dtype=np.longdouble, descending=False,
                record_of_step=False):
    """dict of [T,N] arrays v, f, pred_mean, pred_var (the latter two scaled: mean * scale + offset, max(var, 0) * scale^2) and
    the filtered moments F [T,n], Pf [T,n,n] of one model."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    phi, q, G = np.asarray(phi, dtype=dtype), np.asarray(q, dtype=dtype), np.asarray(G, dtype=dtype)
    R = np.zeros(N, dtype=dtype) if R is None else np.asarray(R, dtype=dtype)
    x = np.zeros(n, dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype)
    P = np.eye(n, dtype=dtype) if P0 is None else np.asarray(P0, dtype=dtype)
    scale = np.ones(N, dtype=dtype) if scale is None else np.asarray(scale, dtype=dtype)
    offset = np.zeros(N, dtype=dtype) if offset is None else np.asarray(offset, dtype=dtype)
    out = {k: np.empty((T, N), dtype=dtype) for k in ("v", "f", "pred_mean", "pred_var")}
    out["F"], out["Pf"] = np.empty((T, n), dtype=dtype), np.empty((T, n, n), dtype=dtype)
    for t in range(T):
        v, f, pm, pv, x1, P1 = step(x, P, y[t], phi, q, G, R, dtype, descending)
        if record_of_step:   # WRONG on purpose: the step predicted from its own filtered moments
            v, f, pm, pv, _, _ = step(x1, P1, y[t], phi, q, G, R, dtype, descending)
        out["v"][t], out["f"][t] = v, f
        out["pred_mean"][t] = pm * scale + offset
        out["pred_var"][t] = np.maximum(pv, dtype(0)) * scale * scale
        x, P = x1, P1
        out["F"][t], out["Pf"][t] = x, P
    return out


def stats(v, f, nlags, t_first=0, calendar=False, dtype=np.longdouble):
    """[N, 4 + nlags] = [m, mean, c_0, Q, r_1 .. r_nlags] of e = v / sqrt(f) per series of one model (v, f [T,N]): over the cells
    with finite v, finite f > 0 and t >= t_first, in time order; lags count successive valid cells.  ``calendar`` (WRONG on
    purpose): lags in calendar steps, missing cells skipped in the products."""
    v, f = np.asarray(v, dtype=dtype), np.asarray(f, dtype=dtype)
    T, N = v.shape
    L = int(nlags)
    out = np.full((N, 4 + L), np.nan, dtype=dtype)
    for j in range(N):
        with np.errstate(invalid="ignore"):
            ok = np.isfinite(v[:, j]) & np.isfinite(f[:, j]) & (f[:, j] > 0) & (np.arange(T) >= t_first)
        m = int(ok.sum())
        out[j, 0] = m
        if m == 0:
            continue
        e = np.full(T, np.nan, dtype=dtype)
        e[ok] = v[ok, j] / np.sqrt(f[ok, j])
        mean = e[ok].sum() / dtype(m)
        if calendar:
            c = np.where(ok, e - mean, dtype(0))
        else:
            c = e[ok] - mean
        acf = np.array([(c[: len(c) - l] * c[l:]).sum() / dtype(m) if l < len(c) else dtype(0) for l in range(L + 1)], dtype=dtype)
        out[j, 1], out[j, 2] = mean, acf[0]
        if m <= L or acf[0] == 0:
            continue
        r = acf[1:] / acf[0]
        out[j, 4:] = r
        out[j, 3] = dtype(m) * dtype(m + 2) * (r * r / (dtype(m) - np.arange(1, L + 1).astype(dtype))).sum()
    return out
