"""numpy restatement of the multi-step-ahead forecasts and the forecast skill by horizon (C ABI mk_forecast; the definitions
of include/metran_hip.h): origin o in {-1, .., T-1} has the filtered moments of step o (the initial moments for o = -1); the
filter's own prediction applied h times gives m_{o,h,j} = z_j x and s_{o,h,j} = z_j P z_j' + R_j.

Built on ``innov_ref.innovations`` for the filtered moments (F, Pf) and on ``innov_ref.step`` with an EMPTY step for one
prediction and the projection (plain loops, left to right), in ``dtype`` arithmetic: ``np.longdouble`` (the default: the
yardstick of the GPU tests) or ``np.float64``.  Three deliberately WRONG variants exist so that the tests can show they would
notice: ``origin_shift`` (origin o uses the record of step o + 1), ``q_once`` (q is added on the first propagated step only)
and ``target_shift`` (the error of the pair (o, h) is taken against y_{o+h-1})."""
import numpy as np

import innov_ref


def table(y, phi, q, G, R=None, x0=None, P0=None, hmax=1, dtype=np.longdouble, origin_shift=False, q_once=False):
    """(M, S) [T+1, hmax, N]: M[o + 1, h - 1, j] = m_{o,h,j} and S[o + 1, h - 1, j] = s_{o,h,j}, unscaled, of one model."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    r = innov_ref.innovations(y, phi, q, G, R, x0, P0, dtype=dtype)
    phi, q, G = np.asarray(phi, dtype=dtype), np.asarray(q, dtype=dtype), np.asarray(G, dtype=dtype)
    Rv = np.zeros(N, dtype=dtype) if R is None else np.asarray(R, dtype=dtype)
    a0 = np.zeros(n, dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype)
    A0 = np.eye(n, dtype=dtype) if P0 is None else np.asarray(P0, dtype=dtype)
    empty = np.full(N, np.nan)
    M = np.empty((T + 1, hmax, N), dtype=dtype)
    S = np.empty((T + 1, hmax, N), dtype=dtype)
    for o in range(-1, T):
        src = min(o + 1, T - 1) if origin_shift else o   # WRONG on purpose when shifted
        x, P = (a0, A0) if src < 0 else (r["F"][src], r["Pf"][src])
        for h in range(1, hmax + 1):
            qh = q if (h == 1 or not q_once) else np.zeros(n, dtype=dtype)   # WRONG on purpose with q_once
            _, _, pm, pv, x, P = innov_ref.step(x, P, empty, phi, qh, G, Rv, dtype)
            M[o + 1, h - 1], S[o + 1, h - 1] = pm, pv
    return M, S


def forecast(y, phi, q, G, R=None, x0=None, P0=None, scale=None, offset=None, horizon=1, origin=None, track_horizon=1, t_first=1,
             z=1.959963984540054, dtype=np.longdouble, origin_shift=False, q_once=False, target_shift=False, tab=None):
    """dict of one model: ``fan_mean, fan_var [H,N]`` from ``origin`` (None = T - 1), ``track_mean, track_var [T,N]`` for
    ``track_horizon`` (both scaled: mean * scale + offset, max(var, 0) * scale^2), ``skill [N,H,6]`` = [count, sum e, sum e^2,
    sum e^2 / s, sum log s, hits] over the pairs (o, t = o + h) with t_first <= o, t <= T - 1 and y[t, j] finite, each sum over the
    origins in ascending order; ``M, S`` the unscaled table [T+1,hmax,N] of ``table`` and ``ratio [T,H,N]`` = e^2 / s of every pair
    (NaN where there is none).  ``tab``: a table computed before (at least max(horizon, track_horizon) columns)."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    H, th = int(horizon), int(track_horizon)
    M, S = tab if tab is not None else table(y, phi, q, G, R, x0, P0, max(H, th), dtype, origin_shift, q_once)
    scale = np.ones(N, dtype=dtype) if scale is None else np.asarray(scale, dtype=dtype)
    offset = np.zeros(N, dtype=dtype) if offset is None else np.asarray(offset, dtype=dtype)
    zero = dtype(0)
    o = T - 1 if origin is None else int(origin)
    out = {"M": M, "S": S}
    out["fan_mean"] = M[o + 1, :H] * scale + offset
    out["fan_var"] = np.maximum(S[o + 1, :H], zero) * scale * scale
    tm, tv = np.empty((T, N), dtype=dtype), np.empty((T, N), dtype=dtype)
    for t in range(T):
        oo = max(t - th, -1)
        tm[t] = M[oo + 1, t - oo - 1] * scale + offset
        tv[t] = np.maximum(S[oo + 1, t - oo - 1], zero) * scale * scale
    out["track_mean"], out["track_var"] = tm, tv
    skill = np.zeros((N, H, 6), dtype=dtype)
    ratio = np.full((T, H, N), np.nan, dtype=dtype)
    z2 = dtype(z) * dtype(z)
    for j in range(N):
        for h in range(1, H + 1):
            for oo in range(max(int(t_first), 0), T - h):
                t = oo + h - 1 if target_shift else oo + h   # WRONG on purpose when shifted
                if not np.isfinite(y[t, j]):
                    continue
                e = dtype(y[t, j]) - M[oo + 1, h - 1, j]
                s = S[oo + 1, h - 1, j]
                ratio[oo, h - 1, j] = e * e / s
                skill[j, h - 1] = skill[j, h - 1] + np.array([1, e, e * e, e * e / s, np.log(s), 1 if e * e <= z2 * s else 0], dtype=dtype)
    out["skill"], out["ratio"] = skill, ratio
    return out


def sum_bars(y, M, S, horizon, t_first, atol_mean, rtol_var):
    """[N,H,6] bars of the skill sums that follow from a per-pair error of ``atol_mean`` on m and a relative ``rtol_var`` on s
    (first order plus the square term): [0, m a, sum (2 |e| a + a^2), sum ((2 |e| a + a^2) / s + (e^2 / s) r), m r, 0]."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    a, r = float(atol_mean), float(rtol_var)
    bars = np.zeros((N, horizon, 6))
    for j in range(N):
        for h in range(1, horizon + 1):
            for o in range(max(int(t_first), 0), T - h):
                if np.isfinite(y[o + h, j]):
                    e, s = abs(float(y[o + h, j] - M[o + 1, h - 1, j])), float(S[o + 1, h - 1, j])
                    d2 = 2.0 * e * a + a * a
                    bars[j, h - 1] += [0.0, a, d2, d2 / s + e * e / s * r, r, 0.0]
    return bars
