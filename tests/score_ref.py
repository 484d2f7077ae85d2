"""numpy restatement of the per-step scores by the tangent filter (C ABI mk_scores; the recursions of include/metran_hip.h): the
derivative of every step's contribution to -2 log L, l_t = sum_j (log f + v^2 / f) over the cells observed at t, with respect to
one parameter per state -- parameter p moves phi_p by dphi[p] and q_p by dq[p] -- and the sums built on them.

``base`` is a plain filter loop (prediction first, then the observed series of the step in ascending order, Z = [I | G]) that
keeps what the tangent needs: the filtered moments of every step, d = P z_j', 1 / f and v of every scalar update (zeros at a
cell that is not observed) and the step's l_t.  ``scores`` runs the n tangents side by side, dense ([n,n,n] for the
covariances), and sums.  In ``dtype`` arithmetic (``np.longdouble`` the default: the yardstick of the GPU tests; ``np.float64``
for the bar).

Beside every output stands its SCALE: the output's own expression with every term replaced by its absolute value --
    score   sum_j |fd / f| + |2 v vd / f| + |v^2 fd / f^2|
    grad    sum_t scale(s_t);   opg  sum_t scale(s_t) scale(s_t)'
    cusum   sum_t A_t A_t',  A_t = sum_{u <= t} (scale(s_u) + scale(grad) / m)
-- and comparisons are relative to it (``differences``).  For ``score`` the scale of an (instance, parameter) pair is that of
its LARGEST step: at the first step of a factor parameter the prediction term 2 phi dphi + dq cancels exactly, and a step's own
scale there is rounding noise.

Six deliberately WRONG variants exist so that the tests can show they would notice: ``half`` (one half of the symmetric term
dphi (e_p (P_p. o phi) + (phi o P_.p) e_p') dropped), ``no_v2`` (the term -v^2 fd / f^2 dropped), ``filtered_t`` (the filtered
moments of step t instead of t - 1 in the prediction's tangent), ``count_before`` (the steps before t_first counted) and
``uncentred`` (cusum without the centring); the sixth, another record's data, is the caller's (tests/score_engine.py
``shift_records``)."""
import numpy as np

import weights_ref

OUTPUTS = ("score", "grad", "opg", "cusum")


def base(y, phi, q, G, R=None, x0=None, P0=None, dtype=np.longdouble):
    """dict of one model: ``xf [T,n]``, ``Pf [T,n,n]`` filtered moments, ``d [T,N,n]``, ``rf [T,N]``, ``v [T,N]`` of every scalar
    update (zeros where a cell is not observed), ``ell [T]`` the step's contribution to the objective, ``x0, P0`` as used."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    phi, q = np.asarray(phi, dtype=dtype), np.asarray(q, dtype=dtype)
    Z = weights_ref._Z(np.asarray(G, dtype=dtype), dtype)
    R = np.zeros(N, dtype=dtype) if R is None else np.asarray(R, dtype=dtype)
    x = np.zeros(n, dtype=dtype) if x0 is None else np.asarray(x0, dtype=dtype)
    P = np.eye(n, dtype=dtype) if P0 is None else np.asarray(P0, dtype=dtype)
    out = {"x0": x.copy(), "P0": P.copy(), "xf": np.zeros((T, n), dtype=dtype), "Pf": np.zeros((T, n, n), dtype=dtype),
           "d": np.zeros((T, N, n), dtype=dtype), "rf": np.zeros((T, N), dtype=dtype), "v": np.zeros((T, N), dtype=dtype),
           "ell": np.zeros(T, dtype=dtype)}
    for t in range(T):
        x = phi * x
        P = (phi[:, None] * P) * phi[None, :] + np.diag(q)
        for j in range(N):
            if not np.isfinite(y[t, j]):
                continue
            d = P @ Z[j]
            f = R[j] + Z[j] @ d
            v = dtype(y[t, j]) - Z[j] @ x
            rf = dtype(1) / f
            out["d"][t, j], out["rf"][t, j], out["v"][t, j] = d, rf, v
            out["ell"][t] += np.log(f) + v * v * rf
            x = x + d * (v * rf)
            P = P - (d * rf)[:, None] * d[None, :]
        out["xf"][t], out["Pf"][t] = x, P
    return out


def sums(score, sscale, counted, dtype=np.longdouble, uncentred=False):
    """(values, scales) of ``grad, count, opg, cusum`` from the scores ``[T,n]``, their scales and the counted steps."""
    T, n = score.shape
    m = int(counted.sum())
    grad, gs = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for t in range(T):
        if counted[t]:
            grad, gs = grad + score[t], gs + sscale[t]
    gbar = grad / dtype(m) if m else np.zeros(n, dtype=dtype)
    gbs = gs / dtype(m) if m else np.zeros(n, dtype=dtype)
    if uncentred:                                                  # WRONG on purpose
        gbar = np.zeros(n, dtype=dtype)
    opg, os_ = np.zeros((n, n), dtype=dtype), np.zeros((n, n), dtype=dtype)
    cus, cs_ = np.zeros((n, n), dtype=dtype), np.zeros((n, n), dtype=dtype)
    S, A = np.zeros(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for t in range(T):
        if not counted[t]:
            continue
        S, A = S + (score[t] - gbar), A + (sscale[t] + gbs)
        opg, os_ = opg + np.outer(score[t], score[t]), os_ + np.outer(sscale[t], sscale[t])
        cus, cs_ = cus + np.outer(S, S), cs_ + np.outer(A, A)
    return ({"grad": grad, "count": m, "opg": opg, "cusum": cus}, {"grad": gs, "opg": os_, "cusum": cs_})


def scores(y, phi, q, G, R=None, x0=None, P0=None, dphi=None, dq=None, t_first=1, dtype=np.longdouble, tape=None, half=False,
           no_v2=False, filtered_t=False, count_before=False, uncentred=False):
    """dict of one model: ``score [T,n], grad [n], count, opg [n,n], cusum [n,n]`` and ``scale`` (a dict of the four float
    outputs' scales).  ``tape``: the dict of ``base`` computed before, in the same dtype."""
    y = np.asarray(y, dtype=np.float64)
    T, N = y.shape
    K = G.shape[1]
    n = N + K
    tp = tape if tape is not None else base(y, phi, q, G, R, x0, P0, dtype)
    phi = np.asarray(phi, dtype=dtype)
    dphi, dq = np.asarray(dphi, dtype=dtype), np.asarray(dq, dtype=dtype)
    Z = weights_ref._Z(np.asarray(G, dtype=dtype), dtype)
    idx = np.arange(n)
    Pd = np.zeros((n, n, n), dtype=dtype)                          # [parameter, row, column]
    xd = np.zeros((n, n), dtype=dtype)                             # [parameter, state]
    score, sscale = np.zeros((T, n), dtype=dtype), np.zeros((T, n), dtype=dtype)
    for t in range(T):
        if filtered_t:                                             # WRONG on purpose
            xprev, Pprev = tp["xf"][t], tp["Pf"][t]
        else:
            xprev, Pprev = (tp["x0"], tp["P0"]) if t == 0 else (tp["xf"][t - 1], tp["Pf"][t - 1])
        xd = xd * phi[None, :]
        xd[idx, idx] += dphi * xprev
        Pd = (Pd * phi[None, :, None]) * phi[None, None, :]
        rows = dphi[:, None] * (Pprev * phi[None, :])              # [p, c] = dphi_p P[p,c] phi_c
        Pd[idx, idx, :] += rows
        if not half:                                               # WRONG on purpose when one half is dropped
            Pd[idx, :, idx] += rows
        Pd[idx, idx, idx] += dq
        for j in range(N):
            rf = tp["rf"][t, j]
            if rf == 0:
                continue
            d, v, z = tp["d"][t, j], tp["v"][t, j], Z[j]
            dd = Pd @ z                                            # [p, n]
            fd = dd @ z                                            # [p]
            vd = -(xd @ z)
            t1, t2, t3 = fd * rf, 2 * v * vd * rf, v * v * fd * rf * rf
            score[t] += t1 + t2 - (0 if no_v2 else t3)             # WRONG on purpose without the last term
            sscale[t] += np.abs(t1) + np.abs(t2) + np.abs(t3)
            xd = xd + (dd * v + d[None, :] * vd[:, None]) * rf - d[None, :] * (v * fd * rf * rf)[:, None]
            dd_d = dd[:, :, None] * d[None, None, :]
            Pd = Pd - (dd_d + dd_d.transpose(0, 2, 1)) * rf + (d[:, None] * d[None, :])[None] * (fd * rf * rf)[:, None, None]
    seen = np.isfinite(y).any(axis=1)
    counted = seen & (np.arange(T) >= (0 if count_before else t_first))   # WRONG on purpose when the steps before count
    out, scale = sums(score, sscale, counted, dtype, uncentred)
    out["score"] = score
    scale["score"] = np.broadcast_to(sscale.max(axis=0) if T else np.zeros(n, dtype=dtype), (T, n)).copy()
    scale["steps"], scale["counted"] = sscale, counted             # every step's own scale: what the four scales are made of
    out["scale"] = scale
    return out


def differences(got, ref):
    """The largest difference of each float output between two results of one instance, relative to the scale of ``ref`` (a
    zero scale counts as 1: the output is then zero in exact arithmetic, term by term)."""
    out = {}
    for key in OUTPUTS:
        g, r = np.asarray(got[key], dtype=np.longdouble), np.asarray(ref[key], dtype=np.longdouble)
        sc = np.asarray(ref["scale"][key], dtype=np.longdouble).copy()
        sc[sc == 0] = 1
        out[key] = float(np.max(np.abs(g - r) / sc)) if g.size else 0.0
    return out
