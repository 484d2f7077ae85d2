"""Host mathematics on the per-step scores of ``BatchedKalman.scores`` (the derivative of every step's contribution to -2 log L
with respect to every parameter, by the tangent filter): covariance matrices of the parameter estimates and the Nyblom-Hansen
test of parameter constancy.  Small matrices, [R,n,n]: numpy or torch in, the same out.

Conventions.  The objective is -2 log L, so with s_t its per-step scores, ``opg = sum s_t s_t'`` and H its Hessian, the
asymptotic covariances of the maximum-likelihood estimate are (``parameter_covariance``)

    "opg"      4 pinv(opg)             outer product of gradients: positive semi-definite by construction
    "hessian"  2 pinv(H)               observed information
    "robust"   pinv(H) opg pinv(H)     the sandwich (quasi-maximum-likelihood, White 1982): valid when the model is slightly wrong

-- what statsmodels calls ``cov_type="opg"``, ``"oim"``-like and ``"robust"``.  ``calibrate_batch(stderr=True)`` keeps the reference's
convention instead, ``fit["pcov"] = pinv(H)`` (metran/solver.py), which is HALF of ``"hessian"``; nothing there changes.
"""
import numpy as np

__all__ = ["parameter_covariance", "nyblom", "cvm_sf", "hessian_alpha", "COVARIANCE_KINDS"]

COVARIANCE_KINDS = ("opg", "hessian", "robust")


def _pinv(a):
    if isinstance(a, np.ndarray):
        return np.linalg.pinv(a)
    import torch

    return torch.linalg.pinv(a)


def parameter_covariance(opg, count=None, grad=None, hessian=None, kind="robust"):
    """Covariance ``[...,n,n]`` of the parameter estimates from ``opg [...,n,n]`` (``BatchedKalman.scores``) and, for ``"hessian"``
    and ``"robust"``, the Hessian of -2 log L (``hessian_alpha``): see the module's conventions.  ``count`` and ``grad`` are taken
    so that the call reads like ``nyblom``'s; the three kinds do not use them (the outer products are not centred, as in
    statsmodels: at an interior optimum the gradient is zero).  A parameter without information (a zero row of opg or H: a
    padding state) gets a zero row by the pseudo-inverse; the facade turns it into NaN."""
    if kind not in COVARIANCE_KINDS:
        raise ValueError("kind must be one of %s" % ", ".join(repr(k) for k in COVARIANCE_KINDS))
    if kind == "opg":
        return 4.0 * _pinv(opg)
    if hessian is None:
        raise ValueError("kind=%r needs the Hessian of -2 log L" % kind)
    hi = _pinv(hessian)
    if kind == "hessian":
        return 2.0 * hi
    return hi @ opg @ hi


def _cf_reach(k):
    """Where the characteristic function's magnitude over u (the integrand's envelope) has fallen below 1e-15."""
    u = 1.0
    while 0.5 * k * (np.log(2.0 * np.sqrt(2.0) * u) - u) - np.log(u) > np.log(1e-15):
        u += 0.5
    return u


def _cvm_zero_from(k):
    """An x beyond which the survival function is below 1e-16, by Chernoff's bound ``exp(-theta x) E exp(theta Q)`` at
    theta = 0.45 pi^2 (the moment generating function, ``(sqrt(2 theta) / sin sqrt(2 theta))^(k/2)``, exists below pi^2 / 2)."""
    theta = 0.45 * np.pi ** 2
    r = np.sqrt(2.0 * theta)
    return (np.log(1e16) + 0.5 * k * np.log(r / np.sin(r))) / theta


_CVM_CHUNK_CELLS = 1 << 21   # complex numbers in one chunk's [values, grid] temporary: 32 MB


def cvm_sf(x, k=1):
    """Survival function of ``sum_j chi2_k,j / (pi^2 j^2)``, j = 1, 2, ...: the limit law of the Nyblom-Hansen statistic with k
    parameters (k = 1: the Cramer-von Mises law).  Its characteristic function is ``(sqrt(2it) / sin sqrt(2it))^(k/2)``, inverted
    numerically (Gil-Pelaez, on t = u^2, Simpson's rule).  The half-integer power is taken of the phase UNWRAPPED along t: the
    principal branch jumps wherever the phase passes pi and gives wrong values for odd k.
    The cost of a value does not depend on the other values of the call: beyond ``_cvm_zero_from(k)`` (about 8.3 + k / 3, where
    the function is below 1e-16) the answer is 0 without a quadrature, and the others are taken in ascending order, in chunks
    whose grid is sized for the chunk's own largest x and whose temporary holds at most ``_CVM_CHUNK_CELLS`` numbers."""
    k = int(k)
    if k < 1:
        raise ValueError("k must be >= 1")
    xs = np.asarray(x, dtype=np.float64).reshape(-1)
    out = np.full(xs.shape, np.nan)
    out[xs <= 0] = 1.0
    out[xs >= _cvm_zero_from(k)] = 0.0
    todo = np.nonzero(np.isnan(out) & np.isfinite(xs))[0]
    todo = todo[np.argsort(xs[todo], kind="stable")]
    U = _cf_reach(k)
    i0 = 0
    while i0 < todo.size:
        # the largest chunk from i0 on (at most 64 values) whose temporary fits: the grid follows the chunk's largest x, because
        # the phase of exp(-i u^2 x) advances by 2 u x du per point -- at most a quarter radian
        rows = min(64, todo.size - i0)
        while True:
            xmax = float(xs[todo[i0 + rows - 1]])
            nu = int(max(U / min(2e-3, 0.125 / (U * max(xmax, 0.1))), 2000))
            nu += nu % 2
            if rows == 1 or rows * nu <= _CVM_CHUNK_CELLS:
                break
            rows = max(1, min(rows - 1, _CVM_CHUNK_CELLS // nu))
        idx = todo[i0:i0 + rows]
        i0 += rows
        u = np.linspace(0.0, U, nu + 1)
        s = u[1:] * (1.0 + 1.0j)                                  # sqrt(2 i t), t = u^2
        g = s / np.sin(s)
        logphi = 0.5 * k * (np.log(np.abs(g)) + 1j * np.unwrap(np.angle(g)))
        w = np.full(nu + 1, 2.0)
        w[1::2] = 4.0
        w[0] = w[-1] = 1.0
        w *= (u[1] - u[0]) / 3.0
        wu = w[1:] * 2.0 / u[1:]                                   # dt / t = 2 du / u; the integrand is 0 at u = 0
        t = u[1:] * u[1:]
        val = np.exp(logphi[None, :] - 1j * xs[idx, None] * t[None, :]).imag @ wu
        out[idx] = 0.5 + val / np.pi
    out = np.clip(out, 0.0, 1.0)
    return out.reshape(np.shape(x)) if np.ndim(x) else float(out[0])


def nyblom(cusum, opg, grad, count, exists=None):
    """Nyblom-Hansen test of parameter constancy (Nyblom 1989, Hansen 1992) from the sums of ``BatchedKalman.scores``, arrays
    ``cusum, opg [...,n,n]``, ``grad [...,n]``, ``count [...]`` = m.  With ``V = opg - grad grad' / m`` (the centred outer products):
    per parameter ``L_p = cusum_pp / (m V_pp)``, jointly ``L = tr(pinv(V) cusum) / m``; under constancy they follow ``cvm_sf(., 1)``
    and ``cvm_sf(., k)``, k the number of parameters.  The scores are centred, so the statistic is also meaningful at a bound or
    at a model that has not converged.  ``exists [...,n]`` (bool): the parameters a model has; the others are left out of the joint
    statistic and get NaN.  Returns a dict ``L_param, pvalue_param [...,n]``, ``L, pvalue, df [...]``."""
    cusum, opg = np.asarray(cusum, dtype=np.float64), np.asarray(opg, dtype=np.float64)
    grad, m = np.asarray(grad, dtype=np.float64), np.asarray(count, dtype=np.float64)
    exists = np.ones(grad.shape, dtype=bool) if exists is None else np.asarray(exists, dtype=bool)
    mm = np.where(m > 0, m, np.nan)
    V = opg - grad[..., :, None] * grad[..., None, :] / mm[..., None, None]
    dV, dC = np.diagonal(V, axis1=-2, axis2=-1), np.diagonal(cusum, axis1=-2, axis2=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        Lp = np.where(exists & (dV > 0), dC / (mm[..., None] * dV), np.nan)
    both = exists[..., :, None] & exists[..., None, :]
    Vz, Cz = np.where(both, V, 0.0), np.where(both, cusum, 0.0)
    good = np.isfinite(Vz).all(axis=(-2, -1)) & np.isfinite(Cz).all(axis=(-2, -1))
    Vi = np.linalg.pinv(np.where(good[..., None, None], Vz, 0.0))
    L = np.where(good, np.einsum("...ij,...ji->...", Vi, Cz) / mm, np.nan)
    df = exists.sum(axis=-1)
    pj = np.full(L.shape, np.nan)
    for k in np.unique(df[df > 0]):
        sel = (df == k) & np.isfinite(L)
        if sel.any():
            pj[sel] = cvm_sf(L[sel], int(k))
    pp = np.full(Lp.shape, np.nan)
    fin = np.isfinite(Lp)
    if fin.any():
        pp[fin] = cvm_sf(Lp[fin], 1)
    return {"L_param": Lp, "pvalue_param": pp, "L": L, "pvalue": pj, "df": df}


def hessian_alpha(kf, alpha, dt=1.0, warmup=1):
    """Hessian ``[R,n,n]`` of -2 log L with respect to alpha, by forward differences of the adjoint gradient
    (``kf.loglik_grad_alpha``): the differencing of ``calibrate_batch(stderr=True)``, step for step -- ``1e-5 max(|alpha|, 0.1)``
    per parameter, the n + 1 gradient evaluations riding as batch, symmetrised -- so that ``2 pinv`` of it is twice ``fit["pcov"]``."""
    import torch

    from .calibrate import _grad_sets_that_fit

    if not kf.has_adjoint():
        raise ValueError("stderr=True differences the adjoint gradient, which this shape (N=%d, K=%d) does not have" % (kf.N, kf.K))
    x = kf._dev(alpha)
    R, n = (int(v) for v in x.shape)
    d = 1e-5 * x.abs().clamp_min(0.1)
    sets = _grad_sets_that_fit(kf, R, n + 1)
    gg = torch.empty((n + 1, R, n), dtype=torch.float64, device=x.device)
    for s0 in range(0, n + 1, sets):
        s1 = min(n + 1, s0 + sets)
        pts = x[None].repeat(s1 - s0, 1, 1)                               # set 0 is x itself, set 1 + j steps x_j
        for s_ in range(max(s0, 1), s1):
            pts[s_ - s0, :, s_ - 1] += d[:, s_ - 1]
        _, gch = kf.loglik_grad_alpha(pts.reshape((s1 - s0) * R, n), dt=dt, warmup=warmup)
        gg[s0:s1] = gch.reshape(s1 - s0, R, n)
    hess = ((gg[1:] - gg[0:1]) / d.transpose(0, 1)[:, :, None]).permute(1, 0, 2)   # [R, j, :] = d grad / d x_j
    return 0.5 * (hess + hess.transpose(1, 2))
