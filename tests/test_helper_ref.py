"""CPU tier of the helper-kernel tests: tests/helper_ref.py (the plain extended-precision references and the shared
inputs of tests/test_helpers_gpu.py) pinned against pandas, the C oracle and metran_amd.params -- before GPU time is spent
comparing kernels with them -- and every tolerance model of the GPU tier checked first as fp64 (pandas / the oracle /
params.py) against extended precision.  Each tolerance check prints the margin it measured (``pytest -s`` shows them)."""
import math

import numpy as np
import pandas as pd
import pytest

import helper_ref as hr
import oracle
from metran_amd.params import phi_q_from_alpha

EPS = hr.EPS
pytestmark = pytest.mark.filterwarnings("ignore::RuntimeWarning")   # inf - inf and 0 / 0 are inputs here

def _same(a, b):
    """Equal as values, NaN == NaN, +inf == +inf."""
    return np.array_equal(np.asarray(a, float), np.asarray(b, float), equal_nan=True)


# ------------------------------------------------------------------------------------------------- standardise
@pytest.mark.parametrize("N", hr.STANDARDIZE_N)
def test_standardize_against_pandas(N):
    """helper_ref.standardize == DataFrame.mean / .std / (df - mean) / std on every GPU input: the NaN pattern and the
    degenerate series exactly, the ordinary ones within STD_TOL = 1e-12 (fp64 pandas against extended precision: the bar
    the kernel is held to)."""
    worst = 0.0
    for T, batch in ((T, b) for T in hr.standardize_lengths(N) for b in range(hr.standardize_batches(N))):
        y, kinds = hr.standardize_case(N, T, batch)
        mean, std, z = hr.standardize_ref(N, T, batch)
        for r in range(y.shape[0]):
            df = pd.DataFrame(y[r])
            pm, ps = df.mean().values, df.std().values
            pz = ((df - df.mean()) / df.std()).values
            assert np.array_equal(np.isnan(pz), np.isnan(z[r])) and not np.isinf(z[r]).any()
            for j in range(N):
                k = kinds[r, j]
                if k in hr.EXACT_KINDS:
                    want = hr.expected_degenerate(k, T)
                    assert _same([mean[r, j], std[r, j]], want), (N, T, r, j, k, mean[r, j], std[r, j])
                    assert _same([pm[j], ps[j]], want), (N, T, r, j, k, pm[j], ps[j])
                    assert np.isnan(z[r, :, j]).all()
            ok = ~np.isin(kinds[r], hr.EXACT_KINDS)
            np.testing.assert_allclose(pm[ok], mean[r, ok], rtol=hr.STD_TOL, atol=1e-14, equal_nan=True)
            np.testing.assert_allclose(ps[ok], std[r, ok], rtol=hr.STD_TOL, equal_nan=True)
            np.testing.assert_allclose(pz[:, ok], z[r][:, ok], rtol=0, atol=hr.STD_TOL, equal_nan=True)
            if np.isfinite(z[r][:, ok]).any():
                worst = max(worst, float(np.nanmax(np.abs(pz[:, ok] - z[r][:, ok]))))
    print("standardise N=%d: pandas - extended, worst |dz| = %.2e (bar %.0e)" % (N, worst, hr.STD_TOL))


@pytest.mark.parametrize("N", hr.STANDARDIZE_N)
def test_every_width_carries_every_kind_and_ordinary_series_that_count(N):
    """From N = 7 on every record holds the six degenerate kinds and ordinary series.  Narrower widths are tested with
    several batches of three records (4 at N = 1, 2 at N = 2, 1 at N = 5): every batch has an ordinary series, every
    column has one in some batch of a narrow width, the six degenerate kinds all appear -- and at every T from RP - 1 on (50 and more
    there), each batch has an ordinary series observed in at least half its rows, so the 1e-12 bars on mean, std and z
    bite."""
    D = hr.standardize_batches(N)
    assert D == {1: 4, 2: 2}.get(N, 1)
    seen, ordinary_columns = set(), set()
    for batch in range(D):
        kinds = hr.series_kinds(hr.STANDARDIZE_R, N, batch)
        assert kinds.shape == (hr.STANDARDIZE_R, N) and (kinds == "ordinary").any()
        if N >= 7:
            for r in range(kinds.shape[0]):
                assert set(kinds[r]) == set(hr.KINDS)
        seen |= set(kinds.ravel())
        ordinary_columns |= set(np.nonzero((kinds == "ordinary").any(0))[0].tolist())
        for T in hr.standardize_lengths(N):
            y, k = hr.standardize_case(N, T, batch)
            assert np.array_equal(k, kinds)
            observed = (~np.isnan(y)).sum(1)[k == "ordinary"]
            if T >= hr.rows_per_pass(N) - 1 and N < 7:
                assert observed.max() >= max(T // 2, 25)
            elif T >= hr.rows_per_pass(N) - 1:
                assert observed.max() >= 2       # RP = 4 at N = 64: T = 3 .. 14
    assert seen == set(hr.KINDS) and (N >= 7 or ordinary_columns == set(range(N)))


def test_offset_bound_holds_for_pandas():
    """Values 1e6 + 1e-2 noise (T = 400, 30 % missing): pandas' standardised values against the extended-precision ones,
    in units of eps (|mean| / std + |z|).  C_OFFSET is four times the worst ratio measured here, rounded up; the mean is
    within gamma eps mean|y| and the std within 1e-12 relative."""
    worst = worst_mean = worst_std = 0.0
    for seed in range(10):
        y = hr.offset_record(seed)
        mean, std, z = hr.standardize(y)
        df = pd.DataFrame(y)
        pz = ((df - df.mean()) / df.std()).values
        unit = EPS * (np.abs(mean) / std + np.abs(z))
        worst = max(worst, float(np.nanmax(np.abs(pz - z) / unit)))
        worst_mean = max(worst_mean, float(np.max(np.abs(df.mean().values - mean) / hr.mean_bound(y, y.shape[1]))))
        worst_std = max(worst_std, float(np.max(np.abs(df.std().values / std - 1))))
    print("offset: pandas - extended = %.3f eps (|mean|/std + |z|); C_OFFSET = %.1f; mean at %.3f of its bound; std rel %.1e"
          % (worst, hr.C_OFFSET, worst_mean, worst_std))
    assert 4 * worst <= hr.C_OFFSET < 8 * worst + 1     # four times the measured figure, not an arbitrary one
    assert worst_mean <= 1.0 and worst_std <= hr.STD_TOL


# ------------------------------------------------------------------------------------------------- pack / mask
@pytest.mark.parametrize("R,T,N", hr.PACK_SHAPES)
def test_pack_against_the_oracle(R, T, N):
    y = hr.pack_case(R, T, N)
    if R * T > 2:
        flat = y.reshape(-1, N)
        assert (flat == -1e10).any() and (flat == np.nextafter(-1e10, 0)).any() and (flat == np.nextafter(-1e10, -np.inf)).any()
        assert np.isinf(flat).any() and np.isnan(flat).all(1).any()
    for r in range(R):
        o, ix, c = hr.pack(y[r])
        ro, ri, rc = oracle.set_observations(y[r])
        assert np.array_equal(o, ro) and np.array_equal(ix, ri) and np.array_equal(c, rc)
        assert not (o == -1e10).any()
        keep = np.isfinite(y[r]) & (y[r] != -1e10)
        assert np.array_equal(c, keep.sum(1)) and np.array_equal(o, np.where(keep, y[r], 0.0))


def test_pack_keeps_the_neighbours_of_the_dropped_value():
    lo, hi = np.nextafter(-1e10, -np.inf), np.nextafter(-1e10, 0.0)
    o, ix, c = hr.pack(np.array([[lo, -1e10, hi]]))
    assert o.tolist() == [[lo, 0.0, hi]] and ix.tolist() == [[0.0, 2.0, 0.0]] and c.tolist() == [2]


@pytest.mark.parametrize("count", hr.MASK_COUNTS)
def test_mask_against_pandas(count):
    y, m = hr.mask_case(count)
    got = hr.mask(y, m)
    want = pd.Series(y).mask(m != 0).values
    hidden = m != 0
    assert np.isnan(got[hidden]).all() and np.array_equal(got.view(np.int64)[~hidden], y.view(np.int64)[~hidden])
    assert np.array_equal(got.view(np.int64)[~hidden], want.view(np.int64)[~hidden]) and np.isnan(want[hidden]).all()
    if count >= 255:
        assert set(m.tolist()) == {0, 1, 2, 255} and np.isnan(y).any() and np.isinf(y).any()
    assert math.copysign(1.0, got[-1]) == -1.0      # -0.0 keeps its sign


# ------------------------------------------------------------------------------------------------- correlation
@pytest.mark.parametrize("N", hr.CORR_N)
def test_corr_against_pandas(N):
    """helper_ref.corr == DataFrame.corr() on the GPU inputs (no inf: pandas' online algorithm returns an artefact
    there): same NaN pattern, diagonal exactly 1 or NaN, off-diagonals within corr_bound (1e-12, loosened for the series
    with mean 1e6).  Prints how much of the bound pandas uses."""
    y, roles = hr.corr_case(N)
    ref = hr.corr_ref(N)
    used = used_offset = 0.0
    for r in range(y.shape[0]):
        want = pd.DataFrame(y[r]).corr().values
        assert np.array_equal(np.isnan(ref[r]), np.isnan(want))
        assert np.array_equal(ref[r], ref[r].T, equal_nan=True)
        d = np.diag(ref[r])
        assert np.all((d == 1.0) | np.isnan(d))
        a, b, c, dd, const, off = (roles[k][r] for k in ("a", "b", "c", "d", "constant", "offset"))
        if a is not None:
            assert np.isnan(ref[r, a, b])                      # no common row
        if c is not None:
            assert np.isnan(ref[r, c, dd])                     # one common row
        if const is not None:
            assert np.isnan(ref[r, const]).all()
        bound = hr.corr_bound(y[r])
        err = np.abs(want - ref[r]) / bound
        assert np.nanmax(err, initial=0.0) <= 1.0
        plain = np.ones(N, bool)
        if off is not None:
            plain[off] = False
            used_offset = max(used_offset, float(np.nanmax(np.abs(want - ref[r])[off], initial=0.0)))
            assert bound[off, (off + 9) % N] > 100 * hr.CORR_TOL
        used = max(used, float(np.nanmax(np.abs(want - ref[r])[np.ix_(plain, plain)], initial=0.0)))
    print("corr N=%d: pandas - extended, ordinary %.1e (bar %.0e), mean-1e6 series %.1e" % (N, used, hr.CORR_TOL, used_offset))


def test_corr_with_inf_is_nan_for_that_series_only():
    y, roles = hr.corr_case(23, with_inf=True)
    ref = hr.corr_ref(23, with_inf=True)
    for r in range(y.shape[0]):
        s = roles["inf"][r]
        assert np.isinf(y[r, :, s]).sum() == 2
        assert (np.sign(y[r, 1, s]), np.sign(y[r, 30, s])) == ((1, 1), (1, -1), (-1, -1))[r]     # both signs, alone and mixed
        assert np.isnan(ref[r, s]).all() and np.isnan(ref[r, :, s]).all()
        clean = np.array(y[r])
        clean[:, s] = np.nan
        other = hr.corr(clean)
        keep = np.arange(23) != s
        assert np.array_equal(other[np.ix_(keep, keep)], ref[r][np.ix_(keep, keep)], equal_nan=True)
        assert np.isfinite(other[np.ix_(keep, keep)]).sum() > 300


@pytest.mark.parametrize("R,T,N,K,nf", hr.FACTOR_CASES)
def test_factor_cases_settle_on_the_stated_number_of_factors(R, T, N, K, nf):
    """The reference's MAP test on the full-width batches: one factor on the two with 2 and 3 true factors, two and four
    on the three with 4 and 8 -- so the GPU tier's varimax runs at N = 33 and N = 64, with two and with four columns."""
    from oracle import factor_oracle as fo

    y = hr.factor_case(R, T, N, K)
    assert [fo.solve(y[r])["nfactors"] for r in range(R)] == [nf] * R
    if N == 64:
        assert max(c[4] for c in hr.FACTOR_CASES if c[2] == 64) >= 4
    assert max(c[4] for c in hr.FACTOR_CASES if c[2] == N) >= 2


# ------------------------------------------------------------------------------------------------- projections
@pytest.mark.parametrize("N,n", hr.PROJECTION_SHAPES)
def test_projections_against_the_oracle(N, n):
    """helper_ref.simulate / decompose == oracle.simulate / oracle.decompose (plain fp64 loops) within
    PROJ_TOL n sum|terms|; the clipped variance is exactly 0 and the NaN covariance gives NaN in both."""
    used = 0.0
    for RZ in (1, 2, 5):
        for T in (1, 3):
            Z, x, P = hr.projection_case(N, n, RZ, T)
            ref = hr.projection_ref(N, n, RZ, T)
            for b in range(x.shape[0]):
                sm, sv = oracle.simulate(Z[b % RZ], x[b], P[b])
                sdf, cdf = oracle.decompose(Z[b % RZ], x[b])
                # np.maximum keeps a NaN (kalmanfilter.py:601-602); the C oracle's "v > 0 ? v : 0" does not
                nan = np.isnan(ref["sim_vars"][b])
                assert np.array_equal(sv[~nan] == 0.0, ref["sim_vars"][b][~nan] == 0.0)
                for got, key, scale in ((sm, "sim_means", "sim_means_abs"), (sv, "sim_vars", "sim_vars_abs"), (sdf, "sdf", "sdf_abs")):
                    tol = hr.PROJ_TOL * n * ref[scale][b]
                    err = np.abs(got - ref[key][b])[~nan] / np.maximum(tol[~nan], 1e-300)
                    assert err.max(initial=0.0) <= 1.0
                    used = max(used, float(err.max(initial=0.0)))
                assert (np.abs(cdf - ref["cdf"][b]) <= EPS * np.abs(ref["cdf"][b])).all()   # single products (the extended one rounds twice)
            nb, nt = hr.SPECIAL_COV["negative"]
            if T > nt:
                raw = np.einsum("jr,rc,jc->j", Z[nb % RZ], P[nb, nt], Z[nb % RZ])
                assert abs(raw[0] + 0.3) < 1e-9 and ref["sim_vars"][nb, nt, 0] == 0.0
            nb, nt = hr.SPECIAL_COV["nan"]
            if T > nt:
                assert np.isnan(ref["sim_vars"][nb, nt]).all() and np.isfinite(ref["sim_means"][nb, nt]).all()
    print("projections (N=%d, n=%d): oracle - extended uses %.3f of PROJ_TOL n sum|terms|" % (N, n, used))


# ------------------------------------------------------------------------------------------------- parameters
@pytest.mark.parametrize("N,K", hr.PARAM_SHAPES)
def test_params_against_params_py(N, K):
    """params.phi_q_from_alpha (fp64) against helper_ref.params (extended): phi within PHI_TOL where 1 - phi^2 does not
    cancel.  The GPU tier compares with phi_q_from_alpha itself (at alpha = 1e8 its 1 - phi^2 has eight digits, which the
    kernel must match, not beat); this test shows that formula and the extended one agree where they can."""
    worst_phi = worst_q = 0.0
    for R in (1, 3, 7):
        for dt in (1.0, 7.0):
            alpha, loadings, _, _ = hr.param_case(N, K, R)
            lb = hr.tile_loadings(loadings, alpha.shape[0])
            phi64, q64 = phi_q_from_alpha(alpha, lb, dt)
            phi, q = hr.params(alpha, lb, dt)
            assert (phi64[alpha < 1e-3] == 0.0).all() and (phi[alpha < 1e-3] == 0.0).all()    # underflow
            assert phi64[0, 0] == 0.0 and 0 < 1 - phi64[0, -1] < 1e-7 * dt
            if K:
                assert (q64[:, 0] == 0.0).all() and (q[:, 0] == 0.0).all()                     # communality exactly 1
            worst_phi = max(worst_phi, float(np.abs(phi64 - phi).max()))
            # 1 - phi^2 in fp64 is off by up to eps absolute (phi^2 rounds at eps / 2, the difference is exact), times |c|
            comm = np.zeros(q.shape)
            comm[:, :N] = (lb ** 2).sum(-1)
            tol = hr.q_bound(lb, q64)
            assert (np.abs(q64 - q) <= tol).all()
            worst_q = max(worst_q, float((np.abs(q64 - q) / np.maximum(tol, 1e-300)).max()))
    print("params (N=%d, K=%d): params.py - extended: phi %.2f eps (bar 8), q at %.3f of q_bound" % (N, K, worst_phi / EPS, worst_q))
    assert worst_phi <= hr.PHI_TOL


@pytest.mark.parametrize("N,K", hr.PARAM_SHAPES)
def test_alpha_grad_against_a_central_difference(N, K):
    """helper_ref.alpha_grad == the central difference of L(alpha) = gphi . phi + gq . q in extended precision, within
    1e-9 of the sum of moduli of the two terms -- and the same formula evaluated in fp64 (libm's exp) is within
    helper_ref.galpha_bound of it: GALPHA_TOL = 16 eps of that sum at every alpha, dt / alpha of several hundred
    included, since the reference takes exp of the same fp64 argument; where phi is subnormal, the extra term derived
    there.  The step moves x = dt / alpha by 1e-6 where x >= 1 (truncation ~1e-12, rounding 1e-19 / 1e-6) and alpha by
    1e-5 of itself below (truncation 1e-10, rounding 1e-14 / x): 1e-9 holds for x >= 1e-4; up to alpha = 1e8, where
    phi = 1 - 1e-8 leaves the difference eleven digits, 1e-4."""
    worst = worst64 = 0.0
    for R in (1, 3):
        for dt in (1.0, 7.0):
            alpha, loadings, gphi, gq = hr.param_case(N, K, R)
            lb = hr.tile_loadings(loadings, alpha.shape[0])
            g, moduli = hr.alpha_grad(alpha, lb, dt, gphi, gq, rounded=False)
            xx = dt / alpha
            h = alpha.astype(hr.LD) * np.where(xx >= 1, 1e-6 / xx, 1e-5).astype(hr.LD)
            php, qp = hr.params(alpha.astype(hr.LD) + h, lb, dt, rounded=False)
            phm, qm = hr.params(alpha.astype(hr.LD) - h, lb, dt, rounded=False)
            # q = c (1 - phi^2): differenced as -c (phi+^2 - phi-^2), since q+ - q- loses phi^2 < 1e-10 against the 1
            c = np.ones(alpha.shape, hr.LD)
            c[:, :N] = 1 - (lb.astype(hr.LD) ** 2).sum(-1)
            assert np.array_equal(hr.f64(qp), hr.f64((1 - php * php) * c))
            fd = (gphi * (php - phm) - gq * c * (php * php - phm * phm)) / (2 * h)
            live = moduli > 0
            assert (g[~live] == 0).all() and (fd[~live] == 0).all()
            sel = live & (xx >= 1e-4)
            worst = max(worst, float((np.abs(fd - g)[sel] / moduli[sel]).max()))
            assert float((np.abs(fd - g)[live] / moduli[live]).max()) < 1e-4
            phi64 = np.exp(-dt / alpha)
            c = np.ones(alpha.shape)
            c[:, :N] = 1.0 - (lb ** 2).sum(-1)
            g64 = (gphi - 2.0 * phi64 * c * gq) * phi64 * dt / (alpha * alpha)
            normal = phi64 >= hr.SMALLEST_NORMAL
            assert (phi64[-1, -1] == 0.0) if dt == 7.0 else (0.0 < phi64[-1, -1] < hr.SMALLEST_NORMAL)   # alpha = 1 / 720
            assert N < 7 or ((xx > 8) & normal).any()                   # large arguments of exp are there
            worst64 = max(worst64, float((np.abs(g64 - hr.f64(g))[normal] / hr.f64(moduli)[normal]).max()))
            assert (np.abs(g64 - hr.f64(g)) <= hr.galpha_bound(alpha, dt, gphi, hr.f64(moduli))).all()
            assert (g64[phi64 == 0.0] == 0.0).all()      # the extended value may be a subnormal there, within the bound
    print("alpha_grad (N=%d, K=%d): central difference within %.1e, fp64 formula within %.2f eps (bar 16) of the moduli"
          % (N, K, worst, worst64 / EPS))
    assert worst < 1e-9 and worst64 <= hr.GALPHA_TOL


# ------------------------------------------------------------------------------------------------- sum
@pytest.mark.parametrize("count", hr.SUM_COUNTS)
def test_sum_bound_holds_for_a_strided_tree_sum(count):
    """The bound of mk_sum, (ceil(count / 1024) + 10) eps sum|v|, checked on a host model of ANY 1024-way strided sum
    followed by a pairwise tree (fp64), against math.fsum; NaN and +inf come through as themselves."""
    used = 0.0
    for kind in hr.SUM_KINDS:
        v = hr.sum_case(count, kind)
        want = hr.fsum(v)
        lanes = np.zeros(1024)
        for start in range(0, count, 1024):
            chunk = v[start:start + 1024]
            lanes[: chunk.size] += chunk
        w = 512
        with np.errstate(invalid="ignore"):
            while w:
                lanes[:w] += lanes[w:2 * w]
                w //= 2
        if kind == "nan":
            assert math.isnan(want) and (count < 1 or math.isnan(lanes[0]))
        elif kind == "inf":
            assert want == math.inf == lanes[0]
        else:
            assert abs(lanes[0] - want) <= hr.sum_bound(v)
            used = max(used, abs(lanes[0] - want) / hr.sum_bound(v))
            if kind == "cancelling" and count > 2:
                assert abs(want) < 1e-6 * np.abs(v).sum()
    print("sum count=%d: strided tree sum - fsum uses %.3f of its bound" % (count, used))
