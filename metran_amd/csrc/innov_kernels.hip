// innov_kernels.hip -- one-step-ahead innovations of every observed cell, the marginal one-step-ahead forecast of every series, and
// the whiteness (Ljung-Box) statistics of the standardised innovations.  Size-generic (run-time N, K; n = N + K <= 64), stand-alone:
// no shape-module entry, no ShapeOps row.
// Reference semantics: seqkalmanfilter (metran/kalmanfilter.py: predict :318-333, sequential scalar updates :341-378) -- whose
// innovation v and variance f of every scalar update the filter kernels fold into sigmas[t] / detfs[t] and never write.
//
// innov_step_kernel   The filtered moments of step t - 1 determine step t completely, so the T steps of an instance are INDEPENDENT
//                     given the filtered records of the recording forward pass (mk_loglik_grad / mk_loo; the observation
//                     adjoint_kernel walks backwards on).  One (instance, step) PAIR per lane group: 16 lanes for n <= 16 (four pairs
//                     per wavefront), one wavefront above.  Lane r holds row r of the covariance in registers, padded to W = 16 / 32 /
//                     64 columns (column blocks of four beyond n are skipped, not computed); what an update needs from the other lanes
//                     -- the observation row z_j, the state x and d = P z_j' -- goes through the group's private LDS vectors, read back as
//                     broadcasts.  The sums run over the columns in ascending order and skip the blocks of four in which z_j is
//                     all zero (a run-time uniform branch per block around compile-time register indices; a zero inside a kept
//                     block adds exactly nothing): the same multiply-adds in the same order as the filter kernels', so v and f
//                     are the filter's own numbers.  No cross-lane instruction chains: the pairs are
//                     independent and occupancy hides the latencies.  With InnovArgs.gain set the kernel also stores d and
//                     1 / f of every scalar update -- lane r its d_r -- into the cell's slot of the gain tape that
//                     weights_kernels.hip walks; v, f and the forecasts are the same numbers with or without it.
// innov_stats_kernel  One wavefront per (instance, series): time in tiles of kInnovTile steps, a lane per step.  TWO passes over v / f:
//                     the mean first, then the lagged products of the centred values -- the second pass RE-READS v and f (a series
//                     is 16 T bytes; the tile's cells were just read and sit in L2) instead of keeping the series in LDS, whose
//                     size would bound T.  Lags count successive VALID cells: each tile's valid values are compacted (ballot prefix)
//                     behind a ring of the last innov_max_lags values, and compacted element i multiplies elements i - l.  Every sum
//                     is a fixed tree over the lanes and a fixed sequence over the tiles: bit-identical for a series whatever the
//                     batch around it.
#include <hip/hip_runtime.h>

#include <cmath>

#include "innov_kernels.h"
#include "mk_prims.h" // wave_lds_sync, rcp_nr: the filter kernels' own -- v and f are the filter's numbers bit for bit
#include "reader_prims.h"

namespace mk {

namespace {

// doubles of LDS per lane group: six W-vectors (z_j, d, x, phi, y, obsvar), the factor block of P (K x K) and the loadings (N x K)
inline long innov_lds_doubles(int W, int N, int K) { return (6L * W + (long)(N + K) * K + 1) & ~1L; }

// bit-identical in every lane: at each stage lanes i and i ^ off add the same two numbers
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

} // namespace

template <int G, int W>
__global__ void __launch_bounds__(G == 16 ? 256 : 64) innov_step_kernel(InnovArgs a)
{
    static_assert(W <= G && W % 4 == 0, "one covariance row per lane, columns in blocks of four");
    extern __shared__ __attribute__((aligned(16))) double ism[];
    constexpr int NT = G == 16 ? 256 : 64, GPB = NT / G;
    const int N = a.N, K = a.K, n = N + K;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const long per = (6L * W + (long)n * K + 1) & ~1L;
    double *zv = ism + grp * per, *dv = zv + W, *xv = dv + W, *ph = xv + W, *yv = ph + W, *rv = yv + W;
    double *PF = rv + W, *Gm = PF + K * K;

    // groups past the last pair replicate it (same loads, no stores): the wavefront stays whole
    const long pairs = a.B * a.T;
    long pair = (long)blockIdx.x * GPB + grp;
    const bool live = pair < pairs;
    if (!live) pair = pairs - 1;
    long b, t; // consecutive pairs are neighbours in memory in either layout
    if (a.ts == 1) {
        b = pair / a.T;
        t = pair - b * a.T;
    } else {
        t = pair / a.B;
        b = pair - t * a.B;
    }
    const long rec = b % a.R;
    const bool act = lane < n, ser = lane < N;
    const int r = act ? lane : n - 1; // lanes beyond the model replicate its last row and contribute zeros
    const int jl = ser ? lane : N - 1;
    const double nan = __builtin_nan("");

    const double phi_r = a.phi[b * n + r], q_r = a.q[b * n + r];
    if (lane < W) {
        ph[lane] = act ? phi_r : 0.0;
        yv[lane] = ser ? a.obs[(rec * a.obs_bs + t * a.obs_ts) * N + lane] : nan;
        rv[lane] = (ser && a.obsvar) ? a.obsvar[rec * N + lane] : 0.0;
    }
    for (int i = lane; i < N * K; i += G) Gm[i] = a.loadings[rec * (long)N * K + i];

    // filtered moments of step t - 1 (the record holds the transpose: position (c, r) is lane r's element c, mk_prims.h), or the
    // initial state
    double x, P[W];
    if (t > 0) {
        const double *p = a.F + (b * a.bs + (t - 1) * a.ts) * a.rs;
        x = p[r];
#pragma unroll
        for (int c0 = 0; c0 < W; c0 += 4) {
#pragma unroll
            for (int c = c0; c < c0 + 4; ++c) P[c] = 0.0;
            if (c0 < n) {
#pragma unroll
                for (int c = c0; c < c0 + 4; ++c) {
                    const double val = p[n + (c < n ? c : 0) * n + r];
                    P[c] = c < n ? val : 0.0;
                }
            }
        }
    } else { // run_filter's defaults (kalmanfilter.py:747-750) or the caller's initial state
        x = a.x0 ? a.x0[b * n + r] : 0.0;
#pragma unroll
        for (int c0 = 0; c0 < W; c0 += 4) {
#pragma unroll
            for (int c = c0; c < c0 + 4; ++c) P[c] = 0.0;
            if (c0 < n) {
#pragma unroll
                for (int c = c0; c < c0 + 4; ++c) {
                    const int cc = c < n ? c : 0;
                    const double val = a.P0 ? a.P0[(b * n + r) * n + cc] : (cc == r ? 1.0 : 0.0);
                    P[c] = c < n ? val : 0.0;
                }
            }
        }
    }
    wave_lds_sync();

    // ---- predict (:318-331; Phi diagonal): x = phi o x, P = (phi phi') o P + diag(q)
    x = phi_r * x;
#pragma unroll
    for (int c0 = 0; c0 < W; c0 += 4) {
        if (c0 < n) {
#pragma unroll
            for (int c = c0; c < c0 + 4; ++c) P[c] = fma(P[c], phi_r * ph[c], c == r ? q_r : 0.0);
        }
    }
    if (lane < W) xv[lane] = act ? x : 0.0;
    const long orow = (b * a.bs + t * a.ts) * N + lane;

    // ---- marginal forecast of every series j, observed or not: z_j x and z_j P z_j' + r_j, Z = [I | loadings]
    if (a.pred_mean || a.pred_var) {
#pragma unroll
        for (int c = 0; c < W; ++c)
            if (c >= N && c < n) {
                if (act && !ser) PF[(lane - N) * K + (c - N)] = P[c];
            }
        wave_lds_sync();
        double diag = 0.0, cross = 0.0, pm = x;
#pragma unroll
        for (int c = 0; c < W; ++c) {
            diag = (c == lane) ? P[c] : diag;
            if (c >= N && c < n) {
                const double g = Gm[jl * K + (c - N)];
                cross = fma(g, P[c], cross);
                pm = fma(g, xv[c], pm);
            }
        }
        double quad = 0.0;
        for (int k = 0; k < K; ++k) {
            double h = 0.0;
            for (int l = 0; l < K; ++l) h = fma(Gm[jl * K + l], PF[k * K + l], h);
            quad = fma(Gm[jl * K + k], h, quad);
        }
        const double pv = fma(2.0, cross, diag) + quad + rv[jl];
        const double sc = a.scale ? a.scale[rec * N + jl] : 1.0, of = a.offset ? a.offset[rec * N + jl] : 0.0;
        if (live && ser) {
            if (a.pred_mean) a.pred_mean[orow] = scaled_mean(pm, sc, of);
            if (a.pred_var) a.pred_var[orow] = scaled_var(pv, sc);
        }
    }
    if (!(a.v || a.f || a.gain)) return;

    // ---- sequential scalar updates (:341-378), ascending series order over the observed series
    double vown = nan, fown = nan;
    for (int j = 0; j < N; ++j) {
        wave_lds_sync();
        const double y = yv[j];
        if (!isfinite(y)) continue; // NaN / inf = missing (:657); the same for every lane of the group
        if (lane < W) {
            zv[lane] = ser ? (lane == j ? 1.0 : 0.0) : (act ? Gm[j * K + (lane - N)] : 0.0);
            xv[lane] = act ? x : 0.0;
        }
        wave_lds_sync();
        double d = 0.0, v = y; // d_r = (P z_j')_r (:349-357), v = y - z_j x (:344-347)
#pragma unroll
        for (int c0 = 0; c0 < W; c0 += 4) {
            if (c0 < n && (c0 + 4 > N || (j >> 2) == (c0 >> 2))) { // z_j is zero in every other block: nothing is left out
#pragma unroll
                for (int c = c0; c < c0 + 4; ++c) {
                    const double z = zv[c];
                    d = fma(P[c], z, d);
                    v = fma(-z, xv[c], v);
                }
            }
        }
        if (lane < W) dv[lane] = act ? d : 0.0;
        wave_lds_sync();
        double f = rv[j]; // f = z_j d + r_j (:359-362)
#pragma unroll
        for (int c0 = 0; c0 < W; c0 += 4) {
            if (c0 < n && (c0 + 4 > N || (j >> 2) == (c0 >> 2))) {
#pragma unroll
                for (int c = c0; c < c0 + 4; ++c) f = fma(zv[c], dv[c], f);
            }
        }
        const double rf = rcp_nr(f), kr = d * rf;
        if (a.gain && live) { // the slot of cell (t, j): lane r its d_r, the first lane 1/f
            double *slot = a.gain + ((b * a.bs + t * a.ts) * N + j) * a.gs;
            if (act) slot[lane] = d;
            if (lane == 0) slot[n] = rf;
        }
#pragma unroll
        for (int c0 = 0; c0 < W; c0 += 4) { // P -= k k' f (:368-372)
            if (c0 < n) {
#pragma unroll
                for (int c = c0; c < c0 + 4; ++c) P[c] = fma(-dv[c], kr, P[c]);
            }
        }
        x = fma(kr, v, x); // :374-375
        vown = (lane == j) ? v : vown;
        fown = (lane == j) ? f : fown;
    }
    if (live && ser) {
        if (a.v) a.v[orow] = vown;
        if (a.f) a.f[orow] = fown;
    }
}

constexpr int kInnovTile = 64; // time steps per pass of a wavefront: one lane per step

__global__ void __launch_bounds__(256) innov_stats_kernel(InnovStatsArgs a)
{
    static_assert(kInnovTile == 64, "one lane of the wavefront per step of a tile");
    __shared__ double ring[4][innov_max_lags + kInnovTile];
    const int lane = threadIdx.x % 64, w = threadIdx.x / 64;
    const int N = a.N, L = a.L;
    const long series = a.B * N;
    long s = (long)blockIdx.x * 4 + w;
    const bool live = s < series;
    if (!live) s = series - 1;
    const long b = s / N;
    const int j = (int)(s - b * N);
    double *buf = ring[w];
    for (int i = lane; i < innov_max_lags + kInnovTile; i += 64) buf[i] = 0.0;

    // the standardised innovation e = v / sqrt(f) of cell (t, j); false where the cell does not count
    auto cell = [&](long t, double &e) -> bool {
        e = 0.0;
        if (t >= a.T || t < a.t_first) return false;
        const long i = (b * a.bs + t * a.ts) * N + j;
        const double v = a.v[i], f = a.f[i];
        const bool ok = isfinite(v) && isfinite(f) && f > 0.0;
        if (ok) e = v / sqrt(f);
        return ok;
    };

    // ---- first pass: the number of valid cells and their mean
    double sum = 0.0;
    long m = 0;
    for (long t0 = 0; t0 < a.T; t0 += kInnovTile) {
        double e;
        const bool ok = cell(t0 + lane, e);
        m += __popcll(__ballot(ok));
        sum += wave_sum(e);
    }
    const double dm = (double)m, mean = sum / dm; // m = 0: NaN

    // ---- second pass: sums of (e_i - mean)(e_{i-l} - mean), l = 0 .. L, over the compacted series
    double acc[innov_max_lags + 1];
#pragma unroll
    for (int l = 0; l <= innov_max_lags; ++l) acc[l] = 0.0;
    long base = 0; // valid cells before this tile
    for (long t0 = 0; t0 < a.T; t0 += kInnovTile) {
        double e;
        const bool ok = cell(t0 + lane, e);
        const unsigned long long ball = __ballot(ok);
        const int pos = __popcll(ball & ((1ull << lane) - 1ull)), cnt = __popcll(ball);
        if (ok) buf[innov_max_lags + pos] = e - mean;
        wave_lds_sync();
        if (lane < cnt) {
            const double own = buf[innov_max_lags + lane];
            const long gi = base + lane;
#pragma unroll
            for (int l = 0; l <= innov_max_lags; ++l)
                if (l <= L) {
                    if (gi >= l) acc[l] = fma(own, buf[innov_max_lags + lane - l], acc[l]);
                }
        }
        wave_lds_sync();
        const double keep = lane < innov_max_lags ? buf[cnt + lane] : 0.0; // the last innov_max_lags values move to the front
        wave_lds_sync();
        if (lane < innov_max_lags) buf[lane] = keep;
        wave_lds_sync();
        base += cnt;
    }
#pragma unroll
    for (int l = 0; l <= innov_max_lags; ++l) acc[l] = wave_sum(acc[l]);

    if (!live || lane != 0) return;
    const double nan = __builtin_nan("");
    double *out = a.stats + s * (4 + L);
    const double c0 = acc[0] / dm;
    const bool white = m > L && c0 > 0.0; // r_l and Q need more cells than lags and a series that varies
    double Q = 0.0;
#pragma unroll
    for (int l = 1; l <= innov_max_lags; ++l)
        if (l <= L) {
            const double rl = white ? (acc[l] / dm) / c0 : nan;
            out[3 + l] = rl;
            Q += rl * rl / (double)(m - l);
        }
    out[0] = dm;
    out[1] = mean;
    out[2] = c0;
    out[3] = white ? dm * (dm + 2.0) * Q : nan;
}

template <int G, int W>
static hipError_t launch_step(const InnovArgs &a, hipStream_t s)
{
    constexpr int NT = G == 16 ? 256 : 64, GPB = NT / G;
    const long pairs = a.B * a.T, blocks = (pairs + GPB - 1) / GPB;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)GPB * innov_lds_doubles(W, a.N, a.K) * sizeof(double);
    hipLaunchKernelGGL((innov_step_kernel<G, W>), dim3((unsigned)blocks), dim3(NT), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_innov_step(const InnovArgs &a, hipStream_t s)
{
    const int n = a.N + a.K;
    if (a.B < 1 || a.T < 1 || a.R < 1 || a.N < 1 || a.K < 1 || n > innov_max_states) return hipErrorInvalidValue;
    if (n <= 16) return launch_step<16, 16>(a, s);
    if (n <= 32) return launch_step<64, 32>(a, s);
    return launch_step<64, 64>(a, s);
}

hipError_t launch_innov_stats(const InnovStatsArgs &a, hipStream_t s)
{
    if (a.B < 1 || a.T < 1 || a.N < 1 || a.L < 1 || a.L > innov_max_lags || a.t_first < 0) return hipErrorInvalidValue;
    const long blocks = (a.B * a.N + 3) / 4;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(innov_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace mk
