// regress_kernels.hip -- intervention effects by GLS (de Jong's augmented filter; statsmodels' mle_regression, KFAS regression
// effects, STAMP interventions): level shifts, outliers and trends of single series as known regressors of the observation
// equation y_t = X_t beta + Z x_t + e_t, estimated for fixed parameters with standard error and the drop of -2 log L.
// Size-generic (run-time N, K; n = N + K <= 64), stand-alone: no shape-module entry, no ShapeOps row.
//
// Input: the GAIN TAPE that innov_step_kernel writes from the filtered records (weights_kernels.h): per cell (t, j) one slot
// [ d = P z_j' (n) | 1/f | pad ], all zeros at a cell that is not observed.  The covariance recursion does not depend on the data,
// so the filter's mean recursion for ANY data column is a replay of that tape and needs no covariance:
//     per step  a <- phi o a;   per cell j ascending  V = col[t,j] - z_j a,  a <- a + (d / f) V.
//
// regress_replay_kernel  One INSTANCE per lane group, lane = state: 16 lanes for n <= 16 (four instances per wavefront), one
//                        wavefront above.  M + 1 replay vectors, one register per lane each: column 0 is y (from x0), columns
//                        1 .. M are the regressors (from zero), GENERATED from the descriptors (series, kind, t0, t1): lane m
//                        evaluates effect m once per step and the group reads it by broadcast; no [R,M,T,N] array exists.  Phi is
//                        diagonal: the prediction is lane-local.  z_j a is a sum over the group: the fixed tree of reader_prims.h
//                        (group_sum), so an instance's numbers are bit-identical whatever batch, grid or neighbours it runs with.
//                        A cell's slot is one coalesced load whose address does not depend on the data: a ring of kAhead cells
//                        in registers, cell i + kAhead loaded when cell i is taken, so the dependent chain of a cell is one
//                        product, one tree and the multiply-adds.  The normal matrix A = sum V'V / f over the cells of the steps
//                        t >= t_first accumulates in time order, lane m holding row m + 1 (A[m+1, q] = sum (V_{m+1} / f) V_q;
//                        the entries q <= m + 1 are stored, and mirrored); every lane sums A[0,0].  A cell that is not observed
//                        has d = 0 and 1/f = 0 and adds exactly nothing, without a branch.  Lane m counts the support of effect
//                        m: the counted observed cells with x != 0.
//                        The same kernel then solves in the group's LDS, lane m = effect m, in a fixed order: S = A[1:,1:] scaled
//                        to unit diagonal; right-looking Cholesky in effect order (row i in lane i); an effect with support 0
//                        or a pivot below regress_min_pivot is DROPPED (its column of L is zero, the others are solved without
//                        it); L^-1 by forward substitution (column m in lane m); w = L^-1 s, gain = w'w, beta = L^-T w,
//                        cov = L^-T L^-1, every sum in ascending index order; scaled back.  A dropped effect has beta = NaN,
//                        NaN in its row and column of cov and its bit in the instance's dropped mask.
//                        Whole arithmetic with contraction off and explicit fma: the same roundings for every M.
// regress_adjust_kernel  out = obs - sum_m beta_m x_m, one thread per cell, the effects of the cell's record in ascending order;
//                        a NaN beta counts as 0, a NaN observation stays NaN.
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

#include "mk_prims.h" // wave_lds_sync
#include "reader_prims.h"
#include "regress_kernels.h"

namespace mk {

namespace {

constexpr int kRegU = regress_max_effects + 1; // row length of the solve's matrix in LDS
// doubles of LDS per lane group: the loadings, the solve's matrix and four vectors (sd, s / sd, w, kept)
__host__ __device__ inline long regress_lds_doubles(int N, int K)
{
    return (((long)N * K + 1) & ~1L) + regress_max_effects * kRegU + 4 * regress_max_effects;
}

} // namespace

template <int G, int kAhead, int MT>
__global__ void __launch_bounds__(64) regress_replay_kernel(RegressArgs a)
{
    static_assert(MT >= 1 && MT <= regress_max_effects && regress_max_effects <= G, "one effect per lane of the group");
    extern __shared__ __attribute__((aligned(16))) double rsm[];
    constexpr int GPB = 64 / G;
    const int N = a.N, K = a.K, n = N + K, M = (int)a.M;
    const long T = a.T;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    double *Gm = rsm + grp * regress_lds_doubles(N, K);
    double *U = Gm + (((long)N * K + 1) & ~1L), *sd = U + regress_max_effects * kRegU, *ss = sd + regress_max_effects;
    double *wv = ss + regress_max_effects, *kp = wv + regress_max_effects;

    // groups past the last instance replicate it (same loads, no stores): the wavefront stays whole
    long b = (long)blockIdx.x * GPB + grp;
    const bool live = b < a.B;
    if (!live) b = a.B - 1;
    const long rec = b % a.R;
    const bool act = lane < n, ser = lane < N;
    const int r = act ? lane : n - 1;
    const int kidx = lane - N < 0 ? 0 : (lane - N > K - 1 ? K - 1 : lane - N);
    const double nan = __builtin_nan("");

    for (int i = lane; i < N * K; i += G) Gm[i] = a.loadings[rec * (long)N * K + i];
    wave_lds_sync();

    const double phi_r = act ? a.phi[b * n + r] : 0.0;
    const double x0_r = (act && a.x0) ? a.x0[b * n + r] : 0.0;
    // lane r's entry of z_j = [e_j | loadings[j, :]]
    auto zentry = [&](int j) -> double {
        const double g = Gm[j * K + kidx];
        return ser ? (lane == j ? 1.0 : 0.0) : (act ? g : 0.0);
    };

    // lane m's own effect; a slot with a negative series is not in use
    const bool mine = lane < M;
    const int64_t *ef = a.effects + (rec * M + (mine ? lane : 0)) * 4;
    const long ejs = ef[0], ekind = ef[1], et0 = ef[2], et1 = ef[3];
    const bool used = mine && ejs >= 0;
    const int js_own = used ? (int)(ejs < N ? ejs : N) : -1;
    auto xstep = [&](long t) -> double { // the regressor of the lane's effect at step t, on its series
        if (!used || t < et0) return 0.0;
        if (ekind == 0) return t < et1 ? 1.0 : 0.0;
        return (double)((t < et1 - 1 ? t : et1 - 1) - et0 + 1);
    };
    int js[MT];
#pragma unroll
    for (int c = 0; c < MT; ++c) js[c] = __shfl(js_own, c, G);

    const double *tape = a.gain + b * a.bs * N * a.gs;                      // cell (t, j) of this instance at (t*ts*N + j)*gs
    const double *yrow = a.obs + rec * a.obs_bs * N + (ser ? lane : N - 1); // row t at t*obs_ts*N

    double av[MT + 1], acc[MT + 1], xt[MT], V[MT + 1];
#pragma unroll
    for (int c = 0; c <= MT; ++c) av[c] = acc[c] = 0.0;
#pragma unroll
    for (int c = 0; c < MT; ++c) xt[c] = 0.0;
    av[0] = x0_r;
    double a00 = 0.0;
    long sup = 0;

    double dq[kAhead], rq[kAhead], zq[kAhead]; // the ring: d_r, 1/f and the lane's entry of z_j of the next kAhead cells
    {
        long tp = 0, t = 0;
        int jp = 0, j = 0;
        // the cell the loading cursor points at, then one cell on; the cursor stays on the last cell of the record
#define MK_R_FETCH(u)                                                        \
    {                                                                        \
        const double *s_ = tape + (tp * a.ts * N + jp) * a.gs;               \
        const double d_ = s_[r];                                             \
        dq[u] = act ? d_ : 0.0;                                              \
        rq[u] = s_[n];                                                       \
        zq[u] = zentry(jp);                                                  \
        if (!(tp == T - 1 && jp == N - 1)) {                                 \
            if (++jp == N) {                                                 \
                jp = 0;                                                      \
                ++tp;                                                        \
            }                                                                \
        }                                                                    \
    }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) MK_R_FETCH(u)
        // y of a step is loaded one step ahead
        double ynext = yrow[0], yown = nan, xo = 0.0;
        bool counted = false;
        for (long left = T * N; left > 0; left -= kAhead) {
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (u < left) {
                    const double d = dq[u], rf = rq[u], z = zq[u];
                    MK_R_FETCH(u)
                    if (j == 0) {
#pragma unroll
                        for (int c = 0; c <= MT; ++c) av[c] = phi_r * av[c];
                        yown = ynext;
                        ynext = yrow[(t + 1 < T ? t + 1 : T - 1) * a.obs_ts * N];
                        xo = xstep(t);
#pragma unroll
                        for (int c = 0; c < MT; ++c) xt[c] = __shfl(xo, c, G);
                        counted = t >= a.t_first;
                    }
                    const double yj = __shfl(yown, j, G);
                    const bool seen = isfinite(yj);
                    V[0] = (seen ? yj : 0.0) - group_sum<G>(z * av[0]);
#pragma unroll
                    for (int c = 1; c <= MT; ++c) V[c] = (j == js[c - 1] ? xt[c - 1] : 0.0) - group_sum<G>(z * av[c]);
                    const double kr = d * rf;
#pragma unroll
                    for (int c = 0; c <= MT; ++c) av[c] = fma(kr, V[c], av[c]);
                    double vown = 0.0;
#pragma unroll
                    for (int c = 1; c <= MT; ++c) vown = lane == c - 1 ? V[c] : vown;
                    const double rc = counted ? rf : 0.0;
                    const double wo = vown * rc;
#pragma unroll
                    for (int c = 0; c <= MT; ++c) acc[c] = fma(wo, V[c], acc[c]);
                    a00 = fma(V[0] * rc, V[0], a00);
                    sup += (counted && seen && j == js_own && xo != 0.0) ? 1 : 0;
                    if (++j == N) {
                        j = 0;
                        ++t;
                    }
                }
            }
        }
#undef MK_R_FETCH
    }

    // ---- A: lane m holds row m + 1, entries q <= m + 1; mirrored into the square
    const long M1 = M + 1;
    if (live && mine) {
        double *An = a.normal + b * M1 * M1;
#pragma unroll
        for (int q = 0; q <= MT; ++q)
            if (q <= lane + 1) {
                An[(lane + 1) * M1 + q] = acc[q];
                An[q * M1 + lane + 1] = acc[q];
            }
        if (lane == 0) An[0] = a00;
        a.support[b * M + lane] = sup;
    }

    // ---- the solve: S = A[1:,1:] to unit diagonal, s = A[0,1:]
    double s_own = 0.0, sii = 0.0;
#pragma unroll
    for (int q = 0; q <= MT; ++q) {
        if (mine && q <= lane + 1) U[lane * kRegU + q] = acc[q];
        sii = q == lane + 1 ? acc[q] : sii;
    }
    s_own = acc[0];
    const bool pos = sii > 0.0;
    const double sd_own = pos ? sqrt(sii) : 1.0;
    if (mine) {
        sd[lane] = sd_own;
        kp[lane] = (used && pos && sup > 0) ? 1.0 : 0.0;
        ss[lane] = s_own / sd_own;
    }
    wave_lds_sync();
    if (mine) { // row i of the scaled matrix, entries j <= i, moved one place down in the row
        for (int jj = 0; jj <= lane; ++jj) U[lane * kRegU + jj] = U[lane * kRegU + jj + 1] / (sd_own * sd[jj]);
    }
    wave_lds_sync();
    // right-looking Cholesky in effect order; the column of a dropped effect is zero
    for (int k = 0; k < M; ++k) {
        const double piv = U[k * kRegU + k];
        const bool keep = kp[k] != 0.0 && piv >= regress_min_pivot;
        const double lk = keep ? sqrt(piv) : 1.0;
        double lik = 0.0;
        if (mine && lane > k) {
            lik = keep ? U[lane * kRegU + k] / lk : 0.0;
            U[lane * kRegU + k] = lik;
        }
        if (lane == k) {
            U[k * kRegU + k] = lk;
            kp[k] = keep ? 1.0 : 0.0;
        }
        wave_lds_sync();
        if (mine && lane > k) {
            for (int jj = k + 1; jj <= lane; ++jj) U[lane * kRegU + jj] = fma(-lik, U[jj * kRegU + k], U[lane * kRegU + jj]);
        }
        wave_lds_sync();
    }
    // L^-1 by forward substitution, column m in lane m: (L^-1)[i, m], i >= m, parked at U[m, i + 1]
    const bool kept = mine && kp[mine ? lane : 0] != 0.0;
    if (mine) {
        for (int i = lane; i < M; ++i) {
            double val = 0.0;
            if (kept && kp[i] != 0.0) {
                if (i == lane) {
                    val = 1.0 / U[i * kRegU + i];
                } else {
                    double sum = 0.0;
                    for (int k = lane; k < i; ++k) sum = fma(U[i * kRegU + k], U[lane * kRegU + k + 1], sum);
                    val = -sum / U[i * kRegU + i];
                }
            }
            U[lane * kRegU + i + 1] = val;
        }
    }
    wave_lds_sync();
    // w = L^-1 (s / sd): lane k its entry, the sum over j <= k ascending
    if (mine) {
        double w = 0.0;
        for (int jj = 0; jj <= lane; ++jj) w = fma(U[jj * kRegU + lane + 1], kp[jj] != 0.0 ? ss[jj] : 0.0, w);
        wv[lane] = kept ? w : 0.0;
    }
    wave_lds_sync();
    if (live && mine) {
        // beta = L^-T w and cov = L^-T L^-1, scaled back: the sums over k >= max(i, j) ascending
        double bsum = 0.0;
        for (int k = lane; k < M; ++k) bsum = fma(U[lane * kRegU + k + 1], wv[k], bsum);
        a.beta[b * M + lane] = kept ? bsum / sd_own : nan;
        for (int jj = 0; jj < M; ++jj) {
            double cs = 0.0;
            for (int k = (jj > lane ? jj : lane); k < M; ++k) cs = fma(U[lane * kRegU + k + 1], U[jj * kRegU + k + 1], cs);
            a.cov[(b * M + lane) * M + jj] = (kept && kp[jj] != 0.0) ? cs / (sd_own * sd[jj]) : nan;
        }
        if (lane == 0) {
            double g = 0.0;
            uint32_t mask = 0;
            for (int k = 0; k < M; ++k) {
                g = fma(wv[k], wv[k], g);
                mask |= kp[k] != 0.0 ? 0u : (1u << k);
            }
            a.gainout[b] = g;
            a.dropped[b] = mask;
        }
    }
}

__global__ void __launch_bounds__(256) regress_adjust_kernel(RegressAdjustArgs a)
{
    const long cells = a.R * a.T * a.N;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= cells) return;
    const long row = i / a.N;
    const int j = (int)(i - row * a.N);
    long rec, t; // row (r, t) at r*bs + t*ts: one of the two strides is 1
    if (a.ts == 1) {
        rec = row / a.T;
        t = row - rec * a.T;
    } else {
        t = row / a.R;
        rec = row - t * a.R;
    }
    double y = a.in[i];
    for (long m = 0; m < a.M; ++m) {
        const int64_t *ef = a.effects + (rec * a.M + m) * 4;
        const long t0 = ef[2], t1 = ef[3];
        if (ef[0] != j || t < t0) continue;
        const double x = ef[1] == 0 ? (t < t1 ? 1.0 : 0.0) : (double)((t < t1 - 1 ? t : t1 - 1) - t0 + 1);
        const double be = a.beta[rec * a.M + m];
        y = fma(-(be == be ? be : 0.0), x, y);
    }
    a.out[i] = y;
}

template <int G, int kAhead, int MT>
static hipError_t launch_replay(const RegressArgs &a, hipStream_t s)
{
    constexpr int GPB = 64 / G;
    const long blocks = (a.B + GPB - 1) / GPB;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)GPB * regress_lds_doubles(a.N, a.K) * sizeof(double);
    hipLaunchKernelGGL((regress_replay_kernel<G, kAhead, MT>), dim3((unsigned)blocks), dim3(64), lds, s, a);
    return hipGetLastError();
}

// M rounded up to 1, 4, 8 or 16 columns (the spare ones replay zeros, and every sum of A is a column pair's own: the numbers of
// an effect do not depend on the rounding).  The ring holds 8 cells, 4 at 16 columns: 244 registers, two wavefronts per SIMD
// (286 with 8).
template <int G>
static hipError_t launch_replay_m(const RegressArgs &a, hipStream_t s)
{
    if (a.M <= 1) return launch_replay<G, 8, 1>(a, s);
    if (a.M <= 4) return launch_replay<G, 8, 4>(a, s);
    if (a.M <= 8) return launch_replay<G, 8, 8>(a, s);
    return launch_replay<G, 4, 16>(a, s);
}

hipError_t launch_regress_replay(const RegressArgs &a, hipStream_t s)
{
    const int n = a.N + a.K;
    if (a.B < 1 || a.T < 1 || a.R < 1 || a.M < 1 || a.M > regress_max_effects || a.N < 1 || a.K < 1 || n > regress_max_states)
        return hipErrorInvalidValue;
    if (n <= 16) return launch_replay_m<16>(a, s);
    return launch_replay_m<64>(a, s);
}

hipError_t launch_regress_adjust(const RegressAdjustArgs &a, hipStream_t s)
{
    if (a.R < 1 || a.T < 1 || a.N < 1 || a.M < 1 || a.M > regress_max_effects) return hipErrorInvalidValue;
    const long cells = a.R * a.T * a.N, blocks = (cells + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(regress_adjust_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace mk
