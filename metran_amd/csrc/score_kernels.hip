// score_kernels.hip -- per-step SCORES of the objective: the derivative of every step's contribution to -2 log L,
// l_t = sum_j (log f + v^2 / f) over the cells observed at t, with respect to every parameter (statsmodels' score_obs), by the
// forward-mode (tangent) filter, and the sums built on them: the gradient, the outer-product information matrix and the
// tied-down cumulative scores of the Nyblom-Hansen test of parameter constancy.
// Size-generic (run-time N, K; n = N + K <= 64), stand-alone: no shape-module entry, no ShapeOps row.
//
// Phi and Q are diagonal with one parameter per state: parameter p moves phi_p and q_p only, by dphi = d phi_p / d theta_p and
// dq = d q_p / d theta_p (inputs: the chain rule stays outside).  Everything the tangent recursion needs from the base filter is
// recorded: the filtered moments of step t - 1 (the recording forward pass), d = P z_j' and 1 / f of every scalar update (the gain
// tape of weights_kernels.h) and the innovation v (innov_step_kernel), so the n tangents of an instance are INDEPENDENT:
//     predict   xd <- phi o xd + dphi x_p e_p
//               Pd <- Phi Pd Phi + dphi (e_p (P_p. o phi) + (phi o P_.p) e_p') + dq e_p e_p'      (x, P filtered at t - 1)
//     cell j    dd = Pd z_j', fd = z_j dd, vd = -z_j xd;   s += fd / f + 2 v vd / f - v^2 fd / f^2
//               xd <- xd + (dd v + d vd) / f - d v fd / f^2;   Pd <- Pd - (dd d' + d dd') / f + d d' fd / f^2
//
// score_tangent_kernel  One lane group per (instance, parameter), b major and p minor: the n groups of an instance are neighbours
//                       in the grid and read the same tape and records.  Lane = state: 16 lanes for n <= 16 (four groups per
//                       wavefront), one wavefront above.  Pd lives in the group's LDS, full square, column c contiguous over the
//                       lanes: lane i reads and writes row i only (address c n + i, conflict-free, and private to the lane --
//                       no ordering between lanes is needed for it); dd_i = Pd[i][j] + sum_k loadings[j,k] Pd[i][N + k] is K + 1
//                       reads; d_c and dd_c of the other lanes are same-address broadcasts of two LDS vectors.  The sums over
//                       the lanes (fd, vd) are the fixed tree of reader_prims.h.  A cell's slot and innovation are loads whose
//                       addresses do not depend on the data: a ring of kAhead cells in registers, as in regress_replay_kernel;
//                       the row of the filtered record is loaded one step ahead.  A cell that is not observed has d = 0 and
//                       1 / f = 0 and adds exactly nothing; a wavefront none of whose groups sees the cell skips it.  The score is
//                       the same number in every lane of the group; lane 0 stores it once per step.
// score_stats_kernel    One workgroup per instance, two passes over its scores in tiles of kScoreTile steps.  A step is COUNTED
//                       when t >= t_first and it holds an observation.  Pass one: grad = sum of the counted scores, count = m.
//                       Pass two: opg = sum s s' and cusum = sum S S' over the counted steps, S_t = sum_{u <= t, counted}
//                       (s_u - grad / m), one accumulator per matrix entry, ascending in time.  Every sum has a fixed order:
//                       an instance's numbers are bit-identical whatever batch, grid, layout or neighbours it runs with.
//                       Whole arithmetic with contraction off and explicit fma.
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

#include "mk_prims.h" // wave_lds_sync
#include "reader_prims.h"
#include "score_kernels.h"

namespace mk {

namespace {

// doubles of LDS per lane group: Pd (n x n), four n-vectors (phi, P_.p, d, dd) and the loadings
__host__ __device__ inline long score_lds_doubles(int N, int K)
{
    const long n = N + K;
    return (n * n + 4 * n + (long)N * K + 1) & ~1L;
}

} // namespace

template <int G, int kAhead>
__global__ void __launch_bounds__(64) score_tangent_kernel(ScoreArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ssm[];
    constexpr int GPB = 64 / G;
    const int N = a.N, K = a.K, n = N + K;
    const long T = a.T;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    double *Pd = ssm + grp * score_lds_doubles(N, K);
    double *ph = Pd + (long)n * n, *prv = ph + n, *dv = prv + n, *ddv = dv + n, *Gm = ddv + n;

    // groups past the last (instance, parameter) pair replicate it (same loads, no stores): the wavefront stays whole
    const long groups = a.B * n;
    long gid = (long)blockIdx.x * GPB + grp;
    const bool live = gid < groups;
    if (!live) gid = groups - 1;
    const long b = gid / n;
    const int p = (int)(gid - b * n);
    const long rec = b % a.R;
    const bool act = lane < n, ser = lane < N;
    const int r = act ? lane : n - 1;
    const int kidx = lane - N < 0 ? 0 : (lane - N > K - 1 ? K - 1 : lane - N);

    for (int i = lane; i < N * K; i += G) Gm[i] = a.loadings[rec * (long)N * K + i];
    const double phi_r = act ? a.phi[b * n + r] : 0.0;
    const double dphi = a.dphi[b * n + p], dq = a.dq[b * n + p];
    if (act) {
        ph[lane] = phi_r;
        for (int c = 0; c < n; ++c) Pd[c * n + lane] = 0.0;
    }
    wave_lds_sync();

    // lane r's entry of z_j = [e_j | loadings[j, :]]
    auto zentry = [&](int j) -> double {
        const double g = Gm[j * K + kidx];
        return ser ? (lane == j ? 1.0 : 0.0) : (act ? g : 0.0);
    };

    const double *tape = a.gain + b * a.bs * N * a.gs; // cell (t, j) of this instance at (t*ts*N + j)*gs
    const double *vrow = a.v + b * a.bs * N;           // ... its innovation at t*ts*N + j
    const double *recs = a.F + b * a.bs * a.rs;        // the filtered record of step t at t*ts*rs

    // filtered x_p and P[r][p] of the step before: the initial state for step 0, then loaded one step ahead
    double x_next = a.x0 ? a.x0[b * n + p] : 0.0;
    double pr_next = a.P0 ? a.P0[(b * n + r) * n + p] : (r == p ? 1.0 : 0.0);

    double xd = 0.0, s = 0.0;
    double dq_[kAhead], rq[kAhead], zq[kAhead], vq[kAhead]; // the ring: d_r, 1/f, the lane's entry of z_j and v of the next kAhead cells
    {
        long tp = 0, t = 0;
        int jp = 0, j = 0;
        // the cell the loading cursor points at, then one cell on; the cursor stays on the last cell of the record
#define MK_S_FETCH(u)                                                        \
    {                                                                        \
        const double *s_ = tape + (tp * a.ts * N + jp) * a.gs;               \
        const double d_ = s_[r];                                             \
        dq_[u] = act ? d_ : 0.0;                                             \
        rq[u] = s_[n];                                                       \
        vq[u] = vrow[tp * a.ts * N + jp];                                    \
        zq[u] = zentry(jp);                                                  \
        if (!(tp == T - 1 && jp == N - 1)) {                                 \
            if (++jp == N) {                                                 \
                jp = 0;                                                      \
                ++tp;                                                        \
            }                                                                \
        }                                                                    \
    }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) MK_S_FETCH(u)
        for (long left = T * N; left > 0; left -= kAhead) {
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (u < left) {
                    const double d = dq_[u], rf = rq[u], z = zq[u], vv = vq[u];
                    MK_S_FETCH(u)
                    if (j == 0) { // ---- the prediction's tangent, from the filtered moments of step t - 1
                        const double px = x_next, pp = pr_next;
                        const double *rp = recs + t * a.ts * a.rs; // step t's own record: what step t + 1 needs
                        x_next = rp[p];
                        pr_next = rp[n + (long)p * n + r];
                        if (act) prv[lane] = pp;
                        wave_lds_sync();
                        xd = phi_r * xd;
                        if (lane == p) xd = fma(dphi, px, xd);
                        if (act) {
                            const double fpp = phi_r * pp;
                            for (int c = 0; c < n; ++c) {
                                double val = (phi_r * ph[c]) * Pd[c * n + lane];
                                if (lane == p) val = fma(dphi, ph[c] * prv[c], val);
                                if (c == p) val = fma(dphi, fpp, val);
                                if (lane == p && c == p) val += dq;
                                Pd[c * n + lane] = val;
                            }
                        }
                        wave_lds_sync();
                    }
                    // ---- the scalar update's tangent; rf is one number per group, the branch one per wavefront
                    if (__builtin_amdgcn_ballot_w64(rf != 0.0) != 0) {
                        const double v = rf != 0.0 ? vv : 0.0; // the innovation row holds NaN where the cell is not observed
                        double dd = 0.0;
                        if (act) {
                            dd = Pd[j * n + lane];
                            for (int k = 0; k < K; ++k) dd = fma(Gm[j * K + k], Pd[(N + k) * n + lane], dd);
                            dv[lane] = d;
                            ddv[lane] = dd;
                        }
                        const double fd = group_sum<G>(z * dd);
                        const double vd = -group_sum<G>(z * xd);
                        wave_lds_sync();
                        const double rf2 = rf * rf;
                        s = fma(fd, rf, s);
                        s = fma((2.0 * v) * vd, rf, s);
                        s = fma(-(v * v) * fd, rf2, s);
                        xd = fma(fma(dd, v, d * vd), rf, xd);
                        xd = fma(-(d * v) * fd, rf2, xd);
                        const double g = fd * rf2;
                        if (act) { // row `lane` of Pd: both products of an entry and of its mirror image are the same numbers
                            for (int c = 0; c < n; ++c) {
                                const double dc = dv[c], ddc = ddv[c];
                                const double tt = dd * dc + d * ddc, w = d * dc;
                                Pd[c * n + lane] = fma(w, g, fma(-tt, rf, Pd[c * n + lane]));
                            }
                        }
                        wave_lds_sync();
                    }
                    if (++j == N) {
                        if (live && lane == 0) a.score[(b * a.bs + t * a.ts) * n + p] = s;
                        s = 0.0;
                        j = 0;
                        ++t;
                    }
                }
            }
        }
#undef MK_S_FETCH
    }
}

constexpr int kScoreTile = 16;     // steps per tile of score_stats_kernel
constexpr int kScoreThreads = 256; // its workgroup
constexpr int kScoreEntries = score_max_states * score_max_states / kScoreThreads; // matrix entries per thread

__global__ void __launch_bounds__(kScoreThreads) score_stats_kernel(ScoreArgs a)
{
    __shared__ double st[kScoreTile][score_max_states]; // the tile's scores (zero at a step that is not counted)
    __shared__ double cs[kScoreTile][score_max_states]; // ... and tied-down cumulative scores
    __shared__ int cnt[kScoreTile];
    const int N = a.N, n = a.N + a.K, tid = threadIdx.x;
    const long T = a.T, b = blockIdx.x, rec = b % a.R;
    const int p = tid < n ? tid : n - 1;

    // whether the steps of the tile from t0 on are counted: t >= t_first and an observation in the row
    auto flags = [&](long t0) {
        if (tid < kScoreTile) {
            const long t = t0 + tid;
            int c = 0;
            if (t < T && t >= a.t_first) {
                const double *y = a.obs + (rec * a.obs_bs + t * a.obs_ts) * N;
                for (int j = 0; j < N; ++j) c |= isfinite(y[j]) ? 1 : 0;
            }
            cnt[tid] = c;
        }
    };
    auto score_at = [&](long t) -> double { return a.score[(b * a.bs + t * a.ts) * n + p]; };

    // ---- pass one: the gradient and the number of counted steps
    double g = 0.0;
    long m = 0;
    for (long t0 = 0; t0 < T; t0 += kScoreTile) {
        flags(t0);
        __syncthreads();
        for (int k = 0; k < kScoreTile; ++k)
            if (cnt[k]) { // every thread counts the steps; only the n threads that hold a parameter read its score
                if (tid < n) g += score_at(t0 + k);
                ++m;
            }
        __syncthreads();
    }
    if (tid < n) a.grad[b * n + tid] = g;
    if (tid == 0) a.count[b] = m; // every thread counted the same steps
    const double gbar = m > 0 ? g / (double)m : 0.0;

    // ---- pass two: one accumulator per matrix entry, ascending in time
    int ep[kScoreEntries], er[kScoreEntries];
    double ao[kScoreEntries], ac[kScoreEntries];
#pragma unroll
    for (int e = 0; e < kScoreEntries; ++e) {
        const int idx = tid + e * kScoreThreads;
        const int i = idx < n * n ? idx : 0;
        ep[e] = i / n;
        er[e] = i - ep[e] * n;
        ao[e] = ac[e] = 0.0;
    }
    double S = 0.0;
    for (long t0 = 0; t0 < T; t0 += kScoreTile) {
        flags(t0);
        __syncthreads();
        if (tid < n) {
            for (int k = 0; k < kScoreTile; ++k) {
                double sc = 0.0;
                if (cnt[k]) {
                    sc = score_at(t0 + k);
                    S += sc - gbar;
                }
                st[k][tid] = sc;
                cs[k][tid] = S;
            }
        }
        __syncthreads();
        for (int k = 0; k < kScoreTile; ++k)
            if (cnt[k]) {
#pragma unroll
                for (int e = 0; e < kScoreEntries; ++e) {
                    ao[e] = fma(st[k][ep[e]], st[k][er[e]], ao[e]);
                    ac[e] = fma(cs[k][ep[e]], cs[k][er[e]], ac[e]);
                }
            }
        __syncthreads();
    }
#pragma unroll
    for (int e = 0; e < kScoreEntries; ++e) {
        const int idx = tid + e * kScoreThreads;
        if (idx < n * n) {
            a.opg[b * n * n + idx] = ao[e];
            a.cusum[b * n * n + idx] = ac[e];
        }
    }
}

template <int G>
static hipError_t launch_tangent(const ScoreArgs &a, hipStream_t s)
{
    constexpr int GPB = 64 / G;
    const long n = a.N + a.K, blocks = (a.B * n + GPB - 1) / GPB;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)GPB * score_lds_doubles(a.N, a.K) * sizeof(double);
    hipLaunchKernelGGL((score_tangent_kernel<G, 8>), dim3((unsigned)blocks), dim3(64), lds, s, a);
    return hipGetLastError();
}

static bool score_args_ok(const ScoreArgs &a)
{
    return a.B >= 1 && a.T >= 1 && a.R >= 1 && a.N >= 1 && a.K >= 1 && a.N + a.K <= score_max_states && a.t_first >= 0;
}

hipError_t launch_score_tangent(const ScoreArgs &a, hipStream_t s)
{
    if (!score_args_ok(a)) return hipErrorInvalidValue;
    if (a.N + a.K <= 16) return launch_tangent<16>(a, s);
    return launch_tangent<64>(a, s);
}

hipError_t launch_score_stats(const ScoreArgs &a, hipStream_t s)
{
    if (!score_args_ok(a) || a.B > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_stats_kernel, dim3((unsigned)a.B), dim3(kScoreThreads), 0, s, a);
    return hipGetLastError();
}

} // namespace mk
