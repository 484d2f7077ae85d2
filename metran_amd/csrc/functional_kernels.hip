// functional_kernels.hip -- exact window means, changes and contrasts of the smoothed signal: the posterior mean and variance of a
// LINEAR functional of the smoothed path,
//     l = sum_t alpha_t c'(scale o Z x_t + offset),   alpha_t = 1/(t1-t0) on [t0,t1),  -1/(t3-t2) on [t2,t3),
// which needs the smoother's covariance ACROSS time (the smoothed state autocovariance: de Jong & Mackinnon 1988; Durbin & Koopman
// 2012, section 4.7; statsmodels' smoothed_state_autocov): Cov(x_t, x_s | Y) = J_t ... J_{s-1} Ps_s for t < s, with the smoother's
// gain J_t = Pf_t Phi Pp_{t+1}^-1.  The [T,T,n,n] object is never formed: with w_t = alpha_t Z'(c o scale) the hull [t_lo, t_hi)
// of the two ranges is walked backwards once,
//     mean += w_t' S_t;   c_t = J_t u_{t+1} (0 at t_hi - 1);   p_t = Ps_t w_t;   var += w_t'(p_t + 2 c_t);   u_t = p_t + c_t
// (c_t is carried through the steps of a gap, where alpha_t = 0).  Size-generic (run-time N, K; n = N + K <= 64), stand-alone: no
// shape-module entry, no ShapeOps row.  Input: the filtered records of the recording forward pass and the smoothed records of the
// smoother, full-square.
//
// functional_walk_kernel  One (instance, window) per lane group, lane = state: 16 lanes for n <= 16 (four walks per wavefront), one
//                         wavefront above.  Per step below the last one of the hull the group forms Pp_{t+1} = Phi Pf_t Phi + Q in
//                         its LDS and factorises it ONCE as L D L' (row r by lane r, right-looking; a positive pivot is inverted, a
//                         pivot <= 0 is dropped with MK_FLAG_RANK_DEFICIENT, < -1e-8 is MK_FLAG_NOT_SPD: the smoothers' contract);
//                         the contrasts of the window are solved against that factor kCH at a time, their vectors one register
//                         per lane and contrast: forward and backward substitution with the entry of the other lane fetched by a
//                         lane exchange (lane_value: a scalar read of the lane in the one-wavefront kernel), then the two
//                         products Pf_t (Phi y) and Ps_t z with the matrix columns read from the records (lane r the element
//                         (k, r): coalesced, kLoads of them in flight).  A window with more than kCH contrasts is walked once
//                         per chunk of kCH.  Every sum has a fixed order -- the products ascending in k, the sums over time
//                         descending in t per lane, the sum over the lanes the fixed tree of group_sum (reader_prims.h) -- so a
//                         functional's value is bit-identical whatever batch, neighbouring windows or other contrasts it runs with.
//                         A window whose first range is empty (after clamping to [0, T]) is NaN in both outputs and walks nothing.
#include <hip/hip_runtime.h>

#include <cmath>

#include "functional_kernels.h"
#include "metran_hip.h" // MK_FLAG_*
#include "mk_prims.h"   // wave_lds_sync
#include "reader_prims.h"

namespace mk {

namespace {

// doubles of LDS per lane group: the factor [n, n | 1] (odd leading dimension: a column read by the lanes meets every bank once), the
// unscaled pivot column [G] and phi [G]
inline long functional_lds_doubles(int n, int G) { return ((long)n * (n | 1) + 2 * G + 1) & ~1L; }

__device__ __forceinline__ long clamp_step(long t, long T) { return t < 0 ? 0 : (t > T ? T : t); }

constexpr int kLoads = 8; // record elements a lane loads before it uses the first of them

// lane k's value of x in every lane of the group (k the same in all lanes): one wavefront reads the lane into scalar registers, a
// 16-lane group exchanges inside its row
template <int G>
__device__ __forceinline__ double lane_value(double x, int k)
{
    if constexpr (G == 64) {
        const int ku = __builtin_amdgcn_readfirstlane(k);
        const int lo = __builtin_amdgcn_readlane(__double2loint(x), ku), hi = __builtin_amdgcn_readlane(__double2hiint(x), ku);
        return __hiloint2double(hi, lo);
    } else {
        return __shfl(x, k, G);
    }
}

} // namespace

template <int G, int kCH>
__global__ void __launch_bounds__(64) functional_walk_kernel(FunctionalArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double fsm[];
    constexpr int GPB = 64 / G;
    const int N = a.N, K = a.K, n = N + K, ld = n | 1;
    const long T = a.T, W = a.W, C = a.C;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    double *A = fsm + grp * (((long)n * ld + 2 * G + 1) & ~1L), *col = A + (long)n * ld, *phis = col + G;

    // groups past the last window replicate it (same loads, no stores): the wavefront stays whole
    const long groups = a.B * W;
    long gid = (long)blockIdx.x * GPB + grp;
    const bool live = gid < groups;
    if (!live) gid = groups - 1;
    const long b = gid / W, w = gid - b * W, rec = b % a.R;
    const bool act = lane < n, ser = lane < N;
    const int r = act ? lane : n - 1;
    const int kidx = lane - N < 0 ? 0 : (lane - N > K - 1 ? K - 1 : lane - N);
    const double nan = __builtin_nan("");

    const int64_t *win = a.windows + (rec * W + w) * 4;
    const long t0 = clamp_step(win[0], T), t1 = clamp_step(win[1], T), t2 = clamp_step(win[2], T), t3 = clamp_step(win[3], T);
    const bool valid = t1 > t0, second = valid && t3 > t2;
    const long tlo = !valid ? 0 : (second && t2 < t0 ? t2 : t0), thi = !valid ? 0 : (second && t3 > t1 ? t3 : t1);
    const double a1 = valid ? 1.0 / (double)(t1 - t0) : 0.0, a2 = second ? -1.0 / (double)(t3 - t2) : 0.0;
    const double asum = second ? 0.0 : 1.0; // sum of alpha_t: the weight of c'offset

    const double phi_r = act ? a.phi[b * n + r] : 0.0, q_r = a.q[b * n + r];
    phis[lane] = phi_r;
    const double of_r = (ser && a.offset) ? a.offset[rec * N + lane] : 0.0;
    const double *recF = a.F + b * a.bs * a.rs, *recS = a.S + b * a.bs * a.rs; // step t at t*ts*rs
    unsigned flags = 0;

    for (long c0 = 0; c0 < C; c0 += kCH) {
        const int nc = C - c0 < kCH ? (int)(C - c0) : kCH;
        // z = Z'(c o scale): lane r < N its own entry, lane N + k the loadings' column k in ascending series order
        double z[kCH], u[kCH], macc[kCH], vacc[kCH], offc[kCH];
#pragma unroll
        for (int c = 0; c < kCH; ++c) {
            z[c] = u[c] = macc[c] = vacc[c] = offc[c] = 0.0;
            if (c < nc) {
                const double *cv = a.contrasts ? a.contrasts + (rec * C + c0 + c) * N : nullptr;
                double own = 0.0, fac = 0.0;
                for (int j = 0; j < N; ++j) {
                    const double cj = cv ? cv[j] : (j == c0 + c ? 1.0 : 0.0);
                    const double cs = cj * (a.scale ? a.scale[rec * N + j] : 1.0);
                    own = j == lane ? cs : own;
                    fac = fma(a.loadings[(rec * N + j) * K + kidx], cs, fac);
                    offc[c] = j == lane ? cj * of_r : offc[c];
                }
                z[c] = ser ? own : (act ? fac : 0.0);
            }
        }

        for (long t = thi - 1; t >= tlo; --t) {
            const double *Ft = recF + t * a.ts * a.rs, *St = recS + t * a.ts * a.rs;
            const double alpha = (t >= t0 && t < t1 ? a1 : 0.0) + (t >= t2 && t < t3 ? a2 : 0.0);
            const bool lag = t < thi - 1, on = alpha != 0.0;
            double y[kCH];
#pragma unroll
            for (int c = 0; c < kCH; ++c) y[c] = 0.0;
            if (lag) {
                // ---- Pp_{t+1} = Phi Pf_t Phi + Q, element (k, r) by lane r
                wave_lds_sync();
                for (int k0 = 0; k0 < n; k0 += kLoads) { // kLoads independent loads in flight, then their stores
                    double pf[kLoads];
#pragma unroll
                    for (int i = 0; i < kLoads; ++i) pf[i] = Ft[n + (k0 + i < n ? k0 + i : n - 1) * n + r];
#pragma unroll
                    for (int i = 0; i < kLoads; ++i) {
                        const int k = k0 + i;
                        if (act && k < n) A[k * ld + lane] = fma(phis[k] * pf[i], phi_r, k == lane ? q_r : 0.0);
                    }
                }
                wave_lds_sync();
                // ---- L D L' in place, row r by lane r: L below the diagonal, the reciprocal pivot of row r in lane r
                double dme = 0.0;
                for (int j = 0; j < n; ++j) {
                    const double piv = A[j * ld + j];
                    double di = 0.0;
                    if (piv > 0.0) di = 1.0 / piv;
                    else if (piv <= 0.0) { // (a NaN pivot sets neither bit, as in the smoothers: metran_hip.h)
                        flags |= MK_FLAG_RANK_DEFICIENT;
                        if (piv < -1e-8) flags |= MK_FLAG_NOT_SPD;
                    }
                    dme = lane == j ? di : dme;
                    const bool below = act && lane > j;
                    double l = 0.0;
                    if (below) {
                        const double av = A[lane * ld + j];
                        col[lane] = av;
                        l = av * di;
                        A[lane * ld + j] = l;
                    }
                    wave_lds_sync();
                    // the row's entries k = j + 1 .. r, four at a time: the loads of a quartet before its multiply-adds (a trip count that
                    // does not depend on the lane; an entry beyond the row's diagonal is read and not stored)
                    for (int k0 = j + 1; k0 < n; k0 += 4) {
                        double av[4], cv[4];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const int k = k0 + i < n ? k0 + i : n - 1;
                            av[i] = A[r * ld + k];
                            cv[i] = col[k];
                        }
#pragma unroll
                        for (int i = 0; i < 4; ++i)
                            if (below && k0 + i <= lane) A[lane * ld + k0 + i] = fma(-l, cv[i], av[i]);
                    }
                    wave_lds_sync();
                }
                // ---- y = Phi Pp_{t+1}^-1 u_{t+1} for the chunk's contrasts: L y' = u, y'' = D^+ y', L' y''' = y''
#pragma unroll
                for (int c = 0; c < kCH; ++c) y[c] = u[c];
                for (int j = 0; j < n - 1; ++j) {
                    const double lrj = A[r * ld + j];
                    const bool below = act && lane > j;
#pragma unroll
                    for (int c = 0; c < kCH; ++c)
                        if (c < nc) {
                            const double yj = lane_value<G>(y[c], j);
                            y[c] = below ? fma(-lrj, yj, y[c]) : y[c];
                        }
                }
#pragma unroll
                for (int c = 0; c < kCH; ++c) y[c] *= dme;
                for (int k = n - 1; k > 0; --k) {
                    const double lkr = A[k * ld + r];
                    const bool above = lane < k;
#pragma unroll
                    for (int c = 0; c < kCH; ++c)
                        if (c < nc) {
                            const double yk = lane_value<G>(y[c], k);
                            y[c] = above ? fma(-lkr, yk, y[c]) : y[c];
                        }
                }
#pragma unroll
                for (int c = 0; c < kCH; ++c) y[c] *= phi_r;
            }
            // ---- c_t = Pf_t y and Ps_t z, ascending in k: lane r reads the element (k, r) of the records
            double cacc[kCH], pacc[kCH];
#pragma unroll
            for (int c = 0; c < kCH; ++c) cacc[c] = pacc[c] = 0.0;
            if (lag || on) {
                for (int k0 = 0; k0 < n; k0 += kLoads / 2) {
                    double pf[kLoads / 2], ps[kLoads / 2];
#pragma unroll
                    for (int i = 0; i < kLoads / 2; ++i) {
                        const int k = k0 + i < n ? k0 + i : n - 1;
                        pf[i] = lag ? Ft[n + k * n + r] : 0.0;
                        ps[i] = on ? St[n + k * n + r] : 0.0;
                    }
#pragma unroll
                    for (int i = 0; i < kLoads / 2; ++i) {
                        const int k = k0 + i;
                        if (k < n) {
#pragma unroll
                            for (int c = 0; c < kCH; ++c)
                                if (c < nc) {
                                    cacc[c] = fma(pf[i], lane_value<G>(y[c], k), cacc[c]);
                                    pacc[c] = fma(ps[i], lane_value<G>(z[c], k), pacc[c]);
                                }
                        }
                    }
                }
            }
            const double s_r = on ? St[r] : 0.0;
#pragma unroll
            for (int c = 0; c < kCH; ++c) {
                const double wv = alpha * z[c], p = alpha * pacc[c], ct = cacc[c];
                macc[c] = fma(wv, s_r, macc[c]);
                vacc[c] = fma(wv, p + 2.0 * ct, vacc[c]);
                u[c] = act ? p + ct : 0.0;
            }
        }

#pragma unroll
        for (int c = 0; c < kCH; ++c) {
            const double m = group_sum<G>(act ? macc[c] : 0.0) + asum * group_sum<G>(offc[c]);
            const double v = group_sum<G>(act ? vacc[c] : 0.0);
            if (live && lane == 0 && c < nc) {
                const long o = (b * W + w) * C + c0 + c;
                a.mean[o] = valid ? m : nan;
                a.var[o] = valid ? scaled_var(v, 1.0) : nan;
            }
        }
    }
    if (live && lane == 0 && flags && a.status) atomicOr(a.status + b, flags);
}

template <int G, int kCH>
static hipError_t launch_walk(const FunctionalArgs &a, hipStream_t s)
{
    constexpr int GPB = 64 / G;
    const long groups = a.B * a.W, blocks = (groups + GPB - 1) / GPB;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)GPB * functional_lds_doubles(a.N + a.K, G) * sizeof(double);
    hipLaunchKernelGGL((functional_walk_kernel<G, kCH>), dim3((unsigned)blocks), dim3(64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_functional_walk(const FunctionalArgs &a, hipStream_t s)
{
    const int n = a.N + a.K;
    if (a.B < 1 || a.T < 1 || a.R < 1 || a.W < 1 || a.C < 1 || a.C > functional_max_contrasts || a.N < 1 || a.K < 1 ||
        n > functional_max_states)
        return hipErrorInvalidValue;
    if (n <= 16) return launch_walk<16, 8>(a, s);
    return launch_walk<64, 8>(a, s);
}

} // namespace mk
