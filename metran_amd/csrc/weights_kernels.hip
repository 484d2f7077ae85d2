// weights_kernels.hip -- observation weights of smoothed series and states (Koopman & Harvey 2003; statsmodels'
// compute_smoothed_state_weights): for fixed parameters the smoother is linear in the data, so a projected smoothed mean
// c' x_{t*|T} is  sum w_{t,j} y_{t,j} + intercept  over the observed cells of the record.  Size-generic (run-time N, K; n = N + K <= 64),
// stand-alone: no shape-module entry, no ShapeOps row.
//
// Input: the filtered records of the recording forward pass and the GAIN TAPE that innov_step_kernel writes from them in parallel
// over time (InnovArgs.gain): per cell (t, j) one slot [ d = P z_j' (n) | 1/f | pad ], P the covariance just before that scalar update;
// all zeros at a cell that is not observed, which then drops out of both walks arithmetically -- no branch on the missing-data
// pattern.
//
// weights_walk_kernel  One TARGET (instance, step t*, column) per lane group, lane = state: 16 lanes for n <= 16 (four targets per
//                      wavefront), one wavefront above.  Two vector walks over time, no covariance and no matrix product:
//                        forward from t*   p = P_{t*|t*-1} c;  per step (t > t*: p <- phi o p), per cell j ascending
//                                          g_{t,j} = (z_j p) / f_{t,j},  p <- p - d_{t,j} g_{t,j}
//                        backward, all t   h = 0;  per step, per cell j descending  w_{t,j} = g_{t,j} + (h d_{t,j}) / f_{t,j},
//                                          h <- h - w_{t,j} z_j';  after the cells of step t* h <- h + c;  then h <- phi o h
//                        intercept = h x0.
//                      p and h are one register per lane; phi, x0, c and the lane's entry of z_j (from the loadings in the group's
//                      LDS) are per-lane values.  z_j p and h d are sums over the group: a fixed tree (group_sum of reader_prims.h: DPP
//                      row reductions inside 16 lanes, two xor exchanges across the rows of a wavefront), so a target's weights
//                      are bit-identical whatever batch, grid or neighbouring targets it runs with.  A cell's slot is one
//                      coalesced load (lane r its d_r) whose address does not depend on the data: the walks keep a ring of kAhead
//                      cells in registers and load cell i + kAhead when cell i is taken, so the dependent chain of a cell is one
//                      product, one tree and one multiply-add.  g of a step is collected in lane j and parked, one row per step,
//                      in the target's own output row [T,N]; the backward walk reads it back (the same lane the same address, one
//                      step ahead) and overwrites it with w -- NaN where the observation is not finite.  The four groups of a
//                      wavefront start the forward walk together at the smallest t* among them; a group is inert (selects, not
//                      arithmetic) before its own.
//                      A target with its step outside [0, T) or its column outside [0, N) (series) / [0, n) (state) gets an
//                      all-NaN row and a NaN intercept, and addresses nothing: its loads are clamped to step 0 / column 0.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mk_prims.h" // wave_lds_sync
#include "reader_prims.h"
#include "weights_kernels.h"

namespace mk {

namespace {

inline long weights_lds_doubles(int N, int K) { return ((long)N * K + 1) & ~1L; }

// the smallest value of a wavefront's lanes, in a scalar register
__device__ __forceinline__ long wave_min(long x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const long o = __shfl_xor(x, off, 64);
        x = o < x ? o : x;
    }
    const int lo = __builtin_amdgcn_readfirstlane((int)(x & 0xffffffffL));
    const int hi = __builtin_amdgcn_readfirstlane((int)(x >> 32));
    return ((long)hi << 32) | (unsigned int)lo;
}

} // namespace

template <int G, int kAhead>
__global__ void __launch_bounds__(64) weights_walk_kernel(WeightsArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    constexpr int GPB = 64 / G;
    const int N = a.N, K = a.K, n = N + K;
    const long T = a.T;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    double *Gm = wsm + grp * (((long)N * K + 1) & ~1L);

    // groups past the last target replicate it (same loads, no stores): the wavefront stays whole
    const long groups = a.B * a.M;
    long gid = (long)blockIdx.x * GPB + grp;
    const bool live = gid < groups;
    if (!live) gid = groups - 1;
    const long b = gid / a.M, m = gid - b * a.M, rec = b % a.R;
    const bool act = lane < n, ser = lane < N;
    const int r = act ? lane : n - 1;
    const int kidx = lane - N < 0 ? 0 : (lane - N > K - 1 ? K - 1 : lane - N);
    const double nan = __builtin_nan("");

    const long tstep = a.targets[(rec * a.M + m) * 2], tcol = a.targets[(rec * a.M + m) * 2 + 1];
    const bool valid = tstep >= 0 && tstep < T && tcol >= 0 && tcol < (a.states ? n : N);
    const long ts = valid ? tstep : T; // the forward walk of a target that is not valid never starts
    const long tsc = valid ? tstep : 0; // ... and what it loads is clamped into the arrays
    const int col = valid ? (int)tcol : 0;

    for (int i = lane; i < N * K; i += G) Gm[i] = a.loadings[rec * (long)N * K + i];
    wave_lds_sync();

    const double phi_r = act ? a.phi[b * n + r] : 0.0, q_r = a.q[b * n + r];
    const double x0_r = (act && a.x0) ? a.x0[b * n + r] : 0.0;
    // lane r's entry of z_j = [e_j | loadings[j, :]]
    auto zentry = [&](int j) -> double {
        const double g = Gm[j * K + kidx];
        return ser ? (lane == j ? 1.0 : 0.0) : (act ? g : 0.0);
    };
    const double c_r = a.states ? ((act && lane == col) ? 1.0 : 0.0) : zentry(col);

    // ---- p = P_{t*|t*-1} c, the predicted covariance of step t* from the filtered record of step t* - 1 (position (c, r) is lane r's
    // element c, mk_prims.h) or from the initial covariance: over the non-zero entries of c in ascending order
    double p = 0.0;
    {
        const double *recp = tsc > 0 ? a.F + (b * a.bs + (tsc - 1) * a.ts) * a.rs + n : nullptr;
        const int ncols = a.states ? 1 : 1 + K;
        for (int i = 0; i < ncols; ++i) {
            const int cc = i == 0 ? col : N + (i - 1);
            const double cv = i == 0 ? 1.0 : Gm[col * K + (i - 1)];
            const double pf = recp ? recp[(long)cc * n + r] : (a.P0 ? a.P0[(b * n + r) * n + cc] : (cc == r ? 1.0 : 0.0));
            const double pp = fma(pf, phi_r * a.phi[b * n + cc], cc == r ? q_r : 0.0);
            p = fma(pp, cv, p);
        }
        p = (act && valid) ? p : 0.0;
    }

    const double *tape = a.gain + b * a.bs * N * a.gs;         // cell (t, j) of this instance at (t*ts*N + j)*gs
    const double *yrow = a.obs + rec * a.obs_bs * N + (ser ? lane : N - 1); // row t at t*obs_ts*N
    double *orow = a.weights + (b * a.M + m) * T * N + (ser ? lane : N - 1); // row t at t*N
    const bool put = live && ser;

    double dq[kAhead], rq[kAhead], zq[kAhead]; // the ring: d_r, 1/f and the lane's entry of z_j of the next kAhead cells

    // ---- forward walk from the smallest t* of the wavefront's groups
    const long tstart = wave_min(ts);
    if (tstart < T) {
        long tp = tstart, t = tstart;
        int jp = 0, j = 0;
        // the cell the loading cursor points at, then one cell on; the cursor stays on the last cell of the record
#define MK_W_FETCH_UP(u)                                                     \
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
        for (int u = 0; u < kAhead; ++u) MK_W_FETCH_UP(u)
        double gown = 0.0;
        for (long left = (T - tstart) * N; left > 0; left -= kAhead) {
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (u < left) {
                    const double d = dq[u], rf = rq[u], z = zq[u];
                    MK_W_FETCH_UP(u)
                    const bool on = t >= ts;
                    if (j == 0) {
                        p = t > ts ? phi_r * p : p;
                        gown = 0.0;
                    }
                    const double g = group_sum<G>(z * p) * rf;
                    p = on ? fma(-d, g, p) : p;
                    gown = lane == j ? g : gown;
                    if (++j == N) {
                        if (put && on) orow[t * N] = gown;
                        j = 0;
                        ++t;
                    }
                }
            }
        }
#undef MK_W_FETCH_UP
    }

    // ---- backward walk over the whole record
    double h = 0.0;
    {
        long tp = T - 1, t = T - 1;
        int jp = N - 1, j = N - 1;
#define MK_W_FETCH_DOWN(u)                                                   \
    {                                                                        \
        const double *s_ = tape + (tp * a.ts * N + jp) * a.gs;               \
        const double d_ = s_[r];                                             \
        dq[u] = act ? d_ : 0.0;                                              \
        rq[u] = s_[n];                                                       \
        zq[u] = zentry(jp);                                                  \
        if (!(tp == 0 && jp == 0)) {                                         \
            if (--jp < 0) {                                                  \
                jp = N - 1;                                                  \
                --tp;                                                        \
            }                                                                \
        }                                                                    \
    }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) MK_W_FETCH_DOWN(u)
        // g and y of a step are loaded one step ahead: the row of step t - 1 when step t begins
        double gnext = (ser && T - 1 >= ts) ? orow[(T - 1) * N] : 0.0, ynext = yrow[(T - 1) * a.obs_ts * N];
        double gown = 0.0, yown = nan, wown = 0.0;
        for (long left = T * N; left > 0; left -= kAhead) {
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                if (u < left) {
                    const double d = dq[u], rf = rq[u], z = zq[u];
                    MK_W_FETCH_DOWN(u)
                    if (j == N - 1) {
                        gown = gnext;
                        yown = ynext;
                        const long tn = t > 0 ? t - 1 : 0;
                        gnext = (ser && tn >= ts) ? orow[tn * N] : 0.0;
                        ynext = yrow[tn * a.obs_ts * N];
                    }
                    const double w = __shfl(gown, j, G) + group_sum<G>(h * d) * rf;
                    h = fma(-w, z, h);
                    wown = lane == j ? w : wown;
                    if (--j < 0) {
                        if (put) orow[t * N] = (valid && isfinite(yown)) ? wown : nan;
                        h = t == ts ? h + c_r : h;
                        h = phi_r * h;
                        j = N - 1;
                        --t;
                    }
                }
            }
        }
#undef MK_W_FETCH_DOWN
    }
    const double ic = group_sum<G>(h * x0_r);
    if (live && lane == 0 && a.intercept) a.intercept[b * a.M + m] = valid ? ic : nan;
}

template <int G, int kAhead>
static hipError_t launch_walk(const WeightsArgs &a, hipStream_t s)
{
    constexpr int GPB = 64 / G;
    const long groups = a.B * a.M, blocks = (groups + GPB - 1) / GPB;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)GPB * weights_lds_doubles(a.N, a.K) * sizeof(double);
    hipLaunchKernelGGL((weights_walk_kernel<G, kAhead>), dim3((unsigned)blocks), dim3(64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_weights_walk(const WeightsArgs &a, hipStream_t s)
{
    const int n = a.N + a.K;
    if (a.B < 1 || a.T < 1 || a.R < 1 || a.M < 1 || a.N < 1 || a.K < 1 || n > weights_max_states) return hipErrorInvalidValue;
    if (n <= 16) return launch_walk<16, 8>(a, s);
    return launch_walk<64, 16>(a, s);
}

} // namespace mk
