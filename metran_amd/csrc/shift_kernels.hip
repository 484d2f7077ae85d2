// shift_kernels.hip -- the level-shift scan: for every observed cell (tau, j) the GLS statistic of a permanent offset of series j
// from step tau on (de Jong & Penzer 1998, "Diagnosing shocks in time series"), all of them from ONE backward walk.
// Size-generic (run-time N, K; n = N + K <= 64), stand-alone: no shape-module entry, no ShapeOps row.
//
// Input: the GAIN TAPE and the innovations that innov_step_kernel writes (block_kernels.hip's header has the notation:
// M = Sigma_y^-1, u = M (y - mu), k_s = d_s / f_s).  The regressor of (series j, date tau) is x = 1 on the observed cells (t, j)
// with t >= tau; its GLS estimate is A / D with standard error 1 / sqrt(D) and t = A / sqrt(D), A = x'u and D = x'Mx.  Per series j
// the walk carries Omega_j (n), the sum of the block kernels' omega_c over the cells of series j already passed, and the scalars
// A_j, D_j; all zero behind the last step.  At a cell s = (t, j'), behind g, u_s and M_ss of the (r, N) walk:
//     m_j = -k'Omega_j,  Omega_j += z_j'' m_j                  for every series j
//     D_j' += M_ss + 2 m_j',  A_j' += u_s,  Omega_j' += M_ss z_j'' - g
// then the (r, N) update; behind the cells of a step, an empty one too, Omega_j <- phi o Omega_j beside the walk's pull-back.
// Behind the cells of step tau, (A_j, D_j) is the pair of the shift of series j that starts at tau.  A cell that is not observed
// has d = 0 and 1/f = 0 and changes nothing, without a branch.
//
// shift_scan_kernel   The launch geometry of block_checkpoint_kernel: one INSTANCE per lane group, 16 lanes for n <= 16 (four
//                     instances per wavefront), one wavefront above; groups past the last instance replicate it without
//                     storing.  lanes = states for the (r, N) walk (walk_prims.h: the block kernels' device functions, the same
//                     numbers); lanes = series for the Omega work, Omega_j[i] at [i*Lw + lane]: the dot k'Omega_j is a serial loop
//                     per lane in ascending i, only the 1 + K nonzero entries of z_j' are updated; A_j and D_j in the lane's
//                     registers.  Behind a step's cells lane j stores num[b,t,j] = A_j and den[b,t,j] = D_j where cell (t, j) is
//                     observed and NaN where it is not: one row of N doubles per output and step.
// Whole arithmetic with contraction off and explicit fma; every sum over lanes is group_sum's fixed tree: an instance's numbers are
// bit-identical whatever the batch, the neighbours in its wavefront or the layout.
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

#include "shift_kernels.h"
#include "walk_prims.h"

namespace mk {

namespace {

// doubles of LDS of one lane group: the walk's and Omega (n rows of Lw = even(N))
__host__ __device__ inline long shift_lds_doubles(int N, int K) { return walk_lds_doubles(N, K) + (long)(N + K) * even(N); }

} // namespace

template <int G, int kAhead>
__global__ void __launch_bounds__(64) shift_scan_kernel(ShiftArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double ssm[];
    constexpr int GPB = 64 / G;
    const int N = a.N, K = a.K, n = N + K;
    const long T = a.T;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    double *base = ssm + grp * shift_lds_doubles(N, K);
    const WalkLds w = carve_walk(base, N, K);
    double *om = base + walk_lds_doubles(N, K);
    const long Lw = even(N);
    const double nan = __builtin_nan("");

    // groups past the last instance replicate it (same loads, no stores): the wavefront stays whole
    long b = (long)blockIdx.x * GPB + grp;
    const bool live = b < a.B;
    if (!live) b = a.B - 1;
    const long rec = b % a.R;
    const bool act = lane < n, ser = lane < N;
    const int rr = act ? lane : n - 1;
    const int kidx = lane - N < 0 ? 0 : (lane - N > K - 1 ? K - 1 : lane - N);

    for (int i = lane; i < N * K; i += G) w.Gm[i] = a.loadings[rec * (long)N * K + i];
    const double phi_r = act ? a.phi[b * n + rr] : 0.0;
    w.ph[lane] = phi_r;
    if (act)
        for (int c = 0; c < n; ++c) w.Nm[lane * w.ns + c] = 0.0;
    if (ser)
        for (int i = 0; i < n; ++i) om[i * Lw + lane] = 0.0;
    wave_lds_sync();

    const double *tape = a.gain + b * a.bs * N * a.gs; // cell (t, j) of this instance at (t*ts*N + j)*gs
    const double *vrow = a.v + b * a.bs * N;           // ... and its innovation at t*ts*N + j
    double *onum = a.num + b * a.bs * N, *oden = a.den + b * a.bs * N;
    double r = 0.0, A = 0.0, D = 0.0;
    bool seen = false; // lane j: cell (t, j) of the step under way is observed

    double dq[kAhead], rq[kAhead], vq[kAhead]; // the ring: d_r, 1/f and v of the next kAhead cells, backwards
    long tp = T - 1, t = T - 1;
    int jp = N - 1, j = N - 1;
    // the cell the loading cursor points at, then one cell back; the cursor stays on the first cell of the record
#define MK_S_FETCH(u)                                          \
    {                                                          \
        const double *s_ = tape + (tp * a.ts * N + jp) * a.gs; \
        const double d_ = s_[rr];                              \
        dq[u] = act ? d_ : 0.0;                                \
        rq[u] = s_[n];                                         \
        vq[u] = vrow[tp * a.ts * N + jp];                      \
        if (!(tp == 0 && jp == 0)) {                           \
            if (--jp < 0) {                                    \
                jp = N - 1;                                    \
                --tp;                                          \
            }                                                  \
        }                                                      \
    }
#pragma unroll
    for (int u = 0; u < kAhead; ++u) MK_S_FETCH(u)
    for (long left = T * N; left > 0; left -= kAhead) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            if (u < left) {
                const double d = dq[u], rf = rq[u], v = rf != 0.0 ? vq[u] : 0.0;
                MK_S_FETCH(u)
                const double gsel = w.Gm[j * K + kidx];
                const double z = ser ? (lane == j ? 1.0 : 0.0) : (act ? gsel : 0.0);
                double g, us, mss;
                cell_products<G>(w, lane, act, n, d, rf, v, r, g, us, mss);
                // lanes = series: m_j = -k'Omega_j, Omega_j += z_j'' m_j; the cell's own series takes M_ss + 2 m and u_s
                if (ser) {
                    double dot = 0.0;
#pragma unroll 4
                    for (int i = 0; i < n; ++i) dot = fma(w.kv[i], om[i * Lw + lane], dot);
                    const double m = -dot;
                    om[j * Lw + lane] = om[j * Lw + lane] + m;
                    for (int l = 0; l < K; ++l) om[(N + l) * Lw + lane] = fma(w.Gm[j * K + l], m, om[(N + l) * Lw + lane]);
                    if (lane == j) {
                        D = D + (mss + 2.0 * m);
                        A = A + us;
                        seen = rf != 0.0;
                    }
                }
                wave_lds_sync();
                // lanes = states: Omega_j' += M_ss z_j'' - g
                if (act) om[lane * Lw + j] = om[lane * Lw + j] + fma(mss, z, -g);
                cell_update(w, lane, act, N, K, j, z, g, us, mss, r);
                if (--j < 0) {
                    // behind the cells of step t: the pair of the shift that starts here, then the pull-back
                    if (live && ser) {
                        onum[t * a.ts * N + lane] = seen ? A : nan;
                        oden[t * a.ts * N + lane] = seen ? D : nan;
                    }
                    seen = false;
                    pull_back(w, lane, act, n, phi_r, r);
                    if (ser) {
#pragma unroll 4
                        for (int i = 0; i < n; ++i) om[i * Lw + lane] = w.ph[i] * om[i * Lw + lane];
                    }
                    wave_lds_sync();
                    j = N - 1;
                    --t;
                }
            }
        }
    }
#undef MK_S_FETCH
}

template <int G>
static hipError_t launch_scan(const ShiftArgs &a, hipStream_t s)
{
    constexpr int GPB = 64 / G;
    const long blocks = (a.B + GPB - 1) / GPB;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)GPB * shift_lds_doubles(a.N, a.K) * sizeof(double);
    if (lds > 64 * 1024) { // beyond the default grant of dynamic LDS (n = 64 with N = 60: 66 KiB of the CU's 160)
        const hipError_t e = hipFuncSetAttribute((const void *)shift_scan_kernel<G, 8>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((shift_scan_kernel<G, 8>), dim3((unsigned)blocks), dim3(64), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_shift_scan(const ShiftArgs &a, hipStream_t s)
{
    if (!(a.B >= 1 && a.T >= 1 && a.R >= 1 && a.N >= 1 && a.K >= 1 && a.N + a.K <= shift_max_states)) return hipErrorInvalidValue;
    if (a.N + a.K <= 16) return launch_scan<16>(a, s);
    return launch_scan<64>(a, s);
}

} // namespace mk
