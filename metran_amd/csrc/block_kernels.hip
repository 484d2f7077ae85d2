// block_kernels.hip -- leave-block-out predictions: E[y_I | every observation except the block I] and its covariance for a run of
// steps [t0, t1) of one series -- how well a gap of that length is filled (de Jong 1989's deletion result for a SET of cells).
// Size-generic (run-time N, K; n = N + K <= 64), stand-alone: no shape-module entry, no ShapeOps row.
//
// Input: the GAIN TAPE and the innovations that innov_step_kernel writes from the filtered records (weights_kernels.h): per cell
// s = (t, j) a slot [ d = P z_j' (n) | 1/f | pad ], all zeros at a cell that is not observed, and v_s.  With k_s = d_s / f_s,
// M = Sigma_y^-1 and u = M (y - mu):   y_I - E[y_I | y_-I] = M_II^-1 u_I,   Cov[y_I | y_-I] = M_II^-1.  u and the entries of M
// come from ONE backward walk, r = 0 and N = 0 (n x n) behind the last step; per step t = T-1 .. 0, per cell with j DESCENDING:
//     g = N k,  u_s = v_s / f_s - k'r,  M_ss = 1 / f_s + k'g
//     for every block cell c already passed:  M_sc = -k'omega_c,  omega_c += z_j' M_sc
//     a block cell starts  omega_s = M_ss z_j' - g
//     r += z_j' u_s,  N += -z_j g' - g z_j' + M_ss z_j' z_j
// and behind the cells of the step, an empty one too, the pull-back through the prediction: r, omega_c <- phi o . and
// N <- (phi phi') o N.  A cell that is not observed has d = 0 and 1/f = 0 and changes nothing, without a branch.
//
// block_checkpoint_kernel  One INSTANCE per lane group, lane = state: 16 lanes for n <= 16 (four instances per wavefront), one
//                          wavefront above.  The (r, N) walk over the whole tape, N a row per lane in the group's LDS (the row
//                          stride odd: the lanes' rows start on different banks), the slots of the next kAhead cells in a ring of
//                          registers (their addresses do not depend on the data).  Behind every step t at which a block of the
//                          record ends the lanes scan its block list and the group stores (r, N) for each block with t1 == t:
//                          everything at the steps >= t1 is taken, the pull-back of step t1 included; zeros for t1 = T.  Blocks in
//                          any order, several per t1; the scan also finds the next such step, so the other steps read no list.
// block_walk_kernel        One wavefront per (instance, block): loads its checkpoint, walks the steps t1-1 .. t0.  lanes = states
//                          for g = N k and the (r, N) update (the same device function as the checkpoint kernel: the same
//                          numbers; the tape slots in the same ring); lanes = block cells (cell c = step t0 + c) for the omega work, omega_c[i] at [i*Lw + lane]: the
//                          dot k'omega_c is a serial loop per lane in ascending i, only the 1 + K nonzero entries of z_j are
//                          updated.  M_II packed, row c in lane c.  Then the solve in LDS, the regression's scheme: M_II scaled to
//                          unit diagonal, right-looking Cholesky in time order, L^-1 by forward substitution (column c in lane c);
//                          e, diag V, 1'V1, quad and the sum of the log pivots each in ascending index order.  A pivot below
//                          regress_min_pivot makes the whole block degenerate: NaN outputs, bit 0 of its flag.
// Whole arithmetic with contraction off and explicit fma; every sum over lanes is group_sum's fixed tree: a block's numbers are
// bit-identical whatever batch, block list or neighbours it runs with.
#include <hip/hip_runtime.h>

#include <cmath>

#pragma clang fp contract(off)

#include "block_kernels.h"
#include "reader_prims.h"
#include "regress_kernels.h" // regress_min_pivot
#include "walk_prims.h"   // the (r, N) walk: WalkLds, cell_products, cell_update, pull_back

namespace mk {

namespace {

// doubles of LDS of block_walk_kernel behind the walk's (walk_prims.h): omega (n rows of Lw), the solve's matrix (L rows of (L + 1) | 1) and four vectors
__host__ __device__ inline long solve_lds_doubles(int n, long L)
{
    return (long)n * even(L) + even(L * ((L + 1) | 1)) + 4 * 64;
}

} // namespace

template <int G, int kAhead>
__global__ void __launch_bounds__(64) block_checkpoint_kernel(BlockArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double bsm[];
    constexpr int GPB = 64 / G;
    const int N = a.N, K = a.K, n = N + K;
    const long T = a.T, W = a.W;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const WalkLds w = carve_walk(bsm + grp * walk_lds_doubles(N, K), N, K);

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
    wave_lds_sync();

    const double *tape = a.gain + b * a.bs * N * a.gs; // cell (t, j) of this instance at (t*ts*N + j)*gs
    const double *vrow = a.v + b * a.bs * N;           // ... and its innovation at t*ts*N + j
    const int64_t *blk = a.blocks + rec * W * 3;
    const long cs = (long)n + (long)n * n;
    double r = 0.0;

    // the last step t1 < below at which a block of the record ends (-1: none): the list is scanned only at those steps
    auto next_end = [&](long below) -> long {
        long best = -1;
        for (long w0 = 0; w0 < W; w0 += G) {
            const long wi = w0 + lane;
            if (wi < W && blk[wi * 3] >= 0) {
                const long e = blk[wi * 3 + 2];
                best = (e < below && e > best) ? e : best;
            }
        }
#pragma unroll
        for (int off = G / 2; off >= 1; off >>= 1) {
            const long o = __shfl_xor(best, off, G);
            best = o > best ? o : best;
        }
        return best;
    };
    long nxt = next_end(T + 1);

    double dq[kAhead], rq[kAhead], vq[kAhead]; // the ring: d_r, 1/f and v of the next kAhead cells, backwards
    long tp = T - 1, t = T - 1;
    int jp = N - 1, j = N - 1;
    // the cell the loading cursor points at, then one cell back; the cursor stays on the first cell of the record
#define MK_B_FETCH(u)                                          \
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
    for (int u = 0; u < kAhead; ++u) MK_B_FETCH(u)
    for (long left = T * N; left > 0; left -= kAhead) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) {
            if (u < left) {
                const double d = dq[u], rf = rq[u], v = rf != 0.0 ? vq[u] : 0.0;
                MK_B_FETCH(u)
                if (j == N - 1 && t + 1 == nxt) {
                    // behind step t + 1, where blocks of the record end: store for each of them, then find the next such step
                    for (long w0 = 0; w0 < W; w0 += G) {
                        const long wi = w0 + lane;
                        const bool hit = wi < W && blk[wi * 3] >= 0 && blk[wi * 3 + 2] == t + 1;
                        unsigned long long m = __ballot(hit);
                        if constexpr (G == 16) m = (m >> (grp * 16)) & 0xffffULL;
                        while (m) {
                            const int bit = __ffsll((long long)m) - 1;
                            m &= m - 1;
                            if (live && act) {
                                double *ck = a.checkpoints + (b * W + w0 + bit) * cs;
                                ck[lane] = r;
                                // N is symmetric bit for bit: column `lane` of row c is this lane's entry c
                                for (int c = 0; c < n; ++c) ck[n + c * n + lane] = w.Nm[lane * w.ns + c];
                            }
                        }
                    }
                    nxt = next_end(nxt);
                }
                const double gsel = w.Gm[j * K + kidx];
                const double z = ser ? (lane == j ? 1.0 : 0.0) : (act ? gsel : 0.0);
                double g, us, mss;
                cell_products<G>(w, lane, act, n, d, rf, v, r, g, us, mss);
                cell_update(w, lane, act, N, K, j, z, g, us, mss, r);
                if (--j < 0) {
                    pull_back(w, lane, act, n, phi_r, r);
                    j = N - 1;
                    --t;
                }
            }
        }
    }
#undef MK_B_FETCH
}

__global__ void __launch_bounds__(64) block_walk_kernel(BlockArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double wsm[];
    const int N = a.N, K = a.K, n = N + K, lane = threadIdx.x;
    const long W = a.W, L = a.L;
    const long bw = blockIdx.x, b = bw / W, wi = bw - b * W, rec = b % a.R;
    const WalkLds w = carve_walk(wsm, N, K);
    const long Lw = even(L);
    const int Ls = (int)((L + 1) | 1);
    double *om = wsm + walk_lds_doubles(N, K), *U = om + (long)n * Lw, *sd = U + even(L * Ls), *ss = sd + 64, *wv = ss + 64, *ov = wv + 64;
    const double nan = __builtin_nan("");

    const int64_t *bl = a.blocks + (rec * W + wi) * 3;
    const long js = bl[0], t0 = bl[1], t1 = bl[2];
    double *omean = a.means + bw * L, *ovar = a.vars + bw * L, *osum = a.summary + bw * 4;
    if (js < 0) { // a slot that is not in use
        if (lane < L) omean[lane] = ovar[lane] = nan;
        if (lane < 4) osum[lane] = nan;
        if (lane == 0) a.flags[bw] = 0u;
        return;
    }
    const int Lb = (int)(t1 - t0); // 1 .. L: checked on the host
    const bool act = lane < n, ser = lane < N, cel = lane < L;
    const int rr = act ? lane : n - 1;
    const int kidx = lane - N < 0 ? 0 : (lane - N > K - 1 ? K - 1 : lane - N);

    for (int i = lane; i < N * K; i += 64) w.Gm[i] = a.loadings[rec * (long)N * K + i];
    const double phi_r = act ? a.phi[b * n + rr] : 0.0;
    w.ph[lane] = phi_r;
    const double *ck = a.checkpoints + bw * ((long)n + (long)n * n);
    double r = act ? ck[rr] : 0.0;
    if (act)
        for (int c = 0; c < n; ++c) w.Nm[lane * w.ns + c] = ck[n + c * n + lane];
    if (cel) {
        for (int i = 0; i < n; ++i) om[i * Lw + lane] = 0.0;
        for (int c = 0; c < Ls; ++c) U[lane * Ls + c] = 0.0;
    }
    wave_lds_sync();

    const double *tape = a.gain + b * a.bs * N * a.gs;
    const double *vrow = a.v + b * a.bs * N;
    // the lane's own block cell: whether it is observed, u_c and M_cc
    bool seen = false;
    double u_own = 0.0, m_own = 1.0;

    // the slots of the next kWalkAhead cells are requested before this one is taken: a ring in registers, as in the checkpoint kernel
    constexpr int kWalkAhead = 8;
    double dq[kWalkAhead], rq[kWalkAhead], vq[kWalkAhead];
    long tp = t1 - 1, t = t1 - 1;
    int jp = N - 1, j = N - 1;
#define MK_W_FETCH(u)                                          \
    {                                                          \
        const double *s_ = tape + (tp * a.ts * N + jp) * a.gs; \
        const double d_ = s_[rr];                              \
        dq[u] = act ? d_ : 0.0;                                \
        rq[u] = s_[n];                                         \
        vq[u] = vrow[tp * a.ts * N + jp];                      \
        if (!(tp == t0 && jp == 0)) {                          \
            if (--jp < 0) {                                    \
                jp = N - 1;                                    \
                --tp;                                          \
            }                                                  \
        }                                                      \
    }
#pragma unroll
    for (int u = 0; u < kWalkAhead; ++u) MK_W_FETCH(u)
    for (long left = (long)Lb * N; left > 0; left -= kWalkAhead) {
#pragma unroll
        for (int u = 0; u < kWalkAhead; ++u) {
            if (u < left) {
                const double d = dq[u], rf = rq[u], v = rf != 0.0 ? vq[u] : 0.0;
                MK_W_FETCH(u)
                const int cc = (int)(t - t0);
                const double gsel = w.Gm[j * K + kidx];
                const double z = ser ? (lane == j ? 1.0 : 0.0) : (act ? gsel : 0.0);
                double g, us, mss;
                cell_products<64>(w, lane, act, n, d, rf, v, r, g, us, mss);
                // lanes = block cells: M_sc = -k'omega_c, omega_c += z_j' M_sc (a cell not yet passed has omega = 0: nothing happens)
                if (cel) {
                    double dot = 0.0;
#pragma unroll 4
                    for (int i = 0; i < n; ++i) dot = fma(w.kv[i], om[i * Lw + lane], dot);
                    const double msc = -dot;
                    om[j * Lw + lane] = om[j * Lw + lane] + msc;
                    for (int l = 0; l < K; ++l) om[(N + l) * Lw + lane] = fma(w.Gm[j * K + l], msc, om[(N + l) * Lw + lane]);
                    if (j == js && lane > cc) U[lane * Ls + cc] = msc; // row of the later cell, column of this one
                }
                wave_lds_sync();
                if (j == js) { // the block's cell of this step starts its own omega
                    if (act) om[lane * Lw + cc] = fma(mss, z, -g);
                    if (lane == cc) {
                        seen = rf != 0.0;
                        u_own = us;
                        m_own = seen ? mss : 1.0;
                    }
                }
                cell_update(w, lane, act, N, K, j, z, g, us, mss, r);
                if (--j < 0) {
                    pull_back(w, lane, act, n, phi_r, r);
                    if (cel) {
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
#undef MK_W_FETCH

    // ---- the solve: M_II to unit diagonal (a cell that is not observed is a unit row), lane c = block cell c
    const bool mine = lane < Lb;
    const long m = __popcll(__ballot(mine && seen));
    const bool pos = m_own > 0.0;
    const double sd_own = pos ? sqrt(m_own) : 1.0;
    bool degenerate = __ballot(mine && !pos) != 0ULL;
    sd[lane] = sd_own;
    ss[lane] = (mine && seen) ? u_own / sd_own : 0.0;
    wave_lds_sync();
    if (mine) {
        for (int jj = 0; jj < lane; ++jj) U[lane * Ls + jj] = U[lane * Ls + jj] / (sd_own * sd[jj]);
        U[lane * Ls + lane] = 1.0;
    }
    wave_lds_sync();
    // right-looking Cholesky in time order, row i in lane i
    double logpiv = 0.0; // sum of log L_kk, every lane the same
    for (int k = 0; k < Lb; ++k) {
        const double piv = U[k * Ls + k];
        const bool ok = piv >= regress_min_pivot;
        degenerate = degenerate || !ok;
        const double lk = ok ? sqrt(piv) : 1.0;
        logpiv += log(lk);
        double lik = 0.0;
        if (mine && lane > k) {
            lik = U[lane * Ls + k] / lk;
            U[lane * Ls + k] = lik;
        }
        if (lane == k) U[k * Ls + k] = lk;
        wave_lds_sync();
        if (mine && lane > k)
            for (int jj = k + 1; jj <= lane; ++jj) U[lane * Ls + jj] = fma(-lik, U[jj * Ls + k], U[lane * Ls + jj]);
        wave_lds_sync();
    }
    // L^-1 by forward substitution, column c in lane c: (L^-1)[i, c], i >= c, parked at U[c, i + 1]
    if (mine) {
        for (int i = lane; i < Lb; ++i) {
            double val;
            if (i == lane) {
                val = 1.0 / U[i * Ls + i];
            } else {
                double sum = 0.0;
                for (int k = lane; k < i; ++k) sum = fma(U[i * Ls + k], U[lane * Ls + k + 1], sum);
                val = -sum / U[i * Ls + i];
            }
            U[lane * Ls + i + 1] = val;
        }
    }
    wave_lds_sync();
    // w = L^-1 (u / sd): lane k its entry, the sum over j <= k ascending
    if (mine) {
        double ws = 0.0;
        for (int jj = 0; jj <= lane; ++jj) ws = fma(U[jj * Ls + lane + 1], ss[jj], ws);
        wv[lane] = ws;
    }
    wave_lds_sync();
    // o = L^-1 (1 / sd over the observed cells), for 1'V1 = o'o (ss is free after w)
    ss[lane] = (mine && seen) ? 1.0 / sd_own : 0.0;
    wave_lds_sync();
    if (mine) {
        double os = 0.0;
        for (int jj = 0; jj <= lane; ++jj) os = fma(U[jj * Ls + lane + 1], ss[jj], os);
        ov[lane] = os;
    }
    wave_lds_sync();

    const double sc = a.scale ? a.scale[rec * N + js] : 1.0, of = a.offset ? a.offset[rec * N + js] : 0.0;
    const double rv = a.obsvar ? a.obsvar[rec * N + js] : 0.0;
    if (cel) {
        double mean = nan, var = nan;
        if (mine && seen && !degenerate) {
            // e = L^-T w / sd and V_cc = sum_k (L^-1)[k, c]^2 / sd^2, the sums over k >= c ascending
            double es = 0.0, vs = 0.0;
            for (int k = lane; k < Lb; ++k) {
                const double li = U[lane * Ls + k + 1];
                es = fma(li, wv[k], es);
                vs = fma(li, li, vs);
            }
            const double y = a.obs[(rec * a.obs_bs + (t0 + lane) * a.obs_ts) * N + js];
            mean = scaled_mean(y - es / sd_own, sc, of);
            var = scaled_var(vs / (sd_own * sd_own) - rv, sc);
        }
        omean[lane] = mean;
        ovar[lane] = var;
    }
    if (lane == 0) {
        double quad = 0.0, one = 0.0, lsd = 0.0;
        for (int k = 0; k < Lb; ++k) {
            quad = fma(wv[k], wv[k], quad);
            one = fma(ov[k], ov[k], one);
            lsd += log(sd[k]);
        }
        const bool good = m > 0 && !degenerate;
        osum[0] = (double)m;
        osum[1] = good ? quad : nan;
        osum[2] = good ? -2.0 * (lsd + logpiv) : nan;
        osum[3] = good ? one / ((double)m * (double)m) * sc * sc : nan;
        a.flags[bw] = (m > 0 && degenerate) ? 1u : 0u;
    }
}

template <int G>
static hipError_t launch_checkpoint(const BlockArgs &a, hipStream_t s)
{
    constexpr int GPB = 64 / G;
    const long blocks = (a.B + GPB - 1) / GPB;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)GPB * walk_lds_doubles(a.N, a.K) * sizeof(double);
    hipLaunchKernelGGL((block_checkpoint_kernel<G, 8>), dim3((unsigned)blocks), dim3(64), lds, s, a);
    return hipGetLastError();
}

static bool block_args_ok(const BlockArgs &a)
{
    return a.B >= 1 && a.T >= 1 && a.R >= 1 && a.W >= 1 && a.L >= 1 && a.L <= block_max_cells && a.N >= 1 && a.K >= 1 &&
           a.N + a.K <= block_max_states;
}

hipError_t launch_block_checkpoint(const BlockArgs &a, hipStream_t s)
{
    if (!block_args_ok(a)) return hipErrorInvalidValue;
    if (a.N + a.K <= 16) return launch_checkpoint<16>(a, s);
    return launch_checkpoint<64>(a, s);
}

hipError_t launch_block_walk(const BlockArgs &a, hipStream_t s)
{
    if (!block_args_ok(a)) return hipErrorInvalidValue;
    const long blocks = a.B * a.W;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)(walk_lds_doubles(a.N, a.K) + solve_lds_doubles(a.N + a.K, a.L)) * sizeof(double);
    if (lds > 64 * 1024) { // beyond the default grant of dynamic LDS (n = 64 with L = 64: 104 KiB of the CU's 160)
        const hipError_t e = hipFuncSetAttribute((const void *)block_walk_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(block_walk_kernel, dim3((unsigned)blocks), dim3(64), lds, s, a);
    return hipGetLastError();
}

} // namespace mk
