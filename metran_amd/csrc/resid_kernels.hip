// resid_kernels.hip -- residual diagnostics of the standardised innovations e = v / sqrt(f) that mk_innovations writes: the moments,
// variance thirds and CUSUM excursions of every series, and the lagged sums of products between the series of an instance.
// Stand-alone reductions over v / f (run-time N): no filter, smoother or reader kernel is involved.
// A cell (t, j) is VALID when v is finite, f is finite and > 0 and t >= t_first -- innov_stats_kernel's rule.
//
// resid_series_kernel  One wavefront per (instance, series): time in tiles of kResidTile steps, a lane per step, four series per
//                      workgroup; wavefronts past the last series replicate it without storing.  THREE passes over the series;
//                      the e of its first kResidKeep tiles (1024 steps) stay in registers after the first, the later passes
//                      RE-READ v / f beyond them (16 bytes a step) instead of keeping them in LDS, so T is unbounded:
//                      (1) m and the mean; (2) the centred power sums S2, S3, S4, the sums of e^2 over the first and the last
//                      h = (m + 1) / 3 valid cells, and max_k |C_k|; (3) max_k |Q_k - (k / m) S2|, which needs the finished S2.
//                      The position k of a cell among the valid ones is the ballot prefix plus the count of the tiles before;
//                      C_k and Q_k are a wave prefix scan (Hillis-Steele, lane l adds lane l - off for off = 1, 2, .. 32) plus
//                      the carry of the tiles before.  ORDER OF EVERY SUM: lane l adds the cells of steps l, 64 + l, 128 + l, ..
//                      into its own accumulator in ascending time, and the 64 accumulators are summed once by a fixed
//                      xor-butterfly tree -- the order of innov_stats_kernel's lagged products; the running sums C_k and Q_k
//                      are the scan of the tile plus the carry, tile after tile.  Nothing depends on the batch size, the
//                      instance's place in the batch or the layout.  Each running maximum keeps its FIRST step on a tie: a
//                      lane replaces its own maximum only by a larger one, and the final reduction compares (value, -t).
// resid_cross_kernel   One workgroup per (instance, block of lags).  A tile of kResidTile steps x N series of the normalised
//                      e~ = (e - mean) / sqrt(S2 / m) (from the statistics rows of resid_series_kernel; 0 at an invalid cell) is
//                      staged in LDS behind a halo of the resid_max_lags steps before it, with one 64-bit validity mask per
//                      series for the tile and one for the tile before.  Each thread owns up to 16 (lag, i, j) triples of its
//                      block of lags -- consecutive lanes hold consecutive j, so a wavefront's reads of e~[t,i] are broadcasts
//                      and those of e~[t-l,j] consecutive doubles: conflict-free -- and walks the tile's steps in ASCENDING
//                      order into ONE accumulator per triple (registers); the steps of all tiles therefore add up in ascending
//                      time.  n_ij(l) is the popcount of mask_i & (mask_j << l | mask_j of the tile before >> (64 - l)).
//                      The number of lags per block depends on N alone (so that a block has at most 4096 triples); the tiles
//                      are read once per block of lags.  LDS: 100 N doubles (51.2 KB at N = 64); 228 VGPRs: two workgroups per CU.
#include <hip/hip_runtime.h>

#include <cmath>

#include "resid_kernels.h"

namespace mk {

namespace {

constexpr int kResidTile = 64; // time steps per tile: one lane per step (series kernel), one mask bit per step (cross kernel)
constexpr int kResidKeep = 16; // tiles of a series whose e stay in registers between the passes of resid_series_kernel

// bit-identical in every lane: at each stage lanes i and i ^ off add the same two numbers
__device__ __forceinline__ double wave_sum(double x)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// inclusive prefix sum over the lanes, a fixed order per lane
__device__ __forceinline__ double wave_scan(double x, int lane)
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const double y = __shfl_up(x, off, 64);
        if (lane >= off) x += y;
    }
    return x;
}

// the largest value of the wavefront and, among equals, the smallest step: the same pair in every lane
__device__ __forceinline__ void wave_first_max(double &val, long &t)
{
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const double ov = __shfl_xor(val, off, 64);
        const long ot = __shfl_xor((long long)t, off, 64);
        const bool take = ov > val || (ov == val && ot < t);
        val = take ? ov : val;
        t = take ? ot : t;
    }
}

} // namespace

__global__ void __launch_bounds__(256) resid_series_kernel(ResidSeriesArgs a)
{
    static_assert(kResidTile == 64, "one lane of the wavefront per step of a tile");
    const int lane = threadIdx.x % 64, w = threadIdx.x / 64;
    const int N = a.N;
    const long series = a.B * N;
    long s = (long)blockIdx.x * 4 + w;
    const bool live = s < series;
    if (!live) s = series - 1;
    const long b = s / N;
    const int j = (int)(s - b * N);

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
    const unsigned long long below = (1ull << lane) - 1ull;

    // This lane's cells of the first kResidKeep tiles stay in registers after the first pass (e, and one validity bit each):
    // the later passes re-read v / f, and divide and take the root again, only for the tiles beyond.  The same values in the
    // same order either way.
    double keep[kResidKeep];
    unsigned kept = 0;

    // ---- first pass: the number of valid cells and their mean
    double sum = 0.0;
    long m = 0;
    auto pass1 = [&](bool ok, double e) {
        m += __popcll(__ballot(ok));
        sum += e;
    };
#pragma unroll
    for (int c = 0; c < kResidKeep; ++c) {
        keep[c] = 0.0;
        if ((long)c * kResidTile < a.T) {
            const bool ok = cell((long)c * kResidTile + lane, keep[c]);
            kept |= ok ? 1u << c : 0u;
            pass1(ok, keep[c]);
        }
    }
    for (long t0 = (long)kResidKeep * kResidTile; t0 < a.T; t0 += kResidTile) {
        double e;
        const bool ok = cell(t0 + lane, e);
        pass1(ok, e);
    }
    const double dm = (double)m, mean = wave_sum(sum) / dm; // m = 0: NaN, and no cell uses it
    const long h = (m + 1) / 3;

    // ---- second pass: centred power sums, the two thirds of the compacted sequence, the excursion of C_k = sum_{i<=k} d_i
    double S2 = 0.0, S3 = 0.0, S4 = 0.0, ssf = 0.0, ssl = 0.0, carry = 0.0, best = -1.0;
    long best_t = -1, base = 0; // base: valid cells before this tile
    auto pass2 = [&](long t0, bool ok, double e) {
        const unsigned long long ball = __ballot(ok);
        const long k = base + __popcll(ball & below) + 1; // 1-based position among the valid cells
        const double d = ok ? e - mean : 0.0, d2 = d * d, e2 = e * e;
        S2 += d2;
        S3 += d2 * d;
        S4 += d2 * d2;
        ssf += ok && k <= h ? e2 : 0.0;
        ssl += ok && k > m - h ? e2 : 0.0;
        const double c = carry + wave_scan(d, lane);
        carry = __shfl(c, 63, 64);
        if (ok && fabs(c) > best) { // this lane's own steps, ascending: the first of equals stays
            best = fabs(c);
            best_t = t0 + lane;
        }
        base += __popcll(ball);
    };
#pragma unroll
    for (int c = 0; c < kResidKeep; ++c)
        if ((long)c * kResidTile < a.T) pass2((long)c * kResidTile, (kept >> c) & 1u, keep[c]);
    for (long t0 = (long)kResidKeep * kResidTile; t0 < a.T; t0 += kResidTile) {
        double e;
        const bool ok = cell(t0 + lane, e);
        pass2(t0, ok, e);
    }
    S2 = wave_sum(S2);
    S3 = wave_sum(S3);
    S4 = wave_sum(S4);
    ssf = wave_sum(ssf);
    ssl = wave_sum(ssl);
    if (best < 0.0) best_t = 0x7fffffffffffffffL; // a lane without a valid cell never wins
    wave_first_max(best, best_t);

    // ---- third pass: the excursion of Q_k = sum_{i<=k} d_i^2 from its straight line (k / m) S2
    double bestq = -1.0;
    long bestq_t = -1;
    carry = 0.0;
    base = 0;
    auto pass3 = [&](long t0, bool ok, double e) {
        const unsigned long long ball = __ballot(ok);
        const long k = base + __popcll(ball & below) + 1;
        const double d = ok ? e - mean : 0.0;
        const double qk = carry + wave_scan(d * d, lane);
        carry = __shfl(qk, 63, 64);
        const double val = fabs(qk - ((double)k / dm) * S2);
        if (ok && val > bestq) {
            bestq = val;
            bestq_t = t0 + lane;
        }
        base += __popcll(ball);
    };
#pragma unroll
    for (int c = 0; c < kResidKeep; ++c)
        if ((long)c * kResidTile < a.T) pass3((long)c * kResidTile, (kept >> c) & 1u, keep[c]);
    for (long t0 = (long)kResidKeep * kResidTile; t0 < a.T; t0 += kResidTile) {
        double e;
        const bool ok = cell(t0 + lane, e);
        pass3(t0, ok, e);
    }
    if (bestq < 0.0) bestq_t = 0x7fffffffffffffffL;
    wave_first_max(bestq, bestq_t);

    if (!live || lane != 0) return;
    const double nan = __builtin_nan("");
    double *out = a.stats + s * resid_stats;
    const bool any = m > 0;
    out[0] = dm;
    out[1] = any ? mean : nan;
    out[2] = any ? S2 : nan;
    out[3] = any ? S3 : nan;
    out[4] = any ? S4 : nan;
    out[5] = (double)h;
    out[6] = any ? ssf : nan;
    out[7] = any ? ssl : nan;
    out[8] = any ? best : nan;
    out[9] = any ? (double)best_t : nan;
    out[10] = any ? bestq : nan;
    out[11] = any ? (double)bestq_t : nan;
}

constexpr int kCrossThreads = 256;
constexpr int kCrossOwn = 16;                                  // (lag, i, j) triples per thread at the most
constexpr int kCrossRows = resid_max_lags + kResidTile;        // rows of the staged tile: the halo, then the tile's steps

// lags per workgroup: at most kCrossThreads * kCrossOwn triples, a function of N alone
static inline int cross_lags_per_block(int N) { return N * N >= kCrossThreads * kCrossOwn ? 1 : (kCrossThreads * kCrossOwn) / (N * N); }

__global__ void __launch_bounds__(kCrossThreads) resid_cross_kernel(ResidCrossArgs a, int LB)
{
    static_assert(kResidTile == 64, "one bit of a 64-bit mask per step of a tile");
    extern __shared__ __attribute__((aligned(16))) double rsm[];
    const int N = a.N, NN = N * N, tid = threadIdx.x;
    const long b = blockIdx.x;
    const int l0 = (int)blockIdx.y * LB;
    const int nl = min(LB, a.L + 1 - l0);
    const int items = NN * nl;
    double *E = rsm;                     // [kCrossRows][N]: row r holds step t0 - resid_max_lags + r
    double *mu = E + kCrossRows * N;     // [N] mean of the series
    double *sd = mu + N;                 // [N] sqrt(S2 / m); 0: the series has no valid cell or does not vary
    unsigned long long *cur = (unsigned long long *)(sd + N), *prev = cur + N; // [N] validity of the tile and of the tile before

    for (int j = tid; j < N; j += kCrossThreads) {
        const double *row = a.stats + (b * N + j) * resid_stats;
        const double m = row[0], S2 = row[2];
        const bool ok = m > 0.0 && S2 > 0.0;
        mu[j] = row[1];
        sd[j] = ok ? sqrt(S2 / m) : 0.0;
        cur[j] = prev[j] = 0ull;
    }
    for (int i = tid; i < resid_max_lags * N; i += kCrossThreads) E[kResidTile * N + i] = 0.0; // becomes the first tile's halo

    // the triples of this thread: x = tid + 256 q -> (lag, i, j), j fastest
    int own[kCrossOwn];
    double acc[kCrossOwn];
    long long cnt[kCrossOwn];
#pragma unroll
    for (int q = 0; q < kCrossOwn; ++q) {
        const int x = tid + kCrossThreads * q;
        int packed = -1;
        if (x < items) {
            const int ll = x / NN, p = x - ll * NN, i = p / N, j = p - i * N;
            packed = i | (j << 8) | ((l0 + ll) << 16);
        }
        own[q] = packed;
        acc[q] = 0.0;
        cnt[q] = 0;
    }

    for (long t0 = 0; t0 < a.T; t0 += kResidTile) {
        __syncthreads(); // the tile before is used up (first tile: the set-up above is written)
        for (int i = tid; i < resid_max_lags * N; i += kCrossThreads) E[i] = E[kResidTile * N + i]; // its last steps: the halo
        for (int j = tid; j < N; j += kCrossThreads) {
            prev[j] = cur[j];
            cur[j] = 0ull;
        }
        __syncthreads();
        for (int c = tid; c < kResidTile * N; c += kCrossThreads) {
            const int st = c / N, j = c - st * N;
            const long t = t0 + st;
            double val = 0.0;
            if (t < a.T && t >= a.t_first && sd[j] > 0.0) {
                const long i = (b * a.bs + t * a.ts) * N + j;
                const double v = a.v[i], f = a.f[i];
                if (isfinite(v) && isfinite(f) && f > 0.0) {
                    val = (v / sqrt(f) - mu[j]) / sd[j];
                    atomicOr(&cur[j], 1ull << st);
                }
            }
            E[(resid_max_lags + st) * N + j] = val;
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kCrossOwn; ++q) {
            if (own[q] >= 0) { // uniform per wavefront but for the last one with triples
                const int i = own[q] & 0xff, j = (own[q] >> 8) & 0xff, l = own[q] >> 16;
                const double *pi = E + resid_max_lags * N + i, *pj = E + (resid_max_lags - l) * N + j;
                double sacc = acc[q];
#pragma unroll 8
                for (int st = 0; st < kResidTile; ++st) sacc = fma(pi[st * N], pj[st * N], sacc);
                acc[q] = sacc;
                const unsigned long long mj = l == 0 ? cur[j] : ((cur[j] << l) | (prev[j] >> (64 - l)));
                cnt[q] += __popcll(cur[i] & mj);
            }
        }
    }

    const double nan = __builtin_nan("");
    const long out0 = (b * (a.L + 1) + l0) * (long)NN;
#pragma unroll
    for (int q = 0; q < kCrossOwn; ++q) {
        if (own[q] >= 0) {
            const int i = own[q] & 0xff, j = (own[q] >> 8) & 0xff;
            const bool ok = sd[i] > 0.0 && sd[j] > 0.0;
            const long o = out0 + tid + kCrossThreads * q;
            a.counts[o] = ok ? cnt[q] : 0;
            a.sums[o] = ok ? acc[q] : nan;
        }
    }
}

hipError_t launch_resid_series(const ResidSeriesArgs &a, hipStream_t s)
{
    if (a.B < 1 || a.T < 1 || a.N < 1 || a.t_first < 0) return hipErrorInvalidValue;
    const long blocks = (a.B * a.N + 3) / 4;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resid_series_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_resid_cross(const ResidCrossArgs &a, hipStream_t s)
{
    if (a.B < 1 || a.T < 1 || a.N < 1 || a.N > resid_max_series || a.L < 0 || a.L > resid_max_lags || a.t_first < 0)
        return hipErrorInvalidValue;
    if (a.B > 0x7fffffffL) return hipErrorInvalidValue;
    const int LB = min(cross_lags_per_block(a.N), a.L + 1);
    const int yblocks = (a.L + 1 + LB - 1) / LB;
    const size_t lds = (size_t)(kCrossRows + 4) * a.N * sizeof(double); // the tile, mean, scale and the two masks per series
    hipLaunchKernelGGL(resid_cross_kernel, dim3((unsigned)a.B, (unsigned)yblocks), dim3(kCrossThreads), lds, s, a, LB);
    return hipGetLastError();
}

} // namespace mk
