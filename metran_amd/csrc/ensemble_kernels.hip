// ensemble_kernels.hip -- WINDOW STATISTICS of posterior draws, reduced on the device: what an ensemble of draws (draw_kernels.hip,
// BatchedKalman.draw_smoothed) is read for -- the uncertainty of a monthly mean, of a yearly minimum, of the time spent below a
// level -- is a few numbers per (model, series, window), not a path per draw.  Two kernels:
//
// path_functionals_kernel: one lane per (path, column), ONE forward walk over time.  The lane carries its current window
// index w, that window's bounds and the five accumulators (sum, min, max, steps below the level, current / longest spell), and
// stores a window's five numbers when the walk leaves the window; windows differ between records, so the lanes of a wavefront
// sit in different windows at the same step -- per-lane state, no loop over windows.  Lane e = id * Wd + j: in the time-major
// layout [T,SB,Wd] step t of lane e is element t * SB * Wd + e, so every load of a wavefront is one contiguous run; in the
// model-major layout [SB,T,Wd] the lanes of one path read Wd neighbouring doubles and the paths lie T * Wd apart (a strided
// gather: the same walk, the same numbers, more memory transactions per load).  The sums add in increasing t whatever the
// layout, batch or grid: adds, compares, one division and integer counts -- nothing for the compiler to contract.
//
// ensemble_summary_kernel: a group of G = 2^k lanes per cell (instance, column, window, functional) of values [S,cells], G half
// the padded number of draws (32 .. 256), 256 / G neighbouring cells per block.  The block loads its cells' S values into LDS
// (neighbouring lanes read neighbouring cells: runs of 8 * 256 / G bytes); the group's lane 0 walks them in increasing s --
// count, sequential sum, extremes of the FINITE values, which it compacts in place on the way (non-finite values are gone
// before the sort), then the second pass of the standard deviation about the mean -- and the group sorts the finite values,
// padded with +inf to the power of two >= S, by a bitonic network in LDS for the quantiles.  The fixed order is the contract
// (tests/ensemble_ref.py); the kernel is bound by lane 0's two passes and the network's barriers, not by its reads.
#include "ensemble_kernels.h"

#include <cmath>

namespace mk {
namespace {

constexpr int kBlock = 256;
static_assert(kBlock == 1 << 8, "ensemble_summary_kernel splits a lane index by shifts");
constexpr int kPathBlock = 64; // one wavefront per block: few lanes (paths x columns) against many CUs
constexpr int kAhead = 16;     // steps per tile of loads; a lane has two tiles in flight

__global__ __launch_bounds__(kPathBlock) void path_functionals_kernel(const PathFunctionalArgs a)
{
    const long pairs = a.SB * a.Wd;
    const long e = (long)blockIdx.x * kPathBlock + threadIdx.x;
    if (e >= pairs) return;
    const long id = e / a.Wd, j = e - id * a.Wd, r = (id % a.B) % a.R;
    const double *y = a.paths + (a.time_major ? e : id * a.T * a.Wd + j);
    const long ystep = a.time_major ? pairs : (long)a.Wd;
    const int64_t *win = a.windows + r * a.W * 2;
    const double nan = __builtin_nan("");
    const double c = a.thresholds ? a.thresholds[r * a.Wd + j] : nan;
    const bool level = c == c;
    double *o = a.out + e * a.W * path_functional_count;

    const int T = (int)a.T, W = (int)a.W;   // both below 2^31 (the launcher's check): the walk's compares are 32-bit
    int w = 0, lo = 0, hi = 0;              // the window the walk is in or ahead of, clamped to 0 <= lo <= hi <= T
    double sum, mn, mx;
    int cnt, below, run, longest;
    bool bad;
    auto open = [&]() {
        if (w < W) {
            const int64_t b0 = win[2 * w], b1 = win[2 * w + 1];
            lo = b0 < 0 ? 0 : (b0 > T ? T : (int)b0);
            hi = b1 < lo ? lo : (b1 > T ? T : (int)b1);
        }
        sum = 0.0;
        mn = __builtin_inf();
        mx = -__builtin_inf();
        cnt = below = run = longest = 0;
        bad = false;
    };
    auto close = [&]() {
        double *f = o + (long)w * path_functional_count;
        const bool ok = cnt > 0 && !bad;
        f[0] = ok ? sum / (double)cnt : nan;
        f[1] = ok ? mn : nan;
        f[2] = ok ? mx : nan;
        f[3] = (ok && level) ? (double)below / (double)cnt : nan;
        f[4] = (ok && level) ? (double)longest : nan;
        ++w;
        open();
    };
    open();
    // Tiles of kAhead steps, the loads of the NEXT tile issued before this one is walked: a lane has up to 2 kAhead loads in
    // flight and waits for memory under its own arithmetic.  A tile is loaded when the window the walk is in or ahead of
    // begins before the tile ends -- lo only grows (sorted windows), so a tile judged unneeded stays unneeded: gaps and the
    // time before the first window are not read.
    double cur[kAhead], nxt[kAhead];
    auto load = [&](double(&v)[kAhead], long t0, bool need) {
#pragma unroll
        for (int u = 0; u < kAhead; ++u) v[u] = (need && t0 + u < T) ? y[(t0 + u) * ystep] : 0.0;
    };
    bool have = lo < kAhead;
    load(cur, 0, have);
    for (long t0 = 0; t0 < T && w < W; t0 += kAhead) {
        const bool want = lo < t0 + 2 * kAhead;
        load(nxt, t0 + kAhead, want);
        if (have) {
#pragma unroll
            for (int u = 0; u < kAhead; ++u) {
                const int t = (int)t0 + u;   // t0 < T
                while (w < W && hi <= t) close();   // sorted windows: at most the empty ones and the one that ended here
                if (w < W && t >= lo && t < T) {
                    const double x = cur[u];
                    sum += x;
                    ++cnt;
                    bad |= x != x;
                    mn = x < mn ? x : mn;
                    mx = x > mx ? x : mx;
                    const bool under = x < c;
                    run = under ? run + 1 : 0;
                    below += under ? 1 : 0;
                    longest = run > longest ? run : longest;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < kAhead; ++u) cur[u] = nxt[u];
        have = want;
    }
    while (w < W) close();
}

__global__ __launch_bounds__(kBlock) void ensemble_summary_kernel(const EnsembleSummaryArgs a, const int cap, const int lg)
{
    extern __shared__ double lds[];
    const int G = 1 << lg, gpb = kBlock >> lg;   // lanes per cell, cells per block
    const int tid = (int)threadIdx.x, grp = tid >> lg, lane = tid & (G - 1);
    double *z = lds + (size_t)grp * (cap + 2), *meta = z + cap;   // this cell's values [cap], cap = 2^k >= S; meta[0] = the finite ones
    const int ncol = 5 + a.nprobs;
    const double nan = __builtin_nan("");
    const long tiles = (a.cells + gpb - 1) / gpb;
    for (long tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        // the tile's gpb neighbouring cells of every draw: neighbouring lanes read neighbouring addresses
        for (long e = tid; e < a.S * gpb; e += kBlock) {
            const long s = e >> (8 - lg), g = e & (gpb - 1), cl = tile * gpb + g;   // kBlock = 2^8
            if (cl < a.cells) lds[(size_t)g * (cap + 2) + s] = a.values[s * a.cells + cl];
        }
        __syncthreads();
        const long cell = tile * gpb + grp;
        const bool live = cell < a.cells;
        double *o = a.out + cell * ncol;
        if (live && lane == 0) {
            long m = 0;
            double sum = 0.0, mn = __builtin_inf(), mx = -__builtin_inf();
            for (long s = 0; s < a.S; ++s) {
                const double x = z[s];
                if (!isfinite(x)) continue;
                z[m++] = x;   // in place: m <= s
                sum += x;
                mn = x < mn ? x : mn;
                mx = x > mx ? x : mx;
            }
            const double mean = m > 0 ? sum / (double)m : nan;
            double ss = 0.0;
            for (long k = 0; k < m; ++k) {
                const double d = z[k] - mean;
                ss += d * d;
            }
            o[0] = (double)m;
            o[1] = mean;
            o[2] = m > 1 ? sqrt(ss / (double)(m - 1)) : nan;
            o[3] = m > 0 ? mn : nan;
            o[4] = m > 0 ? mx : nan;
            meta[0] = (double)m;
        }
        __syncthreads();
        const int m = live ? (int)meta[0] : 0;
        for (int i = m + lane; i < cap; i += G) z[i] = __builtin_inf();
        __syncthreads();
        // the network runs over all cap entries whatever m is: its steps, and with them the barriers, are the block's
        for (int k = 2; k <= cap; k <<= 1) {
            for (int jj = k >> 1; jj > 0; jj >>= 1) {
                for (int i = lane; i < cap; i += G) {
                    const int p = i ^ jj;
                    if (p > i) {
                        const double u = z[i], v = z[p];
                        if ((u > v) == ((i & k) == 0)) {
                            z[i] = v;
                            z[p] = u;
                        }
                    }
                }
                __syncthreads();
            }
        }
        if (live && lane < a.nprobs) {
            double q = nan;
            if (m > 0) {
                const double h = (double)(m - 1) * a.probs[lane], fl = floor(h);
                const int lo = (int)fl, hi = lo + 1 < m ? lo + 1 : m - 1;
                q = z[lo] + (h - fl) * (z[hi] - z[lo]);
            }
            o[5 + lane] = q;
        }
        __syncthreads(); // z is reloaded for the next tile
    }
}

} // namespace

hipError_t launch_path_functionals(const PathFunctionalArgs &a, hipStream_t s)
{
    if (a.SB < 1 || a.B < 1 || a.R < 1 || a.T < 1 || a.T >= 0x7fffffffL - 2 * kAhead || a.Wd < 1 || a.W < 1 || a.W > 0x7fffffffL) return hipErrorInvalidValue;
    const long blocks = (a.SB * a.Wd + kPathBlock - 1) / kPathBlock;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(path_functionals_kernel, dim3((unsigned)blocks), dim3(kPathBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_ensemble_summary(const EnsembleSummaryArgs &a, hipStream_t s)
{
    if (a.S < 1 || a.S > ensemble_max_draws || a.cells < 1 || a.nprobs < 0 || a.nprobs > ensemble_max_probs) return hipErrorInvalidValue;
    int cap = 1;
    while (cap < a.S) cap <<= 1;
    int lg = 5;   // lanes per cell: half the padded length, between 32 (>= ensemble_max_probs) and the block
    while ((2 << lg) < cap && (1 << lg) < kBlock) ++lg;
    const int gpb = kBlock >> lg;
    const size_t lds = (size_t)gpb * (cap + 2) * sizeof(double);
    const long tiles = (a.cells + gpb - 1) / gpb;
    const long blocks = tiles < 65536 ? tiles : 65536;
    hipLaunchKernelGGL(ensemble_summary_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, s, a, cap, lg);
    return hipGetLastError();
}

} // namespace mk
