// draw_kernels.hip -- the device half of the SIMULATION SMOOTHER by mean correction (Durbin & Koopman 2002, "A simple and efficient
// simulation smoother for state space time series analysis", Biometrika 89:603-616): joint draws of the states / the projected
// series given the data cost one unconditional simulation of the model plus one smoothing pass of the perturbed record each.
//
// The model is the one the filter implements (seqkalmanfilter, metran/kalmanfilter.py:315-333; matrices of Metran._get_matrices,
// metran/metran.py:386-416):   x_{-1} ~ N(x0, P0),   x_t = phi o x_{t-1} + w_t,  w_t ~ N(0, diag q),
//                              y_t = [I | Gamma] x_t + e_t,  e_t ~ N(0, diag R).
// For path id = s * B + i (draw s of instance i, record i % R) the kernel below walks time once:
//     x+_{-1} = L0 z_init (zero mean),   x+_t = phi o x+_{t-1} + sqrt(q) o z_t[0:n],   y+_t = [I | Gamma] x+_t + sqrt(R) o z_t[n:n+N],
//     y*_{t,j} = y_{t,j} - y+_{t,j} where (t, j) is observed, NaN where it is not.
// The smoothing pass of y* is the existing mk_filter_smooth on a problem with S * B instances and records; the draw is
// x+ + E[x | y*]  (states)  or  scale o ([I | Gamma] x+) + sim_means(y*)  (series) -- draw_combine_kernel.
//
// The normals are COUNTER-BASED (Philox4x32-10; Salmon et al., SC'11): a value depends on what it is for -- (step, component,
// instance, draw) under the seed -- and not on the launch that computes it, so results do not depend on chunking, on the
// batch a model sits in or on the number of ranks.  key = (seed & 0xffffffff, seed >> 32), counter = (t + 1, c >> 1,
// first_instance + i, d) with t + 1 = 0 the initial state; the four output words give two uniforms of 52 bits each, strictly
// inside (0, 1), and Box-Muller turns them into the normals of components c (even: cosine) and c + 1 (sine).
//
// Mapping (draw_perturb_kernel): a group of G = 2^k >= n lanes per path, 256 / G paths per block.  The normals of a TILE of
// steps are produced first, one Philox call per PAIR of components, the (step, pair) items dealt round-robin over all G lanes
// -- every lane works whatever n is -- into LDS; then the group walks the tile's steps with one lane per state (the recursion
// is one fma), the K factor values passed through a double-buffered LDS row, one lane per series for the projection, the
// observation and the stores (neighbouring lanes, and in the time-major layout neighbouring paths, store neighbouring
// addresses).  No arrays in registers: no scratch.
#include "draw_kernels.h"

#include <cmath>

namespace mk {
namespace {

constexpr int kBlock = 256;
constexpr int kTileBytes = 32768; // LDS of the normals' tile per block

struct Words {
    uint32_t w0, w1, w2, w3;
};

__device__ __forceinline__ Words philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return {c0, c1, c2, c3};
}

// The two normals of component pair `pair` (components 2 pair, 2 pair + 1); raw: the 52-bit integers m1, m2 instead.
__device__ __forceinline__ void normal_pair(uint64_t seed, uint32_t step1, uint32_t pair, uint32_t inst, uint32_t d, bool raw,
                                            double &even, double &odd)
{
    const Words w = philox4x32_10(step1, pair, inst, d, (uint32_t)seed, (uint32_t)(seed >> 32));
    const uint64_t m1 = ((uint64_t)(w.w0 >> 6) << 26) | (uint64_t)(w.w1 >> 6);
    const uint64_t m2 = ((uint64_t)(w.w2 >> 6) << 26) | (uint64_t)(w.w3 >> 6);
    if (raw) {
        even = (double)m1;
        odd = (double)m2;
        return;
    }
    const double u1 = ((double)m1 + 0.5) * 0x1p-52; // exact: 53 significant bits
    const double u2 = ((double)m2 + 0.5) * 0x1p-52;
    const double rho = sqrt(-2.0 * log(u1));
    double sn, cs;
    sincos(6.283185307179586 * u2, &sn, &cs);
    even = rho * cs;
    odd = rho * sn;
}

__global__ __launch_bounds__(kBlock) void draw_perturb_kernel(const DrawArgs a, const int lg, const int TS, const int ZS)
{
    extern __shared__ double lds[];
    const int N = a.N, K = a.K, n = N + K;
    const int G = 1 << lg, gpb = kBlock >> lg;
    const int grp = (int)threadIdx.x >> lg, lane = (int)threadIdx.x & (G - 1);
    const long id = (long)blockIdx.x * gpb + grp;
    const bool live = id < a.S * a.B;
    double *zt = lds + (size_t)grp * TS * ZS;                       // this path's tile of normals [TS][ZS]
    double *fb = lds + (size_t)gpb * TS * ZS + (size_t)grp * 2 * K; // its factor values, double-buffered [2][K]

    const long s = live ? id / a.B : 0, i = live ? id - s * a.B : 0, r = i % a.R;
    const unsigned long ds = (unsigned long)(a.first_draw + s);
    const uint32_t d = (uint32_t)(a.antithetic ? ds >> 1 : ds);
    const double sign = (a.antithetic && (ds & 1)) ? -1.0 : 1.0;
    const uint32_t inst = (uint32_t)(a.first_instance + i);
    const bool state = live && lane < n, series = live && lane < N;
    const double phi = state ? a.phi[i * n + lane] : 0.0;
    const double sq = state ? sqrt(a.q[i * n + lane]) : 0.0;
    const double sr = (series && a.obsvar) ? sqrt(a.obsvar[r * N + lane]) : 0.0;
    const double *grow = a.loadings + (r * N + (series ? lane : 0)) * K;
    const double g0 = (series && K > 0) ? grow[0] : 0.0, g1 = (series && K > 1) ? grow[1] : 0.0;
    const double g2 = (series && K > 2) ? grow[2] : 0.0, g3 = (series && K > 3) ? grow[3] : 0.0;
    const unsigned np = (unsigned)ZS >> 1;          // component pairs per step
    const unsigned np0 = (unsigned)(n + 1) >> 1;    // ... of the initial state (no observation noise)
    double x = 0.0;

    for (long tile0 = 0; tile0 <= a.T; tile0 += TS) {
        const int rows = (int)((a.T + 1 - tile0 < TS) ? a.T + 1 - tile0 : TS);
        if (live) {
            const unsigned items = (unsigned)rows * np;
            for (unsigned it = (unsigned)lane; it < items; it += (unsigned)G) {
                const unsigned row = it / np, p = it - row * np;
                const long tt = tile0 + row;
                if (tt == 0 && p >= np0) continue;
                double ze, zo;
                normal_pair(a.seed, (uint32_t)tt, p, inst, d, false, ze, zo);
                zt[row * ZS + 2 * p] = sign * ze;
                zt[row * ZS + 2 * p + 1] = sign * zo;
            }
        }
        __syncthreads();
        for (int row = 0; row < rows; ++row) {
            const long tt = tile0 + row;
            const double *z = zt + row * ZS;
            if (tt == 0) { // x+_{-1} = L0 z_init
                if (state) {
                    if (a.L0) {
                        const double *l = a.L0 + (i * n + lane) * n;
                        x = 0.0;
                        for (int m = 0; m <= lane; ++m) x += l[m] * z[m];
                    } else {
                        x = z[lane];
                    }
                }
                continue;
            }
            const long t = tt - 1, orow = id * a.bs + t * a.ts;
            double *f = fb + (tt & 1) * K;
            if (state) {
                x = phi * x + sq * z[lane];
                if (lane >= N) f[lane - N] = x;
                if (a.xplus) a.xplus[orow * n + lane] = x;
            }
            __syncthreads();
            if (series) {
                double zx = x;
                if (K > 0) zx += g0 * f[0];
                if (K > 1) zx += g1 * f[1];
                if (K > 2) zx += g2 * f[2];
                if (K > 3) zx += g3 * f[3];
                for (int k = 4; k < K; ++k) zx += grow[k] * f[k];
                const double yp = a.obsvar ? zx + sr * z[n + lane] : zx;
                const double y = a.obs[(r * a.obs_bs + t * a.obs_ts) * N + lane];
                a.ystar[orow * N + lane] = isfinite(y) ? y - yp : __builtin_nan("");
                if (a.zxplus) a.zxplus[orow * N + lane] = zx;
            }
        }
        __syncthreads(); // the tile is rewritten next
    }
}

__global__ __launch_bounds__(kBlock) void draw_combine_kernel(const DrawCombineArgs a)
{
    const long total = a.SB * a.T * a.W;
    for (long e = (long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long)gridDim.x * kBlock) {
        double v = a.plus[e];
        if (a.scale) {
            const long row = e / a.W, j = e - row * a.W;
            const long id = a.time_major ? row % a.SB : row / a.T;
            v *= a.scale[((id % a.B) % a.R) * a.W + j];
        }
        a.inout[e] += v;
    }
}

__global__ __launch_bounds__(kBlock) void draw_normals_kernel(const DrawNormalsArgs a)
{
    const long np = (a.ncomp + 1) >> 1, steps = a.T + 1;
    const long total = a.ndraws * a.ninstances * steps * np;
    for (long e = (long)blockIdx.x * kBlock + threadIdx.x; e < total; e += (long)gridDim.x * kBlock) {
        const long p = e % np, rest = e / np;
        const long tt = rest % steps, path = rest / steps;
        const long i = path % a.ninstances, s = path / a.ninstances;
        const unsigned long ds = (unsigned long)(a.first_draw + s);
        const double sign = (a.antithetic && (ds & 1) && !a.raw) ? -1.0 : 1.0;
        double ze, zo;
        normal_pair(a.seed, (uint32_t)tt, (uint32_t)p, (uint32_t)(a.first_instance + i), (uint32_t)(a.antithetic ? ds >> 1 : ds),
                    a.raw != 0, ze, zo);
        double *o = a.out + (path * steps + tt) * a.ncomp + 2 * p;
        o[0] = sign * ze;
        if (2 * p + 1 < a.ncomp) o[1] = sign * zo;
    }
}

int grid_for(long total)
{
    const long blocks = (total + kBlock - 1) / kBlock;
    return (int)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

} // namespace

hipError_t launch_draw_perturb(const DrawArgs &a, hipStream_t s)
{
    const int n = a.N + a.K;
    if (n < 2 || n > 128 || a.S < 1 || a.B < 1 || a.T < 1) return hipErrorInvalidValue;
    int lg = 2;
    while ((1 << lg) < n) ++lg;
    const int gpb = kBlock >> lg;
    const int ncomp = n + (a.obsvar ? a.N : 0), ZS = (ncomp + 1) & ~1;
    long TS = kTileBytes / ((long)gpb * ZS * (long)sizeof(double));
    TS = TS > 32 ? 32 : (TS < 1 ? 1 : TS);
    if (TS > a.T + 1) TS = a.T + 1;
    const size_t lds = ((size_t)gpb * TS * ZS + (size_t)gpb * 2 * a.K) * sizeof(double);
    const long blocks = (a.S * a.B + gpb - 1) / gpb;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(draw_perturb_kernel, dim3((unsigned)blocks), dim3(kBlock), lds, s, a, lg, (int)TS, ZS);
    return hipGetLastError();
}

hipError_t launch_draw_combine(const DrawCombineArgs &a, hipStream_t s)
{
    hipLaunchKernelGGL(draw_combine_kernel, dim3(grid_for(a.SB * a.T * a.W)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_draw_normals(const DrawNormalsArgs &a, hipStream_t s)
{
    const long total = a.ndraws * a.ninstances * (a.T + 1) * ((a.ncomp + 1) >> 1);
    hipLaunchKernelGGL(draw_normals_kernel, dim3(grid_for(total)), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

} // namespace mk
