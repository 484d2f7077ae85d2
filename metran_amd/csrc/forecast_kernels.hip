// forecast_kernels.hip -- multi-step-ahead forecasts of every series from any origin, and the forecast skill by horizon.
// Size-generic (run-time N, K; n = N + K <= 64), stand-alone: no shape-module entry, no ShapeOps row.
//
// Definitions (include/metran_hip.h, mk_forecast).  Origin o in {-1, 0, .., T-1} has the moments (a_o, P_o): the FILTERED record
// of step o written by the recording forward pass, or the initial moments (x0 / P0, or 0 / I) for o = -1.  For h >= 1 the
// filter's own prediction (kalmanfilter.py:318-331; Phi, Q diagonal) is applied h times, x <- phi o x, P <- (phi phi') o P +
// diag(q), and the forecast of series j is m = z_j x, s = z_j P z_j' + R_j with Z = [I | loadings]: what the filter does on h
// successive empty steps.
//
// Under diagonal Phi and Q the entries of P propagate one by one, and series j needs only x_j, P_jj, P_{j,N+k} (k < K), the K
// factor means and the K x K factor block: 2 + K numbers per series plus K + K^2 per origin -- not the n x n covariance.
//
// WHICH RECORD IMAGE IS READ: position (c, r) of the square, i.e. F[n + c*n + r] for the element that lane r of innov_step_kernel
// holds as column c -- the (c, r) image the specialised recording pass writes.  The size-generic filter writes the transpose of
// that image (equal up to the rounding-level asymmetry of the rank-one updates); the SAME positions are read under either
// family, exactly as innov_step_kernel does, so that a track of horizon 1 is mk_innovations' pred_mean / pred_var bit for bit
// under both.
//
// forecast_path_kernel   fan and track.  One (instance, row) per lane group (8 lanes for N <= 8, 16 for N <= 16, 32 for N <= 32, 64 above); lane
//                        j < N carries x_j and P_jj in registers and P_{j,N+k} in its own LDS column; the factor means and the
//                        factor block are shared through the group's LDS.  A fan group loops h = 1 .. H from its record's origin
//                        and stores a row per h; a track group propagates t - origin steps and stores one row.  The
//                        multiply-adds are innov_step_kernel's (phi_r * x, fma(P, phi_r * phi_c, [r = c] q_r), the same
//                        quadratic form).
// forecast_skill_kernel  A lane group owns (instance, chunk of kForecastChunk consecutive origins, block of kForecastBlock
//                        horizons) and walks the chunk's origins in ascending order: load the entries named above, run the
//                        h-loop, read y_{o+h,j}, accumulate the six sums of its series in registers (sum log s as a product of
//                        mantissas and a sum of exponents: one logarithm per chunk).  Each block of horizons loads the
//                        origin's entries itself: the records are read once per block, twice at H = 14.  A call with one chunk
//                        stores the table itself; otherwise the partial sums go to the workspace and
// forecast_reduce_kernel adds the chunks in ascending order (one thread per (instance, series, horizon); no atomics).
// Every sum is a fixed sequence over the origins of a chunk and over the chunks -- fixed by T alone (t_first and H only mask):
// an instance's outputs are bit-identical whatever batch it sits in and whichever outputs are asked for.
// Groups past the last one replicate it without storing; a group whose lanes exceed N replicates series N - 1 likewise.
#include <hip/hip_runtime.h>

#include <cmath>

#include "forecast_kernels.h"
#include "mk_prims.h" // wave_lds_sync
#include "reader_prims.h"

namespace mk {

namespace {

// doubles of LDS per lane group: phi, q and the means of the factors (3 K), the factor block (K x K), the loadings and the
// series-factor covariances, both as K columns of G lanes
__host__ __device__ inline long fc_lds_doubles(int G, int K) { return (3L * K + (long)K * K + 2L * K * G + 1) & ~1L; }

// what a lane group carries from an origin through the horizons
template <int G>
struct FcState {
    double *phf, *qf, *xf, *PF, *GT, *CR; // the group's LDS
    int N, K, n, lane, jl;
    double phi_j, q_j, r_j; // of the lane's series
    double x, d;            // x_j, P_jj

    __device__ __forceinline__ void init(const ForecastArgs &a, double *lds, int lane_, long b, long rec)
    {
        N = a.N, K = a.K, n = N + K, lane = lane_;
        jl = lane < N ? lane : N - 1;
        phf = lds, qf = phf + K, xf = qf + K, PF = xf + K, GT = PF + K * K, CR = GT + K * G;
        phi_j = a.phi[b * n + jl], q_j = a.q[b * n + jl];
        r_j = a.obsvar ? a.obsvar[rec * N + jl] : 0.0;
        _Pragma("nounroll")
        for (int k = lane; k < K; k += G) {
            phf[k] = a.phi[b * n + N + k];
            qf[k] = a.q[b * n + N + k];
        }
        _Pragma("nounroll")
        for (int k = 0; k < K; ++k) GT[k * G + lane] = a.loadings[(rec * N + jl) * K + k];
    }

    // the moments of origin o: position (c, r) of the record's square is lane r's column c (see the header comment)
    __device__ __forceinline__ void load(const ForecastArgs &a, long b, long o)
    {
        wave_lds_sync(); // the reads of the previous origin are done
        if (o >= 0) {
            const double *p = a.F + (b * a.bs + o * a.ts) * a.rs;
            x = p[jl];
            d = p[n + jl * n + jl];
            _Pragma("nounroll")
            for (int k = 0; k < K; ++k) CR[k * G + lane] = p[n + (N + k) * n + jl];
            _Pragma("nounroll")
            for (int k = lane; k < K; k += G) xf[k] = p[N + k];
            _Pragma("nounroll")
            for (int i = lane; i < K * K; i += G) {
                const int k = i / K, l = i - k * K;
                PF[i] = p[n + (N + l) * n + N + k];
            }
        } else { // run_filter's defaults (kalmanfilter.py:747-750) or the caller's initial state
            x = a.x0 ? a.x0[b * n + jl] : 0.0;
            d = a.P0 ? a.P0[(b * n + jl) * n + jl] : 1.0;
            _Pragma("nounroll")
            for (int k = 0; k < K; ++k) CR[k * G + lane] = a.P0 ? a.P0[(b * n + jl) * n + N + k] : 0.0;
            _Pragma("nounroll")
            for (int k = lane; k < K; k += G) xf[k] = a.x0 ? a.x0[b * n + N + k] : 0.0;
            _Pragma("nounroll")
            for (int i = lane; i < K * K; i += G) {
                const int k = i / K, l = i - k * K;
                PF[i] = a.P0 ? a.P0[(b * n + N + k) * n + N + l] : (k == l ? 1.0 : 0.0);
            }
        }
        wave_lds_sync();
    }

    // one prediction (:318-331; Phi diagonal): x = phi o x, P = (phi phi') o P + diag(q) -- innov_step_kernel's multiply-adds
    __device__ __forceinline__ void predict()
    {
        x = phi_j * x;
        d = fma(d, phi_j * phi_j, q_j);
        _Pragma("nounroll")
        for (int k = 0; k < K; ++k) CR[k * G + lane] = fma(CR[k * G + lane], phi_j * phf[k], 0.0);
        _Pragma("nounroll")
        for (int k = lane; k < K; k += G) xf[k] = phf[k] * xf[k];
        _Pragma("nounroll")
        for (int i = lane; i < K * K; i += G) {
            const int k = i / K, l = i - k * K;
            PF[i] = fma(PF[i], phf[k] * phf[l], k == l ? qf[k] : 0.0);
        }
        wave_lds_sync();
    }

    // m = z_j x and s = z_j P z_j' + r_j, Z = [I | loadings]; the caller syncs before the next predict()
    __device__ __forceinline__ void forecast(double &m, double &s) const
    {
        double cross = 0.0, pm = x;
        _Pragma("nounroll")
        for (int k = 0; k < K; ++k) {
            const double g = GT[k * G + lane];
            cross = fma(g, CR[k * G + lane], cross);
            pm = fma(g, xf[k], pm);
        }
        double quad = 0.0;
        _Pragma("nounroll")
        for (int k = 0; k < K; ++k) {
            double h = 0.0;
            _Pragma("nounroll")
            for (int l = 0; l < K; ++l) h = fma(GT[l * G + lane], PF[k * K + l], h);
            quad = fma(GT[k * G + lane], h, quad);
        }
        m = pm;
        s = fma(2.0, cross, d) + quad + r_j;
    }
};

} // namespace

template <int G>
__global__ void __launch_bounds__(256) forecast_path_kernel(ForecastArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double fsm[];
    const int gpb = blockDim.x / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const long per = fc_lds_doubles(G, a.K);
    const bool want_track = a.track_mean || a.track_var, want_fan = a.fan_mean || a.fan_var;

    // groups past the last row replicate it (same loads, no stores): the wavefront stays whole
    const long ntrack = want_track ? a.B * a.T : 0, rows = ntrack + (want_fan ? a.B : 0);
    long row = (long)blockIdx.x * gpb + grp;
    const bool live = row < rows;
    if (!live) row = rows - 1;
    const bool fan = row >= ntrack;
    long b, t = 0, origin, steps;
    if (fan) {
        b = row - ntrack;
        origin = a.fan_origins ? (long)a.fan_origins[b % a.R] : a.T - 1;
        steps = a.H;
    } else {
        if (a.ts == 1) { // consecutive rows are neighbours in memory in either layout
            b = row / a.T;
            t = row - b * a.T;
        } else {
            t = row / a.B;
            b = row - t * a.B;
        }
        origin = t - a.track_h < -1 ? -1 : t - a.track_h;
        steps = t - origin;
    }
    const long rec = b % a.R;
    FcState<G> st;
    st.init(a, fsm + grp * per, lane, b, rec);
    const bool store = live && lane < a.N;
    const double sc = a.scale ? a.scale[rec * a.N + st.jl] : 1.0, of = a.offset ? a.offset[rec * a.N + st.jl] : 0.0;
    st.load(a, b, origin);
    for (long h = 1; h <= steps; ++h) {
        st.predict();
        if (fan || h == steps) {
            double pm, pv;
            st.forecast(pm, pv);
            const long orow = fan ? (b * a.H + (h - 1)) * a.N + lane : (b * a.bs + t * a.ts) * a.N + lane;
            double *om = fan ? a.fan_mean : a.track_mean, *ov = fan ? a.fan_var : a.track_var;
            if (store) {
                if (om) om[orow] = scaled_mean(pm, sc, of);
                if (ov) ov[orow] = scaled_var(pv, sc);
            }
        }
        wave_lds_sync();
    }
}

static_assert(kForecastBlock == 8, "the accumulation switch of forecast_skill_kernel lists eight horizons");

template <int G>
__global__ void __launch_bounds__(256) forecast_skill_kernel(ForecastArgs a)
{
    extern __shared__ __attribute__((aligned(16))) double fsm[];
    const int gpb = blockDim.x / G;
    const int lane = threadIdx.x % G, grp = threadIdx.x / G;
    const long per = fc_lds_doubles(G, a.K);
    const long chunks = forecast_chunks(a.T), groups = a.B * chunks;
    long gid = (long)blockIdx.x * gpb + grp;
    const bool live = gid < groups;
    if (!live) gid = groups - 1;
    const long b = gid / chunks, c = gid - b * chunks, rec = b % a.R;
    const int h0 = (int)blockIdx.y * kForecastBlock; // this group's horizons are h0 + 1 .. min(h0 + kForecastBlock, H)
    FcState<G> st;
    st.init(a, fsm + grp * per, lane, b, rec);

    // the six sums of the block's horizons: static register indices (the switch below is a uniform branch: i is the same in
    // every lane), pair count and hits as integers
    // sum log s of a chunk is kept as log(product of the mantissas) + ln 2 * (sum of the exponents): one logarithm per chunk and
    // horizon instead of one per pair (the f64 logarithm was more than half of the step's instructions); at most kForecastChunk
    // mantissas in [0.5, 1) are multiplied, so the product cannot underflow and each factor costs half an ulp of the sum
    double acc[kForecastBlock][3], lman[kForecastBlock];
    int cnt[kForecastBlock], hit[kForecastBlock], lexp[kForecastBlock];
#pragma unroll
    for (int i = 0; i < kForecastBlock; ++i) {
        cnt[i] = hit[i] = lexp[i] = 0;
        lman[i] = 1.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) acc[i][k] = 0.0;
    }

    const long o_end = (c + 1) * kForecastChunk < a.T ? (c + 1) * kForecastChunk : a.T;
    for (long o = c * kForecastChunk; o < o_end; ++o) {
        // pairs (o, o + h) with t_first <= o and o + h <= T - 1; an origin without one in this block of horizons adds nothing
        if (o < a.t_first || o + h0 + 1 > a.T - 1) continue;
        long hmax = a.T - 1 - o;
        if (hmax > a.H) hmax = a.H;
        st.load(a, b, o);
        for (int h = 1; h <= h0; ++h) st.predict();
        const double *yrow = a.obs + (rec * a.obs_bs + (o + h0 + 1) * a.obs_ts) * a.N + st.jl;
        const int steps = hmax - h0 < kForecastBlock ? (int)(hmax - h0) : kForecastBlock; // uniform in the group
#pragma nounroll
        for (int i = 0; i < steps; ++i) {
            st.predict();
            double m, s;
            st.forecast(m, s);
            const double y = yrow[i * a.obs_ts * a.N];
            const bool ok = isfinite(y); // NaN / inf = missing (:657)
            const double e = ok ? y - m : 0.0, e2 = e * e, t3 = ok ? e2 / s : 0.0;
            int ex;
            const double mant = frexp(s, &ex);
            const double fm = !ok ? 1.0 : (s > 0.0 ? mant : __builtin_nan("")); // a variance that is not positive has no logarithm
            const int fe = ok ? ex : 0, one = ok ? 1 : 0, in = (ok && e2 <= a.z2 * s) ? 1 : 0;
#define FC_ADD(c)                                                                                                  \
    case c:                                                                                                        \
        cnt[c] += one, hit[c] += in, acc[c][0] += e, acc[c][1] += e2, acc[c][2] += t3, lman[c] *= fm, lexp[c] += fe; \
        break;
            switch (i) {
                FC_ADD(0) FC_ADD(1) FC_ADD(2) FC_ADD(3) FC_ADD(4) FC_ADD(5) FC_ADD(6) FC_ADD(7)
            }
#undef FC_ADD
            wave_lds_sync();
        }
    }

    if (!(live && lane < a.N)) return;
    double *out = chunks == 1 ? a.skill : a.partial;
    out += ((b * chunks + c) * a.N + lane) * (long)a.H * 6;
#pragma unroll
    for (int i = 0; i < kForecastBlock; ++i)
        if (h0 + i < a.H) {
            double *row = out + (h0 + i) * 6;
            row[0] = (double)cnt[i];
#pragma unroll
            for (int k = 0; k < 3; ++k) row[1 + k] = acc[i][k];
            row[4] = fma((double)lexp[i], 0.693147180559945309417, log(lman[i])); // exactly 0 without pairs
            row[5] = (double)hit[i];
        }
}

// skill[b,j,h,:] = the partial sums of the chunks, added in ascending order
__global__ void __launch_bounds__(256) forecast_reduce_kernel(ForecastArgs a)
{
    const long per = (long)a.N * a.H, cells = a.B * per, chunks = forecast_chunks(a.T);
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= cells) return;
    const long b = i / per, jh = i - b * per;
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (long c = 0; c < chunks; ++c) {
        const double *p = a.partial + ((b * chunks + c) * per + jh) * 6;
#pragma unroll
        for (int k = 0; k < 6; ++k) sum[k] += p[k];
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) a.skill[i * 6 + k] = sum[k];
}

namespace {

bool fc_args_ok(const ForecastArgs &a)
{
    return a.B >= 1 && a.T >= 1 && a.R >= 1 && a.N >= 1 && a.K >= 1 && a.N + a.K <= forecast_max_states;
}

// lane groups per block: up to 256 threads and 32 KiB of LDS, so that several blocks stay resident on a CU
template <int G>
int fc_groups_per_block(int K)
{
    const long bytes = fc_lds_doubles(G, K) * (long)sizeof(double);
    long g = 32768 / bytes;
    if (g < 1) g = 1;
    if (g > 256 / G) g = 256 / G;
    return (int)g;
}

template <int G>
hipError_t launch_path(const ForecastArgs &a, hipStream_t s)
{
    const bool want_track = a.track_mean || a.track_var, want_fan = a.fan_mean || a.fan_var;
    const long rows = (want_track ? a.B * a.T : 0) + (want_fan ? a.B : 0);
    if (rows == 0) return hipErrorInvalidValue;
    const int gpb = fc_groups_per_block<G>(a.K);
    const long blocks = (rows + gpb - 1) / gpb;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const size_t lds = (size_t)gpb * fc_lds_doubles(G, a.K) * sizeof(double);
    hipLaunchKernelGGL((forecast_path_kernel<G>), dim3((unsigned)blocks), dim3(gpb * G), lds, s, a);
    return hipGetLastError();
}

template <int G>
hipError_t launch_skill(const ForecastArgs &a, hipStream_t s)
{
    const int gpb = fc_groups_per_block<G>(a.K);
    const long groups = a.B * forecast_chunks(a.T), blocks = (groups + gpb - 1) / gpb;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    const int hblocks = (a.H + kForecastBlock - 1) / kForecastBlock;
    const size_t lds = (size_t)gpb * fc_lds_doubles(G, a.K) * sizeof(double);
    hipLaunchKernelGGL((forecast_skill_kernel<G>), dim3((unsigned)blocks, (unsigned)hblocks), dim3(gpb * G), lds, s, a);
    return hipGetLastError();
}

} // namespace

hipError_t launch_forecast_path(const ForecastArgs &a, hipStream_t s)
{
    if (!fc_args_ok(a) || a.H < 1 || a.H > forecast_max_horizon) return hipErrorInvalidValue;
    if ((a.track_mean || a.track_var) && (a.track_h < 1 || a.track_h > a.T)) return hipErrorInvalidValue;
    if (a.N <= 8) return launch_path<8>(a, s); // one lane per series: the narrowest group that holds them
    if (a.N <= 16) return launch_path<16>(a, s);
    if (a.N <= 32) return launch_path<32>(a, s);
    return launch_path<64>(a, s);
}

hipError_t launch_forecast_skill(const ForecastArgs &a, hipStream_t s)
{
    if (!fc_args_ok(a) || a.H < 1 || a.H > forecast_max_horizon || a.t_first < 0 || !a.skill) return hipErrorInvalidValue;
    const long chunks = forecast_chunks(a.T);
    if (chunks > 1 && !a.partial) return hipErrorInvalidValue;
    hipError_t e;
    if (a.N <= 8) e = launch_skill<8>(a, s);
    else if (a.N <= 16) e = launch_skill<16>(a, s);
    else if (a.N <= 32) e = launch_skill<32>(a, s);
    else e = launch_skill<64>(a, s);
    if (e != hipSuccess || chunks == 1) return e;
    const long cells = a.B * a.N * a.H, blocks = (cells + 255) / 256;
    if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
    hipLaunchKernelGGL(forecast_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

} // namespace mk
