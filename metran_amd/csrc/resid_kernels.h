// resid_kernels.h -- residual diagnostics of the standardised innovations (resid_kernels.hip): per-series moments, variance
// thirds and CUSUM excursions, and the lagged cross-series sums.  Argument blocks shared with the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int resid_max_series = 64; // N served by resid_cross_kernel (a lane per series of a row of pairs)
constexpr int resid_max_lags = 32;   // L of resid_cross_kernel: the halo of its tile (= innov_max_lags)
constexpr int resid_stats = 12;      // doubles per (instance, series) row of resid_series_kernel

struct ResidSeriesArgs {
    long B, T;
    int N;
    long bs, ts;             // cell (b, t, j) at (b*bs + t*ts)*N + j
    long t_first;
    const double *v, *f;
    double *stats;           // [B,N,12] = [m, mean, S2, S3, S4, h, ss_first, ss_last, cusum, cusum_t, cusq, cusq_t]
};

struct ResidCrossArgs {
    long B, T;
    int N, L;
    long bs, ts;
    long t_first;
    const double *v, *f;
    const double *stats;     // [B,N,12] as written by resid_series_kernel
    long long *counts;       // [B,L+1,N,N]: n_ij(l)
    double *sums;            // [B,L+1,N,N]: s_ij(l)
};

hipError_t launch_resid_series(const ResidSeriesArgs &a, hipStream_t s);
hipError_t launch_resid_cross(const ResidCrossArgs &a, hipStream_t s);

} // namespace mk
