// innov_kernels.h -- one-step-ahead innovations and their whiteness statistics (innov_kernels.hip): argument blocks shared
// with the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int innov_max_states = 64; // n = N + K served by innov_step_kernel (one wavefront per (instance, step))
constexpr int innov_max_lags = 32;   // L of innov_stats_kernel

struct InnovArgs {
    long B, R, T;
    int N, K;
    long bs, ts, rs;         // filtered records: (b, t) at (b*bs + t*ts)*rs doubles, rs = record_stride(n); the outputs' rows
                             // of N doubles use the same (bs, ts)
    long obs_bs, obs_ts;     // observations: record (r, t) at row r*obs_bs + t*obs_ts
    const double *obs, *phi, *q, *loadings, *obsvar, *x0, *P0, *scale, *offset; // as in mk_problem
    const double *F;         // filtered record array written by the recording forward pass
    double *v, *f;           // innovation and its variance of every observed cell (NaN elsewhere), or NULL
    double *pred_mean, *pred_var; // marginal one-step-ahead forecast of every series, or NULL
    double *gain;            // gain tape (weights_kernels.h), or NULL: per (b, t, j) one slot [ d = P z_j' (n) | 1/f | pad ] of gs doubles
    long gs;                 // at ((b*bs + t*ts)*N + j)*gs, written for the observed cells only (the caller clears the tape)
};

struct InnovStatsArgs {
    long B, T;
    int N, L;
    long bs, ts;             // cell (b, t, j) at (b*bs + t*ts)*N + j
    long t_first;
    const double *v, *f;
    double *stats;           // [B,N,4+L] = [m, mean, c_0, Q, r_1 .. r_L]
};

hipError_t launch_innov_step(const InnovArgs &a, hipStream_t s);
hipError_t launch_innov_stats(const InnovStatsArgs &a, hipStream_t s);

} // namespace mk
