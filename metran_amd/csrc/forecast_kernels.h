// forecast_kernels.h -- multi-step-ahead forecasts and forecast skill by horizon (forecast_kernels.hip): argument block shared
// with the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int forecast_max_states = 64;  // n = N + K served (one lane per series, N <= 63)
constexpr int forecast_max_horizon = 32; // H of the fan and of the skill table
constexpr int kForecastChunk = 32;       // consecutive origins per lane group of forecast_skill_kernel
constexpr int kForecastBlock = 8;        // horizons per lane group of forecast_skill_kernel: 6 x 8 sums stay in registers

// doubles per (instance, step) of the workspace behind the records: the per-(instance, chunk) partial sums [N,H,6] of a call with
// more than one chunk (T > kForecastChunk, so ceil(T / kForecastChunk) <= 2 T / kForecastChunk) fit in T of them
constexpr long forecast_partial_stride(long N) { return (2L * N * forecast_max_horizon * 6 + kForecastChunk - 1) / kForecastChunk; }

struct ForecastArgs {
    long B, R, T;
    int N, K, H;             // H: horizons of the fan and of the skill table
    long track_h, t_first;
    long bs, ts, rs;         // filtered records: (b, t) at (b*bs + t*ts)*rs doubles; the track's rows of N doubles use the same (bs, ts)
    long obs_bs, obs_ts;     // observations: record (r, t) at row r*obs_bs + t*obs_ts
    double z2;               // coverage_z^2
    const double *obs, *phi, *q, *loadings, *obsvar, *x0, *P0, *scale, *offset; // as in mk_problem
    const double *F;         // filtered record array written by the recording forward pass
    const int64_t *fan_origins;    // [R] or NULL (T - 1)
    double *fan_mean, *fan_var;     // [B,H,N] or NULL
    double *track_mean, *track_var; // [B,T,N] / [T,B,N] or NULL
    double *skill;           // [B,N,H,6] or NULL
    double *partial;         // [B,chunks,N,H,6]: read and written only when there is more than one chunk
};

__host__ __device__ inline long forecast_chunks(long T) { return (T + kForecastChunk - 1) / kForecastChunk; }

hipError_t launch_forecast_path(const ForecastArgs &a, hipStream_t s);  // fan and / or track
hipError_t launch_forecast_skill(const ForecastArgs &a, hipStream_t s); // skill (+ the reduction over the chunks)

} // namespace mk
