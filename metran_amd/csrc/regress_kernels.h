// regress_kernels.h -- intervention effects by GLS (regress_kernels.hip): argument blocks shared with the C ABI.  The gain tape
// is the one of weights_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int regress_max_states = 64;  // n = N + K served by regress_replay_kernel (one state per lane)
constexpr int regress_max_effects = 16; // M: one effect per lane of a 16-lane group
constexpr double regress_min_pivot = 1e-12; // an effect whose Cholesky pivot in the unit-diagonal matrix is below this is dropped

struct RegressArgs {
    long B, R, T, M;
    int N, K;
    long t_first;            // the cells of the steps t >= t_first are counted in the sums
    long bs, ts;             // block (b, t) of the workspace at b*bs + t*ts
    long gs;                 // gain tape: cell (b, t, j) at ((b*bs + t*ts)*N + j)*gs doubles
    long obs_bs, obs_ts;     // observations: record (r, t) at row r*obs_bs + t*obs_ts
    const double *obs, *phi, *q, *loadings, *obsvar, *x0, *P0; // as in mk_problem (q, obsvar and P0 are in the tape already: not read)
    const double *gain;      // gain tape written by innov_step_kernel, zero at the cells that are not observed
    const int64_t *effects;  // [R,M,4] = (series, kind, t0, t1); instance b uses the effects of record b % R
    double *beta;            // [B,M]
    double *cov;             // [B,M,M]
    double *gainout;         // [B]  s' S^-1 s, the drop of -2 log L
    double *normal;          // [B,M+1,M+1]  A
    int64_t *support;        // [B,M]
    uint32_t *dropped;       // [B]
};

struct RegressAdjustArgs {
    long R, T, M;
    int N;
    long bs, ts;             // row (r, t) of N doubles at r*bs + t*ts
    const int64_t *effects;  // [R,M,4]
    const double *beta;      // [R,M]
    const double *in;
    double *out;
};

hipError_t launch_regress_replay(const RegressArgs &a, hipStream_t s);
hipError_t launch_regress_adjust(const RegressAdjustArgs &a, hipStream_t s);

} // namespace mk
