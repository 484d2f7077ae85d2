// score_kernels.h -- per-step scores of the objective by the tangent (forward-mode) filter and their sums (score_kernels.hip):
// argument blocks shared with the C ABI.  The gain tape is the one of weights_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int score_max_states = 64; // n = N + K served by score_tangent_kernel (one state per lane, one parameter per state)

struct ScoreArgs {
    long B, R, T;
    int N, K;
    long t_first;            // a step is counted when t >= t_first and it holds an observation
    long bs, ts, rs;         // filtered records: (b, t) at (b*bs + t*ts)*rs doubles; the tape, v and score use the same (bs, ts)
    long gs;                 // gain tape: cell (b, t, j) at ((b*bs + t*ts)*N + j)*gs doubles
    long obs_bs, obs_ts;     // observations: record (r, t) at row r*obs_bs + t*obs_ts
    const double *obs, *phi, *q, *loadings, *obsvar, *x0, *P0; // as in mk_problem (q and obsvar are in the tape already: not read)
    const double *F;         // filtered record array written by the recording forward pass
    const double *gain;      // gain tape written by innov_step_kernel, zero at the cells that are not observed
    const double *v;         // innovations written by innov_step_kernel: cell (b, t, j) at (b*bs + t*ts)*N + j, NaN where not observed
    const double *dphi, *dq; // [B,n]: d phi_p / d theta_p and d q_p / d theta_p
    double *score;           // [B,T,n] in the (bs, ts) layout: s_t,p at (b*bs + t*ts)*n + p
    double *grad;            // [B,n]
    int64_t *count;          // [B]
    double *opg;             // [B,n,n]
    double *cusum;           // [B,n,n]
};

hipError_t launch_score_tangent(const ScoreArgs &a, hipStream_t s);
hipError_t launch_score_stats(const ScoreArgs &a, hipStream_t s);

} // namespace mk
