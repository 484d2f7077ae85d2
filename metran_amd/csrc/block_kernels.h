// block_kernels.h -- leave-block-out predictions (block_kernels.hip): argument block shared with the C ABI.  The gain tape is the
// one of weights_kernels.h, the innovations are the scores' row behind it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int block_max_states = 64; // n = N + K served by the two kernels (one state per lane)
constexpr int block_max_cells = 64;  // L: the steps of a block, one block cell per lane of a wavefront

struct BlockArgs {
    long B, R, T, W, L;      // W blocks per record, L = row length of means / vars
    int N, K;
    long bs, ts;             // block (b, t) of the workspace at b*bs + t*ts
    long gs;                 // gain tape: cell (b, t, j) at ((b*bs + t*ts)*N + j)*gs doubles
    long obs_bs, obs_ts;     // observations: record (r, t) at row r*obs_bs + t*obs_ts
    const double *obs, *phi, *q, *loadings, *obsvar, *x0, *P0; // as in mk_problem (q, x0 and P0 are in the tape already: not read)
    const double *scale, *offset;
    const double *gain;      // gain tape written by innov_step_kernel, zero at the cells that are not observed
    const double *v;         // innovations written by innov_step_kernel: cell (b, t, j) at (b*bs + t*ts)*N + j, NaN where not observed
    const int64_t *blocks;   // [R,W,3] = (series, t0, t1); instance b uses the blocks of record b % R
    double *checkpoints;     // [B,W,n + n*n]: (r, N) behind step t1 of the block
    double *means, *vars;    // [B,W,L]
    double *summary;         // [B,W,4] = (m, quad, log det V, 1'V1 / m^2 * scale^2)
    uint32_t *flags;         // [B,W]
};

hipError_t launch_block_checkpoint(const BlockArgs &a, hipStream_t s);
hipError_t launch_block_walk(const BlockArgs &a, hipStream_t s);

} // namespace mk
