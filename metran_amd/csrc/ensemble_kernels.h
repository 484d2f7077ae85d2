// ensemble_kernels.h -- window statistics of posterior draws (ensemble_kernels.hip): argument blocks shared with the C ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mk {

constexpr int path_functional_count = 5; // mean, min, max, fraction below, longest spell
constexpr int ensemble_max_draws = 4096; // the cell's values are sorted in LDS: 32 KiB of doubles per block
constexpr int ensemble_max_probs = 16;

struct PathFunctionalArgs {
    long SB, B, R, T;        // paths (draws * instances), instances of the caller's problem, its records, steps
    int Wd;                  // row width: N (series) or n (states)
    int time_major;          // paths stored [T,SB,Wd] instead of [SB,T,Wd]
    long W;                  // windows per record
    const double *paths;
    const int64_t *windows;  // [R,W,2] half-open step ranges, sorted and not overlapping
    const double *thresholds; // [R,Wd] or NULL
    double *out;             // [SB,Wd,W,5]
};

struct EnsembleSummaryArgs {
    long S, cells;
    int nprobs;
    double probs[ensemble_max_probs];
    const double *values;    // [S,cells]
    double *out;             // [cells, 5 + nprobs]
};

hipError_t launch_path_functionals(const PathFunctionalArgs &a, hipStream_t s);
hipError_t launch_ensemble_summary(const EnsembleSummaryArgs &a, hipStream_t s);

} // namespace mk
