// reader_prims.h -- device helpers shared by the kernels that forecast the series from the filtered records (innov_kernels.hip,
// forecast_kernels.hip): one spelling of what the two must agree on bit for bit (a track of horizon 1 is pred_mean / pred_var).
#pragma once
#include <hip/hip_runtime.h>

namespace mk {

// a forecast's mean and variance in the caller's units (mk_problem's scale / offset); a variance that rounding took below zero
// is stored as zero
__device__ __forceinline__ double scaled_mean(double pm, double sc, double of) { return fma(pm, sc, of); }
__device__ __forceinline__ double scaled_var(double pv, double sc) { return (pv < 0.0 ? 0.0 : pv) * sc * sc; }

} // namespace mk
