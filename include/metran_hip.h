/*
 * metran_hip.h -- C ABI of libmetran_hip.so: the MI355X (gfx950) batched Kalman filter,
 * -2 log-likelihood and RTS smoother for Metran's dynamic-factor model.
 *
 * This is the drop-in boundary for the hot path of pastas/metran.
 * The reference has no FFI of its own: its "engine" is a Python callable
 *     SPKalmanFilter.filtermethod(obs, Phi, Q, Z, R, idx, count, x0, P0) -> 7-tuple
 *         /root/reference/metran/kalmanfilter.py:494-504 (binding), :761-771 (call site)
 *     kalmansmoother(F, Pf, Xp, Pp, Phi) -> (S, Ps)
 *         metran/kalmanfilter.py:685-691 (call site), :403-476 (definition)
 *     SPKalmanFilter.get_mle(warmup)            metran/kalmanfilter.py:550-567
 *     SPKalmanFilter.simulate / decompose       metran/kalmanfilter.py:569-644
 *     Metran._get_matrices(p)                   metran/metran.py:246-416
 * Each entry point below names the reference function it replaces.  Python binds this
 * header with ctypes (metran_amd/_lib.py); INTEGRATION.md shows the stub a Metran
 * maintainer would add.
 *
 * Conventions
 *   - extern "C", plain pointers and sizes; no C++ exceptions cross the ABI.
 *   - every function returns 0 (MK_OK) or a negative mk_status; mk_last_error() gives text.
 *   - "d_" pointers are DEVICE pointers (hipMalloc / torch.Tensor.data_ptr()); "h_" are host.
 *   - all launches are asynchronous on the context's stream (mk_set_stream / mk_sync).
 *   - layouts are the reference's, with a leading batch axis, row-major double:
 *       obs [R,T,N] (NaN or +-inf = missing), phi/q [B,n], loadings [R,N,K], obsvar [R,N],
 *       F/Xp/S [B,T,n], Pf/Pp/Ps [B,T,n,n], sigmas/detfs [B,T], n = N + K;
 *     optionally TIME-MAJOR ([T,B,...], mk_outputs.time_major / mk_problem.obs_time_major): the
 *     same per-model [T,...] arrays, interleaved so that one time step of all models is contiguous.
 *     B = number of filter instances, R = number of observation records; instance i reads
 *     record i % R (so the P+1 finite-difference evaluations of one model, or S parameter sets
 *     per model, share one uploaded observation record).
 *   - state order: N specific factors then K common factors (metran/metran.py:283-290).
 *   - the model is Metran's: Phi = diag(phi), Q = diag(q), Z = [I_N | loadings], R = diag(obsvar).
 */
#ifndef METRAN_HIP_H
#define METRAN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MK_API __attribute__((visibility("default")))
#define MK_ABI_VERSION 7

typedef enum mk_status {
    MK_OK = 0,
    MK_ERR_INVALID = -1,     /* bad argument (null pointer, negative size, ...) */
    MK_ERR_SHAPE = -2,       /* (N,K) is not served, or not in the asked-for mode (see mk_shape_supported) */
    MK_ERR_HIP = -3,         /* a HIP runtime call failed */
    MK_ERR_NO_DEVICE = -4,   /* no gfx950 device visible */
    MK_ERR_ALLOC = -5
} mk_status;

/* per-instance status bits written to mk_outputs.d_status */
#define MK_FLAG_NONPOSITIVE_F 1u /* ERROR: an innovation variance f <= 0, or a NaN one, was met in the filter (anywhere in the
                                    record, the warm-up included), or the filtered state ended NaN (a NaN x0, say, with every f
                                    positive).  The instance's d_mle is then NaN -- never a finite number: the
                                    reference's log f is NaN there (kalmanfilter.py:378) -- and its other outputs are unspecified */
#define MK_FLAG_NOT_SPD 2u       /* ERROR: predicted covariance indefinite in the smoother (an LDL^T
                                    pivot < -1e-8); the smoothed moments of that instance are invalid */
#define MK_FLAG_RANK_DEFICIENT 4u /* INFO: a pivot <= 0 was met and that null direction dropped, as
                                    numpy.linalg.pinv does in the reference (kalmanfilter.py:455): q_i = 0
                                    for a series with communality 1 (metran.py:314-316).  Results valid.
                                    A NaN pivot sets NEITHER pivot bit, in every smoother (both comparisons are false; 1/d := 0):
                                    NaN moments in give NaN moments out, and filtered moments that are NaN come from a filter
                                    that has set MK_FLAG_NONPOSITIVE_F for the instance. */

typedef struct mk_context mk_context; /* opaque; one per (process, device) */

/* Inputs of one batched evaluation.  Replaces the 9 positional arguments of
 * seqkalmanfilter (metran/kalmanfilter.py:243-253) for B models at once. */
typedef struct mk_problem {
    int64_t n_instances; /* B */
    int64_t n_records;   /* R, 1 <= R <= B */
    int64_t T, N, K;
    int64_t warmup;            /* get_mle(warmup), metran/kalmanfilter.py:550; Metran uses 1 */
    const double *d_obs;       /* [R,T,N]  observations, NaN/inf = missing (kalmanfilter.py:657); read by the filters and, to tell
                                  the fully observed steps, by mk_smooth / mk_filter_smooth (see mk_smooth) */
    const double *d_phi;       /* [B,n]    diag of transition_matrix      (metran.py:283-290) */
    const double *d_q;         /* [B,n]    diag of transition_covariance  (metran.py:310-322) */
    const double *d_loadings;  /* [R,N,K]  observation_matrix[:, N:]      (metran.py:365-370) */
    const double *d_obsvar;    /* [R,N] or NULL = zeros                   (metran.py:382-384) */
    const double *d_x0;        /* [B,n] or NULL = zeros       (kalmanfilter.py:747-748) */
    const double *d_P0;        /* [B,n,n] or NULL = identity  (kalmanfilter.py:749-750) */
    int64_t obs_time_major;    /* 0: d_obs is [R,T,N] (reference layout); 1: d_obs is [T,R,N] */
    const double *d_scale;     /* [R,N] or NULL = ones: series standard deviations (Metran.oseries_std); with
                                  d_offset the scaled observation matrix of get_scaled_observation_matrix
                                  (metran.py:944-961) for the fused projection outputs d_sim_means/d_sim_vars */
    const double *d_offset;    /* [R,N] or NULL = zeros: series means (metran.py:788-793)              */
} mk_problem;

/* Outputs; any pointer may be NULL (that output is skipped and costs no HBM traffic).
 * Replaces the returned 7-tuple of seqkalmanfilter (kalmanfilter.py:392-400), the 2-tuple of
 * kalmansmoother (:476) and get_mle (:566). */
typedef struct mk_outputs {
    double *d_mle;         /* [B]   -2 log L with warm-up skip                  (:563-566) */
    double *d_sigmas;      /* [B,T] compressed, zero-filled tail                (:380-382) */
    double *d_detfs;       /* [B,T] compressed, zero-filled tail                           */
    int64_t *d_sigmacount; /* [B]                                                          */
    double *d_F;           /* [B,T,n]   filtered_state_means                    (:389)     */
    double *d_Pf;          /* [B,T,n,n] filtered_state_covariances              (:390)     */
    double *d_Xp;          /* [B,T,n]   predicted_state_means                   (:332)     */
    double *d_Pp;          /* [B,T,n,n] predicted_state_covariances             (:333)     */
    double *d_S;           /* [B,T,n]   smoothed_state_means                    (:461-464) */
    double *d_Ps;          /* [B,T,n,n] smoothed_state_covariances              (:465-474) */
    uint32_t *d_status;    /* [B] MK_FLAG_* bits, or NULL                                  */
    int64_t time_major;    /* 0: per-step arrays are [B,T,...] (reference layout with a leading batch
                              axis); 1: they are [T,B,...] -- all models' step-t blocks contiguous, the
                              HBM-friendly layout (a [B,T,...] strided view of it costs nothing).
                              Applies to d_sigmas, d_detfs, d_F, d_Pf, d_Xp, d_Pp, d_S, d_Ps.        */
    double *d_sim_means;   /* [B,T,N] fused projection epilogue of the smoother (mk_smooth /          */
    double *d_sim_vars;    /* [B,T,N] mk_filter_smooth, record layout): SPKalmanFilter.simulate
                              (kalmanfilter.py:569-603) of the SMOOTHED moments with Z~ = diag(scale)
                              [I | loadings] (+ offset on the means) -- what Metran.get_simulation consumes
                              (metran.py:831-883).  With these set, d_S / d_Ps (and d_Xp / d_Pp) may be
                              NULL: the smoothed states are then never written (7x less output at n = 10,
                              40x at n = 36).  time_major applies.  NULL = not computed.              */
    int64_t record_stride; /* 0: every array above is dense.  RS = mk_record_stride(n): PACKED RECORDS, the
                              fast path.  Each moment set is ONE array of RS doubles per (model, step):
                                [ mean(n) | covariance(n*n) | sigma, detf (filtered set only) | zero pad ]
                              and the pointers are views into it: d_Pp = d_Xp + n, d_Pf = d_F + n,
                              d_Ps = d_S + n, d_sigmas = d_F + n + n*n, d_detfs = d_sigmas + 1 (or NULL);
                              element (b,t) of any of them sits RS doubles after element (b,t)-1 of the
                              layout chosen by time_major.  RS*8 is a multiple of 128 bytes: all stores of
                              the kernels then cover whole cache lines (partial-line stores of the small
                              vectors were measured to throttle HBM writes).  mk_filter uses records when
                              the predicted AND filtered sets are both requested this way; mk_smooth when
                              d_F (and d_S) are record arrays.                                         */
    int64_t flags;         /* MK_OUT_* bits (0 = none):
                              MK_OUT_PACKED_SYM  the records are PACKED-SYMMETRIC: RS = mk_record_stride_sym(n),
                                [ mean(n) | upper triangle by rows, n(n+1)/2 | sigma, detf | zero pad ],
                                640 B instead of 896 B per (model, step) at n = 10, 5632 B instead of 10752 B at
                                n = 36 (c_s = n + n(n+1)/2).  Pointer conventions as for
                                records with n*n replaced by n(n+1)/2: d_Pf = d_F + n, d_sigmas = d_F + n +
                                n(n+1)/2, ...  Element (r,c), r <= c, of a covariance sits at
                                r*n - r(r-1)/2 + (c - r) of its triangle.  Requires record_stride != 0.
                              MK_OUT_VAR_ONLY    mk_smooth / mk_filter_smooth write the smoothed state MEANS to
                                d_S [B,T,n] and the smoothed state VARIANCES (diagonals of the covariances) to
                                d_Ps [B,T,n], both dense (time_major applies), instead of smoothed records --
                                what Metran.get_state_means / get_state_variances / get_state consume
                                (metran.py:655-756).  d_F/d_Pf stay a (full or packed-symmetric) record array;
                                d_Xp/d_Pp must be NULL in mk_filter_smooth (filtered record only).
                              MK_OUT_TAPE        (ABI 5; mk_filter_smooth with d_sim_means / d_sim_vars only, shapes
                                with mk_tape_supported(N, K) = 1) d_F is not a filtered record array
                                but the BACKWARD TAPE of the inverse-free smoother, record_stride =
                                mk_tape_stride(N, K) = N (n + 4) doubles per (model, step), same (b, t) addressing
                                and time_major rule as records: per series one entry [ vector(n) | s0 | s1 | s2 | 0 ]
                                in the observable basis -- the gain, v/f, 1/f and the observation of an observed
                                series, T Pf z_u', the filtered observable, its variance and NaN for a series not
                                observed at that step.  The backward pass (Durbin-Koopman r / N recursion of the
                                sequential filter, kalmanfilter.py:341-378 walked backwards) then produces the same
                                projected smoothed means / variances as kalmansmoother + simulate (:403-476,
                                :569-603) without the pseudo-inverse of :455.  d_Pf, d_Xp, d_Pp, d_S, d_Ps must be
                                NULL; d_sigmas / d_detfs, if given, are DENSE [B,T] arrays.
                              MK_OUT_TAPE | MK_OUT_VAR_ONLY   (ABI 6; mk_filter_smooth, d_obsvar = NULL) the STATE tape:
                                record_stride = mk_state_tape_stride(N, K) = (N + K)(n + 4) doubles per (model, step) --
                                the N series entries above followed by K entries [ T Pf e_{N+k} (n) | x_f[N+k] |
                                Pf[N+k][N+k] | NaN | 0 ], the factor columns of the filtered covariance in the observable
                                basis.  The same backward pass then also writes the smoothed state MEANS to d_S [B,T,n]
                                and VARIANCES to d_Ps [B,T,n] (kalmansmoother's S and diag(Ps), :461-474; what
                                get_state_means / get_state_variances / get_state consume, metran.py:655-756) with no
                                filtered record, no LDL^T of the predicted covariance and no n x n product.
                                d_sim_means / d_sim_vars are optional; d_Pf, d_Xp, d_Pp must be NULL.             */
} mk_outputs;
#define MK_OUT_PACKED_SYM 1
#define MK_OUT_VAR_ONLY 2
#define MK_OUT_TAPE 4

/* ---- library / context ------------------------------------------------------------------ */
MK_API int mk_abi_version(void);
MK_API const char *mk_last_error(void);
MK_API int mk_device_count(int *count);
MK_API int mk_create(int device, mk_context **ctx);
MK_API int mk_destroy(mk_context *ctx);
/* Use an existing hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = default. */
MK_API int mk_set_stream(mk_context *ctx, void *hip_stream);
MK_API int mk_sync(mk_context *ctx);
/* Two shape classes have a second, equivalent kernel kept for A/B measurements (both tested against the oracle:
 * tests/test_smoother_variants.py, tests/test_hip_parity.py).  value 0 = the default.  There is no environment
 * variable and no switch that changes results.
 *   MK_VARIANT_SMOOTHER16     n <= 15, packed records: 0 smoother_record_kernel (DPP), 1 smoother_blk_kernel (4x4x4 MFMA),
 *                             2 smoother_record_kernel with the general covariance products at EVERY step: without it, for
 *                             n <= 10, full-square records, no epilogue and d_obsvar == NULL, a step at which the model observed
 *                             all N series (read from prob->d_obs) takes the rank-K form of the same products
 *   MK_VARIANT_WIDE_SMOOTHER  n > 16: 0 the blocked MFMA smoother (n <= 36: rows of A folded into the idle lanes),
 *                             1 smoother_wave_kernel (round 1, row per lane; built for n <= 51, MK_ERR_SHAPE above),
 *                             2 the MFMA smoother without the fold
 *   MK_VARIANT_WIDE_FILTER    n > 16, N <= 32: 0 by batch size -- filter_split_kernel (series on the lanes, factor block
 *                             replicated: 2 or 4 models per wavefront) for more than 2 instances per SIMD of the device,
 *                             filter_wave_kernel<N,K> (one state per lane) below; 1 the latter always; 2 the former always
 *                             (the MK_OUT_TAPE path always runs the split kernel: the tape exists in that layout only)
 *   MK_VARIANT_SINGLE_RECORD  mk_filter with ONE record, at most MK_SPARSE_RECORD_MAX_INSTANCES instances, n <= 16 and both record
 *                             sets (the 7-tuple of seqkalmanfilter for a single Metran model): 0 the observed steps walked one
 *                             after the other and the records of the empty steps written in closed form by a second, parallel
 *                             kernel (kalmanfilter.py:335 skips the update on those steps; examples/data: 343 of 6255 steps
 *                             carry data), 1 the batched filter_kernel step by step
 *   MK_VARIANT_KERNEL_FAMILY  0 the specialised kernels where a shape has them, 1 the size-generic kernels (mk_generic.hip) for EVERY
 *                             shape (mk_filter / mk_loglik / mk_smooth / mk_filter_smooth with dense arrays or full-square records):
 *                             the second, independent implementation of the same recursions, for cross-checks and for timing
 *                             what specialisation buys
 *   MK_VARIANT_TAPE_FILTER    the writer of the backward tape (MK_OUT_TAPE), 16 < n, N <= 32: 0 filter_obs_kernel -- the filter run in the
 *                             observable basis, where gains and columns ARE the tape's entries (round 6) --, 1 filter_split_kernel OUT = 4
 *                             (state basis, every entry converted: round 4).  Same tape, same objective */
enum { MK_VARIANT_SMOOTHER16 = 0, MK_VARIANT_WIDE_SMOOTHER = 1, MK_VARIANT_WIDE_FILTER = 2, MK_VARIANT_SINGLE_RECORD = 3,
       MK_VARIANT_KERNEL_FAMILY = 4, MK_VARIANT_TAPE_FILTER = 5, MK_VARIANT_COUNT = 6 };
#define MK_SPARSE_RECORD_MAX_INSTANCES 16
MK_API int mk_set_kernel_variant(mk_context *ctx, int which, int value);
MK_API int mk_get_kernel_variant(mk_context *ctx, int which, int *value);
/* Tell the context that the CONTENTS of an observation buffer it has seen changed in place (same pointer): per-record
 * data derived from it (the observed-step list of the sparse objective, see mk_loglik; which records the record smoother's
 * rank-K covariance step is taken for, and whether EVERY step of EVERY record is full, in which case mk_smooth /
 * mk_filter_smooth run a form of the kernel that never looks at the observations) is rebuilt on the next call.
 * Not needed when a different buffer is passed. */
MK_API int mk_observations_changed(mk_context *ctx);
/* 1 if the library serves (N,K): a SPECIALISED kernel (compiled ahead of time, or a registered shape module: N + K <= 64,
 * fully unrolled over the state dimension -- the fast path) or, for every other shape with N + K <= mk_generic_max_states()
 * (= 128), the SIZE-GENERIC kernels of mk_generic.hip (one model per workgroup, covariance in LDS; correct for any shape,
 * tuned for none: the reference's loops are size-generic too, kalmanfilter.py:315-390, 453-474).  mk_shape_specialised tells
 * which.  Generic shapes run mk_filter / mk_loglik / mk_smooth / mk_filter_smooth with dense arrays or full-square records,
 * projection and MK_OUT_VAR_ONLY outputs; they have no packed-symmetric records, no tape and no adjoint gradient
 * (MK_ERR_SHAPE). */
MK_API int mk_shape_supported(int64_t N, int64_t K);
MK_API int mk_shape_specialised(int64_t N, int64_t K);
MK_API int64_t mk_generic_max_states(void);
/* Register a run-time shape module: a shared object built from metran_amd/csrc/mk_kernels.hip with
 * -DMK_SHAPE_MODULE '-DMK_SHAPES(X)=X(N,K)' (hipcc --offload-arch=gfx950).  The kernels are fully
 * unrolled over the state dimension, so a model shape outside the ahead-of-time list gets its own
 * specialised kernels this way (metran_amd/jit.py compiles, hazard-checks and caches them). */
MK_API int mk_register_shape_module(const char *path);
/* Doubles per packed record (see mk_outputs.record_stride) for state dimension n = N + K. */
MK_API int64_t mk_record_stride(int64_t n);
/* ... per PACKED-SYMMETRIC record (mk_outputs.flags & MK_OUT_PACKED_SYM). */
MK_API int64_t mk_record_stride_sym(int64_t n);
/* Doubles per (model, step) of the backward tape (mk_outputs.flags & MK_OUT_TAPE): N (N + K + 4); and whether the
 * tape path serves a shape (a specialised shape with 16 < N + K <= 63 -- the backward pass keeps the rows of its n x n matrix and
 * one more on the 64 lanes; written by the split filter of mk_split.hip for N <= 32 and by the lane-per-state filter beyond,
 * read by mk_dk.hip). */
MK_API int64_t mk_tape_stride(int64_t N, int64_t K);
MK_API int mk_tape_supported(int64_t N, int64_t K);
/* ... of the STATE tape (MK_OUT_TAPE | MK_OUT_VAR_ONLY): (N + K)(N + K + 4); served for the same shapes. */
MK_API int64_t mk_state_tape_stride(int64_t N, int64_t K);
/* Writes up to `cap` supported (N,K) pairs into shapes[2*i], shapes[2*i+1]; returns the count. */
MK_API int mk_supported_shapes(int64_t *shapes, int cap);

/* ---- device memory helpers (for hosts without torch) -------------------------------------- */
MK_API int mk_malloc(mk_context *ctx, size_t bytes, void **d_ptr);
MK_API int mk_free(mk_context *ctx, void *d_ptr);
MK_API int mk_memcpy_h2d(mk_context *ctx, void *d_dst, const void *h_src, size_t bytes);
MK_API int mk_memcpy_d2h(mk_context *ctx, void *h_dst, const void *d_src, size_t bytes);
MK_API int mk_memset(mk_context *ctx, void *d_dst, int value, size_t bytes);

/* ---- the hot path --------------------------------------------------------------------------- */
/* Metran._get_matrices restricted to the diagonals (metran/metran.py:246-322):
 *   phi = exp(-dt/alpha);  q_i = (1-phi_i^2)(1 - sum_k loadings[i,k]^2) for i<N, 1-phi_i^2 else.
 * Instance b uses d_loadings[b % R].  K = 0 (no common factor) is served, and d_loadings may then be NULL. */
MK_API int mk_params_from_alpha(mk_context *ctx, int64_t B, int64_t R, int64_t N, int64_t K,
                                const double *d_alpha /* [B,n] */,
                                const double *d_loadings /* [R,N,K] */, double dt,
                                double *d_phi /* [B,n] */, double *d_q /* [B,n] */);

/* kalmansmoother in its literal 5-argument form for B models (kalmanfilter.py:403-476: filtered_state_means [B,T,n],
 * filtered_state_covariances [B,T,n,n], predicted_state_means, predicted_state_covariances, diag of transition_matrix [B,n])
 * -> d_S [B,T,n], d_Ps [B,T,n,n] (either may be NULL).  The predicted moments are READ, not recomputed (:454-474 use
 * predicted_state_covariances[t+1] and predicted_state_means[t+1] as handed in), so no transition covariance is needed and a
 * caller's own predicted moments are honoured.  Size-generic kernel (mk_generic.hip), n <= mk_generic_max_states(); dense
 * model-major arrays.  The fast path for moments that came out of mk_filter is mk_smooth / mk_filter_smooth. */
MK_API int mk_smooth_dense(mk_context *ctx, int64_t B, int64_t T, int64_t n, const double *d_phi, const double *d_F,
                           const double *d_Pf, const double *d_Xp, const double *d_Pp, double *d_S, double *d_Ps,
                           uint32_t *d_status);

/* ---- lock-step L-BFGS of the batched calibration (mk_lbfgs.hip) ----------------------------------
 * What ScipySolve.solve leaves to scipy's L-BFGS-B for ONE model (metran/solver.py:222-305: bounds alpha >= pmin, m history pairs,
 * pgtol on the projected gradient, ftol on the relative reduction) for R models at once, one thread per model.  Arrays are [R,n]
 * row-major doubles; every model has its own history ring d_Sh / d_Yh [history,R,n], d_rho [history,R] with d_hlen [R] live pairs
 * starting at slot d_hpos [R] (int32); masks are bytes.  A host pointer h_*, if given, receives the kernel's count after a stream
 * synchronisation (NULL: asynchronous).
 *   mk_lbfgs_direction  projected gradient d_pg, d_active &= max|pg| > gtol, two-loop recursion, steepest descent where the
 *                       direction is not a descent direction, unit-scale first step, zero on active bounds -> d_d; #active.
 *                       With d_phase / d_step / d_nback (own line search per model): a model with phase 1 keeps direction and step,
 *                       the others start a new search (step 1, nback 0, phase 1)
 *   mk_lbfgs_trial      d_xt = max(x + step d, lo); d_xe = searching ? xt : x_new
 *   mk_lbfgs_armijo     searching models: accept (x_new, f_new <- xt, ft) if ft <= f + 1e-4 pg.(xt - x) and ft finite, else
 *                       step *= clamp(parabola minimiser, 0.1, 0.5); #still searching.  Lock-step form (d_nback NULL): an
 *                       accepted model leaves d_searching.  Own-line-search form: d_accepted marks the accepted models (they stay
 *                       in d_searching = the active mask), a model that has used max_backtracks trial points leaves it; #accepted
 *   mk_lbfgs_update     for the models of d_mask (NULL: all): pair (s, y, rho) of the accepted point into the model's ring if
 *                       s.y > 1e-10 y.y (skipped otherwise, as scipy does), (x, f, g) <- new (lock-step form: models still in
 *                       d_searching keep their old gradient if asked and leave d_active), d_active &= relative reduction > ftol,
 *                       phase <- 0; #usable pairs.  d_nit [R] int32 (may be NULL): the quasi-Newton ITERATIONS every model has
 *                       taken -- incremented for each active model updated here -- and a model whose count reaches maxiter
 *                       (> 0) leaves d_active: scipy's maxiter (solver.py:248 passes it through) counts iterations of ONE
 *                       model, whatever the driver's loop counts */
MK_API int mk_lbfgs_direction(mk_context *ctx, int64_t R, int64_t n, int64_t history, const double *d_x, const double *d_g, const double *d_lo,
                              uint8_t *d_active, const double *d_Sh, const double *d_Yh, const double *d_rho, const int *d_hlen,
                              const int *d_hpos, double gtol, double *d_pg, double *d_d, uint8_t *d_phase, double *d_step, int *d_nback,
                              int *h_nactive);
MK_API int mk_lbfgs_trial(mk_context *ctx, int64_t R, int64_t n, const double *d_x, const double *d_d, const double *d_step,
                          const double *d_lo, const uint8_t *d_searching, const double *d_x_new, double *d_xt, double *d_xe);
MK_API int mk_lbfgs_armijo(mk_context *ctx, int64_t R, int64_t n, const double *d_ft, const double *d_f, const double *d_pg,
                           const double *d_xt, const double *d_x, uint8_t *d_searching, double *d_step, double *d_x_new,
                           double *d_f_new, int *d_nback, int64_t max_backtracks, uint8_t *d_accepted, int *h_nsearching,
                           int *h_naccepted);
MK_API int mk_lbfgs_update(mk_context *ctx, int64_t R, int64_t n, int64_t history, double *d_x, double *d_f, double *d_g,
                           const double *d_x_new, const double *d_f_new, const double *d_g_new, int keep_old_gradient_if_searching,
                           const uint8_t *d_searching, const uint8_t *d_mask, uint8_t *d_active, double ftol, double *d_Sh,
                           double *d_Yh, double *d_rho, int *d_hlen, int *d_hpos, uint8_t *d_phase, int *d_nit, int64_t maxiter,
                           int *h_ngood);

/* seqkalmanfilter + get_mle for B instances (kalmanfilter.py:236-400, 550-567).
 * Uses d_mle, d_sigmas, d_detfs, d_sigmacount, d_F, d_Pf, d_Xp, d_Pp, d_status of `out`. */
MK_API int mk_filter(mk_context *ctx, const mk_problem *prob, const mk_outputs *out);

/* -2 log L only: mk_filter with every state output NULL (the solver's objective,
 * Metran.get_mle, metran/metran.py:605-622).  d_mle [B] required.  There is no status argument: an instance that would carry
 * MK_FLAG_NONPOSITIVE_F (an innovation variance f <= 0 or NaN) returns a NaN d_mle, whatever the parity of its negative f's. */
MK_API int mk_loglik(mk_context *ctx, const mk_problem *prob, double *d_mle);
/* (When every instance shares ONE record -- n_records == 1, the solver's finite-difference points -- and
 * N+K <= 16, mk_loglik walks only the record's observed steps and applies the runs of empty steps in closed
 * form; real Metran records are sparse: examples/data observes 343 of 6255 daily steps.  The list of observed steps is
 * built once per record (pointer, shape, layout) and reused by the following calls: mk_observations_changed.) */

/* Objective AND its gradient in two launches (the reference has no gradient: scipy differences P+1
 * objective evaluations, metran/solver.py:248-255).  Forward: mk_filter writing only the filtered
 * records into d_work (n_instances*T*mk_record_stride(n) doubles; time_major as in mk_outputs);
 * backward: the adjoint kernel re-reads them once.  d_gphi / d_gq [B,n] receive
 * d(-2 log L)/d diag(Phi) and /d diag(Q); d_mle [B], d_sigmacount [B] as in mk_filter; d_status may be
 * NULL.  N+K <= 16: four models per wavefront (adjoint_kernel); 16 < N+K <= 64: one model per wavefront
 * (adjoint_wide_kernel, mk_split.hip) -- at configs[3]'s shape one gradient instead of 37 differenced filter runs. */
MK_API int mk_loglik_grad(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major,
                          double *d_mle, int64_t *d_sigmacount, double *d_gphi, double *d_gq,
                          uint32_t *d_status);
/* The two launches of mk_loglik_grad separately.  A line search evaluates the objective at several trial points and
 * needs the gradient at the accepted one only: with MK_GRAD_FORWARD every trial is the recording forward pass (d_mle,
 * d_sigmacount, d_status, the records in d_work; d_gphi / d_gq may be NULL), and MK_GRAD_BACKWARD then walks the records
 * the LAST forward pass left in d_work -- same prob (parameters included), same d_work, same d_sigmacount -- instead of
 * filtering the accepted point once more.  phases = MK_GRAD_FORWARD | MK_GRAD_BACKWARD is mk_loglik_grad. */
enum { MK_GRAD_FORWARD = 1, MK_GRAD_BACKWARD = 2 };
MK_API int mk_loglik_grad_phases(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major,
                                 double *d_mle, int64_t *d_sigmacount, double *d_gphi, double *d_gq,
                                 uint32_t *d_status, int phases);

/* Wide models (16 < N + K <= 64), optional: an UPDATE TAPE for the adjoint gradient (round 6).  mk_adjoint_update_stride(N, K)
 * doubles per (model, step) -- N slots [ d = P z_j' (n) | pad | 1/f, v ], one per scalar update of the step -- or 0 where the
 * shape has none (n <= 16: the 16-lane kernel recomputes).  With a caller-owned buffer of at least n_instances * T * stride
 * doubles on the context (mk_set_adjoint_updates; NULL detaches), the recording forward pass of mk_loglik_grad /
 * mk_loglik_grad_phases writes the slots (one model per wavefront, whatever the batch size) and the backward walk READS them
 * instead of recomputing every step from the filtered record of the step before -- 38 % of its instructions, and the walk is
 * one wavefront's dependent chain (512 x (32,4), T = 500: backward pass 12.8 -> see DESIGN.md section 6).  Same gradient to
 * rounding.  The buffer must stay valid and unchanged between the two phases of a gradient; too small a buffer for a call
 * is simply not used. */
MK_API int64_t mk_adjoint_update_stride(int64_t N, int64_t K);
MK_API int mk_set_adjoint_updates(mk_context *ctx, double *d_buf, int64_t capacity_doubles);
/* Chain rule of mk_params_from_alpha: d/dalpha = (gphi - 2 phi c gq) phi dt / alpha^2, c = 1 - sum_k
 * loadings^2 for the series, 1 for the factors (metran/metran.py:246-322).  As mk_params_from_alpha: instance b uses
 * d_loadings[b % R], and d_loadings may be NULL when K = 0. */
MK_API int mk_alpha_grad(mk_context *ctx, int64_t B, int64_t R, int64_t N, int64_t K,
                         const double *d_alpha /* [B,n] */, const double *d_loadings /* [R,N,K] */,
                         double dt, const double *d_gphi, const double *d_gq, double *d_galpha /* [B,n] */);

/* Leave-one-out predictions of every observed cell (the outlier screen of Metran's worked example: mask one observation,
 * re-smooth, read get_simulation at that cell -- here for all cells at once, parameters held fixed).  For the observed cell
 * (t, j) de Jong's deletion result on the backward quantities of the sequential filter gives
 *     d_loo_means[b,t,j] = E[y_tj | every other cell] * scale + offset,   d_loo_vars[b,t,j] = Var[z_j x_t | every other cell] * scale^2
 * (scale / offset: mk_problem.d_scale / d_offset; the variance is clipped at 0 as in the projection), NaN at a cell that is not
 * observed (mk_filter_smooth's projection serves those).  [B,T,N], or [T,B,N] with time_major.  Two launches: the recording
 * forward pass into d_work -- n_instances * T * mk_loo_work_stride(N, K) doubles, filtered records for N + K <= 16, the backward
 * tape of MK_OUT_TAPE for 16 < N + K <= 63 -- and one backward walk (adjoint_kernel in its LOO mode, resp. smoother_dk_kernel in
 * its).  prob->warmup is ignored; d_status (may be NULL) receives the filter's MK_FLAG_* bits.  mk_loo_work_stride returns 0 for
 * a shape that is not served (not specialised, or N + K >= 64); mk_loo then fails with MK_ERR_SHAPE, as it does under the
 * size-generic kernel family, and with MK_ERR_INVALID for a buffer that is larger than the allocation it points into. */
MK_API int64_t mk_loo_work_stride(int64_t N, int64_t K);
MK_API int mk_loo(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major, double *d_loo_means,
                  double *d_loo_vars, uint32_t *d_status);

/* Smoothed STATE DISTURBANCES and the auxiliary residuals of the state equation (Harvey & Koopman 1992; statsmodels'
 * smoothed_state_disturbance, KFAS' rstandard(type = "state")): did the state equation x_t = phi o x_{t-1} + eta_t fail somewhere,
 * in which component and when -- a step change in one series' own state, a shift of a common factor.  The backward walk of the
 * adjoint gradient, run with unit weight on every step, carries the Durbin-Koopman pair (r_t, N_t) of the state equation; between
 * the updates of step t and the pull-back through Phi it writes, for every state i of every step (observed or not; t = 0 is the
 * disturbance between the initial state and the first prediction),
 *     d_r[b,t,i] = r_t,i,   d_ninfo[b,t,i] = N_t,ii   (a negative value from rounding is stored as 0)
 * from which     E[eta_t,i | Y] = q_i r_t,i,   Var[eta_t,i | Y] = q_i - q_i^2 N_t,ii,   u_t,i = r_t,i / sqrt(N_t,ii)
 * (u: the standardised auxiliary residual, unit spread under the model; q_i N_t,ii in [0,1] is the share of the disturbance's
 * variance that the data determine -- 0 behind the last observation and for a state with q_i = 0).  The RAW pair is written so that
 * u is never formed from a difference.  [B,T,N+K], or [T,B,N+K] with time_major.  Two launches: the recording forward pass of
 * mk_loglik_grad into d_work -- n_instances * T * mk_disturbance_work_stride(N, K) doubles, filtered full-square records -- and one
 * backward walk (adjoint_kernel for N + K <= 16, adjoint_wide_kernel in its recompute form for 16 < N + K <= 64, each in its
 * disturbance mode).  prob->warmup is ignored; d_status (may be NULL) receives the filter's MK_FLAG_* bits.
 * mk_disturbance_work_stride returns mk_record_stride(N + K) for a specialised shape with N + K <= 64 and 0 otherwise;
 * mk_disturbances then fails with MK_ERR_SHAPE, as it does under the size-generic kernel family, and with MK_ERR_INVALID (no
 * launch) for a missing buffer and for one that is larger than the allocation it points into. */
MK_API int64_t mk_disturbance_work_stride(int64_t N, int64_t K);
MK_API int mk_disturbances(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major, double *d_r, double *d_ninfo,
                           uint32_t *d_status);

/* One-step-ahead INNOVATIONS of every observed cell and the one-step-ahead forecast of every series (the quantities the filter
 * forms in every scalar update, kalmanfilter.py:341-378, and folds into sigmas[t] = sum v^2/f, detfs[t] = sum log f).  For step t,
 * after the prediction from the filtered moments of step t - 1 (x0 / P0 at t = 0) and with the observed series of the step taken
 * in ASCENDING order, the update of series j has
 *     d_v[b,t,j] = y_tj - z_j x,   d_f[b,t,j] = z_j P z_j' + R_j      (x, P: the state after the updates of the observed series < j)
 * in the filter's own units (no scale / offset), NaN at a cell that is not observed.  The standardised one-step-ahead prediction
 * error is e = v / sqrt(f): under the model the e of all observed cells are independent N(0,1).  v and f DEPEND ON THE ORDER of the
 * series (cell (t, j) is predicted from the past and from the cells (t, < j)); the MARGINAL forecast, from the past alone, does not:
 *     d_pred_means[b,t,j] = (z_j x_{t|t-1}) * scale + offset,   d_pred_vars[b,t,j] = max(z_j P_{t|t-1} z_j' + R_j, 0) * scale^2
 * for EVERY series, observed or not (scale / offset: mk_problem.d_scale / d_offset).  For the first observed series of a step
 * v = y - pred_mean and f = pred_var (unscaled).  All four are [B,T,N], or [T,B,N] with time_major; any of them may be NULL (with
 * d_v and d_f both NULL the updates are not run), not all four.  Two launches: the recording forward pass of mk_loglik_grad
 * into d_work -- n_instances * T * mk_innovations_work_stride(N, K) doubles, filtered full-square records -- and innov_step_kernel,
 * one (instance, step) per lane group: step t needs the record of step t - 1 only.  prob->warmup is ignored; d_status (may be
 * NULL) receives the filter's MK_FLAG_* bits -- the outputs of an instance with MK_FLAG_NONPOSITIVE_F are not meaningful.
 *   Served: every supported shape with N + K <= 64, specialised or not, and under either kernel family: the size-generic
 * filter writes the same filtered-only full-square records (the transpose of the specialised kernels' image, equal up to the
 * rounding-level asymmetry of the rank-one updates).  mk_innovations_work_stride returns mk_record_stride(N + K) for those and 0
 * otherwise; mk_innovations then fails with MK_ERR_SHAPE.  MK_ERR_INVALID (no launch) for a missing d_work, for all four outputs
 * NULL, and for a buffer that is larger than the allocation it points into.  The step kernel is timed in the smoother slot of
 * mk_last_kernel_ms / mk_kernel_ms_totals.
 *
 * mk_innovation_stats: the portmanteau (Ljung-Box) statistics of e per (instance, series).  With t_1 < ... < t_m the cells of
 * series j that have finite v, finite f > 0 and t >= t_first, and e_i = v / sqrt(f) at t_i:
 *     mean = sum e_i / m,   c_l = sum_{i=1}^{m-l} (e_i - mean)(e_{i+l} - mean) / m,   r_l = c_l / c_0,
 *     Q = m (m + 2) sum_{l=1}^{nlags} r_l^2 / (m - l)
 * -- lags count successive VALID cells of the series, not calendar steps.  d_stats [B,N,4+nlags] = [m, mean, c_0, Q, r_1 .. r_nlags],
 * 1 <= nlags <= 32; r_l and Q are NaN when m <= nlags or c_0 = 0, mean and c_0 when m = 0.  d_v / d_f as written by mk_innovations
 * ([B,T,N], or [T,B,N] with time_major).  Every sum is taken in an order fixed by T and the series' own cells: a series' statistics
 * are bit-identical whatever the batch around it.  Under the model Q is approximately chi-square with nlags degrees of freedom. */
MK_API int64_t mk_innovations_work_stride(int64_t N, int64_t K);
MK_API int mk_innovations(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major, double *d_v, double *d_f,
                          double *d_pred_means, double *d_pred_vars, uint32_t *d_status);
MK_API int mk_innovation_stats(mk_context *ctx, int64_t B, int64_t T, int64_t N, int time_major, int64_t t_first, int64_t nlags,
                               const double *d_v, const double *d_f, double *d_stats);

/* RESIDUAL DIAGNOSTICS of the standardised innovations e = v / sqrt(f) (d_v / d_f as written by mk_innovations, [B,T,N], or
 * [T,B,N] with time_major): beside the whiteness of mk_innovation_stats, the two other standard checks -- normality and
 * constant variance -- and the one a FACTOR model needs: are the innovations of different series uncorrelated with each other?
 * A cell (t, j) is VALID when v is finite, f is finite and > 0 and t >= t_first (mk_innovation_stats' rule).  Per (instance,
 * series), with t_1 < ... < t_m the valid cells and e_1 .. e_m their values:
 *     mean = sum e_i / m,   d_i = e_i - mean,   S_k = sum d_i^k  (k = 2, 3, 4; sums, not divided),   h = (m + 1) / 3 (integer),
 *     ss_first = sum_{i <= h} e_i^2,   ss_last = sum_{i > m - h} e_i^2     (raw e; thirds of the COMPACTED sequence of valid cells),
 *     cusum = max_k |C_k|,  C_k = sum_{i <= k} d_i;      cusq = max_k |Q_k - (k / m) S2|,  Q_k = sum_{i <= k} d_i^2,
 * cusum_t / cusq_t the calendar step t_k of the FIRST k that attains the maximum.
 * mk_residual_series: d_stats [B,N,12] = [m, mean, S2, S3, S4, h, ss_first, ss_last, cusum, cusum_t, cusq, cusq_t]; for m = 0 the
 * row is [0, NaN x 4, 0, NaN x 6]; for a constant series (S2 = 0) the raw sums are written as they are.
 * mk_residual_cross: with e~[t,j] = d / sqrt(S2 / m) at the valid cells (mean, S2, m from d_stats, the rows mk_residual_series
 * wrote for the same d_v, d_f and t_first), for the lags l = 0 .. nlags (0 <= nlags <= 32) and all ORDERED pairs (i, j)
 *     d_counts[b,l,i,j] = n_ij(l) = the number of t for which both (t, i) and (t - l, j) are valid   (64-bit integers),
 *     d_sums[b,l,i,j]   = s_ij(l) = sum of e~[t,i] e~[t-l,j] over those t,
 * both [B,nlags+1,N,N].  Lags are CALENDAR steps here: two series share a clock, not a sequence of observed cells.  A pair in
 * which either series has m = 0 or S2 = 0 gets n = 0 and s = NaN.  N <= 64.  Under the model r_ij(l) = s / n is approximately
 * N(0, 1/n) for i != j or l > 0.
 *   Every sum is taken in one fixed order that depends on T and the series' own cells alone.  mk_residual_series: 64 accumulators,
 * accumulator l adding the cells of steps l, 64 + l, 128 + l, .. in ascending time, then summed once by a fixed tree (lanes l and
 * l ^ 32, ^ 16, .. ^ 1); the running sums C_k and Q_k: a prefix scan over each tile of 64 steps plus the carry of the tiles
 * before.  mk_residual_cross: ascending time into one accumulator per (lag, i, j).  So an instance's results are bit-identical
 * whatever the batch around it and in either layout.  MK_ERR_INVALID (no launch) with a message that
 * names the argument for a missing pointer, N > 64, nlags outside 0 .. 32 and a buffer larger than the allocation it points into. */
MK_API int mk_residual_series(mk_context *ctx, int64_t B, int64_t T, int64_t N, int time_major, int64_t t_first, const double *d_v,
                              const double *d_f, double *d_stats);
MK_API int mk_residual_cross(mk_context *ctx, int64_t B, int64_t T, int64_t N, int time_major, int64_t t_first, int64_t nlags,
                             const double *d_v, const double *d_f, const double *d_stats, int64_t *d_counts, double *d_sums);

/* MULTI-STEP-AHEAD FORECASTS and FORECAST SKILL BY HORIZON (statsmodels' forecast / get_prediction, KFAS' predict): what the model
 * says about steps it has not seen, and how far ahead that is worth anything.  Model and units as in mk_innovations (Phi and Q
 * diagonal, Z = [I | Gamma], observation variances R_j, zero when d_obsvar is NULL; the filter's standardised units, scale /
 * offset applied only where said).
 *   ORIGIN o in {-1, 0, .., T-1} has the moments (a_o, P_o): the filtered record of step o for o >= 0, the initial moments (d_x0 /
 * d_P0, or 0 / I) for o = -1.  PROPAGATION: for h >= 1 the filter's own prediction (kalmanfilter.py:318-331) applied h times,
 * x <- phi o x, P <- (phi phi') o P + diag(q).  FORECAST of series j: m_{o,h,j} = z_j x and s_{o,h,j} = z_j P z_j' + R_j -- the
 * operations the filter performs on h successive empty steps, so they equal (up to rounding) the filter's predicted moments on
 * a record whose steps after o are all missing.  One call writes any non-empty subset of three outputs:
 *   fan     d_fan_means, d_fan_vars [B,H,N], H = horizon: row h - 1 holds m * scale + offset and max(s, 0) * scale^2 for
 *           h = 1 .. H from the origin of the instance's RECORD, d_fan_origins[record] (int64 [n_records], values -1 .. T-1; NULL:
 *           T - 1 for all).  The targets may lie beyond T: the out-of-sample forecast.
 *   track   d_track_means, d_track_vars [B,T,N], or [T,B,N] with time_major, for ONE horizon track_horizon >= 1: row t is the
 *           forecast of step t made at origin max(t - track_horizon, -1), propagated t - origin steps, scaled as above; defined at
 *           every step, observed or not.  track_horizon = 1 gives mk_innovations' d_pred_means / d_pred_vars.
 *   skill   d_skill [B,N,H,6]: per (instance, series j, horizon h) the sums over the pairs (o, t = o + h) with t_first <= o,
 *           t <= T - 1 and y_{t,j} finite; with e = y_{t,j} - m_{o,h,j} and s = s_{o,h,j} the six columns are
 *               [ m (pair count), sum e, sum e^2, sum e^2 / s, sum log s, hits ],   hits = #{ e^2 <= coverage_z^2 s },
 *           all in the filter's units.  An origin counts whether or not step o itself was observed; without pairs all six are
 *           exactly 0.
 * Every sum is taken in an order fixed by T, H and t_first alone: the outputs of an instance are bit-identical whatever batch it
 * sits in, whatever n_instances is and whichever subset of outputs is asked for.
 *   Limits: 1 <= horizon <= mk_forecast_max_horizon() = 32, 1 <= track_horizon <= T (read only when a track output is set),
 * t_first >= 0, coverage_z > 0 and finite.  prob->warmup is ignored; d_status (may be NULL) receives the filter's MK_FLAG_* bits
 * -- the outputs of an instance with MK_FLAG_NONPOSITIVE_F are not meaningful.
 *   Launches: the recording forward pass of mk_loglik_grad into d_work -- n_instances * T * mk_forecast_work_stride(N, K) doubles:
 * the filtered full-square records packed at its head, the per-chunk partial sums of the skill table behind them -- then
 * forecast_path_kernel (fan and track, one (instance, row) per lane group) and forecast_skill_kernel (one (instance, chunk of
 * origins, block of horizons) per lane group; a second small kernel adds the chunks in ascending order when T exceeds one
 * chunk), on the context's stream, timed in the smoother slot of mk_last_kernel_ms / mk_kernel_ms_totals.  The kernels read the
 * (c, r) image of the records the specialised recording pass writes, at the same positions under the size-generic family (which
 * writes the transpose, equal up to rounding), as innov_step_kernel does.
 *   Served: every supported shape with N + K <= 64, under either kernel family; mk_forecast_work_stride returns 0 otherwise and
 * mk_forecast fails with MK_ERR_SHAPE.  MK_ERR_INVALID (no launch): all outputs NULL, a missing d_work, a limit above violated, a
 * fan origin out of range (checked on the host: n_records integers are copied back), a buffer larger than the allocation it
 * points into. */
typedef struct mk_forecast_request {
    int64_t horizon, t_first, track_horizon;   /* track_horizon read only when a track output is set */
    double coverage_z;
    const int64_t *d_fan_origins;              /* [n_records] or NULL */
    double *d_fan_means, *d_fan_vars;          /* [B,H,N] */
    double *d_track_means, *d_track_vars;      /* [B,T,N] / [T,B,N] */
    double *d_skill;                           /* [B,N,H,6] */
} mk_forecast_request;

MK_API int64_t mk_forecast_max_horizon(void);
MK_API int64_t mk_forecast_work_stride(int64_t N, int64_t K);
MK_API int mk_forecast(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major, const mk_forecast_request *req,
                       uint32_t *d_status);

/* Posterior DRAWS of the states and of the projected series: the simulation smoother by mean correction (Durbin & Koopman 2002,
 * Biometrika 89:603-616).  For the model the filter implements (seqkalmanfilter, metran/kalmanfilter.py:315-333:
 * x_{-1} ~ N(x0, P0), x_t = phi o x_{t-1} + w_t, y_t = [I | Gamma] x_t + e_t) and path id = s * n_instances + i (draw s of instance i,
 * record i % n_records), mk_draw_perturb walks time once and writes
 *     x+_{-1} = L0 z_init,   x+_t = phi o x+_{t-1} + sqrt(q) o z_t[0:n],   y+_t = [I | Gamma] x+_t + sqrt(R) o z_t[n:n+N],
 *     d_ystar  [ndraws * n_instances, T, N]   y*_{t,j} = y_{t,j} - y+_{t,j} where (t, j) is observed (finite), NaN where it is not,
 *     d_zxplus [ndraws * n_instances, T, N]   [I | Gamma] x+_t, unscaled                       (may be NULL),
 *     d_xplus  [ndraws * n_instances, T, n]   x+_t                                             (may be NULL),
 * all three in the layout of prob->obs_time_major ([T, ndraws * n_instances, .] when set).  d_L0 [n_instances,n,n]: the lower
 * Cholesky factor of P0, NULL = identity (the default P0); the initial mean of x+ is zero whatever x0 is; the observation normals
 * are drawn only when prob->d_obsvar is set.  prob->d_x0, d_P0, d_scale, d_offset and warmup are not read.
 *   INVALID parameters are not hidden: a NaN phi, a NaN or negative q or observation variance (the square root is NaN) make x+, y+
 * and with them y* NaN at the cells they reach, observed ones included, and there is no status word.  A smoother takes a NaN y* for
 * a MISSING cell, so a caller must treat a path whose y* is not finite at an observed cell as invalid before smoothing it
 * (BatchedKalman.draw_smoothed sets MK_FLAG_NONPOSITIVE_F for the path and returns NaN draws).
 *   The caller then smooths y* with the EXISTING mk_filter_smooth on a derived problem of ndraws * n_instances instances and as
 * many records (d_obs = d_ystar; d_phi, d_q, d_loadings, d_obsvar, d_scale, d_offset, d_x0, d_P0 replicated per path) and adds the
 * unconditional part with mk_draw_combine, in place on the smoother's output (both arrays in the layout `time_major`):
 *     MK_DRAW_SERIES   d_inout [.,T,N] (d_sim_means of y*)  +=  scale[record, j] * d_plus (= d_zxplus)    -- the offset is in sim_means
 *     MK_DRAW_STATES   d_inout [.,T,n] (smoothed means of y*)  +=  d_plus (= d_xplus)
 * (prob = the ORIGINAL problem: n_instances, n_records, d_scale).  The smoother is affine in the data, so the result is a draw
 * from p(x | y) exactly; at an observed cell with R = 0 a series draw returns the observation.
 *   The normals are counter-based -- a value depends on what it is for, not on the launch that computes it: Philox4x32-10 with
 * key (seed & 0xffffffff, seed >> 32) and counter (t + 1, c >> 1, first_instance + i, d), t + 1 = 0 the initial state, c the
 * component (0..n-1 state noise, n..n+N-1 observation noise), d the draw number first_draw + s.  From the output words:
 * m1 = (w0 >> 6) * 2^26 + (w1 >> 6), u1 = (m1 + 0.5) * 2^-52, likewise m2, u2 from w2, w3; rho = sqrt(-2 ln u1); an even c takes
 * rho cos(2 pi u2), an odd c rho sin(2 pi u2).  antithetic: draw first_draw + s uses d = (first_draw + s) >> 1 and every normal
 * times (-1)^((first_draw + s) & 1): the mean of a pair is the smoothed mean exactly.
 *   mk_draw_normals writes the normals of a block of counters, d_out [ndraws, ninstances, T + 1, ncomp] (time index 0 = the
 * initial state); raw != 0: the integers m1 (even c) / m2 (odd c) as exact doubles, without the antithetic sign.
 *   Refusals (no launch): MK_ERR_INVALID for a missing required pointer or a buffer larger than the allocation it points into,
 * MK_ERR_SHAPE for N + K > mk_generic_max_states(). */
#define MK_DRAW_SERIES 0
#define MK_DRAW_STATES 1
MK_API int mk_draw_perturb(mk_context *ctx, const mk_problem *prob, uint64_t seed, int64_t first_instance, int64_t first_draw,
                           int64_t ndraws, int antithetic, const double *d_L0, double *d_ystar, double *d_zxplus,
                           double *d_xplus);
MK_API int mk_draw_combine(mk_context *ctx, const mk_problem *prob, int64_t ndraws, int what, int time_major,
                           const double *d_plus, double *d_inout);
MK_API int mk_draw_normals(mk_context *ctx, uint64_t seed, int64_t first_instance, int64_t ninstances, int64_t first_draw,
                           int64_t ndraws, int antithetic, int64_t T, int64_t ncomp, int raw, double *d_out);

/* WINDOW STATISTICS of posterior draws, reduced on the device (ensemble_kernels.hip): what an ensemble of draws is read for --
 * the uncertainty of a monthly mean, of a yearly minimum, of the time spent below a level -- without holding the ensemble.
 *   mk_path_functionals reduces every path of a block of combined draws over time windows.  d_paths: logical
 * [ndraws * n_instances, T, Wd], Wd = N (MK_DRAW_SERIES) or N + K (MK_DRAW_STATES), path id = s * n_instances + i as above, stored
 * [T, ndraws * n_instances, Wd] when time_major is set.  d_windows int64 [n_records, W, 2]: window w of record r = i % n_records
 * is the half-open step range [a, b).  PRECONDITION: 0 <= a_w <= b_w <= a_{w+1} <= ... <= T -- sorted, not overlapping; gaps and
 * empty windows (a == b) are allowed.  The library does not read the windows on the host; for ANY input with 0 <= a <= b <= T the
 * kernel stays inside its arrays (bounds outside that range are clamped into it), whatever the order -- the numbers are then
 * those of the windows a forward walk meets.  d_thresholds [n_records, Wd] in the paths' units, or NULL.
 *   d_functionals [ndraws, n_instances, Wd, W, 5] over y_t = path[t, j], t = a .. b - 1, L = b - a:
 *     0 mean             (((y_a + y_{a+1}) + ...) + y_{b-1}) / L: the adds in increasing t, one division
 *     1 min, 2 max       the smallest / largest y_t
 *     3 fraction below   #{t : y_t < c} / L, c the threshold of (record, column)
 *     4 longest spell    the largest number of consecutive steps with y_t < c, as a double; a spell ends at the window's edge
 * An empty window gives NaN for all five, and so does a window that holds a NaN (a flagged path of draw_smoothed); a NaN or absent
 * threshold makes 3 and 4 NaN.  The order of every sum is the definition's: the result does not depend on layout, batch or grid.
 *   mk_ensemble_summary reduces d_values [S, cells] over the S draws of each cell, using the FINITE values x_s only, in
 * increasing s: d_summary [cells, 5 + nprobs] = count m (as a double), mean (sequential sum / m; NaN if m = 0), sd (two-pass,
 * sqrt(sum (x_s - mean)^2 / (m - 1)); NaN if m < 2), min, max (NaN if m = 0), then one quantile per probability p of the HOST array
 * probs: with z the sorted finite values, h = (m - 1) p, lo = floor(h), q = z_lo + (h - lo) (z_min(lo+1, m-1) - z_lo) -- numpy's
 * default "linear" quantile; NaN if m = 0.  Non-finite values are removed before the sort.  S <= mk_ensemble_max_draws() = 4096
 * (the cell's values are sorted in LDS), S any number, nprobs <= 16.
 *   Refusals (MK_ERR_INVALID, no launch, text in mk_last_error): W < 1, S < 1, S above the cap, cells < 1, nprobs < 0 or > 16, a
 * probability outside [0, 1] or NaN, a missing pointer (d_thresholds may be NULL; probs may be NULL when nprobs = 0), `what`
 * neither MK_DRAW_SERIES nor MK_DRAW_STATES, a buffer larger than the allocation it points into. */
MK_API int64_t mk_path_functional_count(void); /* 5 */
MK_API int mk_path_functionals(mk_context *ctx, const mk_problem *prob /* n_instances, n_records, T, N, K are read */, int64_t ndraws,
                               int what /* MK_DRAW_SERIES or MK_DRAW_STATES */, int time_major, const double *d_paths, int64_t W,
                               const int64_t *d_windows /* [n_records,W,2] */, const double *d_thresholds /* [n_records,Wd] or NULL */,
                               double *d_functionals /* [ndraws,n_instances,Wd,W,5] */);
MK_API int64_t mk_ensemble_max_draws(void);
MK_API int mk_ensemble_summary(mk_context *ctx, int64_t S, int64_t cells, const double *d_values /* [S,cells] */, int64_t nprobs,
                               const double *probs /* HOST array, nprobs <= 16 */, double *d_summary /* [cells, 5 + nprobs] */);

/* OBSERVATION WEIGHTS of smoothed series and states (Koopman & Harvey 2003, J. Econ. Dyn. Control 27:1317-1333; statsmodels'
 * compute_smoothed_state_weights): which observations a smoothed number comes from.  For fixed parameters the smoother is linear
 * in the data, so for a TARGET (t*, c) -- c = z_j* (what = MK_DRAW_SERIES: series j*, the unscaled projection z_j* x_{t*|T}) or c = e_i
 * (what = MK_DRAW_STATES: state i) --
 *     c' x_{t*|T} = sum over the observed cells (t, j) of  w_{t,j} y_{t,j}  +  intercept,
 * y the filter's standardised value (no scale, no offset).  Model and filter order as in mk_innovations: prediction first
 * (x <- phi o x, P <- (phi phi') o P + diag q), then the observed series of the step in ascending order, Z = [I | Gamma].
 *   PER CELL, with P the covariance just before the scalar update of the observed cell (t, j):  d_{t,j} = P z_j',
 * rf_{t,j} = 1 / f_{t,j}, k_{t,j} = d_{t,j} rf_{t,j};  d = 0 and rf = 0 at a cell that is not observed, which then drops out of
 * what follows arithmetically.
 *   FORWARD from t*:  p = P_{t*|t*-1} c (the predicted covariance of step t*: from the filtered record of step t* - 1, from d_P0 / I
 * for t* = 0);  for t = t* .. T-1: p <- phi o p if t > t*, then for j ascending  g_{t,j} = (z_j p) rf_{t,j},  p <- p - d_{t,j} g_{t,j};
 * g = 0 at every cell before step t*.
 *   BACKWARD over the whole record:  h = 0;  for t = T-1 .. 0: for j descending  w_{t,j} = g_{t,j} + (h k_{t,j}),  h <- h - w_{t,j} z_j';
 * after the cells of step t, h <- h + c if t = t*; then h <- phi o h.  At the end intercept = h x0 (0 when d_x0 is NULL).
 *   d_weights [B,M,T,N] (model-major whatever time_major says) holds w, in units of (target per unit of the standardised
 * observation), NaN at every cell that is not observed; d_intercept [B,M] (may be NULL) the intercept.  Instance i uses the M
 * targets of record i % n_records, d_targets [n_records,M,2] = (step, column) as 64-bit integers.  A target whose step is outside
 * [0, T) or whose column is outside [0, N) (series) / [0, N + K) (states) gets an all-NaN row and a NaN intercept, and nothing is
 * read back on the host; a negative step marks an unused slot.  For R = 0 the smoothed projection of an observed cell is the
 * observation: its own weight is 1 and all others are 0, up to rounding.
 *   Launches: the recording forward pass of mk_loglik_grad into d_work -- n_instances * T * mk_weights_work_stride(N, K) doubles:
 * the filtered full-square records packed at its head (mk_record_stride(N + K) doubles each, addressed by time_major, as in
 * mk_forecast), the GAIN TAPE behind them: per (instance, step, series) one slot [ d (N + K) | rf | pad ] of (N + K + 3) & ~1 doubles,
 * cell (b, t, j) at ((b, t) block * N + j) slots, the blocks addressed by time_major like the records -- then one asynchronous clear
 * of the tape, innov_step_kernel (which re-forms d and rf of every scalar update from the records, in parallel over time, and
 * stores them; its v / f / forecast outputs are not asked for) and weights_walk_kernel (one target per lane group, lane = state;
 * one forward and one backward vector walk, O(N + K) per cell), all on the context's stream, the three timed in the smoother slot
 * of mk_last_kernel_ms / mk_kernel_ms_totals.  Every sum is a fixed tree over the lanes: a target's weights are bit-identical
 * whatever batch, n_targets or neighbouring targets it runs with.  prob->warmup is ignored; d_status (may be NULL) receives the
 * filter's MK_FLAG_* bits -- the outputs of an instance with MK_FLAG_NONPOSITIVE_F are not meaningful.
 *   Served: every supported shape with N + K <= 64, under either kernel family; mk_weights_work_stride returns 0 otherwise and
 * mk_observation_weights fails with MK_ERR_SHAPE.  MK_ERR_INVALID (no launch): a missing d_work, d_targets or d_weights,
 * n_targets < 1, a `what` that is neither MK_DRAW_SERIES nor MK_DRAW_STATES, a buffer larger than the allocation it points into. */
typedef struct mk_weights_request {
    int64_t n_targets;            /* M per record, >= 1 */
    int what;                     /* MK_DRAW_SERIES: c = z_j;  MK_DRAW_STATES: c = e_i */
    const int64_t *d_targets;     /* [n_records, M, 2] = (step, column); instance i uses the targets of record i % n_records */
    double *d_weights;            /* [B, M, T, N], model-major whatever time_major says */
    double *d_intercept;          /* [B, M] or NULL */
} mk_weights_request;
MK_API int64_t mk_weights_work_stride(int64_t N, int64_t K);
MK_API int mk_observation_weights(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major,
                                  const mk_weights_request *req, uint32_t *d_status);

/* INTERVENTION EFFECTS by GLS (de Jong 1991, Ann. Statist. 19:1073-1083; Durbin & Koopman 2012, section 6.2; statsmodels'
 * mle_regression, KFAS regression effects): level shifts, outliers and trends of single series as KNOWN regressors of the
 * observation equation, y_t = X_t beta + Z x_t + e_t, estimated for fixed parameters.  Model and filter order as in
 * mk_innovations; d_{t,j} and rf_{t,j} = 1 / f_{t,j} of every scalar update as in mk_observation_weights (zero at a cell that is
 * not observed).
 *   EFFECTS.  d_effects [n_records,M,4] = (series j, kind, t0, t1) as 64-bit integers, 0 <= t0 < t1 <= T; instance i uses the M
 * effects of record i % n_records; a negative series marks an unused slot.  The regressor acts on series j alone:
 *     MK_EFFECT_LEVEL  x_t = 1 for t0 <= t < t1, else 0 (a pulse is t1 = t0 + 1, a permanent shift t1 = T);
 *     MK_EFFECT_RAMP   x_t = min(t, t1 - 1) - t0 + 1 for t >= t0, else 0 (one unit per step, held after t1 - 1).
 *   REPLAY.  The covariance recursion does not depend on the data, so the filter's mean recursion of any data column is
 *     a = x0 (column 0: y) or 0 (columns 1 .. M: the regressors);  per step a <- phi o a;  per cell j ascending
 *     V = col[t,j] - z_j a,  a <- a + (d_{t,j} rf_{t,j}) V,
 * with col = y (0 where it is not observed) or x_m on its series, 0 elsewhere.  Over the cells of the steps t >= t_first, in time
 * order,  A[p,q] = sum (V_p rf) V_q  for q <= p, mirrored (d_normal [B,M+1,M+1]): A[0,0] is the filter's sum of sigmas, s = A[0,1:],
 * S = A[1:,1:], and -2 log L(beta) = -2 log L(0) - 2 s'beta + beta'S beta exactly.  d_support [B,M] (int64) counts per effect the
 * counted observed cells with x != 0.
 *   SOLVE, in a fixed order: S scaled to unit diagonal; Cholesky in effect order; an effect with support 0 (or in an unused
 * slot), or whose pivot in the scaled matrix is below 1e-12, is DROPPED and the others are solved without it.  d_beta [B,M] =
 * S^-1 s, d_cov [B,M,M] = S^-1, d_gain [B] = s'S^-1 s = -2 log L(0) - -2 log L(beta); a dropped effect has a NaN beta, NaN in its row
 * and column of d_cov and its bit (1 << m) in d_dropped [B] (uint32).  With t_first = T nothing is counted: every effect is
 * dropped and the gain is 0.
 *   Launches: as mk_observation_weights -- the recording forward pass into d_work (n_instances * T *
 * mk_regression_work_stride(N, K) doubles = the weights stride: records, then the gain tape), the clear of the tape,
 * innov_step_kernel -- then regress_replay_kernel (one instance per lane group, lane = state; the regressors are generated from
 * the descriptors), the three timed in the smoother slot of mk_last_kernel_ms / mk_kernel_ms_totals.  Every sum has a fixed
 * order: an instance's outputs are bit-identical whatever the batch, the layout of d_work or the neighbouring instances, and
 * the block of A of a subset of the effects does not depend on the other effects of the call.  prob->warmup is ignored (t_first
 * says which steps count); d_status (may be NULL) receives the filter's MK_FLAG_* bits -- the outputs of an instance with
 * MK_FLAG_NONPOSITIVE_F are not meaningful.
 *   mk_regression_adjust writes d_obs_out = d_obs_in - sum_m beta_m x_m for R records [R,T,N] (stored [T,R,N] when time_major
 * is set; in place when the two pointers are equal), d_beta [R,M]: a NaN beta counts as 0, a NaN observation stays NaN.
 *   Served: every supported shape with N + K <= 64, under either kernel family; mk_regression_work_stride returns 0 otherwise
 * and mk_regression fails with MK_ERR_SHAPE.  MK_ERR_INVALID (no launch): a missing pointer (all of the request's are
 * required), n_effects outside 1 .. mk_regression_max_effects() = 16, t_first < 0, a buffer larger than the allocation it
 * points into, and -- after one small copy of the effects to the host -- a slot in use with series >= N, an unknown kind or
 * t0 / t1 outside 0 <= t0 < t1 <= T. */
#define MK_EFFECT_LEVEL 0
#define MK_EFFECT_RAMP 1
typedef struct mk_regression_request {
    int64_t n_effects;            /* M per record, 1 .. mk_regression_max_effects() */
    int64_t t_first;              /* the steps t >= t_first are counted (1: as Metran's warm-up) */
    const int64_t *d_effects;     /* [n_records, M, 4] = (series, kind, t0, t1) */
    double *d_beta;               /* [B, M] */
    double *d_cov;                /* [B, M, M] */
    double *d_gain;               /* [B] */
    double *d_normal;             /* [B, M + 1, M + 1] */
    int64_t *d_support;           /* [B, M] */
    uint32_t *d_dropped;          /* [B] */
} mk_regression_request;
MK_API int64_t mk_regression_max_effects(void);
MK_API int64_t mk_regression_work_stride(int64_t N, int64_t K);
MK_API int mk_regression(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major,
                         const mk_regression_request *req, uint32_t *d_status);
MK_API int mk_regression_adjust(mk_context *ctx, int64_t R, int64_t T, int64_t N, int time_major, int64_t n_effects,
                                const int64_t *d_effects, const double *d_beta, const double *d_obs_in, double *d_obs_out);

/* ---- per-step scores by the tangent filter (score_kernels.hip) ------------------------------------------------------------------
 * The SCORE of every time step: the derivative of the step's contribution to -2 log L, l_t = sum_j (log f_{t,j} + v_{t,j}^2 /
 * f_{t,j}) over the cells observed at t (the constant of get_mle is not differentiated), with respect to one parameter per state
 * (what statsmodels calls score_obs), and the sums built on them.  Model and filter order as in mk_innovations; d_{t,j} and
 * rf_{t,j} = 1 / f_{t,j} of every scalar update as in mk_observation_weights (zero at a cell that is not observed).
 *   Parameter p (0 <= p < n = N + K) moves phi_p and q_p only: d_dphi[b,p] = d phi_p / d theta_p and d_dq[b,p] = d q_p / d theta_p
 * are inputs, the chain rule to the caller's parameters stays outside.  x0 and P0 do not depend on the parameters.  The tangent
 * (Pd symmetric n x n, xd) of pair (b, p) starts at zero; with x, P the FILTERED moments of step t - 1 (x0, P0 at t = 0):
 *     predict   xd <- phi o xd + dphi x_p e_p;   Pd <- Phi Pd Phi + dphi (e_p (P_p. o phi) + (phi o P_.p) e_p') + dq e_p e_p'
 *     cell j    dd = Pd z_j',  fd = z_j dd,  vd = -z_j xd;      s_{t,p} += fd rf + 2 v vd rf - v^2 fd rf^2
 *               xd <- xd + (dd v + d vd) rf - d v fd rf^2;      Pd <- Pd - (dd d' + d dd') rf + d d' fd rf^2
 * A step is COUNTED when t >= t_first and it holds at least one observation; m = d_count[b] (int64) is their number.
 *   d_score [B,T,n] (stored [T,B,n] when time_major is set)   s_{t,p} of every step, zero at an empty step, also for t < t_first
 *   d_grad  [B,n]     sum of s_t over the counted steps
 *   d_opg   [B,n,n]   sum of s_t s_t' over the counted steps: positive semi-definite by construction
 *   d_cusum [B,n,n]   sum of S_t S_t' over the counted steps, S_t = sum_{u <= t, counted} (s_u - grad / m): the tied-down cumulative
 *                     scores of the Nyblom-Hansen test of parameter constancy
 *   Launches: as mk_observation_weights -- the recording forward pass into d_work (n_instances * T * mk_scores_work_stride(N, K)
 * doubles = the weights stride + N: records, then the gain tape, then one row of N innovations per (instance, step)), the clear
 * of the tape, innov_step_kernel writing the tape and v -- then score_tangent_kernel (one lane group per (instance, parameter),
 * lane = state) and score_stats_kernel (one workgroup per instance), timed in the smoother slot of mk_last_kernel_ms /
 * mk_kernel_ms_totals.  Every sum has a fixed order: an instance's outputs are bit-identical whatever the batch, the layout of
 * d_work or the neighbouring instances.  prob->warmup is ignored (t_first says which steps count); d_status (may be NULL) receives
 * the filter's MK_FLAG_* bits -- the outputs of an instance with MK_FLAG_NONPOSITIVE_F are not meaningful.
 *   Served: every supported shape with N + K <= mk_scores_max_states() = 64, under either kernel family, full-square records;
 * mk_scores_work_stride returns 0 otherwise and mk_scores fails with MK_ERR_SHAPE.  MK_ERR_INVALID (no launch): a missing pointer
 * (all of the request's are required), t_first < 0, a buffer larger than the allocation it points into. */
typedef struct mk_scores_request {
    const double *d_dphi;         /* [B, n] */
    const double *d_dq;           /* [B, n] */
    int64_t t_first;              /* the steps t >= t_first that hold an observation are counted (1: as Metran's warm-up) */
    double *d_score;              /* [B, T, n] */
    double *d_grad;               /* [B, n] */
    int64_t *d_count;             /* [B] */
    double *d_opg;                /* [B, n, n] */
    double *d_cusum;              /* [B, n, n] */
} mk_scores_request;
MK_API int64_t mk_scores_max_states(void);
MK_API int64_t mk_scores_work_stride(int64_t N, int64_t K);
MK_API int mk_scores(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major, const mk_scores_request *req,
                     uint32_t *d_status);

/* ---- leave-block-out predictions (block_kernels.hip) ----------------------------------------------------------------------------
 * E[y_I | every observation except the block I] and its covariance V for a BLOCK I = the observed cells of one series on the steps
 * [t0, t1): how well a gap of that length is filled from everything else (the single-cell case is mk_loo).  Model and filter order
 * as in mk_innovations: prediction first, then the observed series of the step ascending, Z = [I | loadings]; per observed cell
 * s = (t, j) the gain tape holds d_s = P z_j' and rf_s = 1 / f_s (mk_observation_weights), the innovations hold v_s; k_s = d_s rf_s.
 *   With M = Sigma_y^-1 (the precision of the observed data vector) and u = M (y - mu), for any set I of observed cells
 *     y_I - E[y_I | y_-I] = M_II^-1 u_I,      Cov[y_I | y_-I] = M_II^-1.
 * u and the entries of M come from one backward walk: r = 0 and N = 0 (n x n) behind the last step; a cell that is not observed has
 * d = 0 and rf = 0 and drops out arithmetically.  Per step t = T-1 .. 0, per observed cell s of the step with j DESCENDING:
 *     1.  g = N k_s,   u_s = v_s rf_s - k_s'r,   M_ss = rf_s + k_s'g
 *     2.  for every block cell c already passed (later in filter order), with its vector omega_c:
 *             M_sc = -k_s'omega_c,   omega_c <- omega_c + z_j' M_sc
 *     3.  if s belongs to the block: keep u_s and the row of M, start omega_s = M_ss z_j' - g
 *     4.  r <- r + z_j' u_s,   N <- N - z_j g' - g z_j' + M_ss z_j' z_j
 * and behind the cells of step t, at an empty step too, the pull-back through the prediction: r <- phi o r, N <- (phi phi') o N,
 * omega_c <- phi o omega_c.  At the end, with e = M_II^-1 u_I:  prediction = y_I - e,  V = M_II^-1,  quad = u_I'e,
 * log det V = -log det M_II.
 *   mk_block_max_cells     64: the steps t1 - t0 of a block (one block cell per lane of a wavefront)
 *   mk_block_work_stride   doubles per (instance, step) of d_work: the record, the gain tape and a row of N innovations (the scores'
 *                          layout); 0 where the route does not serve the shape (N + K > 64)
 *   mk_block_predict       Launches: the recording forward pass into d_work, the clear of the tape, innov_step_kernel writing the tape
 *                          and v, then block_checkpoint_kernel (one lane group per instance: the (r, N) walk over the whole tape,
 *                          storing (r, N) behind step t1 of every block into d_checkpoints) and block_walk_kernel (one wavefront per
 *                          (instance, block): the steps t1-1 .. t0 from the checkpoint, then the solve: M_II scaled to unit diagonal,
 *                          Cholesky in time order) -- timed in the smoother slot of mk_last_kernel_ms / mk_kernel_ms_totals.  Every sum
 *                          has a fixed order: a block's outputs are bit-identical whatever the batch, the layout of d_work, the block
 *                          list around it or its position in the list.
 *                          d_means / d_vars hold NaN at the positions that are not observed or lie beyond t1.  A block without an
 *                          observed cell has m = 0, NaN elsewhere and no flag; an unused slot (series < 0) an all-NaN row, m included.
 *                          A pivot of the unit-diagonal M_II below 1e-12 (the regression's bound) makes the block DEGENERATE: its
 *                          outputs except m are NaN and bit 0 of its flag is set; the other blocks are not affected.
 *                          prob->warmup is ignored; d_status (may be NULL) receives the filter's MK_FLAG_* bits -- the outputs of an
 *                          instance with MK_FLAG_NONPOSITIVE_F are not meaningful.
 *   Served: every supported shape with N + K <= 64, under either kernel family; otherwise MK_ERR_SHAPE.  MK_ERR_INVALID (no
 * launch): a missing pointer (all of the request's are required), n_blocks < 1, n_cells outside 1 .. mk_block_max_cells(), a buffer
 * larger than the allocation it points into and, after one small copy of the descriptors to the host, a used slot with series >= N,
 * t0 / t1 outside 0 <= t0 < t1 <= T, or t1 - t0 > n_cells. */
typedef struct mk_block_request {
    int64_t n_blocks;             /* W per record, >= 1 */
    int64_t n_cells;              /* L: row length of the outputs, 1 .. mk_block_max_cells(); every block has t1 - t0 <= L */
    const int64_t *d_blocks;      /* [n_records, W, 3] = (series, t0, t1), 0 <= t0 < t1 <= T; instance i uses record i % n_records;
                                     a negative series marks an unused slot */
    double *d_checkpoints;        /* workspace [B, W, n + n*n] */
    double *d_means;              /* [B, W, L]: E[y | all but the block] * scale + offset at step t0 + c */
    double *d_vars;               /* [B, W, L]: max(V_cc - obsvar_j, 0) * scale^2  (the projected state's variance, as mk_loo) */
    double *d_summary;            /* [B, W, 4] = (m, quad, log det V, 1'V1 / m^2 * scale^2) */
    uint32_t *d_flags;            /* [B, W]: bit 0 = degenerate block */
} mk_block_request;
MK_API int64_t mk_block_max_cells(void);
MK_API int64_t mk_block_work_stride(int64_t N, int64_t K);
MK_API int mk_block_predict(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major, const mk_block_request *req,
                            uint32_t *d_status);

/* ---- level-shift scan (shift_kernels.hip) -----------------------------------------------------------------------------------------
 * For every observed cell (tau, j) the GLS statistic of a LEVEL SHIFT of series j from step tau on, a date that is not known in
 * advance (mk_regression estimates a shift whose date is given): the regressor x = 1 on the observed cells (t, j) with t >= tau,
 *     A = x'u,   D = x'Mx:     estimate = A / D,   standard error = 1 / sqrt(D),   t = A / sqrt(D)
 * with M and u of the leave-block-out predictions above, in the units of the observations the filter runs on (de Jong & Penzer
 * 1998).  All dates come from ONE backward walk over the gain tape: beside (r, N) it carries per series j the vector Omega_j (the sum
 * of omega_c over the cells of series j already passed) and the scalars A_j, D_j, all zero behind the last step.  At an observed cell
 * s = (t, j'), behind step 1 of the walk above:
 *     m_j = -k_s'Omega_j,   Omega_j <- Omega_j + z_j'' m_j                                   for every series j
 *     D_j' <- D_j' + M_ss + 2 m_j',   A_j' <- A_j' + u_s,   Omega_j' <- Omega_j' + M_ss z_j'' - g
 * then step 4; behind the cells of a step, an empty one too, Omega_j <- phi o Omega_j beside the pull-back.  Behind the cells of step
 * tau, (A_j, D_j) is the pair of the shift of series j that starts at tau.
 *   mk_shift_work_stride   doubles per (instance, step) of d_work: mk_block_work_stride
 *   mk_level_shifts        Launches: the recording forward pass into d_work, the clear of the tape, innov_step_kernel writing the tape
 *                          and v, then shift_scan_kernel (one lane group per instance) -- timed in the smoother slot of
 *                          mk_last_kernel_ms / mk_kernel_ms_totals.  d_num[b, t, j] = A and d_den[b, t, j] = D where cell (t, j) is
 *                          observed, NaN where it is not; [B, T, N] addressed by time_major like d_work.  Every sum has a fixed order:
 *                          an instance's outputs are bit-identical whatever the batch or the layout.  prob->warmup is ignored;
 *                          d_status (may be NULL) receives the filter's MK_FLAG_* bits -- the outputs of an instance with
 *                          MK_FLAG_NONPOSITIVE_F are not meaningful.
 *   Served: every supported shape with N + K <= 64, under either kernel family; otherwise MK_ERR_SHAPE.  MK_ERR_INVALID (no
 * launch): a missing pointer or a buffer larger than the allocation it points into. */
typedef struct mk_shift_request {
    double *d_num;                /* [B, T, N]: A = x'u of the shift of series j from step t on */
    double *d_den;                /* [B, T, N]: D = x'Mx */
} mk_shift_request;
MK_API int64_t mk_shift_work_stride(int64_t N, int64_t K);
MK_API int mk_level_shifts(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major, const mk_shift_request *req,
                           uint32_t *d_status);

/* ---- exact window means, changes and contrasts of the smoothed signal (functional_kernels.hip) --------------------------------
 * The posterior mean and variance of LINEAR functionals of the smoothed path, per instance b (record r = b % n_records), window w
 * and contrast c:
 *     l = sum_t alpha_t c'(scale o Z x_t + offset),     alpha_t = 1/(t1 - t0) on [t0, t1),   -1/(t3 - t2) on [t2, t3),
 * (t0, t1, t2, t3) = d_windows[r, w], two half-open step ranges: with t2 == t3 the mean of the signal over a window, with t1 - t0 = 1 a
 * point value, with both ranges "period A minus period B" (disjoint ranges in either order).  It is a functional of the SIGNAL Z x,
 * as d_sim_means / d_sim_vars are: no observation variance is added; scale / offset are those of mk_problem (1 / 0 when NULL).  The
 * posterior is Gaussian, mean = sum_t w_t' S_t + (sum_t alpha_t) c'offset and, with w_t = alpha_t Z'(c o scale),
 *     var = sum_t w_t' Ps_t w_t + 2 sum_{t<s} w_t' J_t ... J_{s-1} Ps_s w_s,      J_t = Pf_t Phi Pp_{t+1}^-1,  Pp_{t+1} = Phi Pf_t Phi + Q,
 * the second sum over the smoother's covariance ACROSS time, Cov(x_t, x_s | Y) = J_t ... J_{s-1} Ps_s (the smoothed state
 * autocovariance: de Jong & Mackinnon 1988; Durbin & Koopman 2012, section 4.7; what statsmodels returns as smoothed_state_autocov),
 * summed by one backward walk of the hull of the two ranges:  c_t = J_t u_{t+1},  p_t = Ps_t w_t,  var += w_t'(p_t + 2 c_t),
 * u_t = p_t + c_t.  The [T,T,n,n] object is never formed.
 *   mk_functionals_max_contrasts  64
 *   mk_functionals_work_stride    doubles per (instance, step) of d_work (the filtered and the smoothed record); 0 where the route
 *                                 does not serve the shape (N + K > 64)
 *   mk_functionals                runs the recording forward pass and the smoother that mk_filter_smooth runs for the shape (full-square
 *                                 records) into d_work, then one walk per (instance, window), the window's contrasts against one
 *                                 factorisation of Pp_{t+1} per step.  d_mean, d_var [B, W, C].  d_contrasts [n_records, C, N], or NULL = the
 *                                 N unit contrasts (n_contrasts must then be N).  Ranges are clamped to [0, T]; a functional whose first
 *                                 range is empty is NaN in both outputs; a variance that rounding takes below zero is stored as zero.
 *                                 Pivots of Pp_{t+1} as in the smoothers: a pivot <= 0 is dropped with MK_FLAG_RANK_DEFICIENT, < -1e-8 sets
 *                                 MK_FLAG_NOT_SPD (ORed into d_status beside the filter's and the smoother's bits).  An instance's
 *                                 results do not depend on the batch, on the other windows or on the other contrasts, bit for bit.
 *                                 MK_ERR_INVALID: a missing pointer, n_windows < 1, n_contrasts outside 1 .. 64, a buffer larger than its
 *                                 allocation; MK_ERR_SHAPE: N + K > 64 (packed-symmetric records are not served: the records are the
 *                                 call's own, full-square). */
typedef struct mk_functional_request {
    int64_t n_windows;            /* W per record, >= 1 */
    int64_t n_contrasts;          /* C per record, 1 .. mk_functionals_max_contrasts() */
    const int64_t *d_windows;     /* [n_records, W, 4] = (t0, t1, t2, t3) */
    const double *d_contrasts;    /* [n_records, C, N], or NULL: the N unit contrasts */
} mk_functional_request;
MK_API int64_t mk_functionals_max_contrasts(void);
MK_API int64_t mk_functionals_work_stride(int64_t N, int64_t K);
MK_API int mk_functionals(mk_context *ctx, const mk_problem *prob, double *d_work, int time_major,
                          const mk_functional_request *req, double *d_mean, double *d_var, uint32_t *d_status);

/* kalmansmoother for B instances (kalmanfilter.py:403-476).  Reads out->d_F and out->d_Pf
 * (as written by mk_filter); predicted moments are recomputed from them (Phi diagonal), so
 * d_Xp/d_Pp are not read.  Writes d_S, d_Ps (either may be NULL), d_status.  d_status is OVERWRITTEN (cleared on the context's
 * stream, then the smoother's bits), as by mk_smooth_dense; only mk_filter_smooth keeps the filter's bits beside the smoother's.
 * Also READS prob->d_obs (as does the smoother half of mk_filter_smooth) when prob->d_obsvar == NULL and prob->d_loadings is given,
 * for n <= 10 and full-square records without projection outputs: which steps observe every series decides the form of the covariance
 * products there (MK_VARIANT_SMOOTHER16).  The observations must be the ones out->d_F / d_Pf were filtered from, unchanged since
 * mk_filter; pass d_obs = NULL (or MK_VARIANT_SMOOTHER16 = 2) to smooth moments that come from elsewhere.  A per-record summary of
 * them is kept in the context: mk_observations_changed() after changing them in place. */
MK_API int mk_smooth(mk_context *ctx, const mk_problem *prob, const mk_outputs *out);

/* run_smoother (kalmanfilter.py:676-694): mk_filter then mk_smooth on the same stream. */
MK_API int mk_filter_smooth(mk_context *ctx, const mk_problem *prob, const mk_outputs *out);

/* SPKalmanFilter.simulate (kalmanfilter.py:569-603) for B instances:
 *   sim_means[b,t,:] = Z_b x[b,t];  sim_vars[b,t,j] = max((Z_b P[b,t] Z_b^T)_jj, 0)
 * Z is dense [RZ,N,n] (instance b uses Z[b % RZ]); Metran passes the std-scaled matrix
 * (metran/metran.py:944-961). */
MK_API int mk_simulate(mk_context *ctx, int64_t B, int64_t RZ, int64_t T, int64_t N, int64_t n,
                       const double *d_Z, const double *d_means /* [B,T,n] */,
                       const double *d_covs /* [B,T,n,n] */, double *d_sim_means /* [B,T,N] */,
                       double *d_sim_vars /* [B,T,N] */);

/* SPKalmanFilter.decompose (kalmanfilter.py:605-644):
 *   sdf[b,t,:] = Z[:, :N] x[b,t,:N];  cdf[b,k,t,:] = Z[:, N+k] * x[b,t,N+k] */
MK_API int mk_decompose(mk_context *ctx, int64_t B, int64_t RZ, int64_t T, int64_t N, int64_t n,
                        const double *d_Z, const double *d_means /* [B,T,n] */,
                        double *d_sdf /* [B,T,N] */, double *d_cdf /* [B,n-N,T,N] */);

/* Sum of d_mle over the local batch in a fixed order (deterministic tree), for the summed
 * objective fed back to the solver; mk_allreduce_sum below combines the ranks. */
MK_API int mk_sum(mk_context *ctx, int64_t count, const double *d_values, double *d_result /* [1] */);

/* ---- the one collective of the path (SURVEY.md 8b "mk_allreduce_sum(ctx, buf, count) (RCCL) or accept an external
 * communicator", 8e): one process per GPU, every model independent, so the only exchange is the summed objective of a
 * shared-parameter calibration -- 1 double, or P + 1 with the adjoint gradient -- fed back to the solver
 * (metran/solver.py:42-63 has one process and no counterpart).  The communicator is RCCL's (ncclComm_t, passed as void *
 * so that this header needs no rccl.h); librccl is bound with dlopen at the first of these calls, preferring a copy the
 * process has already loaded (e.g. PyTorch-ROCm's), so a single-GPU caller never maps it.
 *   mk_comm_set_library    (optional, before the first call below) the path of the librccl.so to bind; the library reads
 *                          no environment variable
 *   mk_comm_unique_id      ncclGetUniqueId into a caller buffer of 128 bytes: ONE rank calls it and hands the bytes to
 *                          the others by whatever side channel the job has (a file, MPI, torch.distributed's store)
 *   mk_comm_init_rank      ncclCommInitRank for this context's device; collective (every rank calls it with the same
 *                          id); the context owns the communicator and destroys it in mk_comm_destroy / mk_destroy
 *   mk_set_communicator    use a communicator the CALLER created and keeps owning (a raw librccl one); NULL detaches
 *   mk_allreduce_sum       in-place all-reduce(sum, float64) of d_buf[count] over the communicator's ranks, ordered on
 *                          the context's stream (mk_set_stream); asynchronous like every launch (mk_sync to wait).
 *                          Without a communicator it FAILS (MK_ERR_INVALID): there is no silent single-rank shortcut --
 *                          a group of one rank still runs the collective, as on eight */
MK_API int mk_comm_set_library(const char *path);
MK_API int mk_comm_unique_id(void *id128 /* [128 bytes] */);
MK_API int mk_comm_init_rank(mk_context *ctx, int nranks, int rank, const void *id128);
MK_API int mk_set_communicator(mk_context *ctx, void *nccl_comm);
MK_API int mk_comm_destroy(mk_context *ctx);
MK_API int mk_allreduce_sum(mk_context *ctx, double *d_buf, int64_t count);

/* ---- observation ingestion (what precedes the filter; batched) ------------------------------ */
/* Metran.standardize (metran/metran.py:102-121) for R models: per series, subtract the mean and
 * divide by the standard deviation (pandas semantics: NaN skipped, ddof = 1).  d_in / d_out are
 * [R,T,N] (or [T,R,N] when time_major != 0); d_out may equal d_in or be NULL (statistics only);
 * d_mean / d_std [R,N] may be NULL.  N <= 64.  +-inf is a value: a series holding one has mean +-inf (NaN with both signs)
 * and std NaN, so all of it standardises to NaN -- as do a series never observed, observed once (std NaN) or constant (std 0). */
MK_API int mk_standardize(mk_context *ctx, int64_t R, int64_t T, int64_t N, int time_major,
                          const double *d_in, double *d_out, double *d_mean, double *d_std);

/* Metran.mask_observations (metran/metran.py:464-494): d_out[i] = d_mask[i] ? NaN : d_obs[i] for
 * `count` observations in whatever layout d_obs has (d_mask: one byte each, non-zero = hide).
 * Unmasking is re-running the filter on the untouched d_obs: no re-upload. */
MK_API int mk_mask_observations(mk_context *ctx, int64_t count, const double *d_obs,
                                const unsigned char *d_mask, double *d_out);

/* SPKalmanFilter.set_observations (metran/kalmanfilter.py:646-674) for R models: the reference's
 * packed arrays from NaN-encoded observations d_obs [R,T,N] (model-major): d_observations [R,T,N]
 * (missing -> 0.0), d_indices [R,T,N] (doubles holding ints, left-packed), d_count [R,T] (int64).
 * Any output may be NULL.  The filter kernels read d_obs directly; this exists for callers that
 * want the reference's representation (the 9-argument engine callable). */
MK_API int mk_pack_observations(mk_context *ctx, int64_t R, int64_t T, int64_t N, const double *d_obs,
                                double *d_observations, double *d_indices, int64_t *d_count);

/* ---- batched factor analysis (what produces the loadings; metran/factoranalysis.py) ----------- */
/* FactorAnalysis._get_correlations (factoranalysis.py:404-418; pandas DataFrame.corr, pearson, pairwise
 * complete): d_corr [R,N,N] from NaN-encoded d_obs [R,T,N] ([T,R,N] when time_major != 0).  N <= 64.  An entry is NaN when
 * the pair has no common row or one of the two series is constant on the common rows (the diagonal is 1 or NaN by the same
 * rule).  +-inf is a value, not a missing one: every pair that has an inf among its common rows is NaN (two-pass definition;
 * pandas' online algorithm returns an artefact there), and the other pairs are not affected. */
MK_API int mk_fa_correlation(mk_context *ctx, int64_t R, int64_t T, int64_t N, int time_major,
                             const double *d_obs, double *d_corr);
/* _get_eigval (:420-460), _maptest (:220-312), the factor-count rules of solve (:66-82; maxfactors <= 0 =
 * None) and the start vector of _minres (:188-203) for B correlation matrices.  d_eigval [B,N] descending,
 * clipped at 0; d_nfactors / d_nfactors_map / d_nfactors_map4 [B]; d_psi0 [B,N]; d_status [B]: 1 = no factors
 * can be derived (NaN correlation or singular matrix; the reference returns None).  Outputs may be NULL.
 * "Singular" is decided on the eigenvalues of the device's own decomposition: smallest eigenvalue <= 1e-14 x the largest.
 * DIVERGENCE from the reference: numpy.linalg.inv (factoranalysis.py:195) raises only on an EXACTLY zero pivot, so a
 * correlation matrix with a condition number above ~1e14 that is not exactly singular (nearly collinear series) makes
 * the reference proceed with an inverse that has no correct digits, while this routine reports status 1 (no factors). */
MK_API int mk_fa_analyse(mk_context *ctx, int64_t B, int64_t N, int64_t maxfactors, const double *d_corr,
                         double *d_eigval, int64_t *d_nfactors, int64_t *d_nfactors_map, int64_t *d_nfactors_map4,
                         double *d_psi0, uint32_t *d_status);
/* _minresfun (:315-347), _minresgrad (:349-373) and _get_loadings (:375-401) for B vectors d_psi [B,N];
 * instance b uses correlation matrix and factor count b % R.  d_fval [B], d_grad [B,N], d_loadings [B,N,KMAX]
 * (columns >= nfactors zero); any output may be NULL.
 * d_order [B,KMAX] (may be NULL): _get_loadings takes eigvec[:, :nf] in the order numpy.linalg.eig (LAPACK dgeev)
 * returns the pairs of psi^-1/2 S psi^-1/2 (:396-398), which is NOT sorted; d_order[b][f] is the rank (0 = largest
 * eigenvalue, < N) of the pair that becomes column f of instance b.  NULL = ranks 0 .. nf-1 (the nf largest,
 * descending).  The jacobian depends on it through the loadings; the objective does not. */
MK_API int mk_fa_minres(mk_context *ctx, int64_t B, int64_t R, int64_t N, int64_t KMAX, const double *d_corr,
                        const int64_t *d_nfactors, const double *d_psi, const int64_t *d_order, double *d_fval,
                        double *d_grad, double *d_loadings);
/* Communality normalisation + varimax rotation (_rotate, :121-171; gamma = 1, maxiter = 20, tol = 1e-6 in the
 * reference) + sign convention of FactorAnalysis.solve (:84-108), in place on d_loadings [B,N,KMAX]. */
MK_API int mk_fa_rotate(mk_context *ctx, int64_t B, int64_t N, int64_t KMAX, const int64_t *d_nfactors,
                        double *d_loadings, double gamma, int maxiter, double tol);
/* Symmetric eigen-decomposition of B matrices d_sym [B,N,N] (cyclic Jacobi): d_val [B,N] descending, d_vec
 * [B,N,N] eigenvectors in columns (may be NULL).  The one dense-linear-algebra routine of the kernels above. */
MK_API int mk_fa_eigh(mk_context *ctx, int64_t B, int64_t N, const double *d_sym, double *d_val, double *d_vec);

/* ---- instrumentation --------------------------------------------------------------------- */
/* When enabled, every kernel launch is bracketed by hipEvents on the context's stream.  enable = 1: the most recent
 * launch of each kind is kept (mk_last_kernel_ms); enable = 2: EVERY launch keeps its own event pair until
 * mk_kernel_ms_totals collects them -- no host synchronisation inside a timed loop. */
MK_API int mk_enable_timing(mk_context *ctx, int enable);
/* Duration of the most recent filter / smoother kernel (ms); synchronises on their events. */
MK_API int mk_last_kernel_ms(mk_context *ctx, float *filter_ms, float *smoother_ms);
/* enable = 2: summed duration (ms) and number of the filter (or objective) and smoother launches since the previous
 * call (or since timing was enabled); synchronises on their events and recycles them. */
MK_API int mk_kernel_ms_totals(mk_context *ctx, double *filter_ms, int64_t *filter_launches, double *smoother_ms,
                               int64_t *smoother_launches);

#ifdef __cplusplus
}
#endif
#endif /* METRAN_HIP_H */
