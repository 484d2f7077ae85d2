"""The compile-time switches of the specialised kernels, restated in Python, and MATRIX: the shapes on which the GPU tier runs
both sides of every one of them (tests/test_shape_matrix_gpu.py).  tests/test_shape_matrix.py checks, without a GPU, that
MATRIX covers both sides of every switch, that every shape of it is prebuilt, and that each switch still reads in the kernel
source as it is restated here.

A switch is ``SWITCHES[name] = (domain, predicate, file, source text, C expression)``:
  domain      "narrow" (n <= 16, 16-lane groups), "wide" (16 < n <= 64, one wavefront), "split" (wide, N <= 32: the split
              layout of mk_split.hip), "dist" (split with DIST), "tape" (16 < n <= 63: the backward tape of mk_dk.hip) or
              "all": the shapes on which the switch exists at all
  predicate   f(N, K) -> bool
  source      the line of the kernel source the switch is decided on, matched textually (a comment after it is ignored)
  C           the expression of that line (None: a derived case, not a switch); evaluated over every shape of the domain
              with N + K <= 64, it must equal the predicate
"""
import re

WAVE_SMOOTHER_MAX_N = 51   # mk_internal.h: wave_smoother_max_n

# file:line as of this writing; the text, not the line number, is what tests/test_shape_matrix.py holds the source to
SWITCHES = {
    # mk_kernels.hip:2419 (launch_filter_nk: filter_kernel, else filter_wave_kernel) / :2474 (launch_smoother_nk): a 16-lane group
    # per model, else one wavefront
    "narrow": ("all", lambda N, K: N + K <= 16, "mk_kernels.hip",
               "constexpr int G = n <= 16 ? 16 : 64;", "n <= 16"),
    # mk_kernels.hip:2481: smoother_blk_kernel (the MFMA record smoother of the narrow models) exists for n <= 15 only
    "blk": ("narrow", lambda N, K: N + K <= 15, "mk_kernels.hip", "if constexpr (n <= 15) {", "n <= 15"),
    # mk_kernels.hip:81 (filter_kernel) / :1818 (sparse objective): Z's loading block replicated in registers; :476
    # (filter_wave_kernel): the loadings picked by readlanes, beyond that from an LDS table
    "HOIST": ("all", lambda N, K: N * K <= 32, "mk_kernels.hip",
              "constexpr bool HOIST = (N * K <= 32);", "(N * K <= 32)"),
    # mk_split.hip:1268 (launch_split_nk): the split layout (and the tape writer filter_obs_kernel) serves N <= 32
    "split": ("wide", lambda N, K: N <= 32, "mk_split.hip", "if constexpr (N + K > 16 && N <= 32) {", "N + K > 16 && N <= 32"),
    # mk_split.hip:1269: H lanes per model
    "H16": ("split", lambda N, K: N <= 16, "mk_split.hip",
            "constexpr int H = N <= 16 ? 16 : 32, M = 64 / H;", "N <= 16"),
    # mk_split.hip:175 (filter_split_kernel) / :720 (filter_obs_kernel): 16-byte factor parts and entry scalars
    "PAIRS": ("split", lambda N, K: K % 2 == 0 and N % 2 == 0, "mk_split.hip",
              "constexpr bool PAIRS = (K % 2 == 0 && N % 2 == 0);", "(K % 2 == 0 && N % 2 == 0)"),
    # mk_split.hip:738 (filter_obs_kernel): the factor block and means one element per lane, read back in 16-byte pairs
    "DIST": ("split", lambda N, K: dist(N, K), "mk_split.hip",
             "constexpr bool DIST = (KF + K <= H) && (K % 2 == 0) && !MK_TUNE_SKIP(a, 512);",
             "(KF + K <= H) && (K % 2 == 0) && !MK_TUNE_SKIP(a, 512)"),
    # mk_split.hip:740: an odd KF + K makes the last pair DIST reads back (:924, :1170) half padding -- not a switch of its
    # own (no C expression), a case of DIST the matrix must hold both sides of
    "DIST_odd": ("dist", lambda N, K: (kf(K) + K) % 2 == 1, "mk_split.hip", "constexpr int FV = (KF + K + 1) & ~1;", None),
    # mk_kernels.hip:2441 (launch_filter_nk): filter_wave_kernel (lane per state) writes the tape of the models beyond the split layout
    "lps_tape": ("wide", lambda N, K: N > 32, "mk_kernels.hip", "if constexpr (n > 16 && N > 32) {", "n > 16 && N > 32"),
    # mk_wide.hip:276 (smoother_mfma_kernel): the rows of A folded into the lanes the model does not use
    "FOLD": ("wide", lambda N, K: N + K <= 36, "mk_wide.hip", "constexpr bool FOLD = FOLDP && n <= 36;", "FOLDP && n <= 36"),
    # mk_wide.hip:286 (smoother_mfma_kernel): MFMA tiles over the series block only
    "STR": ("wide", lambda N, K: N % 16 == 0 and K <= 4, "mk_wide.hip",
            "constexpr bool STR = (N % 16 == 0) && (K <= 4);", "(N % 16 == 0) && (K <= 4)"),
    # mk_wide.hip:1058 (launch_wave_nk): the round-1 smoother (wide_smoother "v1") is instantiated up to n = 51
    # (mk_internal.h:28: its compile time grows steeply beyond)
    "v1": ("wide", lambda N, K: N + K <= WAVE_SMOOTHER_MAX_N, "mk_wide.hip",
           "if constexpr (N + K > 16 && N + K <= wave_smoother_max_n) {", "N + K > 16 && N + K <= wave_smoother_max_n"),
    # mk_dk.hip:539 (launch_dk_nk): the tape (projection, state variances) and the LOO tape walk serve 16 < n <= 63
    "tape": ("wide", lambda N, K: N + K + 1 <= 64 and K <= 16, "mk_dk.hip",
             "if constexpr (N + K > 16 && N + K + 1 <= 64 && K <= 16) {", "N + K > 16 && N + K + 1 <= 64 && K <= 16"),
    # mk_dk.hip:72 (smoother_dk_kernel): 16-byte side rows
    "dk_PAIRS": ("tape", lambda N, K: N % 2 == 0 and K % 2 == 0, "mk_dk.hip",
                 "constexpr bool PAIRS = (N % 2 == 0 && K % 2 == 0);", "(N % 2 == 0 && K % 2 == 0)"),
    # mk_dk.hip:85 (smoother_dk_kernel): the guarded DPP statements beyond two wavefronts' worth of registers
    "GD": ("tape", lambda N, K: N + K > 40, "mk_dk.hip", "constexpr bool GD = (n > 40);", "(n > 40)"),
}

# combinations that must each occur among MATRIX (the gaps the matrix was made to close)
CASES = {
    "DIST with an odd KF + K at H = 32 (K = 6)": lambda N, K: in_domain("dist", N, K) and not SWITCHES["H16"][1](N, K) and K == 6,
    "DIST with an even KF + K and PAIRS false": lambda N, K: in_domain("dist", N, K) and (kf(K) + K) % 2 == 0
    and not SWITCHES["PAIRS"][1](N, K),
    "a full 16-lane group (n = 16) with HOIST false": lambda N, K: N + K == 16 and N * K > 32,
    "split layout with an odd K > 3": lambda N, K: in_domain("split", N, K) and K % 2 == 1 and K > 3,
    "smoother_dk_kernel with GD and PAIRS": lambda N, K: in_domain("tape", N, K) and N + K > 40 and N % 2 == 0 and K % 2 == 0,
    "a non-STR MFMA smoother above 36 states": lambda N, K: N + K > 36 and not SWITCHES["STR"][1](N, K),
    "FOLD's edge from both sides (n = 36)": lambda N, K: N + K == 36,
    "FOLD's edge from both sides (n = 37)": lambda N, K: N + K == 37,
    "one series past the split layout (N = 33)": lambda N, K: N == 33,
    "the widest tape (n = 63)": lambda N, K: N + K == 63,
    "a full wavefront (n = 64)": lambda N, K: N + K == 64,
    "the narrowest wide shape": lambda N, K: N + K == 17,
}

# the shapes of tests/test_shape_matrix_gpu.py: the ones the GPU tier ran before that flip something, then the new ones
MATRIX = [
    (8, 2), (14, 2), (16, 2), (19, 2), (11, 6), (32, 4), (48, 3),
    (12, 4),   # n = 16: a full 16-lane group, HOIST false; LOO, adjoint and sparse objective at n = 16
    (13, 4),   # n = 17, H = 16: DIST with an even KF + K = 14 and PAIRS false
    (20, 6),   # K = 6: DIST with an odd KF + K = 27 at H = 32, PAIRS true, a non-STR smoother with K > 4
    (23, 5),   # odd K above 3: no DIST, PAIRS false, the odd tails of the K-wide rows
    (33, 4),   # one series past the split layout (lane-per-state tape writer), one state past FOLD, not STR, not GD
    (40, 4),   # GD with PAIRS in smoother_dk_kernel, not STR
    (59, 4),   # n = 63: the widest tape / LOO shape (the r row on lane 63)
    (60, 4),   # n = 64: a full wavefront; tape and LOO refuse it
]


def kf(K):
    """Elements of the factor block's upper triangle (mk_split.hip: KF)."""
    return K * (K + 1) // 2


def dist(N, K):
    H = 16 if N <= 16 else 32
    return kf(K) + K <= H and K % 2 == 0


def in_domain(domain, N, K):
    n = N + K
    return {"all": True, "narrow": n <= 16, "wide": n > 16, "split": n > 16 and N <= 32,
            "dist": n > 16 and N <= 32 and dist(N, K), "tape": 16 < n <= 63}[domain]


def c_expression(expr, N, K):
    """Evaluate a switch's C expression (as written in the kernel source) for (N, K): the operators of the expressions above
    only, with the tuning hook MK_TUNE_SKIP off and FOLDP (the folding variant) on."""
    n = N + K
    H = 16 if N <= 16 else 32
    py = expr.replace("&&", " and ").replace("||", " or ")
    py = re.sub(r"!MK_TUNE_SKIP\([^)]*\)", "True", py)
    py = re.sub(r"!(?!=)", " not ", py)
    return bool(eval(py, {"__builtins__": {}}, dict(N=N, K=K, n=n, H=H, KF=kf(K), FOLDP=True,
                                                         wave_smoother_max_n=WAVE_SMOOTHER_MAX_N)))
