// mk_capi.hip -- C ABI of libmetran_hip.so (declared in include/metran_hip.h).
// Thin, exception-free layer: argument validation, ONE lookup of the (N,K) kernels (find_ops), HIP error ->
// mk_status translation, optional hipEvent timing of the two hot kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <dlfcn.h>
#include <mutex>
#include <vector>
#include <new>

#include "block_kernels.h"
#include "shift_kernels.h"
#include "draw_kernels.h"
#include "ensemble_kernels.h"
#include "forecast_kernels.h"
#include "functional_kernels.h"
#include "innov_kernels.h"
#include "resid_kernels.h"
#include "mk_generic.h"
#include "mk_internal.h"
#include "mk_lbfgs.h"
#include "regress_kernels.h"
#include "score_kernels.h"
#include "weights_kernels.h"

struct mk_context {
    int device;
    hipStream_t stream;
    int timing;       // 0 off, 1 the most recent launch of each kind, 2 every launch until mk_kernel_ms_totals
    hipEvent_t ev[4]; // filter start/stop, smoother start/stop (mode 1)
    bool have_filter_time, have_smooth_time;
    std::vector<hipEvent_t> ev_pool;                              // mode 2: recycled events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pending[2]; // mode 2: one (start, stop) pair per launch; 0 filter, 1 smoother
    int *tlist;      // workspace of the sparse objective (observed-step list), grown on demand
    long tlist_cap;
    // the list is rebuilt only when the record it was built from changes: same pointer, shape and layout, and no
    // mk_observations_changed() since (the solver evaluates the objective ~80 times on one uploaded record)
    const double *tlist_obs;
    long tlist_T, tlist_N, tlist_ostep;
    // which records take the record smoother's rank-K covariance step (mk::launch_full_records): device bytes [R] and, in one
    // word (lr_any: mk::MK_FULL_ANY | mk::MK_FULL_GAP), "any of them" and "some record has a step that is not full",
    // counted once per observation set -- same pointer, shape and layout, and no mk_observations_changed() since
    unsigned char *lr_take;
    long lr_cap;
    int *lr_any_dev;
    const double *lr_obs;
    long lr_R, lr_T, lr_N, lr_bs;
    int lr_any;
    int variant[MK_VARIANT_COUNT]; // mk_set_kernel_variant: which of two equivalent (tested) kernels serves a shape class
    double *gws;       // workspace of the size-generic smoother (mk_generic.hip), grown on demand
    size_t gws_cap;    // ... in doubles
    int *lb_counters;  // device int[4] of the L-BFGS kernels (mk_lbfgs.hip)
    double *adj_upd;   // update tape of the wide adjoint gradient (mk_set_adjoint_updates; caller-owned), nullptr = recompute
    size_t adj_upd_cap; // ... its capacity in doubles
    double *cur_upd;   // the tape of the recording forward pass in progress (set around do_filter by mk_loglik_grad_phases)
    void *comm;        // RCCL communicator of mk_allreduce_sum (ncclComm_t), nullptr = none
    bool comm_owned;   // created by mk_comm_init_rank (destroyed with the context) or handed in by mk_set_communicator
};

static thread_local char g_err[512] = "";

static int fail(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

#define MK_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess) return fail(MK_ERR_HIP, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

#define MK_CTX(ctx)                                              \
    if (!(ctx)) return fail(MK_ERR_INVALID, "null mk_context"); \
    MK_HIP(hipSetDevice((ctx)->device))

// ---- hipEvent timing of the hot kernels: kind 0 = filter / objective, 1 = smoother ----
static hipError_t timing_start(mk_context *ctx, int kind)
{
    if (!ctx->timing) return hipSuccess;
    if (ctx->timing == 2) {
        hipEvent_t e[2];
        for (auto &x : e) {
            if (!ctx->ev_pool.empty()) {
                x = ctx->ev_pool.back();
                ctx->ev_pool.pop_back();
            } else {
                const hipError_t err = hipEventCreate(&x);
                if (err != hipSuccess) return err;
            }
        }
        ctx->ev_pending[kind].push_back({e[0], e[1]});
        return hipEventRecord(e[0], ctx->stream);
    }
    return hipEventRecord(ctx->ev[2 * kind], ctx->stream);
}
static hipError_t timing_stop(mk_context *ctx, int kind)
{
    if (!ctx->timing) return hipSuccess;
    if (ctx->timing == 2) return hipEventRecord(ctx->ev_pending[kind].back().second, ctx->stream);
    (kind ? ctx->have_smooth_time : ctx->have_filter_time) = true;
    return hipEventRecord(ctx->ev[2 * kind + 1], ctx->stream);
}

// ---- shape lookup: the ahead-of-time table (mk::shape_ops), then the run-time shape modules' tables (mkmod_ops; see the
// MK_SHAPE_MODULE block of mk_kernels.hip and metran_amd/jit.py) in registration order ----
namespace {
std::vector<const mk::ShapeOps *> g_modules;
std::mutex g_modules_mutex;

// The kernels of (N, K): the first entry that matches.  by_n_only: any entry of the same state dimension n = N + K serves --
// the smoother without projection and without a tape depends on n only (its kernel, instantiated for that entry's shape, runs).
// This is the only place that knows that rule; no two ahead-of-time shapes share an n.
const mk::ShapeOps *find_ops(int64_t N, int64_t K, bool by_n_only = false)
{
    const auto serves = [&](const mk::ShapeOps &o) { return (o.N == N && o.K == K) || (by_n_only && o.N + o.K == N + K); };
    int cnt = 0;
    const mk::ShapeOps *aot = mk::shape_ops(&cnt);
    for (int i = 0; i < cnt; ++i)
        if (serves(aot[i])) return &aot[i];
    std::lock_guard<std::mutex> lock(g_modules_mutex);
    for (const mk::ShapeOps *m : g_modules)
        if (serves(*m)) return m;
    return nullptr;
}
bool specialised(int64_t N, int64_t K) { return find_ops(N, K) != nullptr; }
bool generic_shape(int64_t N, int64_t K) { return N >= 1 && K >= 1 && N + K <= MK_GENERIC_MAX_STATES; }
hipError_t dispatch_filter(int N, int K, const mk::FilterArgs &a, hipStream_t s, bool force_generic = false)
{
    if (force_generic) return generic_shape(N, K) ? mk::launch_filter_generic(N, K, a, s) : hipErrorInvalidValue;
    if (const mk::ShapeOps *o = find_ops(N, K)) return o->filter(a, s);
    if (generic_shape(N, K)) return mk::launch_filter_generic(N, K, a, s); // any shape, not specialised (mk_generic.hip)
    return hipErrorInvalidValue;
}
hipError_t dispatch_sparse(int N, int K, const mk::SparseArgs &a, hipStream_t s)
{
    const mk::ShapeOps *o = find_ops(N, K);
    return o ? o->sparse(a, s) : hipErrorInvalidValue;
}
hipError_t dispatch_adjoint(int N, int K, const mk::AdjointArgs &a, hipStream_t s)
{
    const mk::ShapeOps *o = find_ops(N, K);
    return o ? o->adjoint(a, s) : hipErrorInvalidValue;
}
hipError_t dispatch_loo(int N, int K, const mk::AdjointArgs *na, const mk::SmootherArgs *wa, hipStream_t s)
{
    const mk::ShapeOps *o = find_ops(N, K);
    return o ? o->loo(na, wa, s) : hipErrorInvalidValue;
}
hipError_t dispatch_disturb(int N, int K, const mk::AdjointArgs &a, hipStream_t s)
{
    const mk::ShapeOps *o = find_ops(N, K);
    return o ? o->disturb(a, s) : hipErrorInvalidValue;
}
// workspace of the generic smoother: grown on demand, stream-ordered reuse (every launch of a context is on its stream)
hipError_t generic_workspace(mk_context *ctx, long B, int n, double **ws)
{
    const size_t need = mk::generic_smoother_ws_doubles(B, n);
    if (ctx->gws_cap < need) {
        if (ctx->gws) {
            hipError_t e = hipStreamSynchronize(ctx->stream); // a launch still reading the old buffer
            if (e != hipSuccess) return e;
            e = hipFree(ctx->gws);
            if (e != hipSuccess) return e;
        }
        ctx->gws = nullptr;
        ctx->gws_cap = 0;
        const hipError_t e = hipMalloc((void **)&ctx->gws, need * sizeof(double));
        if (e != hipSuccess) return e;
        ctx->gws_cap = need;
    }
    *ws = ctx->gws;
    return hipSuccess;
}
hipError_t dispatch_smoother(mk_context *ctx, int N, int K, const mk::SmootherArgs &a, hipStream_t s)
{
    // the plain smoother depends on n = N + K only; the projecting one and the tape's backward pass (the state tape without a
    // projection included: a (16,2) tape walked by the (17,1) module's kernel was the defect the (16,2) state-tape test found)
    // need the exact (N, K)
    const bool proj = a.sim_means || a.sim_vars || a.tape != 0;
    const bool force_generic = ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 1;
    if (!force_generic) {
        if (const mk::ShapeOps *o = find_ops(N, K)) return o->smoother(a, s);
        if (!proj)
            if (const mk::ShapeOps *o = find_ops(N, K, true)) {
                mk::SmootherArgs b = a; // a kernel of the same n but another (N, K): the rank-K step reads the loadings as [N, K]
                b.obs = nullptr;
                return o->smoother(b, s);
            }
    }
    if (generic_shape(N, K)) {
        mk::GenericSmootherArgs g;
        g.a = a;
        g.N = N;
        g.K = K;
        g.Xp = g.Pp = nullptr;
        const hipError_t e = generic_workspace(ctx, a.B, N + K, &g.ws);
        if (e != hipSuccess) return e;
        return mk::launch_smoother_generic(g, s);
    }
    return hipErrorInvalidValue;
}
} // namespace

// ---- what the kernels' argument blocks share, filled from mk_problem.  FilterArgs, AdjointArgs, InnovArgs, ForecastArgs, WeightsArgs and DrawArgs
// spell these fields alike (SparseArgs and SmootherArgs a part of them); the structs themselves stay apart, because a kernel that
// takes its block by value is compiled against that block's layout ----
template <class Args>
static void fill_model(Args &a, const mk_problem *p) // sizes, observation strides, model pointers
{
    a.B = p->n_instances;
    a.R = p->n_records;
    a.T = p->T;
    a.obs_bs = p->obs_time_major ? 1 : p->T;
    a.obs_ts = p->obs_time_major ? p->n_records : 1;
    a.obs = p->d_obs;
    a.phi = p->d_phi;
    a.q = p->d_q;
    a.loadings = p->d_loadings;
    a.obsvar = p->d_obsvar;
}
template <class Args>
static void fill_initial(Args &a, const mk_problem *p)
{
    a.x0 = p->d_x0;
    a.P0 = p->d_P0;
}
template <class Args>
static void fill_scaling(Args &a, const mk_problem *p)
{
    a.scale = p->d_scale;
    a.offset = p->d_offset;
}
template <class Args>
static void fill_layout(Args &a, int time_major, int64_t B, int64_t T) // block (b, t) at b*bs + t*ts
{
    a.bs = time_major ? 1 : T;
    a.ts = time_major ? B : 1;
}
template <class Args>
static auto fill_shape(Args &a, const mk_problem *p, int) -> decltype((void)a.K) // the blocks that carry N and K
{
    a.N = (int)p->N;
    a.K = (int)p->K;
}
template <class Args>
static void fill_shape(Args &, const mk_problem *, long) {}
template <class Args>
static auto fill_records(Args &a, const double *d_work, int64_t rs, int) -> decltype((void)a.F) // the blocks that read the records
{
    a.rs = rs;
    a.F = d_work;
}
template <class Args>
static void fill_records(Args &, const double *, int64_t, long) {}

// What the kernel block of every record reader starts from: zeroed, then the problem, the initial moments, the layout, the filtered
// records of rs doubles that the recording forward pass left at the head of d_work, and N and K where the block has them.
template <class Args>
static Args reader_args(const mk_problem *p, const double *d_work, int64_t rs, int time_major)
{
    Args a;
    memset(&a, 0, sizeof(a));
    fill_model(a, p);
    fill_initial(a, p);
    fill_layout(a, time_major, p->n_instances, p->T);
    fill_shape(a, p, 0);
    fill_records(a, d_work, rs, 0);
    return a;
}

// ---- the workspace d_work of the record readers: the one place that knows its format.  The filtered records of B * T steps are
// packed at the head; behind them, each for all B * T steps, the regions of the reader's kind: the gain tape (N slots of gs doubles
// per step) and behind it the scores' row of N innovations, the forecast skill's partial sums, or the smoothed records.
// (mk_loo's wide branch is no record reader: its d_work is the tape of MK_OUT_TAPE.) ----
enum work_kind { WORK_RECORDS, WORK_FORECAST, WORK_GAIN, WORK_SCORES, WORK_FUNCTIONALS };
struct work_layout {
    int64_t rs, gs;                         // doubles per record and per gain slot (0: no tape)
    int64_t stride;                         // doubles per (instance, step) of the whole workspace: what mk_*_work_stride returns
    int64_t tape, innov, partial, smoothed; // where each region starts, in doubles from d_work (0: the kind has none)
};
static work_layout layout_of(work_kind kind, int64_t N, int64_t K, int64_t B = 0, int64_t T = 0)
{
    work_layout w = {};
    w.rs = w.stride = mk::record_stride((int)(N + K));
    const auto region = [&](int64_t doubles_per_step) {
        const int64_t at = B * T * w.stride;
        w.stride += doubles_per_step;
        return at;
    };
    if (kind == WORK_GAIN || kind == WORK_SCORES) {
        w.gs = mk::weights_slot_stride(N + K);
        w.tape = region(N * w.gs);
    }
    if (kind == WORK_SCORES) w.innov = region(N);
    if (kind == WORK_FORECAST) w.partial = region(mk::forecast_partial_stride(N));
    if (kind == WORK_FUNCTIONALS) w.smoothed = region(w.rs);
    return w;
}

// The launches of a record reader behind its forward pass, timed as one: reported in the smoother slot of mk_last_kernel_ms /
// mk_kernel_ms_totals (for mk_functionals beside the smoother's own launch).
template <class Launches>
static int timed_launches(mk_context *ctx, Launches launches)
{
    MK_HIP(timing_start(ctx, 1));
    if (int rc = launches()) return rc;
    MK_HIP(timing_stop(ctx, 1));
    return MK_OK;
}

// Each buffer must end inside the device allocation it starts in (an interior pointer of a pooled allocation passes whenever the
// pool's block is large enough -- the check catches a buffer that is too small, not every misuse).
struct device_buffer { const void *ptr; int64_t doubles; const char *name; };
static int buffers_fit(const char *who, const device_buffer *bufs, int count)
{
    for (int k = 0; k < count; ++k) {
        const device_buffer &b = bufs[k];
        if (!b.ptr) continue;
        hipDeviceptr_t base = nullptr;
        size_t bytes = 0;
        if (hipMemGetAddressRange(&base, &bytes, (hipDeviceptr_t)b.ptr) != hipSuccess) {
            (void)hipGetLastError(); // not a hipMalloc allocation: its size cannot be known here
            continue;
        }
        if ((const char *)b.ptr + b.doubles * (int64_t)sizeof(double) > (const char *)base + bytes)
            return fail(MK_ERR_INVALID, "%s: %s is larger than the device allocation it points into", who, b.name);
    }
    return MK_OK;
}

// the refusal of the entry points whose kernels hold one state per lane
static int too_many_states(const char *who, const mk_problem *p, int max_states)
{
    return fail(MK_ERR_SHAPE, "%s serves N + K <= %d states (got N=%lld, K=%lld)", who, max_states, (long long)p->N, (long long)p->K);
}

extern "C" {

MK_API int mk_register_shape_module(const char *path)
{
    if (!path) return fail(MK_ERR_INVALID, "null module path");
    void *h = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!h) return fail(MK_ERR_INVALID, "dlopen(%s): %s", path, dlerror());
    const auto refuse = [&](const char *why) {
        dlclose(h);
        return fail(MK_ERR_INVALID, "%s %s", path, why);
    };
    auto abi = (int (*)(void))dlsym(h, "mkmod_abi");
    if (!abi) return refuse("is not a metran_hip shape module");
    // checked before anything else of the module is touched: one built for other structs or another table is refused, not misread
    if (abi() != mk::module_abi()) return refuse("was built against different kernel-argument structs (stale cache)");
    auto ops = (const mk::ShapeOps *(*)(int *))dlsym(h, "mkmod_ops");
    if (!ops) return refuse("is not a metran_hip shape module");
    int cnt = 0;
    const mk::ShapeOps *o = ops(&cnt);
    if (cnt != 1) return refuse("must contain exactly one (N,K) shape");
    std::lock_guard<std::mutex> lock(g_modules_mutex);
    for (const mk::ShapeOps *m : g_modules)
        if (m->N == o->N && m->K == o->K) {
            dlclose(h);
            return MK_OK; // already registered
        }
    g_modules.push_back(o); // the handle stays open for the life of the process
    return MK_OK;
}

MK_API int mk_abi_version(void) { return MK_ABI_VERSION; }
MK_API const char *mk_last_error(void) { return g_err; }

MK_API int mk_device_count(int *count)
{
    if (!count) return fail(MK_ERR_INVALID, "null count");
    int c = 0;
    hipError_t e = hipGetDeviceCount(&c);
    if (e != hipSuccess) {
        *count = 0;
        return fail(MK_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = c;
    return MK_OK;
}

MK_API int mk_create(int device, mk_context **out)
{
    if (!out) return fail(MK_ERR_INVALID, "null ctx out-pointer");
    *out = nullptr;
    int c = 0;
    if (hipGetDeviceCount(&c) != hipSuccess || c <= 0)
        return fail(MK_ERR_NO_DEVICE, "no HIP device visible (libmetran_hip needs an MI355X / gfx950)");
    if (device < 0 || device >= c) return fail(MK_ERR_INVALID, "device %d out of range [0,%d)", device, c);
    MK_HIP(hipSetDevice(device));
    hipDeviceProp_t prop;
    MK_HIP(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(MK_ERR_NO_DEVICE, "device %d is %s; this library is built for gfx950 only", device,
                    prop.gcnArchName);
    mk_context *ctx = new (std::nothrow) mk_context();
    if (!ctx) return fail(MK_ERR_ALLOC, "out of host memory");
    ctx->device = device;
    ctx->stream = nullptr;
    ctx->timing = 0;
    ctx->have_filter_time = ctx->have_smooth_time = false;
    ctx->tlist = nullptr;
    ctx->tlist_cap = 0;
    ctx->tlist_obs = nullptr;
    ctx->tlist_T = ctx->tlist_N = ctx->tlist_ostep = 0;
    ctx->lr_take = nullptr;
    ctx->lr_cap = 0;
    ctx->lr_any_dev = nullptr;
    ctx->lr_obs = nullptr;
    ctx->lr_R = ctx->lr_T = ctx->lr_N = ctx->lr_bs = 0;
    ctx->lr_any = 0;
    ctx->gws = nullptr;
    ctx->gws_cap = 0;
    ctx->lb_counters = nullptr;
    ctx->comm = nullptr;
    ctx->comm_owned = false;
    ctx->adj_upd = ctx->cur_upd = nullptr;
    ctx->adj_upd_cap = 0;
    for (int &v : ctx->variant) v = 0;
    for (auto &e : ctx->ev) {
        if (hipEventCreate(&e) != hipSuccess) {
            delete ctx;
            return fail(MK_ERR_HIP, "hipEventCreate failed");
        }
    }
    *out = ctx;
    return MK_OK;
}

// ---- the one collective of the design: all-reduce(sum, f64) of the summed objective over the ranks ----
// librccl is bound at first use with dlopen -- the library has no link-time dependency on it, so a single-GPU caller never
// loads it -- preferring a copy the process has already mapped (PyTorch-ROCm ships its own librccl.so: two RCCL runtimes in
// one process would each bootstrap their own network state).  Only the five entry points below are used; their
// signatures are RCCL's public C API (rccl/rccl.h: ncclGetUniqueId :187, ncclCommInitRank :220, ncclCommDestroy :260,
// ncclAllReduce, ncclGetErrorString :339), restated here so that the header is not needed to build.
namespace {
struct RcclUniqueId {
    char internal[128]; // NCCL_UNIQUE_ID_BYTES
};
struct RcclApi {
    void *handle;
    int (*GetUniqueId)(RcclUniqueId *);
    int (*CommInitRank)(void **, int, RcclUniqueId, int);
    int (*CommDestroy)(void *);
    int (*AllReduce)(const void *, void *, size_t, int /*ncclDataType_t*/, int /*ncclRedOp_t*/, void *, hipStream_t);
    const char *(*GetErrorString)(int);
    char why[256];
};
RcclApi g_rccl = {};
char g_rccl_path[1024] = "";
std::mutex g_rccl_mutex;
constexpr int kNcclFloat64 = 8, kNcclSum = 0; // rccl.h: ncclFloat64 = 8, ncclSum = 0

const RcclApi *rccl_api()
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.handle) return &g_rccl;
    const char *names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *h = nullptr;
    if (g_rccl_path[0]) h = dlopen(g_rccl_path, RTLD_NOW | RTLD_GLOBAL);
    for (int pass = 0; pass < 2 && !h; ++pass) // pass 0: a copy that is already mapped; pass 1: load one
        for (const char *nm : names) {
            h = dlopen(nm, (pass == 0 ? RTLD_NOLOAD : 0) | RTLD_NOW | RTLD_GLOBAL);
            if (h) break;
        }
    if (!h) {
        snprintf(g_rccl.why, sizeof(g_rccl.why), "librccl.so could not be loaded (%s); name it with mk_comm_set_library", dlerror());
        return nullptr;
    }
    RcclApi a = {};
    a.GetUniqueId = (decltype(a.GetUniqueId))dlsym(h, "ncclGetUniqueId");
    a.CommInitRank = (decltype(a.CommInitRank))dlsym(h, "ncclCommInitRank");
    a.CommDestroy = (decltype(a.CommDestroy))dlsym(h, "ncclCommDestroy");
    a.AllReduce = (decltype(a.AllReduce))dlsym(h, "ncclAllReduce");
    a.GetErrorString = (decltype(a.GetErrorString))dlsym(h, "ncclGetErrorString");
    if (!a.GetUniqueId || !a.CommInitRank || !a.CommDestroy || !a.AllReduce || !a.GetErrorString) {
        snprintf(g_rccl.why, sizeof(g_rccl.why), "the loaded librccl lacks one of ncclGetUniqueId / ncclCommInitRank / ncclCommDestroy / "
                                                 "ncclAllReduce / ncclGetErrorString");
        return nullptr;
    }
    a.handle = h;
    g_rccl = a;
    return &g_rccl;
}
} // namespace

#define MK_RCCL(api, call)                                                                          \
    do {                                                                                            \
        const int r_ = (call);                                                                      \
        if (r_ != 0) return fail(MK_ERR_HIP, "%s: RCCL error %d: %s", #call, r_, (api)->GetErrorString(r_)); \
    } while (0)

MK_API int mk_comm_set_library(const char *path)
{
    std::lock_guard<std::mutex> lock(g_rccl_mutex);
    if (g_rccl.handle) return fail(MK_ERR_INVALID, "mk_comm_set_library: librccl is already bound in this process");
    if (!path || strlen(path) >= sizeof(g_rccl_path)) return fail(MK_ERR_INVALID, "mk_comm_set_library: bad path");
    strcpy(g_rccl_path, path);
    return MK_OK;
}

MK_API int mk_comm_unique_id(void *id128)
{
    if (!id128) return fail(MK_ERR_INVALID, "mk_comm_unique_id: null buffer (128 bytes)");
    const RcclApi *api = rccl_api();
    if (!api) return fail(MK_ERR_HIP, "mk_comm_unique_id: %s", g_rccl.why);
    RcclUniqueId id;
    MK_RCCL(api, api->GetUniqueId(&id));
    memcpy(id128, id.internal, sizeof(id.internal));
    return MK_OK;
}

MK_API int mk_comm_destroy(mk_context *ctx)
{
    if (!ctx) return fail(MK_ERR_INVALID, "null mk_context");
    if (ctx->comm && ctx->comm_owned) {
        const RcclApi *api = rccl_api();
        if (api) {
            (void)hipSetDevice(ctx->device);
            (void)api->CommDestroy(ctx->comm);
        }
    }
    ctx->comm = nullptr;
    ctx->comm_owned = false;
    return MK_OK;
}

MK_API int mk_comm_init_rank(mk_context *ctx, int nranks, int rank, const void *id128)
{
    MK_CTX(ctx);
    if (nranks < 1 || rank < 0 || rank >= nranks || !id128)
        return fail(MK_ERR_INVALID, "mk_comm_init_rank: bad argument (nranks %d, rank %d)", nranks, rank);
    const RcclApi *api = rccl_api();
    if (!api) return fail(MK_ERR_HIP, "mk_comm_init_rank: %s", g_rccl.why);
    (void)mk_comm_destroy(ctx);
    RcclUniqueId id;
    memcpy(id.internal, id128, sizeof(id.internal));
    void *comm = nullptr;
    MK_RCCL(api, api->CommInitRank(&comm, nranks, id, rank)); // collective: every rank of the job calls it
    ctx->comm = comm;
    ctx->comm_owned = true;
    return MK_OK;
}

MK_API int mk_set_communicator(mk_context *ctx, void *nccl_comm)
{
    if (!ctx) return fail(MK_ERR_INVALID, "null mk_context");
    (void)mk_comm_destroy(ctx); // an owned communicator is released; a borrowed one is just forgotten
    ctx->comm = nccl_comm;      // the caller keeps ownership (ncclCommDestroy is the caller's to call, after mk_destroy / a detach)
    ctx->comm_owned = false;
    return MK_OK;
}

MK_API int mk_allreduce_sum(mk_context *ctx, double *d_buf, int64_t count)
{
    if (!ctx) return fail(MK_ERR_INVALID, "null mk_context");
    if (!ctx->comm)
        return fail(MK_ERR_INVALID, "mk_allreduce_sum: this context has no communicator -- call mk_comm_init_rank (every rank, with "
                                    "the id of mk_comm_unique_id) or mk_set_communicator first; there is no single-rank shortcut");
    if (!d_buf || count <= 0) return fail(MK_ERR_INVALID, "mk_allreduce_sum: bad argument");
    MK_HIP(hipSetDevice(ctx->device));
    const RcclApi *api = rccl_api();
    if (!api) return fail(MK_ERR_HIP, "mk_allreduce_sum: %s", g_rccl.why);
    MK_RCCL(api, api->AllReduce(d_buf, d_buf, (size_t)count, kNcclFloat64, kNcclSum, ctx->comm, ctx->stream)); // in place, stream-ordered
    return MK_OK;
}

MK_API int mk_destroy(mk_context *ctx)
{
    if (!ctx) return MK_OK;
    (void)hipSetDevice(ctx->device);
    for (auto &e : ctx->ev) (void)hipEventDestroy(e);
    for (auto &e : ctx->ev_pool) (void)hipEventDestroy(e);
    for (auto &v : ctx->ev_pending)
        for (auto &pr : v) {
            (void)hipEventDestroy(pr.first);
            (void)hipEventDestroy(pr.second);
        }
    if (ctx->tlist) (void)hipFree(ctx->tlist);
    if (ctx->gws) (void)hipFree(ctx->gws);
    if (ctx->lr_take) (void)hipFree(ctx->lr_take);
    if (ctx->lr_any_dev) (void)hipFree(ctx->lr_any_dev);
    if (ctx->lb_counters) (void)hipFree(ctx->lb_counters);
    (void)mk_comm_destroy(ctx);
    delete ctx;
    return MK_OK;
}

MK_API int mk_set_stream(mk_context *ctx, void *s)
{
    MK_CTX(ctx);
    if (ctx->stream != (hipStream_t)s) ctx->tlist_obs = ctx->lr_obs = nullptr; // the cached observed-step list and the records' flags were built in the OLD stream's order
    ctx->stream = (hipStream_t)s;
    return MK_OK;
}

MK_API int mk_set_kernel_variant(mk_context *ctx, int which, int value)
{
    MK_CTX(ctx);
    if (which < 0 || which >= MK_VARIANT_COUNT) return fail(MK_ERR_INVALID, "mk_set_kernel_variant: unknown selector %d", which);
    if (value < 0 || value > ((which == MK_VARIANT_SINGLE_RECORD || which == MK_VARIANT_KERNEL_FAMILY || which == MK_VARIANT_TAPE_FILTER) ? 1 : 2))
        return fail(MK_ERR_INVALID, "mk_set_kernel_variant: value must be 0 or 1 (0, 1 or 2 for the smoother selectors and the wide filter)");
    ctx->variant[which] = value;
    return MK_OK;
}

MK_API int mk_get_kernel_variant(mk_context *ctx, int which, int *value)
{
    MK_CTX(ctx);
    if (which < 0 || which >= MK_VARIANT_COUNT || !value) return fail(MK_ERR_INVALID, "mk_get_kernel_variant: bad argument");
    *value = ctx->variant[which];
    return MK_OK;
}

MK_API int mk_observations_changed(mk_context *ctx)
{
    MK_CTX(ctx);
    ctx->tlist_obs = nullptr;
    ctx->lr_obs = nullptr;
    return MK_OK;
}

MK_API int mk_sync(mk_context *ctx)
{
    MK_CTX(ctx);
    MK_HIP(hipStreamSynchronize(ctx->stream));
    return MK_OK;
}

MK_API int mk_shape_supported(int64_t N, int64_t K)
{
    return (specialised(N, K) || generic_shape(N, K)) ? 1 : 0;
}
MK_API int mk_shape_specialised(int64_t N, int64_t K) { return specialised(N, K) ? 1 : 0; }
MK_API int64_t mk_generic_max_states(void) { return MK_GENERIC_MAX_STATES; }

MK_API int64_t mk_record_stride(int64_t n) { return mk::record_stride((int)n); }
MK_API int64_t mk_record_stride_sym(int64_t n) { return mk::record_stride_sym((int)n); }
MK_API int64_t mk_tape_stride(int64_t N, int64_t K) { return mk::tape_stride_c((int)N, (int)K); }
MK_API int64_t mk_state_tape_stride(int64_t N, int64_t K) { return mk::state_tape_stride_c((int)N, (int)K); }
MK_API int mk_tape_supported(int64_t N, int64_t K)
{
    return (N + K > 16 && K <= 16 && N + K + 1 <= 64 && specialised(N, K)) ? 1 : 0;
}
// MK_OUT_TAPE (mk_outputs.flags): 0 = not asked for, 1 = asked for and consistent, 2 = the STATE tape (with MK_OUT_VAR_ONLY:
// d_S / d_Ps are the smoothed state means / variances [B,T,n]), < 0 = an inconsistent description
static int tape_outputs(const mk_problem *p, const mk_outputs *o)
{
    if (!(o->flags & MK_OUT_TAPE)) return 0;
    if (o->flags & MK_OUT_PACKED_SYM) return fail(MK_ERR_INVALID, "MK_OUT_TAPE excludes MK_OUT_PACKED_SYM");
    if (!mk_tape_supported(p->N, p->K))
        return fail(MK_ERR_SHAPE, "MK_OUT_TAPE serves specialised shapes with 16 < N + K <= 63 (got N=%lld, K=%lld)", (long long)p->N, (long long)p->K);
    if (!p->d_loadings) return fail(MK_ERR_INVALID, "MK_OUT_TAPE needs d_loadings");
    if (o->flags & MK_OUT_VAR_ONLY) {
        if (!o->d_F || o->d_Pf || o->d_Xp || o->d_Pp || !o->d_S || !o->d_Ps)
            return fail(MK_ERR_INVALID, "MK_OUT_TAPE | MK_OUT_VAR_ONLY: d_F is the state tape, d_S / d_Ps the smoothed state means / "
                                        "variances [B,T,n]; d_Pf / d_Xp / d_Pp must be NULL");
        if (o->record_stride != mk_state_tape_stride(p->N, p->K))
            return fail(MK_ERR_INVALID, "MK_OUT_TAPE | MK_OUT_VAR_ONLY: record_stride must be mk_state_tape_stride(N, K) = %lld doubles",
                        (long long)mk_state_tape_stride(p->N, p->K));
        if (p->d_obsvar)
            return fail(MK_ERR_INVALID, "MK_OUT_TAPE | MK_OUT_VAR_ONLY serves zero observation variances (d_obsvar = NULL, Metran's R); "
                                        "use filtered records + MK_OUT_VAR_ONLY otherwise");
        return 2;
    }
    if (!o->d_F || o->d_Pf || o->d_Xp || o->d_Pp || o->d_S || o->d_Ps)
        return fail(MK_ERR_INVALID, "MK_OUT_TAPE: d_F is the tape, d_Pf / d_Xp / d_Pp / d_S / d_Ps must be NULL");
    if (o->record_stride != mk_tape_stride(p->N, p->K))
        return fail(MK_ERR_INVALID, "MK_OUT_TAPE: record_stride must be mk_tape_stride(N, K) = %lld doubles",
                    (long long)mk_tape_stride(p->N, p->K));
    return 1;
}

MK_API int mk_supported_shapes(int64_t *shapes, int cap)
{
    int cnt = 0;
    const mk::ShapeOps *aot = mk::shape_ops(&cnt);
    for (int i = 0; i < cnt && i < cap && shapes; ++i) {
        shapes[2 * i] = aot[i].N;
        shapes[2 * i + 1] = aot[i].K;
    }
    std::lock_guard<std::mutex> lock(g_modules_mutex);
    for (const mk::ShapeOps *m : g_modules) {
        if (cnt < cap && shapes) {
            shapes[2 * cnt] = m->N;
            shapes[2 * cnt + 1] = m->K;
        }
        ++cnt;
    }
    return cnt;
}

MK_API int mk_malloc(mk_context *ctx, size_t bytes, void **p)
{
    MK_CTX(ctx);
    if (!p) return fail(MK_ERR_INVALID, "null out-pointer");
    *p = nullptr;
    if (bytes == 0) return MK_OK;
    hipError_t e = hipMalloc(p, bytes);
    if (e != hipSuccess) return fail(MK_ERR_ALLOC, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e));
    return MK_OK;
}

MK_API int mk_free(mk_context *ctx, void *p)
{
    MK_CTX(ctx);
    if (p) MK_HIP(hipFree(p));
    return MK_OK;
}

MK_API int mk_memcpy_h2d(mk_context *ctx, void *d, const void *h, size_t bytes)
{
    MK_CTX(ctx);
    if (bytes && (!d || !h)) return fail(MK_ERR_INVALID, "null pointer in memcpy_h2d");
    if (bytes) {
        MK_HIP(hipMemcpyAsync(d, h, bytes, hipMemcpyHostToDevice, ctx->stream));
        MK_HIP(hipStreamSynchronize(ctx->stream)); // h may be pageable / freed by the caller
    }
    return MK_OK;
}

MK_API int mk_memcpy_d2h(mk_context *ctx, void *h, const void *d, size_t bytes)
{
    MK_CTX(ctx);
    if (bytes && (!d || !h)) return fail(MK_ERR_INVALID, "null pointer in memcpy_d2h");
    if (bytes) {
        MK_HIP(hipMemcpyAsync(h, d, bytes, hipMemcpyDeviceToHost, ctx->stream));
        MK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MK_OK;
}

MK_API int mk_memset(mk_context *ctx, void *d, int value, size_t bytes)
{
    MK_CTX(ctx);
    if (bytes && !d) return fail(MK_ERR_INVALID, "null pointer in memset");
    if (bytes) MK_HIP(hipMemsetAsync(d, value, bytes, ctx->stream));
    return MK_OK;
}

MK_API int mk_params_from_alpha(mk_context *ctx, int64_t B, int64_t R, int64_t N, int64_t K, const double *alpha,
                                const double *loadings, double dt, double *phi, double *q)
{
    MK_CTX(ctx);
    if (B <= 0 || R <= 0 || N <= 0 || K < 0 || !alpha || !phi || !q || (K > 0 && !loadings))
        return fail(MK_ERR_INVALID, "mk_params_from_alpha: bad argument");
    MK_HIP(mk::launch_params(B, R, (int)N, (int)K, alpha, loadings, dt, phi, q, ctx->stream));
    return MK_OK;
}

static int check_problem(const mk_problem *p)
{
    if (!p) return fail(MK_ERR_INVALID, "null mk_problem");
    if (p->n_instances <= 0 || p->n_records <= 0 || p->n_records > p->n_instances)
        return fail(MK_ERR_INVALID, "need 1 <= n_records <= n_instances (got R=%lld, B=%lld)",
                    (long long)p->n_records, (long long)p->n_instances);
    if (p->T <= 0 || p->N <= 0 || p->K <= 0)
        return fail(MK_ERR_INVALID, "need T, N, K >= 1 (got T=%lld N=%lld K=%lld)", (long long)p->T,
                    (long long)p->N, (long long)p->K);
    if (p->warmup < 0) return fail(MK_ERR_INVALID, "warmup must be >= 0");
    if (!mk_shape_supported(p->N, p->K))
        return fail(MK_ERR_SHAPE,
                    "no kernel for (N=%lld series, K=%lld factors): the size-generic kernels serve N + K <= %d states, specialised "
                    "ones (metran_amd.jit.ensure_shape / mk_register_shape_module / MK_SHAPES in mk_internal.h) N + K <= 64",
                    (long long)p->N, (long long)p->K, MK_GENERIC_MAX_STATES);
    if (!p->d_phi || !p->d_q) return fail(MK_ERR_INVALID, "d_phi and d_q are required");
    return MK_OK;
}

// Packed-record convention of mk_outputs.record_stride: returns 0 if `o` does not use records,
// 1 if it does (and is consistent), < 0 on an inconsistent description.
static int records_filter(const mk_problem *p, const mk_outputs *o)
{
    const bool sym = (o->flags & MK_OUT_PACKED_SYM) != 0;
    if (o->record_stride == 0) {
        if (sym) return fail(MK_ERR_INVALID, "MK_OUT_PACKED_SYM needs the record layout (record_stride = mk_record_stride_sym(n))");
        return 0;
    }
    const int64_t n = p->N + p->K, nc = sym ? n * (n + 1) / 2 : n * n, nv = n + nc;
    const int64_t want = sym ? mk::record_stride_sym((int)n) : mk::record_stride((int)n);
    if (o->record_stride != want)
        return fail(MK_ERR_INVALID, "record_stride must be %s(n) = %lld doubles", sym ? "mk_record_stride_sym" : "mk_record_stride",
                    (long long)want);
    const bool any = o->d_F || o->d_Pf || o->d_Xp || o->d_Pp;
    if (!any) return 0; // bookkeeping-only / loglik launches do not touch state arrays
    if (!(o->d_F && o->d_Pf == o->d_F + n))
        return fail(MK_ERR_INVALID, "record layout needs a filtered record array d_F with d_Pf = d_F + n");
    if ((o->d_Xp || o->d_Pp) && !(o->d_Xp && o->d_Pp == o->d_Xp + n))
        return fail(MK_ERR_INVALID, "record layout needs d_Pp = d_Xp + n (or both NULL: filtered record only)");
    if (o->d_sigmas || o->d_detfs)
        if (o->d_sigmas != o->d_F + nv || (o->d_detfs && o->d_detfs != o->d_sigmas + 1))
            return fail(MK_ERR_INVALID, "record layout needs d_sigmas = d_F + n + %s and d_detfs = d_sigmas + 1",
                        sym ? "n*(n+1)/2" : "n*n");
    return 1;
}

// The single-record routes (loglik_sparse_kernel): every instance shares ONE uploaded record, whose observed steps are
// listed once per record on the device; the objective (mk_loglik) and -- round 5 -- the record-writing filter of a few
// instances walk that list, the runs of empty steps in closed form.  d_F / d_Xp NULL: objective only.
static int sparse_route(mk_context *ctx, const mk_problem *p, double *d_mle, double *d_F, double *d_Xp, int64_t rs, int time_major,
                        int64_t *d_sigmacount, uint32_t *d_status)
{
    if (ctx->tlist_cap < p->T + 1) {
        if (ctx->tlist) MK_HIP(hipFree(ctx->tlist));
        ctx->tlist = nullptr;
        ctx->tlist_cap = 0;
        MK_HIP(hipMalloc((void **)&ctx->tlist, sizeof(int) * (size_t)(p->T + 1)));
        ctx->tlist_cap = p->T + 1;
        ctx->tlist_obs = nullptr;
    }
    mk::SparseArgs a;
    a.B = p->n_instances;
    a.T = p->T;
    a.warmup = p->warmup;
    a.ostep = (p->obs_time_major ? p->n_records : 1) * p->N; // one record: both layouts coincide
    a.obs = p->d_obs;
    a.phi = p->d_phi;
    a.q = p->d_q;
    a.loadings = p->d_loadings;
    a.obsvar = p->d_obsvar;
    fill_initial(a, p);
    a.tlist = ctx->tlist;
    a.rebuild = !(ctx->tlist_obs == p->d_obs && ctx->tlist_T == p->T && ctx->tlist_N == p->N && ctx->tlist_ostep == a.ostep);
    // the list is only known to describe this record once the launch that (re)builds it has been accepted: the key
    // is dropped first and committed after a successful dispatch, so a failed call leaves no stale key behind.
    // (Stream order: the list is built and read on ctx->stream; mk_set_stream drops the key when the stream changes.)
    ctx->tlist_obs = nullptr;
    a.mle = d_mle;
    a.status = d_status;
    a.F = d_F;
    a.Xp = d_Xp;
    a.rs = rs;
    fill_layout(a, time_major, p->n_instances, p->T);
    a.sigmacount = (long long *)d_sigmacount;
    MK_HIP(timing_start(ctx, 0));
    MK_HIP(dispatch_sparse((int)p->N, (int)p->K, a, ctx->stream));
    ctx->tlist_obs = p->d_obs;
    ctx->tlist_T = p->T;
    ctx->tlist_N = p->N;
    ctx->tlist_ostep = a.ostep;
    MK_HIP(timing_stop(ctx, 0));
    return MK_OK;
}

static int do_filter(mk_context *ctx, const mk_problem *p, const mk_outputs *o)
{
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    const int tape = tape_outputs(p, o);
    if (tape < 0) return tape;
    const int rec = tape ? 0 : records_filter(p, o);
    if (rec < 0) return rec;
    // ONE record, a handful of instances, both record sets (the 7-tuple of seqkalmanfilter: what Metran.solve() asks of the
    // engine ~80 times): a launch of the batched filter is T sequential steps for at most a few wavefronts -- latency, not
    // throughput.  Real Metran records are sparse (examples/data: 343 observed of 6255 daily steps, kalmanfilter.py:335 skips
    // the update on the others), so the observed steps are walked one after the other and every empty step's records are
    // written in closed form by a second, fully parallel kernel (mk_kernels.hip: loglik_sparse_kernel<.., REC>, fill_gaps_kernel).
    if (rec && p->n_records == 1 && p->n_instances <= MK_SPARSE_RECORD_MAX_INSTANCES && p->N + p->K <= 16 && o->d_Xp &&
        !(o->flags & MK_OUT_PACKED_SYM) && specialised(p->N, p->K) && !ctx->variant[MK_VARIANT_SINGLE_RECORD] &&
        !ctx->variant[MK_VARIANT_KERNEL_FAMILY])
        return sparse_route(ctx, p, o->d_mle, o->d_F, o->d_Xp, o->record_stride, (int)o->time_major, o->d_sigmacount, o->d_status);
    mk::FilterArgs a;
    a.variant = ctx->variant[MK_VARIANT_WIDE_FILTER]; // 0 auto, 1 lane per state, 2 split
    a.tape = tape;
    a.tape_basis = ctx->variant[MK_VARIANT_TAPE_FILTER]; // 0 observable basis (filter_obs_kernel), 1 state basis (filter_split_kernel OUT = 4)
    a.upd = ctx->cur_upd;                                // recording pass of the wide adjoint gradient: the update tape (or NULL)
    a.us = a.upd ? mk::adjoint_update_stride_c((int)p->N, (int)p->K) : 0;
    if (a.upd) a.variant = 1;                            // ... is written by the one-model-per-wavefront filter, whatever the batch size
    a.rs = (rec || tape) ? o->record_stride : 0;
    a.sym = (rec && (o->flags & MK_OUT_PACKED_SYM)) ? 1 : 0;
    // dense sigmas/detfs are [B,T] (stride 1); inside filtered records they are RS doubles apart
    a.sig_stride = (o->record_stride && !tape) ? o->record_stride : 1;
    fill_model(a, p);
    fill_initial(a, p);
    fill_layout(a, (int)o->time_major, p->n_instances, p->T);
    a.warmup = p->warmup;
    a.mle = o->d_mle;
    a.sigmas = o->d_sigmas;
    a.detfs = o->d_detfs;
    a.sigmacount = (long long *)o->d_sigmacount;
    a.F = o->d_F;
    a.Pf = o->d_Pf;
    a.Xp = o->d_Xp;
    a.Pp = o->d_Pp;
    a.status = o->d_status;
    if ((a.sym || a.tape) && (!specialised(p->N, p->K) || ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 1))
        return fail(MK_ERR_SHAPE, "packed-symmetric records and the tape exist for specialised shapes only (N=%lld, K=%lld runs the size-generic "
                                  "kernels: mk_shape_specialised)", (long long)p->N, (long long)p->K);
    MK_HIP(timing_start(ctx, 0));
    {
        const hipError_t e = dispatch_filter((int)p->N, (int)p->K, a, ctx->stream, ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 1);
        if (e == hipErrorNotSupported)
            return fail(MK_ERR_SHAPE, "a model of N=%lld series and K=%lld factors is not served on this device in this mode (the size-generic "
                                      "filter keeps the %lld x %lld covariance in LDS: %zu bytes)", (long long)p->N, (long long)p->K,
                        (long long)(p->N + p->K), (long long)(p->N + p->K), mk::generic_filter_lds_bytes((int)p->N, (int)p->K));
        MK_HIP(e);
    }
    MK_HIP(timing_stop(ctx, 0));
    return MK_OK;
}

// The records for which the record smoother takes its rank-K covariance step: at least 7 of 8 of the record's steps observe every
// series.  Counted on the device once per observation set (the count reads every cell; the answer is kept until the pointer, the
// shape or the layout changes or mk_observations_changed() is called) and read back once, so that a launch in which no record
// qualifies runs the parent's kernel.  *take = nullptr: do not take the step (also while the stream is being captured and the
// answer is not there yet: the read-back would need a synchronisation).  *all: every step of every record is full (the second bit of
// the same word, mk::MK_FULL_GAP, is clear) -- the launch may run the form of the kernel that looks at no observation.
static hipError_t full_records(mk_context *ctx, const mk_problem *p, const unsigned char **take, long *all)
{
    *take = nullptr;
    *all = 0;
    const long bs = p->obs_time_major ? 1 : p->T;
    if (!(ctx->lr_obs == p->d_obs && ctx->lr_R == p->n_records && ctx->lr_T == p->T && ctx->lr_N == p->N && ctx->lr_bs == bs)) {
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(ctx->stream, &cap) != hipSuccess) (void)hipGetLastError();
        if (cap != hipStreamCaptureStatusNone) return hipSuccess;
        ctx->lr_obs = nullptr;
        if (ctx->lr_cap < p->n_records) {
            if (ctx->lr_take) {
                hipError_t e = hipStreamSynchronize(ctx->stream); // a launch still reading the old buffer
                if (e != hipSuccess) return e;
                (void)hipFree(ctx->lr_take);
                ctx->lr_take = nullptr;
                ctx->lr_cap = 0;
            }
            hipError_t e = hipMalloc((void **)&ctx->lr_take, (size_t)p->n_records);
            if (e != hipSuccess) return e;
            ctx->lr_cap = p->n_records;
        }
        if (!ctx->lr_any_dev) {
            hipError_t e = hipMalloc((void **)&ctx->lr_any_dev, sizeof(int));
            if (e != hipSuccess) return e;
        }
        hipError_t e = hipMemsetAsync(ctx->lr_any_dev, 0, sizeof(int), ctx->stream);
        if (e != hipSuccess) return e;
        e = mk::launch_full_records(p->n_records, p->T, (int)p->N, bs, p->obs_time_major ? p->n_records : 1, p->d_obs, ctx->lr_take,
                                    ctx->lr_any_dev, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipMemcpyAsync(&ctx->lr_any, ctx->lr_any_dev, sizeof(int), hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) return e;
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return e;
        ctx->lr_obs = p->d_obs;
        ctx->lr_R = p->n_records;
        ctx->lr_T = p->T;
        ctx->lr_N = p->N;
        ctx->lr_bs = bs;
    }
    if (ctx->lr_any & mk::MK_FULL_ANY) *take = ctx->lr_take;
    *all = ctx->lr_any == mk::MK_FULL_ANY;
    return hipSuccess;
}

// clear_status: the smoother kernels OR their bits into d_status -- behind mk_filter_smooth the filter's stay, called on its own mk_smooth
// WRITES the word: it is cleared on the stream once every argument check has passed, right before the launch
static int do_smooth(mk_context *ctx, const mk_problem *p, const mk_outputs *o, bool clear_status)
{
    const int tape = tape_outputs(p, o);
    if (tape < 0) return tape;
    if (!o->d_F || (!o->d_Pf && !tape))
        return fail(MK_ERR_INVALID, "the smoother reads d_F and d_Pf (filtered moments); both must be non-NULL");
    if (tape == 1 && !(o->d_sim_means || o->d_sim_vars))
        return fail(MK_ERR_INVALID, "MK_OUT_TAPE: nothing to write, give d_sim_means / d_sim_vars");
    mk::SmootherArgs a;
    a.tape = tape;
    a.obsvar = tape ? p->d_obsvar : nullptr;
    a.variant = (ctx->variant[MK_VARIANT_SMOOTHER16] == 1 ? 1 : 0) | (ctx->variant[MK_VARIANT_WIDE_SMOOTHER] == 1 ? 2 : 0) |
                (ctx->variant[MK_VARIANT_WIDE_SMOOTHER] == 2 ? 4 : 0);
    a.rs = 0;
    a.sym = 0;
    a.state_means = a.state_vars = nullptr;
    const bool sym = (o->flags & MK_OUT_PACKED_SYM) != 0, var = (o->flags & MK_OUT_VAR_ONLY) != 0;
    if (tape) {
        a.rs = o->record_stride;
    } else if (o->record_stride) {
        const int64_t n = p->N + p->K;
        const int64_t want = sym ? mk::record_stride_sym((int)n) : mk::record_stride((int)n);
        if (o->record_stride != want)
            return fail(MK_ERR_INVALID, "record_stride must be %s(n) = %lld doubles", sym ? "mk_record_stride_sym" : "mk_record_stride",
                        (long long)want);
        const bool proj = o->d_sim_means || o->d_sim_vars;
        if (o->d_Pf != o->d_F + n) return fail(MK_ERR_INVALID, "record layout needs d_Pf = d_F + n");
        if (var) {
            if (!o->d_S || !o->d_Ps || proj)
                return fail(MK_ERR_INVALID, "MK_OUT_VAR_ONLY needs d_S [B,T,n] (means) and d_Ps [B,T,n] (variances), no projection outputs");
        } else {
            if ((o->d_S || o->d_Ps) && !(o->d_S && o->d_Ps == o->d_S + n))
                return fail(MK_ERR_INVALID, "record layout needs a smoothed record array d_S with d_Ps = d_S + n");
            if (!o->d_S && !proj)
                return fail(MK_ERR_INVALID, "nothing to write: give d_S/d_Ps records or d_sim_means/d_sim_vars");
        }
        if (proj && !p->d_loadings) return fail(MK_ERR_INVALID, "the projection outputs need d_loadings");
        a.rs = o->record_stride;
        a.sym = sym ? 1 : 0;
    } else if (o->d_sim_means || o->d_sim_vars || sym || var) {
        return fail(MK_ERR_INVALID, "d_sim_means / d_sim_vars, MK_OUT_PACKED_SYM and MK_OUT_VAR_ONLY need the record layout "
                                    "(record_stride = mk_record_stride[_sym](n))");
    }
    // the record smoother's rank-K covariance step (smoother_record_kernel, LR) rests on R = 0: the guard is the NULL pointer, not
    // the values behind it.  MK_VARIANT_SMOOTHER16 = 2 keeps the general products at every step
    a.obs = nullptr;
    a.lr_take = nullptr;
    a.lr_all = 0;
    a.obs_bs = a.obs_ts = 0;
    // (the kernel addresses a cell by a 32-bit byte offset from a base that walks in time: observations below 4 GiB)
    if (p->d_obs && p->d_loadings && !p->d_obsvar && !tape && ctx->variant[MK_VARIANT_SMOOTHER16] != 2 &&
        (double)p->n_records * (double)p->T * (double)p->N * sizeof(double) < 4294967296.0) {
        // ... and only for shapes and record forms whose kernel has the step (everything else never looks at the observations)
        const bool served = !sym && !var && o->record_stride && !(o->d_sim_means || o->d_sim_vars) && p->N + p->K <= 10 &&
                            ctx->variant[MK_VARIANT_SMOOTHER16] == 0 && ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 0;
        if (served) MK_HIP(full_records(ctx, p, &a.lr_take, &a.lr_all));
        if (a.lr_take) {
            a.obs = p->d_obs;
            a.obs_bs = p->obs_time_major ? 1 : p->T;
            a.obs_ts = p->obs_time_major ? p->n_records : 1;
        }
    }
    a.R = p->n_records;
    a.loadings = p->d_loadings;
    fill_scaling(a, p);
    a.sim_means = o->d_sim_means;
    a.sim_vars = o->d_sim_vars;
    a.B = p->n_instances;
    a.T = p->T;
    fill_layout(a, (int)o->time_major, p->n_instances, p->T);
    a.phi = p->d_phi;
    a.q = p->d_q;
    a.F = o->d_F;
    a.Pf = o->d_Pf;
    if (tape == 2 && !p->d_loadings) return fail(MK_ERR_INVALID, "the state tape needs d_loadings");
    a.S = var ? nullptr : o->d_S;
    a.Ps = var ? nullptr : o->d_Ps;
    if (var) {
        a.state_means = o->d_S;
        a.state_vars = o->d_Ps;
    }
    a.status = o->d_status;
    MK_HIP(timing_start(ctx, 1));
    if ((sym || tape) && (!specialised(p->N, p->K) || ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 1))
        return fail(MK_ERR_SHAPE, "packed-symmetric records and the tape exist for specialised shapes only (N=%lld, K=%lld runs the "
                                  "size-generic kernels: mk_shape_specialised)", (long long)p->N, (long long)p->K);
    if ((a.variant & 2) && !sym && !var && !tape && p->N + p->K > mk::wave_smoother_max_n && specialised(p->N, p->K) &&
        ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 0)
        return fail(MK_ERR_SHAPE, "the round-1 wide smoother (MK_VARIANT_WIDE_SMOOTHER 1) is built for N + K <= %d (got N=%lld, K=%lld)",
                    mk::wave_smoother_max_n, (long long)p->N, (long long)p->K);
    if (clear_status && o->d_status) MK_HIP(hipMemsetAsync(o->d_status, 0, (size_t)p->n_instances * sizeof(uint32_t), ctx->stream));
    MK_HIP(dispatch_smoother(ctx, (int)p->N, (int)p->K, a, ctx->stream));
    MK_HIP(timing_stop(ctx, 1));
    return MK_OK;
}

MK_API int mk_filter(mk_context *ctx, const mk_problem *p, const mk_outputs *o)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!o) return fail(MK_ERR_INVALID, "null mk_outputs");
    return do_filter(ctx, p, o);
}

MK_API int mk_loglik(mk_context *ctx, const mk_problem *p, double *d_mle)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!d_mle) return fail(MK_ERR_INVALID, "d_mle is required");
    if (p->n_records == 1 && p->N + p->K <= 16 && p->d_obs && p->d_loadings && specialised(p->N, p->K) && !ctx->variant[MK_VARIANT_KERNEL_FAMILY]) {
        // every instance shares the one record (the solver's finite-difference points): walk only its
        // observed steps, the runs of empty steps in closed form (loglik_sparse_kernel)
        return sparse_route(ctx, p, d_mle, nullptr, nullptr, 0, 0, nullptr, nullptr);
    }
    mk_outputs o;
    memset(&o, 0, sizeof(o));
    o.d_mle = d_mle;
    return do_filter(ctx, p, &o);
}

MK_API int mk_smooth(mk_context *ctx, const mk_problem *p, const mk_outputs *o)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!o) return fail(MK_ERR_INVALID, "null mk_outputs");
    return do_smooth(ctx, p, o, true);
}

MK_API int mk_smooth_dense(mk_context *ctx, int64_t B, int64_t T, int64_t n, const double *d_phi, const double *d_F,
                           const double *d_Pf, const double *d_Xp, const double *d_Pp, double *d_S, double *d_Ps, uint32_t *d_status)
{
    MK_CTX(ctx);
    if (B <= 0 || T <= 0 || n <= 0 || !d_phi || !d_F || !d_Pf || !d_Xp || !d_Pp || !(d_S || d_Ps))
        return fail(MK_ERR_INVALID, "mk_smooth_dense: bad argument (all five inputs and one of d_S / d_Ps are required)");
    if (n > MK_GENERIC_MAX_STATES)
        return fail(MK_ERR_SHAPE, "mk_smooth_dense serves n <= %d states (got %lld)", MK_GENERIC_MAX_STATES, (long long)n);
    mk::GenericSmootherArgs g;
    memset(&g, 0, sizeof(g));
    g.a.B = B;
    g.a.T = T;
    g.a.bs = T; // dense [B,T,...] arrays, the reference's layout with a leading batch axis
    g.a.ts = 1;
    g.a.R = 1;
    g.a.phi = d_phi;
    g.a.q = nullptr; // not needed: the predicted covariances are the caller's
    g.a.F = d_F;
    g.a.Pf = d_Pf;
    g.a.S = d_S;
    g.a.Ps = d_Ps;
    g.a.status = d_status;
    g.N = (int)n; // no projection outputs: only n = N + K matters
    g.K = 0;
    g.Xp = d_Xp;
    g.Pp = d_Pp;
    MK_HIP(generic_workspace(ctx, B, (int)n, &g.ws));
    if (d_status) MK_HIP(hipMemsetAsync(d_status, 0, (size_t)B * sizeof(uint32_t), ctx->stream)); // the kernel ORs; this call writes
    MK_HIP(timing_start(ctx, 1));
    MK_HIP(mk::launch_smoother_generic(g, ctx->stream));
    MK_HIP(timing_stop(ctx, 1));
    return MK_OK;
}

MK_API int mk_filter_smooth(mk_context *ctx, const mk_problem *p, const mk_outputs *o)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!o) return fail(MK_ERR_INVALID, "null mk_outputs");
    if ((o->flags & MK_OUT_VAR_ONLY) && !(o->flags & MK_OUT_TAPE) && (o->d_Xp || o->d_Pp))
        return fail(MK_ERR_INVALID, "MK_OUT_VAR_ONLY: d_Xp / d_Pp must be NULL (the filter writes the filtered record only)");
    if (int rc = do_filter(ctx, p, o)) return rc;
    return do_smooth(ctx, p, o, false);
}

MK_API int mk_simulate(mk_context *ctx, int64_t B, int64_t RZ, int64_t T, int64_t N, int64_t n, const double *Z,
                       const double *means, const double *covs, double *sm, double *sv)
{
    MK_CTX(ctx);
    if (B <= 0 || RZ <= 0 || T <= 0 || N <= 0 || n < N || !Z || !means || (sv && !covs))
        return fail(MK_ERR_INVALID, "mk_simulate: bad argument");
    MK_HIP(mk::launch_simulate(B, RZ, T, (int)N, (int)n, Z, means, covs, sm, sv, ctx->stream));
    return MK_OK;
}

MK_API int mk_decompose(mk_context *ctx, int64_t B, int64_t RZ, int64_t T, int64_t N, int64_t n, const double *Z,
                        const double *means, double *sdf, double *cdf)
{
    MK_CTX(ctx);
    if (B <= 0 || RZ <= 0 || T <= 0 || N <= 0 || n < N || !Z || !means)
        return fail(MK_ERR_INVALID, "mk_decompose: bad argument");
    MK_HIP(mk::launch_decompose(B, RZ, T, (int)N, (int)n, Z, means, sdf, cdf, ctx->stream));
    return MK_OK;
}

MK_API int mk_sum(mk_context *ctx, int64_t count, const double *v, double *out)
{
    MK_CTX(ctx);
    if (count <= 0 || !v || !out) return fail(MK_ERR_INVALID, "mk_sum: bad argument");
    MK_HIP(mk::launch_sum(count, v, out, ctx->stream));
    return MK_OK;
}

MK_API int64_t mk_adjoint_update_stride(int64_t N, int64_t K)
{
    if (N < 1 || K < 1 || N + K <= 16 || N + K > 64) return 0; // the 16-lane adjoint kernel recomputes (n <= 16)
    return mk::adjoint_update_stride_c((int)N, (int)K);
}

MK_API int mk_set_adjoint_updates(mk_context *ctx, double *d_buf, int64_t capacity_doubles)
{
    if (!ctx) return fail(MK_ERR_INVALID, "null mk_context");
    if ((d_buf && capacity_doubles <= 0) || ((uintptr_t)d_buf & 15)) return fail(MK_ERR_INVALID, "mk_set_adjoint_updates: need a 16-byte aligned buffer and its capacity");
    ctx->adj_upd = d_buf;
    ctx->adj_upd_cap = d_buf ? (size_t)capacity_doubles : 0;
    return MK_OK;
}

// The opening checks of the entry points that take a request struct, in this order: the context, too many states (refused first:
// every other shape that the entry point's work stride does not serve is one check_problem refuses), the problem, the request, d_work.
static int reader_preamble(mk_context *ctx, const char *who, const char *request_type, const mk_problem *p, int max_states,
                           const void *req, const double *d_work)
{
    MK_CTX(ctx);
    if (p && p->N >= 1 && p->K >= 1 && p->N + p->K > max_states) return too_many_states(who, p, max_states);
    if (int rc = check_problem(p)) return rc;
    if (!req) return fail(MK_ERR_INVALID, "%s: null %s", who, request_type);
    if (!d_work) return fail(MK_ERR_INVALID, "%s: d_work is required", who);
    return MK_OK;
}

// The recording forward pass every record reader starts with: filtered records only (+ the per-step bookkeeping in the record
// pads) of record_stride doubles per (instance, step) at the head of d_work; with d_mle / d_sigmacount also the objective and the
// step count (the gradient's forward phase).
static int record_pass(mk_context *ctx, const mk_problem *p, double *d_work, int64_t record_stride, int time_major, uint32_t *d_status,
                       double *d_mle = nullptr, int64_t *d_sigmacount = nullptr)
{
    const int64_t n = p->N + p->K;
    mk_outputs o;
    memset(&o, 0, sizeof(o));
    o.d_mle = d_mle;
    o.d_sigmacount = d_sigmacount;
    o.d_status = d_status;
    o.d_F = d_work;
    o.d_Pf = d_work + n;
    o.d_sigmas = d_work + n + n * n;
    o.d_detfs = o.d_sigmas + 1;
    o.time_major = time_major;
    o.record_stride = record_stride;
    return do_filter(ctx, p, &o);
}

// The gain-tape stage of the weights, the regression and the scores, inside the caller's timed launches: innov_step_kernel
// writes the gains of every observed cell behind the records (and, for the scores, the innovations behind the tape).
static int gain_tape_stage(mk_context *ctx, const mk_problem *p, double *d_work, const work_layout &w, int time_major,
                           double *d_innov = nullptr)
{
    mk::InnovArgs g = reader_args<mk::InnovArgs>(p, d_work, w.rs, time_major);
    g.v = d_innov;
    g.gain = d_work + w.tape;
    g.gs = w.gs;
    // a cell that is not observed keeps an all-zero slot: innov_step_kernel writes the observed ones only
    MK_HIP(hipMemsetAsync(g.gain, 0, sizeof(double) * (size_t)(p->n_instances * p->T * p->N * w.gs), ctx->stream));
    MK_HIP(mk::launch_innov_step(g, ctx->stream));
    return MK_OK;
}

MK_API int mk_loglik_grad(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, double *d_mle,
                          int64_t *d_sigmacount, double *d_gphi, double *d_gq, uint32_t *d_status)
{
    return mk_loglik_grad_phases(ctx, p, d_work, time_major, d_mle, d_sigmacount, d_gphi, d_gq, d_status,
                                 MK_GRAD_FORWARD | MK_GRAD_BACKWARD);
}

MK_API int mk_loglik_grad_phases(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, double *d_mle,
                                 int64_t *d_sigmacount, double *d_gphi, double *d_gq, uint32_t *d_status, int phases)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!(phases & (MK_GRAD_FORWARD | MK_GRAD_BACKWARD)) || (phases & ~(MK_GRAD_FORWARD | MK_GRAD_BACKWARD)))
        return fail(MK_ERR_INVALID, "mk_loglik_grad_phases: phases must be MK_GRAD_FORWARD, MK_GRAD_BACKWARD or both");
    if (!d_work || !d_sigmacount || ((phases & MK_GRAD_FORWARD) && !d_mle) || ((phases & MK_GRAD_BACKWARD) && (!d_gphi || !d_gq)))
        return fail(MK_ERR_INVALID, "mk_loglik_grad: d_work and d_sigmacount are required; d_mle by the forward pass, d_gphi and d_gq by the backward pass");
    if (!specialised(p->N, p->K) || ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 1)
        return fail(MK_ERR_SHAPE, "the adjoint gradient exists for specialised shapes (N + K <= 64: ahead-of-time list or a shape "
                                  "module); N=%lld, K=%lld runs the size-generic kernels, difference mk_loglik instead",
                    (long long)p->N, (long long)p->K);
    const int64_t rs = mk::record_stride((int)(p->N + p->K));
    // wide models (16 < N + K): with an update tape on the context that holds this call (mk_set_adjoint_updates), the forward pass
    // records (d, 1/f, v) of every scalar update and the backward walk reads them instead of recomputing the step (round 6).
    // The decision depends on the tape, the shape and the sizes only: the two phases of one gradient agree.
    double *upd = nullptr;
    const int64_t us = mk_adjoint_update_stride(p->N, p->K);
    if (us > 0 && ctx->adj_upd && (size_t)(p->n_instances * p->T * us) <= ctx->adj_upd_cap) upd = ctx->adj_upd;
    if (phases & MK_GRAD_FORWARD) { // filtered records, objective, step count
        ctx->cur_upd = upd;
        const int rc = record_pass(ctx, p, d_work, rs, time_major, d_status, d_mle, d_sigmacount);
        ctx->cur_upd = nullptr;
        if (rc) return rc;
    }
    if (!(phases & MK_GRAD_BACKWARD)) return MK_OK;
    mk::AdjointArgs a = reader_args<mk::AdjointArgs>(p, d_work, rs, time_major);
    a.upd = upd;
    a.us = upd ? us : 0;
    a.warmup = p->warmup;
    a.sigmacount = (const long long *)d_sigmacount;
    a.gphi = d_gphi;
    a.gq = d_gq;
    return timed_launches(ctx, [&]() -> int {
        MK_HIP(dispatch_adjoint((int)p->N, (int)p->K, a, ctx->stream));
        return MK_OK;
    });
}

// ---- leave-one-out predictions (de Jong's deletion result on the two backward walks) ----
MK_API int64_t mk_loo_work_stride(int64_t N, int64_t K)
{
    if (N < 1 || K < 1 || !specialised(N, K)) return 0;
    if (N + K <= 16) return layout_of(WORK_RECORDS, N, K).stride;
    return mk_tape_supported(N, K) ? mk::tape_stride_c((int)N, (int)K) : 0;
}

MK_API int mk_loo(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, double *d_loo_means, double *d_loo_vars,
                  uint32_t *d_status)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!d_work || !d_loo_means || !d_loo_vars) return fail(MK_ERR_INVALID, "mk_loo: d_work, d_loo_means and d_loo_vars are required");
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    const int64_t ws = mk_loo_work_stride(p->N, p->K);
    if (!ws || ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 1)
        return fail(MK_ERR_SHAPE, "mk_loo serves specialised shapes with N + K <= 63 (ahead-of-time list or a shape module); "
                                  "N=%lld, K=%lld is not one%s", (long long)p->N, (long long)p->K,
                    ws ? " in this context (the size-generic kernel family is selected)" : "");
    const device_buffer bufs[3] = {{d_work, p->n_instances * p->T * ws, "d_work (n_instances * T * mk_loo_work_stride(N, K) doubles)"},
                                   {d_loo_means, p->n_instances * p->T * p->N, "d_loo_means (n_instances * T * N doubles)"},
                                   {d_loo_vars, p->n_instances * p->T * p->N, "d_loo_vars (n_instances * T * N doubles)"}};
    if (int rc = buffers_fit("mk_loo", bufs, 3)) return rc;
    if (p->N + p->K <= 16) { // the recording forward pass, then the adjoint walk in its LOO mode
        if (int rc = record_pass(ctx, p, d_work, ws, time_major, d_status)) return rc;
        mk::AdjointArgs a = reader_args<mk::AdjointArgs>(p, d_work, ws, time_major);
        a.loo_means = d_loo_means;
        a.loo_vars = d_loo_vars;
        fill_scaling(a, p);
        return timed_launches(ctx, [&]() -> int {
            MK_HIP(dispatch_loo((int)p->N, (int)p->K, &a, nullptr, ctx->stream));
            return MK_OK;
        });
    }
    // wide models: the tape writer of the projection, then the tape walk in its LOO mode
    mk_outputs o;
    memset(&o, 0, sizeof(o));
    o.d_status = d_status;
    o.d_F = d_work;
    o.time_major = time_major;
    o.record_stride = ws;
    o.flags = MK_OUT_TAPE;
    o.d_sim_means = d_loo_means;
    o.d_sim_vars = d_loo_vars;
    if (int rc = do_filter(ctx, p, &o)) return rc;
    mk::SmootherArgs a;
    memset(&a, 0, sizeof(a));
    a.tape = 1;
    a.obsvar = p->d_obsvar;
    a.rs = ws;
    a.R = p->n_records;
    a.loadings = p->d_loadings;
    fill_scaling(a, p);
    a.sim_means = d_loo_means;
    a.sim_vars = d_loo_vars;
    a.B = p->n_instances;
    a.T = p->T;
    fill_layout(a, time_major, p->n_instances, p->T);
    a.phi = p->d_phi;
    a.q = p->d_q;
    a.F = d_work;
    a.status = d_status;
    return timed_launches(ctx, [&]() -> int {
        MK_HIP(dispatch_loo((int)p->N, (int)p->K, nullptr, &a, ctx->stream));
        return MK_OK;
    });
}

// ---- simulation smoother (Durbin & Koopman 2002): the unconditional paths and the perturbed records (draw_kernels.hip) ----
static int draw_counts(const char *who, int64_t first_instance, int64_t first_draw, int64_t ndraws)
{
    if (ndraws < 1 || first_draw < 0 || first_instance < 0)
        return fail(MK_ERR_INVALID, "%s: need ndraws >= 1, first_draw >= 0 and first_instance >= 0 (got %lld, %lld, %lld)", who,
                    (long long)ndraws, (long long)first_draw, (long long)first_instance);
    return MK_OK;
}

MK_API int mk_draw_perturb(mk_context *ctx, const mk_problem *p, uint64_t seed, int64_t first_instance, int64_t first_draw,
                           int64_t ndraws, int antithetic, const double *d_L0, double *d_ystar, double *d_zxplus, double *d_xplus)
{
    MK_CTX(ctx);
    if (!p) return fail(MK_ERR_INVALID, "null mk_problem");
    if (p->N >= 1 && p->K >= 1 && p->N + p->K > MK_GENERIC_MAX_STATES)
        return fail(MK_ERR_SHAPE, "mk_draw_perturb: N=%lld, K=%lld has %lld states; the library serves N + K <= %d", (long long)p->N,
                    (long long)p->K, (long long)(p->N + p->K), MK_GENERIC_MAX_STATES);
    if (int rc = check_problem(p)) return rc;
    if (int rc = draw_counts("mk_draw_perturb", first_instance, first_draw, ndraws)) return rc;
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "mk_draw_perturb: d_obs and d_loadings are required");
    if (!d_ystar) return fail(MK_ERR_INVALID, "mk_draw_perturb: d_ystar is required");
    const int64_t n = p->N + p->K, SB = ndraws * p->n_instances;
    const device_buffer bufs[4] = {{d_ystar, SB * p->T * p->N, "d_ystar (ndraws * n_instances * T * N doubles)"},
                                   {d_zxplus, SB * p->T * p->N, "d_zxplus (ndraws * n_instances * T * N doubles)"},
                                   {d_xplus, SB * p->T * n, "d_xplus (ndraws * n_instances * T * (N + K) doubles)"},
                                   {d_L0, p->n_instances * n * n, "d_L0 (n_instances * (N + K)^2 doubles)"}};
    if (int rc = buffers_fit("mk_draw_perturb", bufs, 4)) return rc;
    mk::DrawArgs a;
    memset(&a, 0, sizeof(a));
    fill_model(a, p);
    fill_layout(a, (int)p->obs_time_major, SB, p->T); // the S * B paths follow the observations' layout
    a.N = (int)p->N;
    a.K = (int)p->K;
    a.S = ndraws;
    a.seed = seed;
    a.first_instance = first_instance;
    a.first_draw = first_draw;
    a.antithetic = antithetic != 0;
    a.L0 = d_L0;
    a.ystar = d_ystar;
    a.zxplus = d_zxplus;
    a.xplus = d_xplus;
    MK_HIP(mk::launch_draw_perturb(a, ctx->stream));
    return MK_OK;
}

MK_API int mk_draw_combine(mk_context *ctx, const mk_problem *p, int64_t ndraws, int what, int time_major, const double *d_plus,
                           double *d_inout)
{
    MK_CTX(ctx);
    if (!p) return fail(MK_ERR_INVALID, "null mk_problem");
    if (p->n_instances <= 0 || p->n_records <= 0 || p->n_records > p->n_instances || p->T <= 0 || p->N <= 0 || p->K <= 0 || ndraws < 1)
        return fail(MK_ERR_INVALID, "mk_draw_combine: need 1 <= n_records <= n_instances, T, N, K >= 1 and ndraws >= 1");
    if (what != MK_DRAW_SERIES && what != MK_DRAW_STATES)
        return fail(MK_ERR_INVALID, "mk_draw_combine: what must be MK_DRAW_SERIES or MK_DRAW_STATES (got %d)", what);
    if (!d_plus || !d_inout) return fail(MK_ERR_INVALID, "mk_draw_combine: d_plus and d_inout are required");
    const int64_t W = what == MK_DRAW_SERIES ? p->N : p->N + p->K, SB = ndraws * p->n_instances;
    const device_buffer bufs[2] = {{d_plus, SB * p->T * W, "d_plus (ndraws * n_instances * T * width doubles)"},
                                   {d_inout, SB * p->T * W, "d_inout (ndraws * n_instances * T * width doubles)"}};
    if (int rc = buffers_fit("mk_draw_combine", bufs, 2)) return rc;
    mk::DrawCombineArgs a;
    memset(&a, 0, sizeof(a));
    a.SB = SB;
    a.B = p->n_instances;
    a.R = p->n_records;
    a.T = p->T;
    a.W = (int)W;
    a.time_major = time_major != 0;
    a.scale = what == MK_DRAW_SERIES ? p->d_scale : nullptr;
    a.plus = d_plus;
    a.inout = d_inout;
    MK_HIP(mk::launch_draw_combine(a, ctx->stream));
    return MK_OK;
}

MK_API int mk_draw_normals(mk_context *ctx, uint64_t seed, int64_t first_instance, int64_t ninstances, int64_t first_draw, int64_t ndraws,
                           int antithetic, int64_t T, int64_t ncomp, int raw, double *d_out)
{
    MK_CTX(ctx);
    if (int rc = draw_counts("mk_draw_normals", first_instance, first_draw, ndraws)) return rc;
    if (ninstances < 1 || T < 0 || ncomp < 1 || ncomp > 2 * MK_GENERIC_MAX_STATES)
        return fail(MK_ERR_INVALID, "mk_draw_normals: need ninstances >= 1, T >= 0 and 1 <= ncomp <= %d", 2 * MK_GENERIC_MAX_STATES);
    if (!d_out) return fail(MK_ERR_INVALID, "mk_draw_normals: d_out is required");
    const device_buffer buf = {d_out, ndraws * ninstances * (T + 1) * ncomp, "d_out (ndraws * ninstances * (T + 1) * ncomp doubles)"};
    if (int rc = buffers_fit("mk_draw_normals", &buf, 1)) return rc;
    mk::DrawNormalsArgs a;
    memset(&a, 0, sizeof(a));
    a.seed = seed;
    a.first_instance = first_instance;
    a.ninstances = ninstances;
    a.first_draw = first_draw;
    a.ndraws = ndraws;
    a.T = T;
    a.ncomp = (int)ncomp;
    a.antithetic = antithetic != 0;
    a.raw = raw != 0;
    a.out = d_out;
    MK_HIP(mk::launch_draw_normals(a, ctx->stream));
    return MK_OK;
}

// ---- window statistics of posterior draws (ensemble_kernels.hip) ----
MK_API int64_t mk_path_functional_count(void) { return mk::path_functional_count; }

MK_API int mk_path_functionals(mk_context *ctx, const mk_problem *p, int64_t ndraws, int what, int time_major, const double *d_paths,
                               int64_t W, const int64_t *d_windows, const double *d_thresholds, double *d_functionals)
{
    MK_CTX(ctx);
    if (!p) return fail(MK_ERR_INVALID, "null mk_problem");
    if (p->n_instances <= 0 || p->n_records <= 0 || p->n_records > p->n_instances || p->T <= 0 || p->N <= 0 || p->K <= 0 || ndraws < 1)
        return fail(MK_ERR_INVALID, "mk_path_functionals: need 1 <= n_records <= n_instances, T, N, K >= 1 and ndraws >= 1");
    if (what != MK_DRAW_SERIES && what != MK_DRAW_STATES)
        return fail(MK_ERR_INVALID, "mk_path_functionals: what must be MK_DRAW_SERIES or MK_DRAW_STATES (got %d)", what);
    if (W < 1) return fail(MK_ERR_INVALID, "mk_path_functionals: need W >= 1 windows per record (got %lld)", (long long)W);
    if (!d_paths || !d_windows || !d_functionals)
        return fail(MK_ERR_INVALID, "mk_path_functionals: d_paths, d_windows and d_functionals are required");
    const int64_t Wd = what == MK_DRAW_SERIES ? p->N : p->N + p->K, SB = ndraws * p->n_instances;
    static_assert(sizeof(int64_t) == sizeof(double), "buffers_fit counts 8-byte words");
    const device_buffer bufs[4] = {{d_paths, SB * p->T * Wd, "d_paths (ndraws * n_instances * T * width doubles)"},
                                   {d_windows, p->n_records * W * 2, "d_windows (n_records * W * 2 int64)"},
                                   {d_thresholds, p->n_records * Wd, "d_thresholds (n_records * width doubles)"},
                                   {d_functionals, SB * Wd * W * mk::path_functional_count, "d_functionals (ndraws * n_instances * width * W * 5 doubles)"}};
    if (int rc = buffers_fit("mk_path_functionals", bufs, 4)) return rc;
    mk::PathFunctionalArgs a;
    memset(&a, 0, sizeof(a));
    a.SB = SB;
    a.B = p->n_instances;
    a.R = p->n_records;
    a.T = p->T;
    a.Wd = (int)Wd;
    a.time_major = time_major != 0;
    a.W = W;
    a.paths = d_paths;
    a.windows = d_windows;
    a.thresholds = d_thresholds;
    a.out = d_functionals;
    MK_HIP(mk::launch_path_functionals(a, ctx->stream));
    return MK_OK;
}

MK_API int64_t mk_ensemble_max_draws(void) { return mk::ensemble_max_draws; }

MK_API int mk_ensemble_summary(mk_context *ctx, int64_t S, int64_t cells, const double *d_values, int64_t nprobs, const double *probs,
                               double *d_summary)
{
    MK_CTX(ctx);
    if (S < 1 || S > mk::ensemble_max_draws)
        return fail(MK_ERR_INVALID, "mk_ensemble_summary: need 1 <= S <= mk_ensemble_max_draws() = %d draws (got %lld)", mk::ensemble_max_draws,
                    (long long)S);
    if (cells < 1) return fail(MK_ERR_INVALID, "mk_ensemble_summary: need cells >= 1 (got %lld)", (long long)cells);
    if (nprobs < 0 || nprobs > mk::ensemble_max_probs)
        return fail(MK_ERR_INVALID, "mk_ensemble_summary: need 0 <= nprobs <= %d (got %lld)", mk::ensemble_max_probs, (long long)nprobs);
    if (!d_values || !d_summary || (nprobs > 0 && !probs))
        return fail(MK_ERR_INVALID, "mk_ensemble_summary: d_values, d_summary and (with nprobs > 0) probs are required");
    mk::EnsembleSummaryArgs a;
    memset(&a, 0, sizeof(a));
    for (int64_t k = 0; k < nprobs; ++k) {
        if (!(probs[k] >= 0.0 && probs[k] <= 1.0))
            return fail(MK_ERR_INVALID, "mk_ensemble_summary: probs[%lld] = %g is not a probability in [0, 1]", (long long)k, probs[k]);
        a.probs[k] = probs[k];
    }
    const device_buffer bufs[2] = {{d_values, S * cells, "d_values (S * cells doubles)"},
                                   {d_summary, cells * (5 + nprobs), "d_summary (cells * (5 + nprobs) doubles)"}};
    if (int rc = buffers_fit("mk_ensemble_summary", bufs, 2)) return rc;
    a.S = S;
    a.cells = cells;
    a.nprobs = (int)nprobs;
    a.values = d_values;
    a.out = d_summary;
    MK_HIP(mk::launch_ensemble_summary(a, ctx->stream));
    return MK_OK;
}

// ---- smoothed state disturbances (the adjoint walks in their disturbance mode) ----
MK_API int64_t mk_disturbance_work_stride(int64_t N, int64_t K)
{
    if (N < 1 || K < 1 || N + K > 64 || !specialised(N, K)) return 0;
    return layout_of(WORK_RECORDS, N, K).stride;
}

MK_API int mk_disturbances(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, double *d_r, double *d_ninfo,
                           uint32_t *d_status)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!d_work || !d_r || !d_ninfo) return fail(MK_ERR_INVALID, "mk_disturbances: d_work, d_r and d_ninfo are required");
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    const int64_t ws = mk_disturbance_work_stride(p->N, p->K);
    if (!ws || ctx->variant[MK_VARIANT_KERNEL_FAMILY] == 1)
        return fail(MK_ERR_SHAPE, "mk_disturbances serves specialised shapes with N + K <= 64 (ahead-of-time list or a shape module); "
                                  "N=%lld, K=%lld is not one%s", (long long)p->N, (long long)p->K,
                    ws ? " in this context (the size-generic kernel family is selected)" : "");
    const int64_t n = p->N + p->K;
    const device_buffer bufs[3] = {{d_work, p->n_instances * p->T * ws, "d_work (n_instances * T * mk_disturbance_work_stride(N, K) doubles)"},
                                   {d_r, p->n_instances * p->T * n, "d_r (n_instances * T * (N + K) doubles)"},
                                   {d_ninfo, p->n_instances * p->T * n, "d_ninfo (n_instances * T * (N + K) doubles)"}};
    if (int rc = buffers_fit("mk_disturbances", bufs, 3)) return rc;
    // the recording forward pass (no update tape: the walk recomputes), then the walk
    if (int rc = record_pass(ctx, p, d_work, ws, time_major, d_status)) return rc;
    mk::AdjointArgs a = reader_args<mk::AdjointArgs>(p, d_work, ws, time_major);
    a.dist_r = d_r;
    a.dist_n = d_ninfo;
    return timed_launches(ctx, [&]() -> int {
        MK_HIP(dispatch_disturb((int)p->N, (int)p->K, a, ctx->stream));
        return MK_OK;
    });
}

// ---- one-step-ahead innovations and their whiteness statistics (innov_kernels.hip) ----
MK_API int64_t mk_innovations_work_stride(int64_t N, int64_t K)
{
    if (N < 1 || K < 1 || N + K > mk::innov_max_states || !mk_shape_supported(N, K)) return 0;
    return layout_of(WORK_RECORDS, N, K).stride;
}

MK_API int mk_innovations(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, double *d_v, double *d_f,
                          double *d_pred_means, double *d_pred_vars, uint32_t *d_status)
{
    MK_CTX(ctx);
    if (int rc = check_problem(p)) return rc;
    if (!d_work) return fail(MK_ERR_INVALID, "mk_innovations: d_work is required");
    if (!d_v && !d_f && !d_pred_means && !d_pred_vars)
        return fail(MK_ERR_INVALID, "mk_innovations: nothing to write, give one of d_v, d_f, d_pred_means, d_pred_vars");
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    const int64_t ws = mk_innovations_work_stride(p->N, p->K);
    if (!ws) return too_many_states("mk_innovations", p, mk::innov_max_states);
    const int64_t cells = p->n_instances * p->T * p->N;
    const device_buffer bufs[5] = {{d_work, p->n_instances * p->T * ws, "d_work (n_instances * T * mk_innovations_work_stride(N, K) doubles)"},
                                   {d_v, cells, "d_v (n_instances * T * N doubles)"},
                                   {d_f, cells, "d_f (n_instances * T * N doubles)"},
                                   {d_pred_means, cells, "d_pred_means (n_instances * T * N doubles)"},
                                   {d_pred_vars, cells, "d_pred_vars (n_instances * T * N doubles)"}};
    if (int rc = buffers_fit("mk_innovations", bufs, 5)) return rc;
    if (int rc = record_pass(ctx, p, d_work, ws, time_major, d_status)) return rc;
    mk::InnovArgs a = reader_args<mk::InnovArgs>(p, d_work, ws, time_major);
    fill_scaling(a, p);
    a.v = d_v;
    a.f = d_f;
    a.pred_mean = d_pred_means;
    a.pred_var = d_pred_vars;
    return timed_launches(ctx, [&]() -> int {
        MK_HIP(mk::launch_innov_step(a, ctx->stream));
        return MK_OK;
    });
}

MK_API int mk_innovation_stats(mk_context *ctx, int64_t B, int64_t T, int64_t N, int time_major, int64_t t_first, int64_t nlags,
                               const double *d_v, const double *d_f, double *d_stats)
{
    MK_CTX(ctx);
    if (B < 1 || T < 1 || N < 1 || t_first < 0 || nlags < 1 || nlags > mk::innov_max_lags)
        return fail(MK_ERR_INVALID, "mk_innovation_stats: need B, T, N >= 1, t_first >= 0 and 1 <= nlags <= %d", mk::innov_max_lags);
    if (!d_v || !d_f || !d_stats) return fail(MK_ERR_INVALID, "mk_innovation_stats: d_v, d_f and d_stats are required");
    const device_buffer bufs[3] = {{d_v, B * T * N, "d_v (B * T * N doubles)"},
                                   {d_f, B * T * N, "d_f (B * T * N doubles)"},
                                   {d_stats, B * N * (4 + nlags), "d_stats (B * N * (4 + nlags) doubles)"}};
    if (int rc = buffers_fit("mk_innovation_stats", bufs, 3)) return rc;
    mk::InnovStatsArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B;
    a.T = T;
    a.N = (int)N;
    a.L = (int)nlags;
    fill_layout(a, time_major, B, T);
    a.t_first = t_first;
    a.v = d_v;
    a.f = d_f;
    a.stats = d_stats;
    MK_HIP(mk::launch_innov_stats(a, ctx->stream));
    return MK_OK;
}

// ---- residual diagnostics of the standardised innovations (resid_kernels.hip) ----
MK_API int mk_residual_series(mk_context *ctx, int64_t B, int64_t T, int64_t N, int time_major, int64_t t_first, const double *d_v,
                              const double *d_f, double *d_stats)
{
    MK_CTX(ctx);
    if (B < 1 || T < 1 || N < 1 || t_first < 0) return fail(MK_ERR_INVALID, "mk_residual_series: need B, T, N >= 1 and t_first >= 0");
    if (!d_v) return fail(MK_ERR_INVALID, "mk_residual_series: d_v is required");
    if (!d_f) return fail(MK_ERR_INVALID, "mk_residual_series: d_f is required");
    if (!d_stats) return fail(MK_ERR_INVALID, "mk_residual_series: d_stats is required");
    const device_buffer bufs[3] = {{d_v, B * T * N, "d_v (B * T * N doubles)"},
                                   {d_f, B * T * N, "d_f (B * T * N doubles)"},
                                   {d_stats, B * N * mk::resid_stats, "d_stats (B * N * 12 doubles)"}};
    if (int rc = buffers_fit("mk_residual_series", bufs, 3)) return rc;
    mk::ResidSeriesArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B;
    a.T = T;
    a.N = (int)N;
    fill_layout(a, time_major, B, T);
    a.t_first = t_first;
    a.v = d_v;
    a.f = d_f;
    a.stats = d_stats;
    MK_HIP(mk::launch_resid_series(a, ctx->stream));
    return MK_OK;
}

MK_API int mk_residual_cross(mk_context *ctx, int64_t B, int64_t T, int64_t N, int time_major, int64_t t_first, int64_t nlags,
                             const double *d_v, const double *d_f, const double *d_stats, int64_t *d_counts, double *d_sums)
{
    MK_CTX(ctx);
    if (B < 1 || T < 1 || N < 1 || t_first < 0) return fail(MK_ERR_INVALID, "mk_residual_cross: need B, T, N >= 1 and t_first >= 0");
    if (N > mk::resid_max_series) return fail(MK_ERR_INVALID, "mk_residual_cross: N = %lld, need N <= %d", (long long)N, mk::resid_max_series);
    if (nlags < 0 || nlags > mk::resid_max_lags)
        return fail(MK_ERR_INVALID, "mk_residual_cross: nlags = %lld, need 0 <= nlags <= %d", (long long)nlags, mk::resid_max_lags);
    if (!d_v) return fail(MK_ERR_INVALID, "mk_residual_cross: d_v is required");
    if (!d_f) return fail(MK_ERR_INVALID, "mk_residual_cross: d_f is required");
    if (!d_stats) return fail(MK_ERR_INVALID, "mk_residual_cross: d_stats is required (the rows written by mk_residual_series)");
    if (!d_counts) return fail(MK_ERR_INVALID, "mk_residual_cross: d_counts is required");
    if (!d_sums) return fail(MK_ERR_INVALID, "mk_residual_cross: d_sums is required");
    const int64_t pairs = B * (nlags + 1) * N * N;
    const device_buffer bufs[5] = {{d_v, B * T * N, "d_v (B * T * N doubles)"},
                                   {d_f, B * T * N, "d_f (B * T * N doubles)"},
                                   {d_stats, B * N * mk::resid_stats, "d_stats (B * N * 12 doubles)"},
                                   {d_counts, pairs, "d_counts (B * (nlags + 1) * N * N 64-bit integers)"},
                                   {d_sums, pairs, "d_sums (B * (nlags + 1) * N * N doubles)"}};
    if (int rc = buffers_fit("mk_residual_cross", bufs, 5)) return rc;
    mk::ResidCrossArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B;
    a.T = T;
    a.N = (int)N;
    a.L = (int)nlags;
    fill_layout(a, time_major, B, T);
    a.t_first = t_first;
    a.v = d_v;
    a.f = d_f;
    a.stats = d_stats;
    a.counts = (long long *)d_counts;
    a.sums = d_sums;
    MK_HIP(mk::launch_resid_cross(a, ctx->stream));
    return MK_OK;
}

// ---- multi-step-ahead forecasts and forecast skill by horizon (forecast_kernels.hip) ----
MK_API int64_t mk_forecast_max_horizon(void) { return mk::forecast_max_horizon; }

MK_API int64_t mk_forecast_work_stride(int64_t N, int64_t K)
{
    if (N < 1 || K < 1 || N + K > mk::forecast_max_states || !mk_shape_supported(N, K)) return 0;
    return layout_of(WORK_FORECAST, N, K).stride;
}

MK_API int mk_forecast(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, const mk_forecast_request *req,
                       uint32_t *d_status)
{
    if (int rc = reader_preamble(ctx, "mk_forecast", "mk_forecast_request", p, mk::forecast_max_states, req, d_work)) return rc;
    const bool fan = req->d_fan_means || req->d_fan_vars, track = req->d_track_means || req->d_track_vars, skill = req->d_skill != nullptr;
    if (!fan && !track && !skill)
        return fail(MK_ERR_INVALID, "mk_forecast: nothing to write, give one of d_fan_means, d_fan_vars, d_track_means, d_track_vars, d_skill");
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    if (req->horizon < 1 || req->horizon > mk::forecast_max_horizon)
        return fail(MK_ERR_INVALID, "mk_forecast: need 1 <= horizon <= %d (got %lld)", mk::forecast_max_horizon, (long long)req->horizon);
    if (track && (req->track_horizon < 1 || req->track_horizon > p->T))
        return fail(MK_ERR_INVALID, "mk_forecast: need 1 <= track_horizon <= T = %lld (got %lld)", (long long)p->T,
                    (long long)req->track_horizon);
    if (req->t_first < 0) return fail(MK_ERR_INVALID, "mk_forecast: t_first must be >= 0");
    if (!(req->coverage_z > 0.0) || !std::isfinite(req->coverage_z))
        return fail(MK_ERR_INVALID, "mk_forecast: coverage_z must be positive and finite");
    const int64_t B = p->n_instances;
    const work_layout w = layout_of(WORK_FORECAST, p->N, p->K, B, p->T);
    const device_buffer bufs[7] = {{d_work, B * p->T * w.stride, "d_work (n_instances * T * mk_forecast_work_stride(N, K) doubles)"},
                                   {req->d_fan_origins, p->n_records, "d_fan_origins (n_records 64-bit integers)"},
                                   {req->d_fan_means, B * req->horizon * p->N, "d_fan_means (n_instances * horizon * N doubles)"},
                                   {req->d_fan_vars, B * req->horizon * p->N, "d_fan_vars (n_instances * horizon * N doubles)"},
                                   {req->d_track_means, B * p->T * p->N, "d_track_means (n_instances * T * N doubles)"},
                                   {req->d_track_vars, B * p->T * p->N, "d_track_vars (n_instances * T * N doubles)"},
                                   {req->d_skill, B * p->N * req->horizon * 6, "d_skill (n_instances * N * horizon * 6 doubles)"}};
    if (int rc = buffers_fit("mk_forecast", bufs, 7)) return rc;
    if (fan && req->d_fan_origins) { // R integers to the host: an origin out of range would index outside the records
        std::vector<int64_t> h((size_t)p->n_records);
        MK_HIP(hipMemcpyAsync(h.data(), req->d_fan_origins, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
        MK_HIP(hipStreamSynchronize(ctx->stream));
        for (int64_t r = 0; r < p->n_records; ++r)
            if (h[(size_t)r] < -1 || h[(size_t)r] > p->T - 1)
                return fail(MK_ERR_INVALID, "mk_forecast: d_fan_origins[%lld] = %lld is outside -1 .. T - 1 = %lld", (long long)r,
                            (long long)h[(size_t)r], (long long)(p->T - 1));
    }
    if (int rc = record_pass(ctx, p, d_work, w.rs, time_major, d_status)) return rc;
    mk::ForecastArgs a = reader_args<mk::ForecastArgs>(p, d_work, w.rs, time_major);
    fill_scaling(a, p);
    a.H = (int)req->horizon;
    a.track_h = track ? req->track_horizon : 1;
    a.t_first = req->t_first;
    a.z2 = req->coverage_z * req->coverage_z;
    a.fan_origins = req->d_fan_origins;
    a.fan_mean = req->d_fan_means;
    a.fan_var = req->d_fan_vars;
    a.track_mean = req->d_track_means;
    a.track_var = req->d_track_vars;
    a.skill = req->d_skill;
    a.partial = d_work + w.partial;
    return timed_launches(ctx, [&]() -> int {
        if (fan || track) MK_HIP(mk::launch_forecast_path(a, ctx->stream));
        if (skill) MK_HIP(mk::launch_forecast_skill(a, ctx->stream));
        return MK_OK;
    });
}

// ---- observation weights of smoothed series and states (weights_kernels.hip) ----
MK_API int64_t mk_weights_work_stride(int64_t N, int64_t K)
{
    if (N < 1 || K < 1 || N + K > mk::weights_max_states || !mk_shape_supported(N, K)) return 0;
    return layout_of(WORK_GAIN, N, K).stride;
}

MK_API int mk_observation_weights(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, const mk_weights_request *req,
                                  uint32_t *d_status)
{
    if (int rc = reader_preamble(ctx, "mk_observation_weights", "mk_weights_request", p, mk::weights_max_states, req, d_work)) return rc;
    if (!req->d_targets || !req->d_weights) return fail(MK_ERR_INVALID, "mk_observation_weights: d_targets and d_weights are required");
    if (req->n_targets < 1) return fail(MK_ERR_INVALID, "mk_observation_weights: need n_targets >= 1 (got %lld)", (long long)req->n_targets);
    if (req->what != MK_DRAW_SERIES && req->what != MK_DRAW_STATES)
        return fail(MK_ERR_INVALID, "mk_observation_weights: what must be MK_DRAW_SERIES or MK_DRAW_STATES (got %d)", req->what);
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    if (!mk_weights_work_stride(p->N, p->K)) return too_many_states("mk_observation_weights", p, mk::weights_max_states);
    const int64_t B = p->n_instances, M = req->n_targets;
    const work_layout w = layout_of(WORK_GAIN, p->N, p->K, B, p->T);
    static_assert(sizeof(int64_t) == sizeof(double), "buffers_fit counts 8-byte words");
    const device_buffer bufs[4] = {{d_work, B * p->T * w.stride, "d_work (n_instances * T * mk_weights_work_stride(N, K) doubles)"},
                                   {req->d_targets, p->n_records * M * 2, "d_targets (n_records * n_targets * 2 64-bit integers)"},
                                   {req->d_weights, B * M * p->T * p->N, "d_weights (n_instances * n_targets * T * N doubles)"},
                                   {req->d_intercept, B * M, "d_intercept (n_instances * n_targets doubles)"}};
    if (int rc = buffers_fit("mk_observation_weights", bufs, 4)) return rc;
    if (int rc = record_pass(ctx, p, d_work, w.rs, time_major, d_status)) return rc;
    mk::WeightsArgs a = reader_args<mk::WeightsArgs>(p, d_work, w.rs, time_major);
    a.M = M;
    a.states = req->what == MK_DRAW_STATES ? 1 : 0;
    a.gs = w.gs;
    a.gain = d_work + w.tape;
    a.targets = req->d_targets;
    a.weights = req->d_weights;
    a.intercept = req->d_intercept;
    return timed_launches(ctx, [&]() -> int {
        if (int rc = gain_tape_stage(ctx, p, d_work, w, time_major)) return rc;
        MK_HIP(mk::launch_weights_walk(a, ctx->stream));
        return MK_OK;
    });
}

// ---- intervention effects by GLS (regress_kernels.hip) ----
MK_API int64_t mk_regression_max_effects(void) { return mk::regress_max_effects; }

MK_API int64_t mk_regression_work_stride(int64_t N, int64_t K)
{
    static_assert(mk::regress_max_states == mk::weights_max_states, "the regression runs on the weights' workspace");
    return mk_weights_work_stride(N, K);
}

// the effects of a request, copied to the host: a slot in use must name a series, a kind and a step range that exist
static int check_effects(mk_context *ctx, const char *who, const int64_t *d_effects, int64_t R, int64_t M, int64_t T, int64_t N)
{
    std::vector<int64_t> h((size_t)(R * M * 4));
    MK_HIP(hipMemcpyAsync(h.data(), d_effects, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MK_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < R * M; ++i) {
        const int64_t *e = &h[(size_t)i * 4];
        if (e[0] < 0) continue;
        if (e[0] >= N)
            return fail(MK_ERR_INVALID, "%s: d_effects[%lld, %lld]: series %lld is outside 0 .. N - 1 = %lld", who, (long long)(i / M),
                        (long long)(i % M), (long long)e[0], (long long)(N - 1));
        if (e[1] != MK_EFFECT_LEVEL && e[1] != MK_EFFECT_RAMP)
            return fail(MK_ERR_INVALID, "%s: d_effects[%lld, %lld]: kind must be MK_EFFECT_LEVEL or MK_EFFECT_RAMP (got %lld)", who,
                        (long long)(i / M), (long long)(i % M), (long long)e[1]);
        if (!(0 <= e[2] && e[2] < e[3] && e[3] <= T))
            return fail(MK_ERR_INVALID, "%s: d_effects[%lld, %lld]: need 0 <= t0 < t1 <= T = %lld (got t0 = %lld, t1 = %lld)", who,
                        (long long)(i / M), (long long)(i % M), (long long)T, (long long)e[2], (long long)e[3]);
    }
    return MK_OK;
}

MK_API int mk_regression(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, const mk_regression_request *req,
                         uint32_t *d_status)
{
    if (int rc = reader_preamble(ctx, "mk_regression", "mk_regression_request", p, mk::regress_max_states, req, d_work)) return rc;
    if (!req->d_effects || !req->d_beta || !req->d_cov || !req->d_gain || !req->d_normal || !req->d_support || !req->d_dropped)
        return fail(MK_ERR_INVALID, "mk_regression: d_effects, d_beta, d_cov, d_gain, d_normal, d_support and d_dropped are required");
    if (req->n_effects < 1 || req->n_effects > mk::regress_max_effects)
        return fail(MK_ERR_INVALID, "mk_regression: need 1 <= n_effects <= %d (got %lld)", mk::regress_max_effects, (long long)req->n_effects);
    if (req->t_first < 0) return fail(MK_ERR_INVALID, "mk_regression: t_first must be >= 0");
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    if (!mk_regression_work_stride(p->N, p->K)) return too_many_states("mk_regression", p, mk::regress_max_states);
    const int64_t B = p->n_instances, M = req->n_effects;
    const work_layout w = layout_of(WORK_GAIN, p->N, p->K, B, p->T);
    static_assert(sizeof(int64_t) == sizeof(double), "buffers_fit counts 8-byte words");
    const device_buffer bufs[8] = {{d_work, B * p->T * w.stride, "d_work (n_instances * T * mk_regression_work_stride(N, K) doubles)"},
                                   {req->d_effects, p->n_records * M * 4, "d_effects (n_records * n_effects * 4 64-bit integers)"},
                                   {req->d_beta, B * M, "d_beta (n_instances * n_effects doubles)"},
                                   {req->d_cov, B * M * M, "d_cov (n_instances * n_effects^2 doubles)"},
                                   {req->d_gain, B, "d_gain (n_instances doubles)"},
                                   {req->d_normal, B * (M + 1) * (M + 1), "d_normal (n_instances * (n_effects + 1)^2 doubles)"},
                                   {req->d_support, B * M, "d_support (n_instances * n_effects 64-bit integers)"},
                                   {req->d_dropped, (B + 1) / 2, "d_dropped (n_instances 32-bit words)"}};
    if (int rc = buffers_fit("mk_regression", bufs, 8)) return rc;
    if (int rc = check_effects(ctx, "mk_regression", req->d_effects, p->n_records, M, p->T, p->N)) return rc;
    if (int rc = record_pass(ctx, p, d_work, w.rs, time_major, d_status)) return rc;
    mk::RegressArgs a = reader_args<mk::RegressArgs>(p, d_work, w.rs, time_major); // the replay reads the tape, not the records
    a.M = M;
    a.t_first = req->t_first;
    a.gs = w.gs;
    a.gain = d_work + w.tape;
    a.effects = req->d_effects;
    a.beta = req->d_beta;
    a.cov = req->d_cov;
    a.gainout = req->d_gain;
    a.normal = req->d_normal;
    a.support = req->d_support;
    a.dropped = req->d_dropped;
    return timed_launches(ctx, [&]() -> int {
        if (int rc = gain_tape_stage(ctx, p, d_work, w, time_major)) return rc;
        MK_HIP(mk::launch_regress_replay(a, ctx->stream));
        return MK_OK;
    });
}

MK_API int mk_regression_adjust(mk_context *ctx, int64_t R, int64_t T, int64_t N, int time_major, int64_t n_effects,
                                const int64_t *d_effects, const double *d_beta, const double *d_obs_in, double *d_obs_out)
{
    MK_CTX(ctx);
    if (R < 1 || T < 1 || N < 1) return fail(MK_ERR_INVALID, "mk_regression_adjust: need R, T, N >= 1");
    if (n_effects < 1 || n_effects > mk::regress_max_effects)
        return fail(MK_ERR_INVALID, "mk_regression_adjust: need 1 <= n_effects <= %d (got %lld)", mk::regress_max_effects, (long long)n_effects);
    if (!d_effects || !d_beta || !d_obs_in || !d_obs_out)
        return fail(MK_ERR_INVALID, "mk_regression_adjust: d_effects, d_beta, d_obs_in and d_obs_out are required");
    const device_buffer bufs[4] = {{d_effects, R * n_effects * 4, "d_effects (R * n_effects * 4 64-bit integers)"},
                                   {d_beta, R * n_effects, "d_beta (R * n_effects doubles)"},
                                   {d_obs_in, R * T * N, "d_obs_in (R * T * N doubles)"},
                                   {d_obs_out, R * T * N, "d_obs_out (R * T * N doubles)"}};
    if (int rc = buffers_fit("mk_regression_adjust", bufs, 4)) return rc;
    if (int rc = check_effects(ctx, "mk_regression_adjust", d_effects, R, n_effects, T, N)) return rc;
    mk::RegressAdjustArgs a;
    memset(&a, 0, sizeof(a));
    a.R = R;
    a.T = T;
    a.M = n_effects;
    a.N = (int)N;
    a.bs = time_major ? 1 : T;
    a.ts = time_major ? R : 1;
    a.effects = d_effects;
    a.beta = d_beta;
    a.in = d_obs_in;
    a.out = d_obs_out;
    MK_HIP(mk::launch_regress_adjust(a, ctx->stream));
    return MK_OK;
}

// ---- per-step scores by the tangent filter (score_kernels.hip) ----
MK_API int64_t mk_scores_max_states(void) { return mk::score_max_states; }

MK_API int64_t mk_scores_work_stride(int64_t N, int64_t K)
{
    static_assert(mk::score_max_states == mk::weights_max_states, "the scores run on the weights' workspace and a row of innovations");
    return mk_weights_work_stride(N, K) ? layout_of(WORK_SCORES, N, K).stride : 0;
}

MK_API int mk_scores(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, const mk_scores_request *req, uint32_t *d_status)
{
    if (int rc = reader_preamble(ctx, "mk_scores", "mk_scores_request", p, mk::score_max_states, req, d_work)) return rc;
    if (!req->d_dphi || !req->d_dq || !req->d_score || !req->d_grad || !req->d_count || !req->d_opg || !req->d_cusum)
        return fail(MK_ERR_INVALID, "mk_scores: d_dphi, d_dq, d_score, d_grad, d_count, d_opg and d_cusum are required");
    if (req->t_first < 0) return fail(MK_ERR_INVALID, "mk_scores: t_first must be >= 0");
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    if (!mk_scores_work_stride(p->N, p->K)) return too_many_states("mk_scores", p, mk::score_max_states);
    const int64_t B = p->n_instances, n = p->N + p->K;
    const work_layout w = layout_of(WORK_SCORES, p->N, p->K, B, p->T);
    static_assert(sizeof(int64_t) == sizeof(double), "buffers_fit counts 8-byte words");
    const device_buffer bufs[8] = {{d_work, B * p->T * w.stride, "d_work (n_instances * T * mk_scores_work_stride(N, K) doubles)"},
                                   {req->d_dphi, B * n, "d_dphi (n_instances * (N + K) doubles)"},
                                   {req->d_dq, B * n, "d_dq (n_instances * (N + K) doubles)"},
                                   {req->d_score, B * p->T * n, "d_score (n_instances * T * (N + K) doubles)"},
                                   {req->d_grad, B * n, "d_grad (n_instances * (N + K) doubles)"},
                                   {req->d_count, B, "d_count (n_instances 64-bit integers)"},
                                   {req->d_opg, B * n * n, "d_opg (n_instances * (N + K)^2 doubles)"},
                                   {req->d_cusum, B * n * n, "d_cusum (n_instances * (N + K)^2 doubles)"}};
    if (int rc = buffers_fit("mk_scores", bufs, 8)) return rc;
    if (int rc = record_pass(ctx, p, d_work, w.rs, time_major, d_status)) return rc;
    mk::ScoreArgs a = reader_args<mk::ScoreArgs>(p, d_work, w.rs, time_major);
    a.t_first = req->t_first;
    a.gs = w.gs;
    a.gain = d_work + w.tape;
    a.v = d_work + w.innov;
    a.dphi = req->d_dphi;
    a.dq = req->d_dq;
    a.score = req->d_score;
    a.grad = req->d_grad;
    a.count = req->d_count;
    a.opg = req->d_opg;
    a.cusum = req->d_cusum;
    return timed_launches(ctx, [&]() -> int {
        if (int rc = gain_tape_stage(ctx, p, d_work, w, time_major, d_work + w.innov)) return rc;
        MK_HIP(mk::launch_score_tangent(a, ctx->stream));
        MK_HIP(mk::launch_score_stats(a, ctx->stream));
        return MK_OK;
    });
}

// ---- leave-block-out predictions (block_kernels.hip) ----
MK_API int64_t mk_block_max_cells(void) { return mk::block_max_cells; }

MK_API int64_t mk_block_work_stride(int64_t N, int64_t K)
{
    static_assert(mk::block_max_states == mk::score_max_states, "the blocks run on the scores' workspace");
    return mk_scores_work_stride(N, K);
}

// the blocks of a request, copied to the host: a slot in use must name a series and a step range that exist and fit a row
static int check_blocks(mk_context *ctx, const int64_t *d_blocks, int64_t R, int64_t W, int64_t L, int64_t T, int64_t N)
{
    std::vector<int64_t> h((size_t)(R * W * 3));
    MK_HIP(hipMemcpyAsync(h.data(), d_blocks, sizeof(int64_t) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    MK_HIP(hipStreamSynchronize(ctx->stream));
    for (int64_t i = 0; i < R * W; ++i) {
        const int64_t *e = &h[(size_t)i * 3];
        if (e[0] < 0) continue;
        if (e[0] >= N)
            return fail(MK_ERR_INVALID, "mk_block_predict: d_blocks[%lld, %lld]: series %lld is outside 0 .. N - 1 = %lld", (long long)(i / W),
                        (long long)(i % W), (long long)e[0], (long long)(N - 1));
        if (!(0 <= e[1] && e[1] < e[2] && e[2] <= T))
            return fail(MK_ERR_INVALID, "mk_block_predict: d_blocks[%lld, %lld]: need 0 <= t0 < t1 <= T = %lld (got t0 = %lld, t1 = %lld)",
                        (long long)(i / W), (long long)(i % W), (long long)T, (long long)e[1], (long long)e[2]);
        if (e[2] - e[1] > L)
            return fail(MK_ERR_INVALID, "mk_block_predict: d_blocks[%lld, %lld]: t1 - t0 = %lld is more than n_cells = %lld", (long long)(i / W),
                        (long long)(i % W), (long long)(e[2] - e[1]), (long long)L);
    }
    return MK_OK;
}

MK_API int mk_block_predict(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, const mk_block_request *req,
                            uint32_t *d_status)
{
    if (int rc = reader_preamble(ctx, "mk_block_predict", "mk_block_request", p, mk::block_max_states, req, d_work)) return rc;
    if (!req->d_blocks || !req->d_checkpoints || !req->d_means || !req->d_vars || !req->d_summary || !req->d_flags)
        return fail(MK_ERR_INVALID, "mk_block_predict: d_blocks, d_checkpoints, d_means, d_vars, d_summary and d_flags are required");
    if (req->n_blocks < 1) return fail(MK_ERR_INVALID, "mk_block_predict: need n_blocks >= 1 (got %lld)", (long long)req->n_blocks);
    if (req->n_cells < 1 || req->n_cells > mk::block_max_cells)
        return fail(MK_ERR_INVALID, "mk_block_predict: need 1 <= n_cells <= %d (got %lld)", mk::block_max_cells, (long long)req->n_cells);
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    if (!mk_block_work_stride(p->N, p->K)) return too_many_states("mk_block_predict", p, mk::block_max_states);
    const int64_t B = p->n_instances, W = req->n_blocks, L = req->n_cells, n = p->N + p->K;
    const work_layout w = layout_of(WORK_SCORES, p->N, p->K, B, p->T);
    static_assert(sizeof(int64_t) == sizeof(double), "buffers_fit counts 8-byte words");
    const device_buffer bufs[7] = {{d_work, B * p->T * w.stride, "d_work (n_instances * T * mk_block_work_stride(N, K) doubles)"},
                                   {req->d_blocks, p->n_records * W * 3, "d_blocks (n_records * n_blocks * 3 64-bit integers)"},
                                   {req->d_checkpoints, B * W * (n + n * n), "d_checkpoints (n_instances * n_blocks * (n + n^2) doubles)"},
                                   {req->d_means, B * W * L, "d_means (n_instances * n_blocks * n_cells doubles)"},
                                   {req->d_vars, B * W * L, "d_vars (n_instances * n_blocks * n_cells doubles)"},
                                   {req->d_summary, B * W * 4, "d_summary (n_instances * n_blocks * 4 doubles)"},
                                   {req->d_flags, (B * W + 1) / 2, "d_flags (n_instances * n_blocks 32-bit words)"}};
    if (int rc = buffers_fit("mk_block_predict", bufs, 7)) return rc;
    if (int rc = check_blocks(ctx, req->d_blocks, p->n_records, W, L, p->T, p->N)) return rc;
    if (int rc = record_pass(ctx, p, d_work, w.rs, time_major, d_status)) return rc;
    mk::BlockArgs a = reader_args<mk::BlockArgs>(p, d_work, w.rs, time_major); // the walks read the tape, not the records
    fill_scaling(a, p);
    a.W = W;
    a.L = L;
    a.gs = w.gs;
    a.gain = d_work + w.tape;
    a.v = d_work + w.innov;
    a.blocks = req->d_blocks;
    a.checkpoints = req->d_checkpoints;
    a.means = req->d_means;
    a.vars = req->d_vars;
    a.summary = req->d_summary;
    a.flags = req->d_flags;
    return timed_launches(ctx, [&]() -> int {
        if (int rc = gain_tape_stage(ctx, p, d_work, w, time_major, d_work + w.innov)) return rc;
        MK_HIP(mk::launch_block_checkpoint(a, ctx->stream));
        MK_HIP(mk::launch_block_walk(a, ctx->stream));
        return MK_OK;
    });
}

// ---- level-shift scan (shift_kernels.hip) ----
MK_API int64_t mk_shift_work_stride(int64_t N, int64_t K)
{
    static_assert(mk::shift_max_states == mk::block_max_states, "the scan runs on the blocks' workspace");
    return mk_block_work_stride(N, K);
}

MK_API int mk_level_shifts(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, const mk_shift_request *req,
                           uint32_t *d_status)
{
    if (int rc = reader_preamble(ctx, "mk_level_shifts", "mk_shift_request", p, mk::shift_max_states, req, d_work)) return rc;
    if (!req->d_num || !req->d_den) return fail(MK_ERR_INVALID, "mk_level_shifts: d_num and d_den are required");
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    if (!mk_shift_work_stride(p->N, p->K)) return too_many_states("mk_level_shifts", p, mk::shift_max_states);
    const int64_t B = p->n_instances;
    const work_layout w = layout_of(WORK_SCORES, p->N, p->K, B, p->T);
    const device_buffer bufs[3] = {{d_work, B * p->T * w.stride, "d_work (n_instances * T * mk_shift_work_stride(N, K) doubles)"},
                                   {req->d_num, B * p->T * p->N, "d_num (n_instances * T * N doubles)"},
                                   {req->d_den, B * p->T * p->N, "d_den (n_instances * T * N doubles)"}};
    if (int rc = buffers_fit("mk_level_shifts", bufs, 3)) return rc;
    if (int rc = record_pass(ctx, p, d_work, w.rs, time_major, d_status)) return rc;
    mk::ShiftArgs a = reader_args<mk::ShiftArgs>(p, d_work, w.rs, time_major); // the scan reads the tape, not the records
    a.gs = w.gs;
    a.gain = d_work + w.tape;
    a.v = d_work + w.innov;
    a.num = req->d_num;
    a.den = req->d_den;
    return timed_launches(ctx, [&]() -> int {
        if (int rc = gain_tape_stage(ctx, p, d_work, w, time_major, d_work + w.innov)) return rc;
        MK_HIP(mk::launch_shift_scan(a, ctx->stream));
        return MK_OK;
    });
}

// ---- exact window means, changes and contrasts of the smoothed signal (functional_kernels.hip) ----
MK_API int64_t mk_functionals_max_contrasts(void) { return mk::functional_max_contrasts; }

MK_API int64_t mk_functionals_work_stride(int64_t N, int64_t K)
{
    if (N < 1 || K < 1 || N + K > mk::functional_max_states || !mk_shape_supported(N, K)) return 0;
    return layout_of(WORK_FUNCTIONALS, N, K).stride; // the filtered and the smoothed record of a step
}

MK_API int mk_functionals(mk_context *ctx, const mk_problem *p, double *d_work, int time_major, const mk_functional_request *req,
                          double *d_mean, double *d_var, uint32_t *d_status)
{
    if (int rc = reader_preamble(ctx, "mk_functionals", "mk_functional_request", p, mk::functional_max_states, req, d_work)) return rc;
    if (!req->d_windows || !d_mean || !d_var) return fail(MK_ERR_INVALID, "mk_functionals: d_windows, d_mean and d_var are required");
    if (req->n_windows < 1) return fail(MK_ERR_INVALID, "mk_functionals: need n_windows >= 1 (got %lld)", (long long)req->n_windows);
    if (req->n_contrasts < 1 || req->n_contrasts > mk::functional_max_contrasts)
        return fail(MK_ERR_INVALID, "mk_functionals: need 1 <= n_contrasts <= %d (got %lld)", mk::functional_max_contrasts,
                    (long long)req->n_contrasts);
    if (!req->d_contrasts && req->n_contrasts != p->N)
        return fail(MK_ERR_INVALID, "mk_functionals: d_contrasts = NULL stands for the N unit contrasts, n_contrasts must be N = %lld (got %lld)",
                    (long long)p->N, (long long)req->n_contrasts);
    if (!p->d_obs || !p->d_loadings) return fail(MK_ERR_INVALID, "d_obs and d_loadings are required");
    if (!mk_functionals_work_stride(p->N, p->K)) return too_many_states("mk_functionals", p, mk::functional_max_states);
    const int64_t B = p->n_instances, W = req->n_windows, C = req->n_contrasts, n = p->N + p->K;
    const work_layout w = layout_of(WORK_FUNCTIONALS, p->N, p->K, B, p->T);
    static_assert(sizeof(int64_t) == sizeof(double), "buffers_fit counts 8-byte words");
    const device_buffer bufs[5] = {{d_work, B * p->T * w.stride, "d_work (n_instances * T * mk_functionals_work_stride(N, K) doubles)"},
                                   {req->d_windows, p->n_records * W * 4, "d_windows (n_records * n_windows * 4 64-bit integers)"},
                                   {req->d_contrasts, p->n_records * C * p->N, "d_contrasts (n_records * n_contrasts * N doubles)"},
                                   {d_mean, B * W * C, "d_mean (n_instances * n_windows * n_contrasts doubles)"},
                                   {d_var, B * W * C, "d_var (n_instances * n_windows * n_contrasts doubles)"}};
    if (int rc = buffers_fit("mk_functionals", bufs, 5)) return rc;
    // the forward pass and the smoother of mk_filter_smooth for the shape (full-square records, no projection), then the walk
    if (int rc = record_pass(ctx, p, d_work, w.rs, time_major, d_status)) return rc;
    double *smoothed = d_work + w.smoothed;
    mk_outputs o;
    memset(&o, 0, sizeof(o));
    o.d_status = d_status;
    o.d_F = d_work;
    o.d_Pf = d_work + n;
    o.d_S = smoothed;
    o.d_Ps = smoothed + n;
    o.time_major = time_major;
    o.record_stride = w.rs;
    if (int rc = do_smooth(ctx, p, &o, false)) return rc;
    mk::FunctionalArgs a;
    memset(&a, 0, sizeof(a));
    a.B = B;
    a.R = p->n_records;
    a.T = p->T;
    a.W = W;
    a.C = C;
    a.N = (int)p->N;
    a.K = (int)p->K;
    fill_layout(a, time_major, B, p->T);
    fill_scaling(a, p);
    a.rs = w.rs;
    a.phi = p->d_phi;
    a.q = p->d_q;
    a.loadings = p->d_loadings;
    a.F = d_work;
    a.S = smoothed;
    a.windows = req->d_windows;
    a.contrasts = req->d_contrasts;
    a.mean = d_mean;
    a.var = d_var;
    a.status = d_status;
    return timed_launches(ctx, [&]() -> int {
        MK_HIP(mk::launch_functional_walk(a, ctx->stream));
        return MK_OK;
    });
}

// ---- lock-step L-BFGS of the batched calibration (mk_lbfgs.hip) ----
static int lbfgs_run(mk_context *ctx, int which, mk::LbfgsArgs &a, int counter, int *h_count)
{
    if (a.R <= 0 || a.n <= 0 || a.n > MK_LBFGS_MAX_N || a.H < 1 || a.H > MK_LBFGS_MAX_H)
        return fail(MK_ERR_INVALID, "mk_lbfgs: need R >= 1, 1 <= n <= %d, 1 <= ring slots <= %d", MK_LBFGS_MAX_N, MK_LBFGS_MAX_H);
    if (!ctx->lb_counters) MK_HIP(hipMalloc((void **)&ctx->lb_counters, 4 * sizeof(int)));
    a.counters = ctx->lb_counters;
    if (counter >= 0) MK_HIP(hipMemsetAsync(ctx->lb_counters + counter, 0, sizeof(int), ctx->stream));
    MK_HIP(mk::launch_lbfgs(which, a, ctx->stream));
    if (counter >= 0 && h_count) {
        MK_HIP(hipMemcpyAsync(h_count, ctx->lb_counters + counter, sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MK_HIP(hipStreamSynchronize(ctx->stream));
    }
    return MK_OK;
}

MK_API int mk_lbfgs_direction(mk_context *ctx, int64_t R, int64_t n, int64_t history, const double *d_x, const double *d_g, const double *d_lo,
                              uint8_t *d_active, const double *d_Sh, const double *d_Yh, const double *d_rho, const int *d_hlen,
                              const int *d_hpos, double gtol, double *d_pg, double *d_d, uint8_t *d_phase, double *d_step, int *d_nback,
                              int *h_nactive)
{
    MK_CTX(ctx);
    if (!d_x || !d_g || !d_lo || !d_active || !d_pg || !d_d || !d_Sh || !d_Yh || !d_rho || !d_hlen || !d_hpos)
        return fail(MK_ERR_INVALID, "mk_lbfgs_direction: null pointer");
    mk::LbfgsArgs a;
    memset(&a, 0, sizeof(a));
    a.R = R;
    a.n = (int)n;
    a.H = (int)history;
    a.gtol = gtol;
    a.x = const_cast<double *>(d_x);
    a.g = const_cast<double *>(d_g);
    a.lo = d_lo;
    a.active = d_active;
    a.Sh = const_cast<double *>(d_Sh);
    a.Yh = const_cast<double *>(d_Yh);
    a.rho = const_cast<double *>(d_rho);
    a.hlen = const_cast<int *>(d_hlen);
    a.hpos = const_cast<int *>(d_hpos);
    a.pg = d_pg;
    a.d = d_d;
    a.phase = d_phase;
    a.step = d_step;
    a.nback = d_nback;
    return lbfgs_run(ctx, 0, a, 0, h_nactive);
}

MK_API int mk_lbfgs_trial(mk_context *ctx, int64_t R, int64_t n, const double *d_x, const double *d_d, const double *d_step, const double *d_lo,
                          const uint8_t *d_searching, const double *d_x_new, double *d_xt, double *d_xe)
{
    MK_CTX(ctx);
    if (!d_x || !d_d || !d_step || !d_lo || !d_searching || !d_x_new || !d_xt || !d_xe) return fail(MK_ERR_INVALID, "mk_lbfgs_trial: null pointer");
    mk::LbfgsArgs a;
    memset(&a, 0, sizeof(a));
    a.R = R;
    a.n = (int)n;
    a.H = 1;
    a.x = const_cast<double *>(d_x);
    a.d = const_cast<double *>(d_d);
    a.step = const_cast<double *>(d_step);
    a.lo = d_lo;
    a.searching = const_cast<uint8_t *>(d_searching);
    a.x_new = const_cast<double *>(d_x_new);
    a.xt = d_xt;
    a.xe = d_xe;
    return lbfgs_run(ctx, 1, a, -1, nullptr);
}

MK_API int mk_lbfgs_armijo(mk_context *ctx, int64_t R, int64_t n, const double *d_ft, const double *d_f, const double *d_pg, const double *d_xt,
                           const double *d_x, uint8_t *d_searching, double *d_step, double *d_x_new, double *d_f_new, int *d_nback,
                           int64_t max_backtracks, uint8_t *d_accepted, int *h_nsearching, int *h_naccepted)
{
    MK_CTX(ctx);
    if (!d_ft || !d_f || !d_pg || !d_xt || !d_x || !d_searching || !d_step || !d_x_new || !d_f_new || (d_nback && !d_accepted))
        return fail(MK_ERR_INVALID, "mk_lbfgs_armijo: null pointer");
    mk::LbfgsArgs a;
    memset(&a, 0, sizeof(a));
    a.R = R;
    a.n = (int)n;
    a.H = 1;
    a.ft = d_ft;
    a.f = const_cast<double *>(d_f);
    a.pg = const_cast<double *>(d_pg);
    a.xt = const_cast<double *>(d_xt);
    a.x = const_cast<double *>(d_x);
    a.searching = d_searching;
    a.step = d_step;
    a.x_new = d_x_new;
    a.f_new = d_f_new;
    a.nback = d_nback;
    a.max_backtracks = (int)max_backtracks;
    a.mask = d_accepted;
    if (!ctx->lb_counters) MK_HIP(hipMalloc((void **)&ctx->lb_counters, 4 * sizeof(int)));
    MK_HIP(hipMemsetAsync(ctx->lb_counters + 3, 0, sizeof(int), ctx->stream));
    if (int rc = lbfgs_run(ctx, 2, a, 1, h_naccepted ? nullptr : h_nsearching)) return rc;
    if (h_naccepted) { // both counts with one synchronisation
        int two[4];
        MK_HIP(hipMemcpyAsync(two, ctx->lb_counters, 4 * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        MK_HIP(hipStreamSynchronize(ctx->stream));
        if (h_nsearching) *h_nsearching = two[1];
        *h_naccepted = two[3];
    }
    return MK_OK;
}

MK_API int mk_lbfgs_update(mk_context *ctx, int64_t R, int64_t n, int64_t history, double *d_x, double *d_f, double *d_g, const double *d_x_new,
                           const double *d_f_new, const double *d_g_new, int keep_old_gradient_if_searching, const uint8_t *d_searching,
                           const uint8_t *d_mask, uint8_t *d_active, double ftol, double *d_Sh, double *d_Yh, double *d_rho, int *d_hlen,
                           int *d_hpos, uint8_t *d_phase, int *d_nit, int64_t maxiter, int *h_ngood)
{
    MK_CTX(ctx);
    if (!d_x || !d_f || !d_g || !d_x_new || !d_f_new || !d_g_new || !(d_searching || d_mask) || !d_active || !d_Sh || !d_Yh || !d_rho || !d_hlen ||
        !d_hpos)
        return fail(MK_ERR_INVALID, "mk_lbfgs_update: null pointer");
    mk::LbfgsArgs a;
    memset(&a, 0, sizeof(a));
    a.R = R;
    a.n = (int)n;
    a.H = (int)history;
    a.keep_old = keep_old_gradient_if_searching;
    a.ftol = ftol;
    a.x = d_x;
    a.f = d_f;
    a.g = d_g;
    a.x_new = const_cast<double *>(d_x_new);
    a.f_new = const_cast<double *>(d_f_new);
    a.g_new = d_g_new;
    a.searching = const_cast<uint8_t *>(d_searching);
    a.mask = const_cast<uint8_t *>(d_mask);
    a.active = d_active;
    a.Sh = d_Sh;
    a.Yh = d_Yh;
    a.rho = d_rho;
    a.hlen = d_hlen;
    a.hpos = d_hpos;
    a.phase = d_phase;
    a.nit = d_nit;
    a.maxiter = (int)maxiter;
    return lbfgs_run(ctx, 3, a, 2, h_ngood);
}

MK_API int mk_alpha_grad(mk_context *ctx, int64_t B, int64_t R, int64_t N, int64_t K, const double *alpha,
                         const double *loadings, double dt, const double *gphi, const double *gq, double *galpha)
{
    MK_CTX(ctx);
    if (B <= 0 || R <= 0 || N <= 0 || K < 0 || !alpha || (K > 0 && !loadings) || !gphi || !gq || !galpha)
        return fail(MK_ERR_INVALID, "mk_alpha_grad: bad argument");
    MK_HIP(mk::launch_alpha_grad(B, R, (int)N, (int)K, alpha, loadings, dt, gphi, gq, galpha, ctx->stream));
    return MK_OK;
}

MK_API int mk_standardize(mk_context *ctx, int64_t R, int64_t T, int64_t N, int time_major, const double *in,
                          double *out, double *mean, double *stdev)
{
    MK_CTX(ctx);
    if (R <= 0 || T <= 0 || N <= 0 || N > 64 || !in) return fail(MK_ERR_INVALID, "mk_standardize: bad argument (1 <= N <= 64)");
    MK_HIP(mk::launch_standardize(R, T, (int)N, time_major, in, out, mean, stdev, ctx->stream));
    return MK_OK;
}

MK_API int mk_mask_observations(mk_context *ctx, int64_t count, const double *obs, const unsigned char *mask,
                                double *out)
{
    MK_CTX(ctx);
    if (count <= 0 || !obs || !mask || !out) return fail(MK_ERR_INVALID, "mk_mask_observations: bad argument");
    MK_HIP(mk::launch_mask(count, obs, mask, out, ctx->stream));
    return MK_OK;
}

MK_API int mk_pack_observations(mk_context *ctx, int64_t R, int64_t T, int64_t N, const double *obs,
                                double *observations, double *indices, int64_t *count)
{
    MK_CTX(ctx);
    if (R <= 0 || T <= 0 || N <= 0 || !obs) return fail(MK_ERR_INVALID, "mk_pack_observations: bad argument");
    static_assert(sizeof(long) == sizeof(int64_t), "LP64");
    MK_HIP(mk::launch_pack(R * T, (int)N, obs, observations, indices, reinterpret_cast<long *>(count), ctx->stream));
    return MK_OK;
}

MK_API int mk_fa_correlation(mk_context *ctx, int64_t R, int64_t T, int64_t N, int time_major, const double *obs,
                             double *corr)
{
    MK_CTX(ctx);
    if (R <= 0 || T <= 0 || N <= 0 || N > 64 || !obs || !corr)
        return fail(MK_ERR_INVALID, "mk_fa_correlation: bad argument (1 <= N <= 64)");
    MK_HIP(mk::launch_fa_corr(R, T, (int)N, time_major, obs, corr, ctx->stream));
    return MK_OK;
}

MK_API int mk_fa_analyse(mk_context *ctx, int64_t B, int64_t N, int64_t maxfactors, const double *corr, double *eigval,
                         int64_t *nfactors, int64_t *nfactors_map, int64_t *nfactors_map4, double *psi0, uint32_t *status)
{
    MK_CTX(ctx);
    if (B <= 0 || N < 2 || N > 64 || !corr) return fail(MK_ERR_INVALID, "mk_fa_analyse: bad argument (2 <= N <= 64)");
    MK_HIP(mk::launch_fa_analyse(B, (int)N, maxfactors, corr, eigval, (long long *)nfactors, (long long *)nfactors_map,
                                 (long long *)nfactors_map4, psi0, status, ctx->stream));
    return MK_OK;
}

MK_API int mk_fa_minres(mk_context *ctx, int64_t B, int64_t R, int64_t N, int64_t KMAX, const double *corr,
                        const int64_t *nfactors, const double *psi, const int64_t *order, double *fval, double *grad,
                        double *loadings)
{
    MK_CTX(ctx);
    if (B <= 0 || R <= 0 || R > B || N < 2 || N > 64 || KMAX < 1 || KMAX > N || !corr || !nfactors || !psi)
        return fail(MK_ERR_INVALID, "mk_fa_minres: bad argument (2 <= N <= 64, 1 <= KMAX <= N)");
    MK_HIP(mk::launch_fa_minres(B, R, (int)N, (int)KMAX, corr, (const long long *)nfactors, psi, (const long long *)order,
                                fval, grad, loadings, ctx->stream));
    return MK_OK;
}

MK_API int mk_fa_rotate(mk_context *ctx, int64_t B, int64_t N, int64_t KMAX, const int64_t *nfactors, double *loadings,
                        double gamma, int maxiter, double tol)
{
    MK_CTX(ctx);
    if (B <= 0 || N < 1 || N > 64 || KMAX < 1 || KMAX > N || !nfactors || !loadings)
        return fail(MK_ERR_INVALID, "mk_fa_rotate: bad argument");
    MK_HIP(mk::launch_fa_rotate(B, (int)N, (int)KMAX, (const long long *)nfactors, loadings, gamma, maxiter, tol, ctx->stream));
    return MK_OK;
}

MK_API int mk_fa_eigh(mk_context *ctx, int64_t B, int64_t N, const double *sym, double *val, double *vec)
{
    MK_CTX(ctx);
    if (B <= 0 || N < 1 || N > 64 || !sym || !val) return fail(MK_ERR_INVALID, "mk_fa_eigh: bad argument (1 <= N <= 64)");
    MK_HIP(mk::launch_fa_eigh(B, (int)N, sym, val, vec, ctx->stream));
    return MK_OK;
}

MK_API int mk_enable_timing(mk_context *ctx, int enable)
{
    MK_CTX(ctx);
    ctx->timing = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    ctx->have_filter_time = ctx->have_smooth_time = false;
    for (auto &v : ctx->ev_pending) { // pairs nobody asked for: back to the pool
        for (auto &pr : v) {
            ctx->ev_pool.push_back(pr.first);
            ctx->ev_pool.push_back(pr.second);
        }
        v.clear();
    }
    return MK_OK;
}

MK_API int mk_kernel_ms_totals(mk_context *ctx, double *filter_ms, int64_t *filter_launches, double *smoother_ms,
                               int64_t *smoother_launches)
{
    MK_CTX(ctx);
    double tot[2] = {0.0, 0.0};
    int64_t cnt[2] = {0, 0};
    for (int kind = 0; kind < 2; ++kind) {
        for (auto &pr : ctx->ev_pending[kind]) {
            float ms = 0.f;
            MK_HIP(hipEventSynchronize(pr.second));
            MK_HIP(hipEventElapsedTime(&ms, pr.first, pr.second));
            tot[kind] += ms;
            ++cnt[kind];
            ctx->ev_pool.push_back(pr.first);
            ctx->ev_pool.push_back(pr.second);
        }
        ctx->ev_pending[kind].clear();
    }
    if (filter_ms) *filter_ms = tot[0];
    if (filter_launches) *filter_launches = cnt[0];
    if (smoother_ms) *smoother_ms = tot[1];
    if (smoother_launches) *smoother_launches = cnt[1];
    return MK_OK;
}

MK_API int mk_last_kernel_ms(mk_context *ctx, float *filter_ms, float *smoother_ms)
{
    MK_CTX(ctx);
    if (filter_ms) {
        *filter_ms = -1.f;
        if (ctx->have_filter_time) {
            MK_HIP(hipEventSynchronize(ctx->ev[1]));
            MK_HIP(hipEventElapsedTime(filter_ms, ctx->ev[0], ctx->ev[1]));
        }
    }
    if (smoother_ms) {
        *smoother_ms = -1.f;
        if (ctx->have_smooth_time) {
            MK_HIP(hipEventSynchronize(ctx->ev[3]));
            MK_HIP(hipEventElapsedTime(smoother_ms, ctx->ev[2], ctx->ev[3]));
        }
    }
    return MK_OK;
}

} // extern "C"
