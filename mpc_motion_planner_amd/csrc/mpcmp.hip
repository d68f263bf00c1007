// mpcmp.hip — C-ABI entry points (include/mpcmp.h) of the MI355X-native batched min-time MPC solver.
// Host logic only orchestrates HIP launches; there is NO CPU fallback: without a HIP device every compute
// entry point fails with MPCMP_ENODEVICE.
// The kernels of the SQP chain and their launch code are solver.hip's (reached through solver.hpp), the entry points that touch no device are
// model_host.cpp's; this unit holds the context's life cycle, the argument checks and staging of every entry point, and the leaf kernels.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/mpcmp.h"
#include "context.hpp"
#include "solver.hpp"
#include "leaf_kernels.hpp"
#include "jerk_device.hpp"
#include "ik_device.hpp"
#include "payload.hpp"
#include "time_sync.hpp"
#include "clearance.hpp"
#include "moving.hpp"
#include "field.hpp"
#include "field_cert.hpp"
#include "frame.hpp"
#include "limits.hpp"
#include "retime.hpp"
#include "retimed_check.hpp"
#include "toolpath.hpp"
#include "route.hpp"

using namespace mpcmp;

// the three per-problem row tables of a context: where the count of rows in force lies, and the words of their messages
struct RowTable { int mpcmp_ctx::*rows; const char *what, *setter, *usage; bool refused_in_loop; };
static const RowTable PAYLOAD_ROWS = {&mpcmp_ctx::pay_rows, "payload", "mpcmp_set_payloads", "p given (or 0 with p NULL: clear)", false};
static const RowTable TIME_ROWS = {&mpcmp_ctx::tw_rows, "final-time", "mpcmp_set_time_windows", "lbT and ubT given (or 0 with both NULL: clear)", true};
static const RowTable BOUND_ROWS = {&mpcmp_ctx::bnd_rows, "bound", "mpcmp_set_bounds", "rows given (or 0 with NULL: clear)", true};
// a call for B problems needs a row for each of them (when rows are set)
static int rows_ok(mpcmp_ctx *ctx, int B, const RowTable &t) {
    const int rows = ctx->*t.rows;
    if (rows > 0 && B > rows) {
        ctx->err = "more problems (" + std::to_string(B) + ") than " + t.what + " rows (" + std::to_string(rows) + "): see " + t.setter;
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}
static int solve_rows_ok(mpcmp_ctx *ctx, int B) {
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    if (int rc = rows_ok(ctx, B, TIME_ROWS)) return rc;
    return rows_ok(ctx, B, BOUND_ROWS);
}
static int warm_all_or_none(mpcmp_ctx *ctx, const double *wx, const double *wu, const double *wT) {
    if ((wx != nullptr) != (wu != nullptr) || (wx != nullptr) != (wT != nullptr)) { ctx->err = "warm_x, warm_u, warm_T must be all given or all NULL"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// context
extern "C" const char *mpcmp_last_error(const mpcmp_ctx *ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

extern "C" int mpcmp_destroy(mpcmp_ctx *ctx) {
    if (!ctx) return MPCMP_OK;
    (void)hipSetDevice(ctx->device);
    if (ctx->rh_exec) (void)hipGraphExecDestroy(ctx->rh_exec);
    if (ctx->rh_graph) (void)hipGraphDestroy(ctx->rh_graph);
    for (void *p : ctx->allocs) (void)hipFree(p);
    for (auto &e : ctx->sol.ev) { (void)hipEventDestroy(e.e[0]); (void)hipEventDestroy(e.e[1]); }
    if (ctx->scratch) (void)hipFree(ctx->scratch);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    for (int k = 0; k < 3; k++) { if (ctx->stream_x[k]) (void)hipStreamDestroy(ctx->stream_x[k]); if (ctx->ev_join[k]) (void)hipEventDestroy(ctx->ev_join[k]); }
    if (ctx->ev_fork) (void)hipEventDestroy(ctx->ev_fork);
    for (auto &e : ctx->ev_upd) if (e) (void)hipEventDestroy(e);
    delete ctx;
    return MPCMP_OK;
}

static int create_impl(const mpcmp_config *cfg, const mpcmp_model *model, int narm, int device, int max_batch, mpcmp_ctx **out);

extern "C" int mpcmp_create(const mpcmp_config *cfg, const mpcmp_model *model, int device, int max_batch, mpcmp_ctx **out) {
    return create_impl(cfg, model, 1, device, max_batch, out);
}

// Multi-arm robot: `models` points at narm models (independent 7-joint chains on one base; a chain's base placement is folded
// into its first joint placement).  The OCP is the reference's (robot_ocp.hpp:31-213) with NX = 14 narm, NU = 7 narm,
// NG = 8 narm; the arms couple only through the final time.  BASELINE.json configs[3]: narm = 2, num_seg = 8.
extern "C" int mpcmp_create_multi(const mpcmp_config *cfg, const mpcmp_model *models, int narm, int device, int max_batch, mpcmp_ctx **out) {
    if (narm < 1 || narm > 2 || (narm > 1 && !models)) { g_err = "narm must be 1 or 2 (with narm models)"; return MPCMP_EINVAL; }
    return create_impl(cfg, models, narm, device, max_batch, out);
}

static int create_impl(const mpcmp_config *cfg, const mpcmp_model *model, int narm, int device, int max_batch, mpcmp_ctx **out) {
    if (!cfg || !out || max_batch < 1) return MPCMP_EINVAL;
    *out = nullptr;
    if (int rc = validate(cfg, g_err)) return rc;
    if (narm == 2) {
        if (cfg->num_seg != 6 && cfg->num_seg != 8) { g_err = "multi-arm OCPs need num_seg 6 or 8 (k_qp3)"; return MPCMP_EINVAL; }
        if (8 + cfg->qp_iters + 1 + 8 * (cfg->qp_iters / cfg->check_every + 1) > MPCMP_XCH_STRIDE) { g_err = "multi-arm OCPs: qp_iters too large for the exchange slots"; return MPCMP_EINVAL; }
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1 || device >= ndev) {
        g_err = "no HIP device available: the mpcmp product path has no CPU fallback";
        return MPCMP_ENODEVICE;
    }
    mpcmp_ctx *ctx = new mpcmp_ctx();
    ctx->cfg = *cfg; ctx->device = device; ctx->max_batch = max_batch; ctx->nseg = cfg->num_seg; ctx->narm = narm;
    ctx->nx = 14 * narm; ctx->nu = 7 * narm;
    const Dims d = dims_of(cfg->num_seg, narm);
    ctx->N = d.N; ctx->n = d.n; ctx->meq = d.meq; ctx->m = d.m; ctx->mn = d.mn;
    auto fail = [&](int rc) { g_err = ctx->err; mpcmp_destroy(ctx); return rc; };
#define TRY(x) do { int rc_ = (x); if (rc_) return fail(rc_); } while (0)
#define HIPTRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return fail(MPCMP_ERUNTIME); } } while (0)
    HIPTRY(hipSetDevice(device));
    HIPTRY(hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking));
    for (int k = 0; k < 3; k++) {
        HIPTRY(hipStreamCreateWithFlags(&ctx->stream_x[k], hipStreamNonBlocking));
        HIPTRY(hipEventCreateWithFlags(&ctx->ev_join[k], hipEventDisableTiming));
    }
    HIPTRY(hipEventCreateWithFlags(&ctx->ev_fork, hipEventDisableTiming));
    for (auto &e : ctx->ev_upd) HIPTRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    mpcmp_model mdl[2];
    for (int a = 0; a < narm; a++) { if (model) mdl[a] = model[a]; else mpcmp_default_model(&mdl[a]); }
    TRY(dalloc(ctx, &ctx->d_model, narm));
    HIPTRY(hipMemcpy(ctx->d_model, mdl, sizeof(mpcmp_model) * narm, hipMemcpyHostToDevice));
    ctx->model = mdl[0];
    TRY(solver_create(ctx));      // (environment knobs, structure and stream tables, factor workspace, LDS limits: solver.hip)
    const size_t B = max_batch, N = ctx->N, n = ctx->n, mn = ctx->mn;
    WS &w = ctx->ws;
    w.model = ctx->d_model;
    TRY(dalloc(ctx, &w.z, B * n)); TRY(dalloc(ctx, &w.lam, B * mn)); TRY(dalloc(ctx, &w.ceq, B * ctx->meq));
    HIPTRY(hipMemset(w.lam, 0, sizeof(double) * B * mn));        // (mpcmp_config.carry_multipliers: a fresh context starts every slot from lambda = 0)
    ctx->lam_count = B * mn;
    TRY(dalloc(ctx, &w.g, B * 8 * N * narm)); TRY(dalloc(ctx, &w.Gk, B * N * 176 * narm)); TRY(dalloc(ctx, &w.p, B * n));
    TRY(dalloc(ctx, &w.y, B * mn)); TRY(dalloc(ctx, &w.qpit, B)); TRY(dalloc(ctx, &w.perm, B)); TRY(dalloc(ctx, &w.okey, B)); TRY(dalloc(ctx, &w.done, 4));
    HIPTRY(hipMemset(w.done, 0, 4 * sizeof(int))); TRY(dalloc(ctx, &w.qp_total, B));
    TRY(dalloc(ctx, &w.status, B)); HIPTRY(hipMemset(w.status, 0, sizeof(*w.status) * B)); TRY(dalloc(ctx, &w.alpha, B)); TRY(dalloc(ctx, &w.dbg, (size_t)B * MPCMP_DBG_WORDS));
    const size_t nx = ctx->nx, nu = ctx->nu;
    TRY(dalloc(ctx, &ctx->d_x0, B * nx)); TRY(dalloc(ctx, &ctx->d_xf, B * nx));
    TRY(dalloc(ctx, &ctx->d_wx, B * nx * N)); TRY(dalloc(ctx, &ctx->d_wu, B * nu * N)); TRY(dalloc(ctx, &ctx->d_wT, B));
    TRY(dalloc(ctx, &ctx->d_sx, B * nx * N)); TRY(dalloc(ctx, &ctx->d_su, B * nu * N)); TRY(dalloc(ctx, &ctx->d_sT, B));
    TRY(dalloc(ctx, &ctx->d_info, B));
    if (narm == 2) {
        TRY(dalloc(ctx, &ctx->xch.buf, B * 2 * MPCMP_XCH_STRIDE));
        // per-arm staging of the warm-start generator: states, node trajectories, durations of B * narm arm problems
        TRY(dalloc(ctx, &ctx->d_ax0, B * nx)); TRY(dalloc(ctx, &ctx->d_axf, B * nx));
        TRY(dalloc(ctx, &ctx->d_awx, B * nx * N)); TRY(dalloc(ctx, &ctx->d_awu, B * nu * N)); TRY(dalloc(ctx, &ctx->d_awT, B * narm));
    }
    TRY(dalloc(ctx, &ctx->d_retired, B)); HIPTRY(hipMemset(ctx->d_retired, 0, sizeof(int) * B));
    TRY(dalloc(ctx, &ctx->d_rh_count, 2)); HIPTRY(hipMemset(ctx->d_rh_count, 0, 2 * sizeof(unsigned long long)));
    TRY(dalloc(ctx, &ctx->d_clr_sph, 2 * CLR_MAX_SPH));
#undef TRY
#undef HIPTRY
    *out = ctx;
    return MPCMP_OK;
}

// a captured receding-horizon step holds what it was captured with as kernel arguments (the configuration by value, the model pointer and stride):
// whoever changes one of them drops the graph, and the next mpcmp_rh_run with use_graph captures again
static void drop_rh_graph(mpcmp_ctx *ctx) {
    if (ctx->rh_exec) { (void)hipGraphExecDestroy(ctx->rh_exec); ctx->rh_exec = nullptr; }
    if (ctx->rh_graph) { (void)hipGraphDestroy(ctx->rh_graph); ctx->rh_graph = nullptr; }
}

extern "C" int mpcmp_set_config(mpcmp_ctx *ctx, const mpcmp_config *cfg) {
    if (!ctx || !cfg) return MPCMP_EINVAL;
    if (cfg->num_seg != ctx->nseg) { ctx->err = "num_seg cannot change after mpcmp_create"; return MPCMP_EINVAL; }
    if (int rc = validate(cfg, ctx->err)) return rc;
    if (ctx->narm == 2 && 8 + cfg->qp_iters + 1 + 8 * (cfg->qp_iters / cfg->check_every + 1) > MPCMP_XCH_STRIDE) {
        ctx->err = "multi-arm OCPs: qp_iters too large for the exchange slots"; return MPCMP_EINVAL;
    }
    ctx->cfg = *cfg;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// what the *_device setters and mpcmp_rh_update_device share: body(ctx->stream) runs after the caller's work on its stream (which writes the inputs) and
// the context's own (solves that read what body replaces), before the context's later work; the caller's later work waits for body's reads of its buffers
template <typename F>
static int with_caller_stream(mpcmp_ctx *ctx, void *hip_stream, F body) {
    hipStream_t cs = (hipStream_t)hip_stream;
    HIPCHK(ctx, hipEventRecord(ctx->ev_upd[0], cs));
    HIPCHK(ctx, hipStreamWaitEvent(ctx->stream, ctx->ev_upd[0], 0));
    if (int rc = body(ctx->stream)) return rc;
    HIPCHK(ctx, hipEventRecord(ctx->ev_upd[1], ctx->stream));
    HIPCHK(ctx, hipStreamWaitEvent(cs, ctx->ev_upd[1], 0));
    return MPCMP_OK;
}

// the front half of the checks of the three row setters (host and device variant alike).  given / none: every row pointer of the call is set / is NULL
static int rows_check(mpcmp_ctx *ctx, const RowTable &t, int n, bool given, bool none) {
    if (!ctx) { g_err = std::string(t.setter) + ": no context"; return MPCMP_EINVAL; }
    if (t.refused_in_loop && ctx->rh_B > 0) {
        ctx->err = std::string(t.setter) + ": the receding-horizon driver does not read " + t.what + " rows (a loop is running)"; return MPCMP_EINVAL;
    }
    if (n == 0 && none) return MPCMP_OK;
    if (n < 1 || n > ctx->max_batch || !given) { ctx->err = std::string(t.setter) + ": n must be in [1, max_batch] with " + t.usage; return MPCMP_EINVAL; }
    return MPCMP_OK;
}
// first use of a row table: [max_batch] rows of `per_row` entries
template <typename T>
static int rows_alloc(mpcmp_ctx *ctx, T **p, size_t per_row) {
    if (*p) return MPCMP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return dalloc(ctx, p, per_row * ctx->max_batch);
}

// n rows of narm payloads at d_p (device) -> ctx->d_pmodel on stream st; the scalar checks are the caller's
static int payloads_enqueue(mpcmp_ctx *ctx, int n, const mpcmp_payload *d_p, hipStream_t st) {
    const int threads = n * ctx->narm;
    hipLaunchKernelGGL(k_lump_payloads, dim3((threads + 255) / 256), dim3(256), 0, st, (const mpcmp_model *)ctx->d_model, ctx->narm, n, d_p, ctx->d_pmodel);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

// (payload rows may change while a receding-horizon loop runs, as long as every instance keeps one; the setters then drop the captured step)
static int payloads_check(mpcmp_ctx *ctx, int n, const mpcmp_payload *p) {
    if (int rc = rows_check(ctx, PAYLOAD_ROWS, n, p != nullptr, !p)) return rc;
    if (n == 0) return MPCMP_OK;
    if (ctx->rh_B > 0 && n < ctx->rh_B) { ctx->err = "mpcmp_set_payloads: fewer rows than the instances of the receding-horizon loop"; return MPCMP_EINVAL; }
    if (int rc = rows_alloc(ctx, &ctx->d_pmodel, ctx->narm)) return rc;      // (1,472 + 104 B per arm)
    return rows_alloc(ctx, &ctx->d_pay, ctx->narm);
}

extern "C" int mpcmp_set_payloads(mpcmp_ctx *ctx, int n, const mpcmp_payload *p) {
    if (int rc = payloads_check(ctx, n, p)) return rc;
    if (n > 0)
        for (int i = 0; i < n * ctx->narm; i++)
            if (int rc = check_payload(p + i, ctx->err)) { ctx->err = "mpcmp_set_payloads: row " + std::to_string(i / ctx->narm) + ": " + ctx->err; return rc; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (n > 0) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_pay, p, sizeof(mpcmp_payload) * n * ctx->narm, hipMemcpyHostToDevice, st));
        if (int rc = payloads_enqueue(ctx, n, ctx->d_pay, st)) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->pay_rows = n;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

extern "C" int mpcmp_set_payloads_device(mpcmp_ctx *ctx, int n, const mpcmp_payload *d_p, void *hip_stream) {
    if (int rc = payloads_check(ctx, n, d_p)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n > 0)
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) { return payloads_enqueue(ctx, n, d_p, st); })) return rc;
    ctx->pay_rows = n;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// per-problem final-time windows
static int time_windows_check(mpcmp_ctx *ctx, int n, const double *lb, const double *ub) {
    if (int rc = rows_check(ctx, TIME_ROWS, n, lb && ub, !lb && !ub)) return rc;
    return n > 0 ? rows_alloc(ctx, &ctx->d_tbox, 2) : MPCMP_OK;
}

extern "C" int mpcmp_set_time_windows(mpcmp_ctx *ctx, int n, const double *lbT, const double *ubT) {
    if (int rc = time_windows_check(ctx, n, lbT, ubT)) return rc;
    std::vector<double> rows((size_t)2 * n);
    for (int i = 0; i < n; i++) {
        // the rule validate() applies to the configuration's pair (no NaN, lb <= ub, not empty), and lbT >= 0
        if (!(lbT[i] <= ubT[i] && lbT[i] < INFINITY && ubT[i] > -INFINITY && lbT[i] >= 0.0)) {
            ctx->err = "mpcmp_set_time_windows: row " + std::to_string(i) + ": 0 <= lbT <= ubT required (no NaN, no empty window)";
            return MPCMP_EINVAL;
        }
        rows[2 * i] = lbT[i]; rows[2 * i + 1] = ubT[i];
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n > 0) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_tbox, rows.data(), sizeof(double) * 2 * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->tw_rows = n;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_time_windows_device(mpcmp_ctx *ctx, int n, const double *d_lbT, const double *d_ubT, void *hip_stream) {
    if (int rc = time_windows_check(ctx, n, d_lbT, d_ubT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n > 0)
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
                HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_tbox, 2 * sizeof(double), d_lbT, sizeof(double), sizeof(double), n, hipMemcpyDeviceToDevice, st));
                HIPCHK(ctx, hipMemcpy2DAsync(ctx->d_tbox + 1, 2 * sizeof(double), d_ubT, sizeof(double), sizeof(double), n, hipMemcpyDeviceToDevice, st));
                return MPCMP_OK;
            })) return rc;
    ctx->tw_rows = n;
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// per-problem bounds
static int bounds_check(mpcmp_ctx *ctx, int n, const mpcmp_bounds *rows) {
    if (int rc = rows_check(ctx, BOUND_ROWS, n, rows != nullptr, !rows)) return rc;
    return n > 0 ? rows_alloc(ctx, &ctx->d_bnd, 1) : MPCMP_OK;
}

extern "C" int mpcmp_set_bounds(mpcmp_ctx *ctx, int n, const mpcmp_bounds *rows) {
    if (int rc = bounds_check(ctx, n, rows)) return rc;
    for (int i = 0; i < n; i++) {
        std::string why;
        if (validate_boxes(rows + i, why) || validate_general_rows(rows + i, ctx->nseg, why)) { ctx->err = "mpcmp_set_bounds: row " + std::to_string(i) + ": " + why; return MPCMP_EINVAL; }
    }
    if (n > 0) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_bnd, rows, sizeof(mpcmp_bounds) * n, hipMemcpyHostToDevice, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    ctx->bnd_rows = n;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_bounds_device(mpcmp_ctx *ctx, int n, const mpcmp_bounds *d_rows, void *hip_stream) {
    if (int rc = bounds_check(ctx, n, d_rows)) return rc;
    if (n > 0) {
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
                HIPCHK(ctx, hipMemcpyAsync(ctx->d_bnd, d_rows, sizeof(mpcmp_bounds) * n, hipMemcpyDeviceToDevice, st));
                return MPCMP_OK;
            })) return rc;
    }
    ctx->bnd_rows = n;
    return MPCMP_OK;
}

// the solve of a checked call (the kernels and their launch code: solver.hip)
static int solve_dispatch(mpcmp_ctx *ctx, const SolveCall &c) {
    if (!ctx) return MPCMP_EINVAL;
    if (c.B < 1) return MPCMP_EINVAL;
    if (c.B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (int rc = c.rh_step ? rows_ok(ctx, c.B, PAYLOAD_ROWS) : solve_rows_ok(ctx, c.B)) return rc;
    if (!c.x0 || !c.xf) return MPCMP_EINVAL;
    if (int rc = warm_all_or_none(ctx, c.wx, c.wu, c.wT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (ctx->narm == 2) {
        if (c.only_qp) { ctx->err = "mpcmp_qp_batch is defined for single-arm contexts only"; return MPCMP_EINVAL; }
        if (!c.wx) { ctx->err = "multi-arm solves need a warm start (mpcmp_warm_start_jerk_batch)"; return MPCMP_EINVAL; }
    }
    return solver_run(ctx, c);
}

// ---- the host-buffer entry points' staging: the context's d_x0 / d_xf / d_w* in, d_s* / d_info (or another triple) out ----
static int upload_problems(mpcmp_ctx *ctx, size_t B, const double *x0, const double *xf, const double *wx, const double *wu, const double *wT, hipStream_t st) {
    const size_t N = ctx->N, nx = ctx->nx, nu = ctx->nu;
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_x0, x0, sizeof(double) * nx * B, hipMemcpyHostToDevice, st));
    HIPCHK(ctx, hipMemcpyAsync(ctx->d_xf, xf, sizeof(double) * nx * B, hipMemcpyHostToDevice, st));
    if (wx) {
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_wx, wx, sizeof(double) * nx * N * B, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_wu, wu, sizeof(double) * nu * N * B, hipMemcpyHostToDevice, st));
        HIPCHK(ctx, hipMemcpyAsync(ctx->d_wT, wT, sizeof(double) * B, hipMemcpyHostToDevice, st));
    }
    return MPCMP_OK;
}
// (every host pointer may be NULL: not wanted)
static int download_trajectories(mpcmp_ctx *ctx, size_t B, const double *d_x, const double *d_u, const double *d_T, double *x, double *u, double *T,
                                 mpcmp_info *info, hipStream_t st) {
    const size_t N = ctx->N, nx = ctx->nx, nu = ctx->nu;
    if (x) HIPCHK(ctx, hipMemcpyAsync(x, d_x, sizeof(double) * nx * N * B, hipMemcpyDeviceToHost, st));
    if (u) HIPCHK(ctx, hipMemcpyAsync(u, d_u, sizeof(double) * nu * N * B, hipMemcpyDeviceToHost, st));
    if (T) HIPCHK(ctx, hipMemcpyAsync(T, d_T, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    if (info) HIPCHK(ctx, hipMemcpyAsync(info, ctx->d_info, sizeof(mpcmp_info) * B, hipMemcpyDeviceToHost, st));
    return MPCMP_OK;
}
// the solve of the staged problems into the staged outputs; warm: with the staged start guess
static SolveCall staged_call(const mpcmp_ctx *ctx, int B, bool warm, hipStream_t st) {
    SolveCall c;
    c.B = B; c.x0 = ctx->d_x0; c.xf = ctx->d_xf;
    if (warm) { c.wx = ctx->d_wx; c.wu = ctx->d_wu; c.wT = ctx->d_wT; }
    c.sx = ctx->d_sx; c.su = ctx->d_su; c.sT = ctx->d_sT; c.info = ctx->d_info; c.stream = st;
    return c;
}

extern "C" int mpcmp_solve_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf,
                                        const double *d_wx, const double *d_wu, const double *d_wT, double *d_sx,
                                        double *d_su, double *d_sT, mpcmp_info *d_info, void *hip_stream) {
    if (!d_sx || !d_su || !d_sT) return MPCMP_EINVAL;
    return solve_dispatch(ctx, SolveCall{B, d_x0, d_xf, d_wx, d_wu, d_wT, d_sx, d_su, d_sT, d_info, (hipStream_t)hip_stream});
}

extern "C" int mpcmp_solve_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *wx,
                                 const double *wu, const double *wT, double *sx, double *su, double *sT, mpcmp_info *info) {
    if (!ctx || !x0 || !xf || !sx || !su || !sT) return MPCMP_EINVAL;
    if (B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (int rc = solve_rows_ok(ctx, B)) return rc;
    if (int rc = warm_all_or_none(ctx, wx, wu, wT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = upload_problems(ctx, B, x0, xf, wx, wu, wT, st)) return rc;
    if (int rc = solve_dispatch(ctx, staged_call(ctx, B, wx != nullptr, st))) return rc;
    if (int rc = download_trajectories(ctx, B, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

#define SINGLE_ARM_ONLY(ctx) do { if ((ctx)->narm != 1) { (ctx)->err = "this entry point is defined for single-arm contexts only"; return MPCMP_EINVAL; } } while (0)

extern "C" int mpcmp_warm_start_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, double *wx, double *wu, double *wT) {
    if (!ctx || !x0 || !xf || !wx || !wu || !wT || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    if (int rc = rows_ok(ctx, B, TIME_ROWS)) return rc;
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t N = ctx->N, n = ctx->n;
    hipStream_t st = ctx->stream;
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = solver_init_guess(ctx, B, st)) return rc;      // k_init alone: the built-in initialiser writes the iterate z = [xs|us|T]
    std::vector<double> z((size_t)B * n);
    HIPCHK(ctx, hipMemcpyAsync(z.data(), ctx->ws.z, sizeof(double) * n * B, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    for (int b = 0; b < B; b++) {
        std::memcpy(wx + (size_t)b * 14 * N, z.data() + (size_t)b * n, sizeof(double) * 14 * N);
        std::memcpy(wu + (size_t)b * 7 * N, z.data() + (size_t)b * n + 14 * N, sizeof(double) * 7 * N);
        wT[b] = z[(size_t)b * n + 21 * N];
    }
    return MPCMP_OK;
}

// Device staging of the host-pointer entry points, in the context's scratch: owned by the context and only ever grown, so that after the first call
// of a given size these entry points do not allocate (a control loop calls get_MPC_point / get_RK_point every tick).
// An entry point DECLARES every device array it needs, each with the variable that will hold its device pointer, an element count and what happens to
// it: in() is copied from a host pointer by upload(), out() is copied to one by finish(), inout() both.  upload() adds up the aligned sizes, grows the
// scratch at most once and only then fills the variables in, so no pointer exists that a growth could leave dangling.  A NULL host pointer is an array
// the caller did not give: its device pointer stays NULL, and nothing is reserved or copied for it.
struct Stage {
    explicit Stage(mpcmp_ctx *c) : ctx(c) {}
    template <typename T> void in(T **dev, const T *host, size_t count) { *dev = nullptr; add(dev, host, nullptr, count * sizeof(T)); }
    template <typename T> void out(T **dev, T *host, size_t count) { *dev = nullptr; add(dev, nullptr, host, count * sizeof(T)); }
    template <typename T> void inout(T **dev, T *host, size_t count) { *dev = nullptr; add(dev, host, host, count * sizeof(T)); }
    // after the last declaration, before the launch: the scratch, the device pointers, and every input copy on ctx->stream
    int upload() {
        size_t total = 0;
        for (int i = 0; i < n; i++) total += aligned(items[i].bytes);
        if (total > ctx->scratch_bytes) {
            if (ctx->scratch) { (void)hipStreamSynchronize(ctx->stream); (void)hipFree(ctx->scratch); ctx->scratch = nullptr; ctx->scratch_bytes = 0; }
            const size_t want = total < (1u << 20) ? (1u << 20) : total;
            if (hipMalloc(&ctx->scratch, want) != hipSuccess) { ctx->scratch = nullptr; ctx->err = "device scratch allocation failed"; return MPCMP_ERUNTIME; }
            ctx->scratch_bytes = want;
        }
        char *p = static_cast<char *>(ctx->scratch);
        for (int i = 0; i < n; i++) {
            items[i].dev = p;
            std::memcpy(items[i].var, &p, sizeof p);      // (the variables are pointers of several types: no cast of one to the other's address)
            p += aligned(items[i].bytes);
        }
        for (int i = 0; i < n; i++)
            if (items[i].src) HIPCHK(ctx, hipMemcpyAsync(items[i].dev, items[i].src, items[i].bytes, hipMemcpyHostToDevice, ctx->stream));
        return MPCMP_OK;
    }
    // after the launch: every output copy on ctx->stream, and the wait for it
    int finish() {
        for (int i = 0; i < n; i++)
            if (items[i].dst) HIPCHK(ctx, hipMemcpyAsync(items[i].dst, items[i].dev, items[i].bytes, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        return MPCMP_OK;
    }

private:
    struct Item { void *var, *dev; const void *src; void *dst; size_t bytes; };
    static constexpr int MAX_ITEMS = 12;
    static size_t aligned(size_t bytes) { return (bytes + 255) / 256 * 256; }
    void add(void *var, const void *src, void *dst, size_t bytes) {
        if (!src && !dst) return;
        assert(n < MAX_ITEMS);
        items[n++] = {var, nullptr, src, dst, bytes};
    }
    mpcmp_ctx *ctx;
    Item items[MAX_ITEMS];
    int n = 0;
};

// ---- time scaling and the time-synchronised solve (time_sync.hpp) ----
static int time_scale_enqueue(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_sx, const double *d_su, const double *d_sT,
                              const double *d_Tn, const int *d_skip, double *d_ox, double *d_ou, double *d_oT, hipStream_t st) {
    hipLaunchKernelGGL(k_time_scale, dim3(B), dim3(256), 0, st, ctx->N, ctx->narm, d_x0, d_xf, d_sx, d_su, d_sT, d_Tn, d_skip, d_ox, d_ou, d_oT);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_time_scale_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_sx, const double *d_su,
                                             const double *d_sT, const double *d_Tn, double *d_ox, double *d_ou, double *d_oT, void *hip_stream) {
    if (!ctx || B < 1 || !d_x0 || !d_xf || !d_sx || !d_su || !d_sT || !d_Tn || !d_ox || !d_ou || !d_oT) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return time_scale_enqueue(ctx, B, d_x0, d_xf, d_sx, d_su, d_sT, d_Tn, nullptr, d_ox, d_ou, d_oT, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_time_scale_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *sx, const double *su, const double *sT,
                                      const double *Tn, double *ox, double *ou, double *oT) {
    if (!ctx || B < 1 || !x0 || !xf || !sx || !su || !sT || !Tn || !ox || !ou || !oT) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, nx = ctx->nx * nb, nxN = nx * ctx->N, nuN = ctx->nu * nb * ctx->N;
    Stage sg(ctx);
    double *d0, *d1, *dx, *du, *dT, *dn, *qx, *qu, *qT;
    sg.in(&d0, x0, nx); sg.in(&d1, xf, nx); sg.in(&dx, sx, nxN); sg.in(&du, su, nuN); sg.in(&dT, sT, nb); sg.in(&dn, Tn, nb);
    sg.out(&qx, ox, nxN); sg.out(&qu, ou, nuN); sg.out(&qT, oT, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = time_scale_enqueue(ctx, B, d0, d1, dx, du, dT, dn, nullptr, qx, qu, qT, ctx->stream)) return rc;
    return sg.finish();
}

static int synced_check(mpcmp_ctx *ctx, int B, int n_groups, const double *wx, const double *wu, const double *wT) {
    if (B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (n_groups < 0 || n_groups > ctx->max_batch) { ctx->err = "mpcmp_solve_batch_synced: n_groups must be in [0, max_batch]"; return MPCMP_EINVAL; }
    if (int rc = warm_all_or_none(ctx, wx, wu, wT)) return rc;
    if (int rc = solve_rows_ok(ctx, B)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_sg_count) {            // first use
        const size_t M = ctx->max_batch, N = ctx->N;
        if (int rc = dalloc(ctx, &ctx->d_sg_count, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_skip, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_status, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_key, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_T, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_rows, 2 * M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_Tn, M)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_wx, M * ctx->nx * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_wu, M * ctx->nu * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_sg_wT, M)) return rc;
    }
    return MPCMP_OK;
}

// pass 1 (the call as given), the group times, the pass-2 mask / rows / start guess, pass 2: all on the call's stream, no host round trip
static int synced_enqueue(mpcmp_ctx *ctx, const SolveCall &pass1, const int *d_group, int n_groups, double *d_gT) {
    const int B = pass1.B;
    hipStream_t st = pass1.stream;
    if (int rc = solve_dispatch(ctx, pass1)) return rc;
    const int G = n_groups > 0 ? n_groups : 1;
    HIPCHK(ctx, hipMemsetAsync(ctx->d_sg_key, 0, sizeof(unsigned long long) * G, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_sg_count, 0, sizeof(int) * G, st));
    hipLaunchKernelGGL(k_sync_tmax, dim3((B + 255) / 256), dim3(256), 0, st, B, d_group, n_groups, (const int *)ctx->ws.status, (const double *)pass1.sT,
                       ctx->d_sg_key, ctx->d_sg_count);
    const int np = B > n_groups ? B : n_groups;
    hipLaunchKernelGGL(k_sync_prepare, dim3((np + 255) / 256), dim3(256), 0, st, B, d_group, n_groups, (const int *)ctx->ws.status, (const double *)pass1.sT,
                       (const unsigned long long *)ctx->d_sg_key, (const int *)ctx->d_sg_count, d_gT, ctx->d_sg_skip, ctx->d_sg_rows, ctx->d_sg_Tn,
                       ctx->d_sg_status);
    HIPCHK(ctx, hipGetLastError());
    if (int rc = time_scale_enqueue(ctx, B, pass1.x0, pass1.xf, pass1.sx, pass1.su, pass1.sT, ctx->d_sg_Tn, ctx->d_sg_skip, ctx->d_sg_wx, ctx->d_sg_wu, ctx->d_sg_wT, st))
        return rc;
    // pass 2: every slot is launched; the ones not re-solved return at once (WS::retired) and keep their pass-1 outputs
    SolveCall pass2 = pass1;
    pass2.wx = ctx->d_sg_wx; pass2.wu = ctx->d_sg_wu; pass2.wT = ctx->d_sg_wT;
    pass2.tw_rows = ctx->d_sg_rows; pass2.skip = ctx->d_sg_skip;
    if (int rc = solve_dispatch(ctx, pass2)) return rc;
    // (at N = 25 the skipped slots' QP kernels ran in pass 2 and added to their status words: the next solve sees pass 1's, as after a plain solve)
    hipLaunchKernelGGL(k_sync_restore, dim3((B + 255) / 256), dim3(256), 0, st, B, (const int *)ctx->d_sg_skip, (const int *)ctx->d_sg_status,
                       ctx->ws.status);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_solve_batch_synced_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_wx, const double *d_wu,
                                               const double *d_wT, const int *d_group, int n_groups, double *d_sx, double *d_su, double *d_sT,
                                               mpcmp_info *d_info, double *d_group_T, void *hip_stream) {
    if (!ctx || !d_x0 || !d_xf || !d_group || !d_sx || !d_su || !d_sT) return MPCMP_EINVAL;
    if (int rc = synced_check(ctx, B, n_groups, d_wx, d_wu, d_wT)) return rc;
    return synced_enqueue(ctx, SolveCall{B, d_x0, d_xf, d_wx, d_wu, d_wT, d_sx, d_su, d_sT, d_info, (hipStream_t)hip_stream}, d_group, n_groups,
                          d_group_T ? d_group_T : ctx->d_sg_T);
}

extern "C" int mpcmp_solve_batch_synced(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *wx, const double *wu, const double *wT,
                                        const int *group, int n_groups, double *sx, double *su, double *sT, mpcmp_info *info, double *group_T) {
    if (!ctx || !x0 || !xf || !group || !sx || !su || !sT) return MPCMP_EINVAL;
    if (int rc = synced_check(ctx, B, n_groups, wx, wu, wT)) return rc;
    for (int i = 0; i < B; i++)
        if (group[i] < -1 || group[i] >= n_groups) {
            ctx->err = "mpcmp_solve_batch_synced: group[" + std::to_string(i) + "] must be -1 or in [0, n_groups)"; return MPCMP_EINVAL;
        }
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    int *dg;
    sg.in(&dg, group, B);
    if (int rc = upload_problems(ctx, B, x0, xf, wx, wu, wT, st)) return rc;
    if (int rc = sg.upload()) return rc;
    if (int rc = synced_enqueue(ctx, staged_call(ctx, B, wx != nullptr, st), dg, n_groups, ctx->d_sg_T)) return rc;
    if (int rc = download_trajectories(ctx, B, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    if (group_T && n_groups > 0) HIPCHK(ctx, hipMemcpyAsync(group_T, ctx->d_sg_T, sizeof(double) * n_groups, hipMemcpyDeviceToHost, st));
    return sg.finish();
}

// ---- jerk-limited, time-synchronised warm start / comparison trajectory (stands in for Ruckig) ----
// vmax / amax: NULL = the context's margin-applied bounds (the *_lim_* entry points pass a caller's own: ruckig::InputParameter::max_velocity / max_acceleration)
static int jerk_limits(mpcmp_ctx *ctx, const double *vmax, const double *amax, const double *jmax, JerkLimits &lim) {
    for (int j = 0; j < 7; j++) {
        lim.v[j] = vmax ? vmax[j] : ctx->cfg.ubx[7 + j]; lim.a[j] = amax ? amax[j] : ctx->cfg.ubu[j]; lim.j[j] = jmax[j];
        if (!(lim.v[j] > 0.0) || !(lim.a[j] > 0.0) || !(lim.j[j] > 0.0)) { ctx->err = "velocity, acceleration and jerk limits must be positive"; return MPCMP_EINVAL; }
    }
    return MPCMP_OK;
}

// boundary accelerations d_acc0 / d_accT: device [B][7], either may be NULL (= zero); single-arm contexts only (a multi-arm warm start has none)
static int warm_start_jerk_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_acc0, const double *d_accT,
                                  const double *vmax, const double *amax, const double *jmax, double *d_wx, double *d_wu, double *d_wT, void *hip_stream,
                                  const int *need_status = nullptr, int need_mask = 0) {
    if (!ctx || !d_x0 || !d_xf || !jmax || !d_wx || !d_wu || !d_wT || B < 1) return MPCMP_EINVAL;
    if ((d_acc0 || d_accT) && ctx->narm != 1) { ctx->err = "boundary accelerations: single-arm contexts only"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    JerkLimits lim;
    if (int rc = jerk_limits(ctx, vmax, amax, jmax, lim)) return rc;
    if (ctx->narm == 2) {
        // per-arm generator on B * narm arm problems, then the merge to the common (slowest arm's) duration: jerk_device.hpp
        if (B > ctx->max_batch) return MPCMP_ETOOBIG;
        hipStream_t s2 = (hipStream_t)hip_stream;
        const int cnt = B * 2 * 14;
        hipLaunchKernelGGL((k_split_states<2>), dim3((cnt + 255) / 256), dim3(256), 0, s2, B, d_x0, ctx->d_ax0);
        hipLaunchKernelGGL((k_split_states<2>), dim3((cnt + 255) / 256), dim3(256), 0, s2, B, d_xf, ctx->d_axf);
        hipLaunchKernelGGL(k_warm_jerk, dim3(B * 2), dim3(64), 0, s2, ctx->nseg, lim, ctx->d_ax0, ctx->d_axf, (const double *)nullptr, (const double *)nullptr, ctx->d_awx, ctx->d_awu, ctx->d_awT,
                           need_status, need_mask, 2);
        hipLaunchKernelGGL((k_warm_merge<2>), dim3(B), dim3(256), 0, s2, ctx->N, B, ctx->d_awx, ctx->d_awu, ctx->d_awT, d_x0, d_xf, d_wx, d_wu, d_wT);
        HIPCHK(ctx, hipGetLastError());
        return MPCMP_OK;
    }
    // the stream exactly as given (NULL = the legacy default stream), like the other *_device entry points: the solve that
    // consumes the warm start is enqueued on the same stream and is ordered behind this launch
    hipLaunchKernelGGL(k_warm_jerk, dim3(B), dim3(64), 0, (hipStream_t)hip_stream, ctx->nseg, lim, d_x0, d_xf, d_acc0, d_accT, d_wx, d_wu, d_wT, need_status, need_mask, 1);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}
extern "C" int mpcmp_warm_start_jerk_acc_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *d_acc0, const double *d_accT,
                                                      const double *jmax, double *d_wx, double *d_wu, double *d_wT, void *hip_stream) {
    return warm_start_jerk_device(ctx, B, d_x0, d_xf, d_acc0, d_accT, nullptr, nullptr, jmax, d_wx, d_wu, d_wT, hip_stream);
}
extern "C" int mpcmp_warm_start_jerk_batch_device(mpcmp_ctx *ctx, int B, const double *d_x0, const double *d_xf, const double *jmax,
                                                  double *d_wx, double *d_wu, double *d_wT, void *hip_stream) {
    return mpcmp_warm_start_jerk_acc_batch_device(ctx, B, d_x0, d_xf, nullptr, nullptr, jmax, d_wx, d_wu, d_wT, hip_stream);
}

// Boundary states the generator cannot honour: the acceleration limit yields to a boundary acceleration above it (include/mpcmp.h), but an
// acceleration that cannot be brought to zero inside the VELOCITY limit — |v0 + a0 |a0| / 2J| > V at the start, |vT - aT |aT| / 2J| > V at the target —
// would overshoot the state box of the OCP: MPCMP_EINVAL, as Ruckig rejects such an input (ErrorInvalidInput; the shim's otg.calculate returns it).
// Host-pointer entry points only: the *_device variants never read their inputs on the host.
static int check_boundary_acc(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                              const double *vmax, const double *jmax) {
    if ((!acc0 && !accT) || ctx->narm != 1) return MPCMP_OK;
    for (int b = 0; b < B; b++)
        for (int j = 0; j < 7; j++) {
            const double V = (vmax ? vmax[j] : ctx->cfg.ubx[7 + j]) * (1.0 + 1e-9), J = jmax[j];
            if (!(J > 0.0)) continue;      // (reported by jerk_limits)
            const double a0 = acc0 ? acc0[7 * b + j] : 0.0, aT = accT ? accT[7 * b + j] : 0.0;
            const double v0 = x0[14 * b + 7 + j], vT = xf[14 * b + 7 + j];
            const double va = v0 + a0 * std::fabs(a0) / (2.0 * J), vb = vT - aT * std::fabs(aT) / (2.0 * J);
            // (a boundary VELOCITY outside the limit is the caller's business, as before: that joint falls back to the quintic of the common duration)
            if ((std::fabs(v0) <= V && std::fabs(va) > V) || (std::fabs(vT) <= V && std::fabs(vb) > V)) {
                std::ostringstream os;
                os << "problem " << b << ", joint " << j << ": the boundary acceleration cannot be brought to zero inside the velocity limit";
                ctx->err = os.str();
                return MPCMP_EINVAL;
            }
        }
    return MPCMP_OK;
}

extern "C" int mpcmp_warm_start_jerk_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *vmax, const double *amax, const double *jmax, double *wx, double *wu, double *wT) {
    if (!ctx || !x0 || !xf || !jmax || !wx || !wu || !wT || B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = check_boundary_acc(ctx, B, x0, xf, acc0, accT, vmax, jmax)) return rc;
    if ((acc0 || accT) && ctx->narm != 1) { ctx->err = "boundary accelerations: single-arm contexts only"; return MPCMP_EINVAL; }
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *da0, *daT;
    sg.in(&da0, acc0, 7 * (size_t)B); sg.in(&daT, accT, 7 * (size_t)B);
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = sg.upload()) return rc;
    if (int rc = warm_start_jerk_device(ctx, B, ctx->d_x0, ctx->d_xf, da0, daT, vmax, amax, jmax, ctx->d_wx, ctx->d_wu, ctx->d_wT, st)) return rc;
    if (int rc = download_trajectories(ctx, B, ctx->d_wx, ctx->d_wu, ctx->d_wT, wx, wu, wT, nullptr, st)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_warm_start_jerk_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *jmax, double *wx, double *wu, double *wT) {
    return mpcmp_warm_start_jerk_lim_batch(ctx, B, x0, xf, acc0, accT, nullptr, nullptr, jmax, wx, wu, wT);
}
extern "C" int mpcmp_warm_start_jerk_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax,
                                           double *wx, double *wu, double *wT) {
    return mpcmp_warm_start_jerk_acc_batch(ctx, B, x0, xf, nullptr, nullptr, jmax, wx, wu, wT);
}

extern "C" int mpcmp_jerk_trajectory_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *vmax, const double *amax, const double *jmax, int n_pts, double *out, double *T_out) {
    if (!ctx || !x0 || !xf || !jmax || !out || B < 1 || n_pts < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    JerkLimits lim;
    if (int rc = jerk_limits(ctx, vmax, amax, jmax, lim)) return rc;
    if (int rc = check_boundary_acc(ctx, B, x0, xf, acc0, accT, vmax, jmax)) return rc;
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *da0, *daT, *dout;
    sg.in(&da0, acc0, 7 * (size_t)B); sg.in(&daT, accT, 7 * (size_t)B); sg.out(&dout, out, (size_t)B * (n_pts + 1) * 22);
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = sg.upload()) return rc;
    hipLaunchKernelGGL(k_jerk_traj, dim3(B), dim3(64), 0, st, lim, ctx->d_x0, ctx->d_xf, da0, daT, n_pts, dout, ctx->d_wT);
    HIPCHK(ctx, hipGetLastError());
    if (T_out) HIPCHK(ctx, hipMemcpyAsync(T_out, ctx->d_wT, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    return sg.finish();
}

extern "C" int mpcmp_jerk_trajectory_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                               const double *jmax, int n_pts, double *out, double *T_out) {
    return mpcmp_jerk_trajectory_lim_batch(ctx, B, x0, xf, acc0, accT, nullptr, nullptr, jmax, n_pts, out, T_out);
}
extern "C" int mpcmp_jerk_trajectory_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax, int n_pts,
                                           double *out, double *T_out) {
    return mpcmp_jerk_trajectory_acc_batch(ctx, B, x0, xf, nullptr, nullptr, jmax, n_pts, out, T_out);
}

// MotionPlanner::get_RK_point (motionPlanner.hpp:130-142)
extern "C" int mpcmp_jerk_point_lim_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                          const double *vmax, const double *amax, const double *jmax, const double *time, double *out, double *T_out) {
    if (!ctx || !x0 || !xf || !jmax || !time || !out || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    JerkLimits lim;
    if (int rc = jerk_limits(ctx, vmax, amax, jmax, lim)) return rc;
    if (int rc = check_boundary_acc(ctx, B, x0, xf, acc0, accT, vmax, jmax)) return rc;
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *dt, *da0, *daT, *dout;
    sg.in(&dt, time, B); sg.in(&da0, acc0, 7 * (size_t)B); sg.in(&daT, accT, 7 * (size_t)B); sg.out(&dout, out, 28 * (size_t)B);
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    if (int rc = sg.upload()) return rc;
    hipLaunchKernelGGL(k_jerk_point, dim3(B), dim3(64), 0, st, ctx->d_model, lim, ctx->d_x0, ctx->d_xf, da0, daT, dt, dout, ctx->d_wT);
    HIPCHK(ctx, hipGetLastError());
    if (T_out) HIPCHK(ctx, hipMemcpyAsync(T_out, ctx->d_wT, sizeof(double) * B, hipMemcpyDeviceToHost, st));
    return sg.finish();
}

extern "C" int mpcmp_jerk_point_acc_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *acc0, const double *accT,
                                          const double *jmax, const double *time, double *out, double *T_out) {
    return mpcmp_jerk_point_lim_batch(ctx, B, x0, xf, acc0, accT, nullptr, nullptr, jmax, time, out, T_out);
}
extern "C" int mpcmp_jerk_point_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *jmax, const double *time,
                                      double *out, double *T_out) {
    return mpcmp_jerk_point_acc_batch(ctx, B, x0, xf, nullptr, nullptr, jmax, time, out, T_out);
}

// MotionPlanner::get_MPC_point (motionPlanner.hpp:118-128)
extern "C" int mpcmp_mpc_point_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, const double *time,
                                     double *out) {
    if (!ctx || !sx || !su || !sT || !time || !out || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *dt, *dout;
    sg.in(&dx, sx, 14 * NB); sg.in(&du, su, 7 * NB); sg.in(&dT, sT, nb); sg.in(&dt, time, nb); sg.out(&dout, out, 28 * nb);
    if (int rc = sg.upload()) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_mpc_point, dim3((B + 63) / 64), dim3(64), 0, ctx->stream, md, ms, ctx->nseg, B, dx, du, dT, dt, dout);
    HIPCHK(ctx, hipGetLastError());
    return sg.finish();
}

extern "C" int mpcmp_qp_batch(mpcmp_ctx *ctx, int B, const double *x0, const double *xf, const double *xs,
                              const double *us, const double *T, double *p, double *y, int *iters) {
    if (!ctx || !x0 || !xf || !xs || !us || !T || !p || !y || B < 1) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    if (int rc = solve_rows_ok(ctx, B)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = upload_problems(ctx, B, x0, xf, xs, us, T, st)) return rc;
    SolveCall c = staged_call(ctx, B, true, st);
    c.info = nullptr; c.only_qp = 1;
    if (int rc = solve_dispatch(ctx, c)) return rc;
    HIPCHK(ctx, hipMemcpyAsync(p, ctx->ws.p, sizeof(double) * ctx->n * B, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipMemcpyAsync(y, ctx->ws.y, sizeof(double) * ctx->mn * B, hipMemcpyDeviceToHost, st));
    if (iters) HIPCHK(ctx, hipMemcpyAsync(iters, ctx->ws.qpit, sizeof(int) * B, hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

// ------------------------------------------------------------------------------------------------
// leaf kernels
extern "C" int mpcmp_rnea_batch(mpcmp_ctx *ctx, int n, const double *q, const double *qd, const double *qdd, double *tau) {
    if (!ctx || n < 1 || !q || !qd || !qdd || !tau) return MPCMP_EINVAL;
    if (int rc = rows_ok(ctx, n, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n7 = 7 * (size_t)n;
    Stage sg(ctx);
    double *dq, *dv, *da, *dt;
    sg.in(&dq, q, n7); sg.in(&dv, qd, n7); sg.in(&da, qdd, n7); sg.out(&dt, tau, n7);
    if (int rc = sg.upload()) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_rnea_batch, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, md, ms, n, dq, dv, da, dt);
    HIPCHK(ctx, hipGetLastError());
    return sg.finish();
}

extern "C" int mpcmp_eval_constraints_batch(mpcmp_ctx *ctx, int n, const double *x, const double *u, double *g, double *G) {
    if (!ctx || n < 1 || !x || !u || !g || !G) return MPCMP_EINVAL;
    if (int rc = rows_ok(ctx, n, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t np = n;
    Stage sg(ctx);
    double *dx, *du, *dg, *dG;
    sg.in(&dx, x, 14 * np); sg.in(&du, u, 7 * np); sg.out(&dg, g, 8 * np); sg.out(&dG, G, 176 * np);
    if (int rc = sg.upload()) return rc;
    if (int rc = solver_eval_constraints(ctx, n, dx, du, dg, dG)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_sample_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT,
                                         int n_pts, double *d_out, void *hip_stream) {
    if (!ctx || B < 1 || n_pts < 1 || !d_sx || !d_su || !d_sT || !d_out) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const long total = (long)B * (n_pts + 1);
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_sample, dim3((unsigned)((total + 127) / 128)), dim3(128), 0, (hipStream_t)hip_stream, md, ms,
                       ctx->nseg, B, n_pts, d_sx, d_su, d_sT, d_out);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_sample_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_pts, double *out) {
    if (!ctx || B < 1 || n_pts < 1 || !sx || !su || !sT || !out) return MPCMP_EINVAL;
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *dout;
    sg.in(&dx, sx, 14 * NB); sg.in(&du, su, 7 * NB); sg.in(&dT, sT, nb); sg.out(&dout, out, nb * (n_pts + 1) * 29);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_sample_batch_device(ctx, B, dx, du, dT, n_pts, dout, ctx->stream)) return rc;
    return sg.finish();
}


// examples/benchmark.cpp:58-160 for a batch of trajectories (either the initial guess or the MPC solution)
extern "C" int mpcmp_traj_stats_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, const double *xf,
                                      int n_pts, double *out) {
    if (!ctx || B < 1 || n_pts < 1 || !sx || !su || !sT || !xf || !out) return MPCMP_EINVAL;
    SINGLE_ARM_ONLY(ctx);
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    // the kernel keeps the n_pts+1 samples of one trajectory (28 doubles each) in LDS: 160 KB per workgroup on gfx950
    if (sizeof(double) * 28 * (size_t)(n_pts + 1) > 150 * 1024) { ctx->err = "mpcmp_traj_stats_batch: n_pts must be <= 684 (the samples of one trajectory are held in LDS)"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    double jerk[7], j10[7];
    mpcmp_default_limits(nullptr, nullptr, nullptr, nullptr, jerk, nullptr);
    for (int r = 0; r < 7; r++) j10[r] = 10.0 * jerk[r];                     // benchmark.cpp:128
    const size_t nb = B, NB = ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *df, *dj, *dout;
    sg.in(&dx, sx, 14 * NB); sg.in(&du, su, 7 * NB); sg.in(&dT, sT, nb); sg.in(&df, xf, 14 * nb); sg.in(&dj, j10, 7); sg.out(&dout, out, 74 * nb);
    if (int rc = sg.upload()) return rc;
    const size_t lds = sizeof(double) * 28 * (size_t)(n_pts + 1);
    if (int rc = set_lds(ctx, k_traj_stats, lds)) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    hipLaunchKernelGGL(k_traj_stats, dim3(B), dim3(256), lds, ctx->stream, md, ms, ctx->nseg, n_pts, dx, du, dT, df, 1.7, 2.5, dj, dout);   // pandaWrapper.hpp:37-38
    HIPCHK(ctx, hipGetLastError());
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// clearance checks (clearance.hpp; the kernels are in clearance.hip)
extern "C" int mpcmp_set_robot_spheres(mpcmp_ctx *ctx, int arm, int n, const mpcmp_sphere *sp) {
    if (!ctx) { g_err = "mpcmp_set_robot_spheres: no context"; return MPCMP_EINVAL; }
    if (arm < 0 || arm >= ctx->narm || n < 0 || n > CLR_MAX_SPH || (n > 0 && !sp)) {
        ctx->err = "mpcmp_set_robot_spheres: arm must be in [0, narm) and n in [0, 64] with the spheres given"; return MPCMP_EINVAL;
    }
    for (int i = 0; i < n; i++) {
        const mpcmp_sphere &s = sp[i];
        if (s.joint < 0 || s.joint > 6 || !std::isfinite(s.c[0]) || !std::isfinite(s.c[1]) || !std::isfinite(s.c[2]) || !std::isfinite(s.r) || !(s.r > 0.0)) {
            ctx->err = "mpcmp_set_robot_spheres: sphere " + std::to_string(i) + ": joint in 0..6, finite centre and r > 0 required"; return MPCMP_EINVAL;
        }
    }
    int cnt[2] = {ctx->clr_nsph[0], ctx->clr_nsph[1]};
    cnt[arm] = n;
    ClrSphere tab[2 * CLR_MAX_SPH];
    int k = 0;
    for (int a = 0; a < ctx->narm; a++)
        for (int i = 0; i < cnt[a]; i++, k++) {
            const mpcmp_sphere &s = a == arm ? sp[i] : ctx->clr_sph[a][i];
            tab[k].c[0] = s.c[0]; tab[k].c[1] = s.c[1]; tab[k].c[2] = s.c[2]; tab[k].r = s.r; tab[k].joint = s.joint; tab[k].arm = a;
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());          // (checks may be in flight on any stream of the caller: they read this table)
    if (k > 0) HIPCHK(ctx, hipMemcpy(ctx->d_clr_sph, tab, sizeof(ClrSphere) * k, hipMemcpyHostToDevice));
    for (int i = 0; i < n; i++) ctx->clr_sph[arm][i] = sp[i];
    ctx->clr_nsph[arm] = n;
    return MPCMP_OK;
}

static int obstacles_check(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *obs) {
    if (!ctx) { g_err = "mpcmp_set_obstacles: no context"; return MPCMP_EINVAL; }
    if (n_sets < 0 || n_sets > ctx->max_batch || n_obs < 0 || n_obs > CLR_MAX_OBS || (n_sets > 0 && n_obs > 0 && !obs)) {
        ctx->err = "mpcmp_set_obstacles: n_sets must be in [0, max_batch] and n_obs in [0, 256] with the obstacles given"; return MPCMP_EINVAL;
    }
    const size_t want = (size_t)n_sets * n_obs;
    if (want > ctx->clr_obs_cap) {          // grow: later launches read the new buffer; wait for the ones that read the old one
        HIPCHK(ctx, hipSetDevice(ctx->device));
        void *q = nullptr;
        HIPCHK(ctx, hipMalloc(&q, want * sizeof(mpcmp_obstacle)));
        if (ctx->d_clr_obs) {
            HIPCHK(ctx, hipDeviceSynchronize());
            ctx->allocs.erase(std::find(ctx->allocs.begin(), ctx->allocs.end(), (void *)ctx->d_clr_obs));
            (void)hipFree(ctx->d_clr_obs);
        }
        ctx->allocs.push_back(q); ctx->d_clr_obs = (mpcmp_obstacle *)q; ctx->clr_obs_cap = want;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_set_obstacles(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *obs) {
    if (ctx && n_sets > 0 && n_sets <= ctx->max_batch && n_obs > 0 && n_obs <= CLR_MAX_OBS && obs)
        for (size_t i = 0; i < (size_t)n_sets * n_obs; i++) {
            const mpcmp_obstacle &o = obs[i];
            bool ok = o.type >= MPCMP_OBS_SPHERE && o.type <= MPCMP_OBS_HALFSPACE && std::isfinite(o.r);
            for (int d = 0; d < 3 && ok; d++) ok = std::isfinite(o.a[d]) && std::isfinite(o.b[d]);
            if (ok && o.type != MPCMP_OBS_HALFSPACE) ok = o.r >= 0.0;
            if (ok && o.type == MPCMP_OBS_BOX) ok = o.b[0] > 0.0 && o.b[1] > 0.0 && o.b[2] > 0.0;
            if (ok && o.type == MPCMP_OBS_HALFSPACE) ok = std::fabs(std::sqrt(o.a[0] * o.a[0] + o.a[1] * o.a[1] + o.a[2] * o.a[2]) - 1.0) <= 1e-9;
            if (!ok) {
                ctx->err = "mpcmp_set_obstacles: set " + std::to_string(i / n_obs) + ", obstacle " + std::to_string(i % n_obs) +
                           ": known type, finite values, r >= 0, box half extents > 0 and a unit half-space normal required";
                return MPCMP_EINVAL;
            }
        }
    if (int rc = obstacles_check(ctx, n_sets, n_obs, obs)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());          // (checks may be in flight on any stream of the caller: they read these sets)
    if (n_sets > 0 && n_obs > 0) HIPCHK(ctx, hipMemcpy(ctx->d_clr_obs, obs, sizeof(mpcmp_obstacle) * n_sets * n_obs, hipMemcpyHostToDevice));
    ctx->clr_sets = n_obs > 0 ? n_sets : 0; ctx->clr_nobs = n_sets > 0 ? n_obs : 0;
    ctx->mv_tracks = 0;                           // (new obstacle sets stand still until mpcmp_set_obstacle_tracks says otherwise)
    return MPCMP_OK;
}

extern "C" int mpcmp_set_obstacles_device(mpcmp_ctx *ctx, int n_sets, int n_obs, const mpcmp_obstacle *d_obs, void *hip_stream) {
    if (int rc = obstacles_check(ctx, n_sets, n_obs, d_obs)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_sets > 0 && n_obs > 0)      // (the caller's later work: a clearance check on its stream, which waits for the copy)
        if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
                HIPCHK(ctx, hipMemcpyAsync(ctx->d_clr_obs, d_obs, sizeof(mpcmp_obstacle) * n_sets * n_obs, hipMemcpyDeviceToDevice, st));
                return MPCMP_OK;
            })) return rc;
    ctx->clr_sets = n_obs > 0 ? n_sets : 0; ctx->clr_nobs = n_sets > 0 ? n_obs : 0;
    ctx->mv_tracks = 0;
    return MPCMP_OK;
}

// the tables of every clearance check as its kernel reads them: the arms, the spheres and the obstacle sets in force
static ClrTables clearance_tables(const mpcmp_ctx *ctx) {
    ClrTables t;
    t.d_model = ctx->d_model; t.narm = ctx->narm; t.nseg = ctx->nseg;
    t.d_sph = ctx->d_clr_sph; t.n_sph[0] = ctx->clr_nsph[0]; t.n_sph[1] = ctx->narm > 1 ? ctx->clr_nsph[1] : 0;
    t.d_obs = ctx->d_clr_obs; t.n_obs = ctx->clr_nobs; t.obs_stride = ctx->clr_sets > 1 ? ctx->clr_nobs : 0;
    return t;
}
// with more than one obstacle set, problem b reads set b
static int obstacle_sets_check(mpcmp_ctx *ctx, int B) {
    if (ctx->clr_sets > 1 && B > ctx->clr_sets) {
        ctx->err = "more problems (" + std::to_string(B) + ") than obstacle sets (" + std::to_string(ctx->clr_sets) + "): see mpcmp_set_obstacles";
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}

static int clearance_check(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_pts, double margin, int self_gap, const mpcmp_clearance *out) {
    if (!ctx) { g_err = "mpcmp_clearance_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || n_pts < 1 || n_pts > CLR_MAX_PTS || !sx || !sT || !out || !std::isfinite(margin) || self_gap < 0) {
        ctx->err = "mpcmp_clearance_batch: B >= 1, 1 <= n_pts <= 4096, a finite margin, self_gap >= 0 and all pointers required"; return MPCMP_EINVAL;
    }
    return obstacle_sets_check(ctx, B);
}

static int clearance_enqueue(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_pts, double margin, int self_gap,
                             mpcmp_clearance *d_out, hipStream_t st) {
    const ClrTables t = clearance_tables(ctx);
    if (!ctx->clr_ready) { HIPCHK(ctx, clearance_prepare()); ctx->clr_ready = true; }
    HIPCHK(ctx, clearance_launch(t, B, d_sx, d_sT, n_pts, margin, self_gap, d_out, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_pts, double margin, int self_gap,
                                            mpcmp_clearance *d_out, void *hip_stream) {
    if (int rc = clearance_check(ctx, B, d_sx, d_sT, n_pts, margin, self_gap, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return clearance_enqueue(ctx, B, d_sx, d_sT, n_pts, margin, self_gap, d_out, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_clearance_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_pts, double margin, int self_gap,
                                     mpcmp_clearance *out) {
    if (int rc = clearance_check(ctx, B, sx, sT, n_pts, margin, self_gap, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT;
    mpcmp_clearance *dout;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = clearance_enqueue(ctx, B, dx, dT, n_pts, margin, self_gap, dout, ctx->stream)) return rc;
    return sg.finish();
}

// the certified check (include/mpcmp_clearance_cert.h; the kernel is in clearance_cert.hip)
static int clearance_cert_check(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, double margin, int self_gap, int n_start, int max_depth,
                                const mpcmp_clearance *out) {
    if (!ctx) { g_err = "mpcmp_clearance_certified_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !sx || !sT || !out || !std::isfinite(margin) || self_gap < 0 || n_start < 1 || n_start > MPCMP_CLR_CERT_CAPACITY ||
        ctx->nseg * n_start > MPCMP_CLR_CERT_CAPACITY || max_depth < 0 || max_depth > 16) {
        ctx->err = "mpcmp_clearance_certified_batch: B >= 1, n_start >= 1 with num_seg n_start <= 4096, max_depth in [0, 16], a finite margin, "
                   "self_gap >= 0 and all pointers (but cert) required";
        return MPCMP_EINVAL;
    }
    return obstacle_sets_check(ctx, B);
}

static int clearance_cert_enqueue(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, double margin, int self_gap, int n_start, int max_depth,
                                  mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, hipStream_t st) {
    const ClrTables t = clearance_tables(ctx);
    if (!ctx->clr_cert_ready) { HIPCHK(ctx, clearance_cert_prepare()); ctx->clr_cert_ready = true; }
    const CertPlans p = {d_sx, d_sT, nullptr, nullptr, nullptr};
    // (no timeline: the obstacles stand where mpcmp_set_obstacles put them, whatever tracks the context holds)
    HIPCHK(ctx, clearance_cert_launch(t, nullptr, p, B, margin, self_gap, n_start, 0, max_depth, d_out, d_cert, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_certified_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, double margin, int self_gap,
                                                      int n_start, int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert,
                                                      void *hip_stream) {
    if (int rc = clearance_cert_check(ctx, B, d_sx, d_sT, margin, self_gap, n_start, max_depth, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return clearance_cert_enqueue(ctx, B, d_sx, d_sT, margin, self_gap, n_start, max_depth, d_out, d_cert, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_clearance_certified_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, double margin, int self_gap, int n_start,
                                               int max_depth, mpcmp_clearance *out, mpcmp_clearance_cert *cert) {
    if (int rc = clearance_cert_check(ctx, B, sx, sT, margin, self_gap, n_start, max_depth, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT;
    mpcmp_clearance *dout;
    mpcmp_clearance_cert *dcert = nullptr;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.out(&dout, out, B);
    if (cert) sg.out(&dcert, cert, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = clearance_cert_enqueue(ctx, B, dx, dT, margin, self_gap, n_start, max_depth, dout, dcert, ctx->stream)) return rc;
    return sg.finish();
}

// ---- clearance in a moving world (include/mpcmp_moving.h; the kernels are in moving.hip, the rule in moving_rule.hpp) ----
static int tracks_check(mpcmp_ctx *ctx, int n_sets, int n_obs, const int *track_of, int n_tracks, int n_key, double t0, double dt,
                        const double *offsets) {
    if (!ctx) { g_err = "mpcmp_set_obstacle_tracks: no context"; return MPCMP_EINVAL; }
    if (n_tracks == 0) return MPCMP_OK;
    if (n_tracks < 0 || n_tracks > MV_MAX_TRACKS || n_key < 1 || n_key > MV_MAX_KEYS || !track_of || !offsets || !std::isfinite(t0) ||
        !std::isfinite(dt) || !(dt > 0.0)) {
        ctx->err = "mpcmp_set_obstacle_tracks: n_tracks in [0, 64], n_key in [1, 1024], a finite clock with dt > 0 and both arrays required";
        return MPCMP_EINVAL;
    }
    if (n_sets < 1 || n_sets != ctx->clr_sets || n_obs != ctx->clr_nobs) {
        ctx->err = "mpcmp_set_obstacle_tracks: " + std::to_string(n_sets) + " sets of " + std::to_string(n_obs) + " obstacles, but " +
                   std::to_string(ctx->clr_sets) + " sets of " + std::to_string(ctx->clr_nobs) + " are in force: see mpcmp_set_obstacles";
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}
// room for the table; growth waits for the checks that read the old buffers
static int tracks_reserve(mpcmp_ctx *ctx, size_t n_tof, size_t n_off) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (n_tof > ctx->mv_tof_cap) {
        void *q = nullptr;
        HIPCHK(ctx, hipMalloc(&q, n_tof * sizeof(int)));
        if (ctx->d_mv_track_of) {
            HIPCHK(ctx, hipDeviceSynchronize());
            ctx->allocs.erase(std::find(ctx->allocs.begin(), ctx->allocs.end(), (void *)ctx->d_mv_track_of));
            (void)hipFree(ctx->d_mv_track_of);
        }
        ctx->allocs.push_back(q); ctx->d_mv_track_of = (int *)q; ctx->mv_tof_cap = n_tof;
    }
    if (n_off > ctx->mv_off_cap) {
        void *q = nullptr;
        HIPCHK(ctx, hipMalloc(&q, n_off * sizeof(double)));
        if (ctx->d_mv_off) {
            HIPCHK(ctx, hipDeviceSynchronize());
            ctx->allocs.erase(std::find(ctx->allocs.begin(), ctx->allocs.end(), (void *)ctx->d_mv_off));
            (void)hipFree(ctx->d_mv_off);
        }
        ctx->allocs.push_back(q); ctx->d_mv_off = (double *)q; ctx->mv_off_cap = n_off;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_set_obstacle_tracks(mpcmp_ctx *ctx, int n_sets, int n_obs, const int *track_of, int n_tracks, int n_key, double t0, double dt,
                                         const double *offsets) {
    if (int rc = tracks_check(ctx, n_sets, n_obs, track_of, n_tracks, n_key, t0, dt, offsets)) return rc;
    if (n_tracks == 0) { ctx->mv_tracks = 0; return MPCMP_OK; }
    const size_t n_tof = (size_t)n_sets * n_obs, n_off = (size_t)n_sets * n_tracks * n_key * 3;
    for (size_t i = 0; i < n_tof; i++)
        if (track_of[i] < -1 || track_of[i] >= n_tracks) {
            ctx->err = "mpcmp_set_obstacle_tracks: track_of[" + std::to_string(i) + "] must be in [-1, n_tracks)"; return MPCMP_EINVAL;
        }
    for (size_t i = 0; i < n_off; i++)
        if (!std::isfinite(offsets[i])) { ctx->err = "mpcmp_set_obstacle_tracks: offset " + std::to_string(i) + " is not finite"; return MPCMP_EINVAL; }
    if (int rc = tracks_reserve(ctx, n_tof, n_off)) return rc;
    HIPCHK(ctx, hipDeviceSynchronize());          // (checks may be in flight on any stream of the caller: they read this table)
    HIPCHK(ctx, hipMemcpy(ctx->d_mv_track_of, track_of, sizeof(int) * n_tof, hipMemcpyHostToDevice));
    HIPCHK(ctx, hipMemcpy(ctx->d_mv_off, offsets, sizeof(double) * n_off, hipMemcpyHostToDevice));
    ctx->mv_tracks = n_tracks; ctx->mv_keys = n_key; ctx->mv_t0 = t0; ctx->mv_dt = dt;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_obstacle_tracks_device(mpcmp_ctx *ctx, int n_sets, int n_obs, const int *d_track_of, int n_tracks, int n_key, double t0,
                                                double dt, const double *d_offsets, void *hip_stream) {
    if (int rc = tracks_check(ctx, n_sets, n_obs, d_track_of, n_tracks, n_key, t0, dt, d_offsets)) return rc;
    if (n_tracks == 0) { ctx->mv_tracks = 0; return MPCMP_OK; }
    const size_t n_tof = (size_t)n_sets * n_obs, n_off = (size_t)n_sets * n_tracks * n_key * 3;
    if (int rc = tracks_reserve(ctx, n_tof, n_off)) return rc;
    if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_mv_track_of, d_track_of, sizeof(int) * n_tof, hipMemcpyDeviceToDevice, st));
            HIPCHK(ctx, hipMemcpyAsync(ctx->d_mv_off, d_offsets, sizeof(double) * n_off, hipMemcpyDeviceToDevice, st));
            return MPCMP_OK;
        })) return rc;
    ctx->mv_tracks = n_tracks; ctx->mv_keys = n_key; ctx->mv_t0 = t0; ctx->mv_dt = dt;
    return MPCMP_OK;
}

// the track table in force beside clearance_tables
static MvTracks moving_tracks(const mpcmp_ctx *ctx) {
    MvTracks trk;
    trk.d_track_of = ctx->d_mv_track_of; trk.d_offsets = ctx->d_mv_off; trk.n_tracks = ctx->mv_tracks;
    trk.n_key = ctx->mv_tracks > 0 ? ctx->mv_keys : 1; trk.t0 = ctx->mv_t0; trk.dt = ctx->mv_dt;
    return trk;
}
static int moving_ready(mpcmp_ctx *ctx) {
    if (!ctx->mv_ready) { HIPCHK(ctx, moving_prepare()); ctx->mv_ready = true; }
    return MPCMP_OK;
}
static bool profile_args_ok(const double *prof, int n_grid) { return !prof || (n_grid >= 1 && n_grid <= MV_MAX_GRID); }

static int clearance_timed_check(mpcmp_ctx *ctx, const char *who, int B, const double *sx, const double *sT, int n_grid, const double *prof, int n_pts,
                                 double margin, int self_gap, const void *out) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    if (B < 1 || n_pts < 1 || n_pts > CLR_MAX_PTS || !sx || !sT || !out || !std::isfinite(margin) || self_gap < 0 || !profile_args_ok(prof, n_grid)) {
        ctx->err = std::string(who) + ": B >= 1, 1 <= n_pts <= 4096, a finite margin, self_gap >= 0, with a profile 1 <= n_grid <= 4096 and all "
                   "pointers (but prof, t_start, d_min_all) required";
        return MPCMP_EINVAL;
    }
    return obstacle_sets_check(ctx, B);
}

extern "C" int mpcmp_clearance_timed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_grid, const double *d_prof,
                                                  const double *d_t_start, int n_pts, double margin, int self_gap, mpcmp_clearance *d_out,
                                                  void *hip_stream) {
    if (int rc = clearance_timed_check(ctx, "mpcmp_clearance_timed_batch", B, d_sx, d_sT, n_grid, d_prof, n_pts, margin, self_gap, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = moving_ready(ctx)) return rc;
    const ClrTables t = clearance_tables(ctx);
    const MvTracks trk = moving_tracks(ctx);
    const MvPlans p = {d_sx, d_sT, d_prof, d_t_start, n_grid};
    HIPCHK(ctx, clearance_timed_launch(t, trk, p, B, n_pts, margin, self_gap, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_timed_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_grid, const double *prof,
                                           const double *t_start, int n_pts, double margin, int self_gap, mpcmp_clearance *out) {
    if (int rc = clearance_timed_check(ctx, "mpcmp_clearance_timed_batch", B, sx, sT, n_grid, prof, n_pts, margin, self_gap, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT, *dp, *dts;
    mpcmp_clearance *dout;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.in(&dp, prof, prof ? (size_t)B * (n_grid + 1) * 2 : 0);
    sg.in(&dts, t_start, B); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_clearance_timed_batch_device(ctx, B, dx, dT, n_grid, dp, dts, n_pts, margin, self_gap, dout, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_start_delay_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_grid, const double *d_prof, int K,
                                              const double *d_delays, int check_wait, int n_pts, double margin, int self_gap, double *d_min_all,
                                              mpcmp_start_delay *d_out, void *hip_stream) {
    if (int rc = clearance_timed_check(ctx, "mpcmp_start_delay_batch", B, d_sx, d_sT, n_grid, d_prof, n_pts, margin, self_gap, d_out)) return rc;
    if (K < 1 || K > MV_MAX_DELAYS || !d_delays) { ctx->err = "mpcmp_start_delay_batch: 1 <= K <= 256 delays required"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = moving_ready(ctx)) return rc;
    const ClrTables t = clearance_tables(ctx);
    const MvTracks trk = moving_tracks(ctx);
    const MvPlans p = {d_sx, d_sT, d_prof, nullptr, n_grid};
    HIPCHK(ctx, start_delay_launch(t, trk, p, B, K, d_delays, check_wait, n_pts, margin, self_gap, d_min_all, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_start_delay_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_grid, const double *prof, int K,
                                       const double *delays, int check_wait, int n_pts, double margin, int self_gap, double *d_min_all,
                                       mpcmp_start_delay *out) {
    if (int rc = clearance_timed_check(ctx, "mpcmp_start_delay_batch", B, sx, sT, n_grid, prof, n_pts, margin, self_gap, out)) return rc;
    bool ok = K >= 1 && K <= MV_MAX_DELAYS && delays;
    for (int k = 0; ok && k < K; k++) ok = std::isfinite(delays[k]) && delays[k] >= 0.0 && (k == 0 || delays[k] >= delays[k - 1]);
    if (!ok) { ctx->err = "mpcmp_start_delay_batch: 1 <= K <= 256 delays, finite, >= 0 and ascending, required"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT, *dp, *dd, *dall;
    mpcmp_start_delay *dout;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.in(&dp, prof, prof ? (size_t)B * (n_grid + 1) * 2 : 0);
    sg.in(&dd, delays, K); sg.out(&dall, d_min_all, (size_t)B * K); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_start_delay_batch_device(ctx, B, dx, dT, n_grid, dp, K, dd, check_wait, n_pts, margin, self_gap, dall, dout, ctx->stream))
        return rc;
    return sg.finish();
}

static int sphere_tracks_check(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_grid, const double *prof, double t0, double dt,
                               int n_key, const double *out) {
    if (!ctx) { g_err = "mpcmp_sphere_tracks_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !sx || !sT || !out || n_key < 1 || n_key > MV_MAX_KEYS || !std::isfinite(t0) || !std::isfinite(dt) || !(dt > 0.0) ||
        !profile_args_ok(prof, n_grid)) {
        ctx->err = "mpcmp_sphere_tracks_batch: B >= 1, n_key in [1, 1024], a finite clock with dt > 0, with a profile 1 <= n_grid <= 4096 and all "
                   "pointers (but prof, t_start) required";
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_sphere_tracks_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_grid, const double *d_prof,
                                                const double *d_t_start, double t0, double dt, int n_key, double *d_out, void *hip_stream) {
    if (int rc = sphere_tracks_check(ctx, B, d_sx, d_sT, n_grid, d_prof, t0, dt, n_key, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = moving_ready(ctx)) return rc;
    const ClrTables t = clearance_tables(ctx);
    const MvPlans p = {d_sx, d_sT, d_prof, d_t_start, n_grid};
    HIPCHK(ctx, sphere_tracks_launch(t, p, B, t0, dt, n_key, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_sphere_tracks_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_grid, const double *prof,
                                         const double *t_start, double t0, double dt, int n_key, double *out) {
    if (int rc = sphere_tracks_check(ctx, B, sx, sT, n_grid, prof, t0, dt, n_key, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const int nsph = ctx->clr_nsph[0] + (ctx->narm > 1 ? ctx->clr_nsph[1] : 0);
    if (nsph < 1) return MPCMP_OK;
    Stage sg(ctx);
    double *dx, *dT, *dp, *dts, *dout;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.in(&dp, prof, prof ? (size_t)B * (n_grid + 1) * 2 : 0);
    sg.in(&dts, t_start, B); sg.out(&dout, out, (size_t)B * nsph * n_key * 3);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_sphere_tracks_batch_device(ctx, B, dx, dT, n_grid, dp, dts, t0, dt, n_key, dout, ctx->stream)) return rc;
    return sg.finish();
}

// ---- certified clearance in a moving world (include/mpcmp_moving_cert.h; the kernel is k_clearance_cert with a timeline, the rule moving_cert_rule.hpp) ----
static int clearance_cert_timed_check(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, double margin, int self_gap, int n_start, int n_rest,
                                      int max_depth, const mpcmp_clearance *out) {
    if (!ctx) { g_err = "mpcmp_clearance_certified_timed_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !sx || !sT || !out || !std::isfinite(margin) || self_gap < 0 || n_start < 1 || n_start > MPCMP_CLR_CERT_CAPACITY || n_rest < 1 ||
        n_rest > MPCMP_CLR_CERT_CAPACITY || (long)ctx->nseg * n_start + 2l * n_rest > MPCMP_CLR_CERT_CAPACITY || max_depth < 0 || max_depth > 16) {
        ctx->err = "mpcmp_clearance_certified_timed_batch: B >= 1, n_start >= 1 and n_rest >= 1 with num_seg n_start + 2 n_rest <= 4096, max_depth in "
                   "[0, 16], a finite margin, self_gap >= 0 and all pointers (but t_start, wait_before, hold_after, cert) required";
        return MPCMP_EINVAL;
    }
    return obstacle_sets_check(ctx, B);
}

extern "C" int mpcmp_clearance_certified_timed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, const double *d_t_start,
                                                            const double *d_wait, const double *d_hold, double margin, int self_gap, int n_start,
                                                            int n_rest, int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert,
                                                            void *hip_stream) {
    if (int rc = clearance_cert_timed_check(ctx, B, d_sx, d_sT, margin, self_gap, n_start, n_rest, max_depth, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!ctx->clr_cert_ready) { HIPCHK(ctx, clearance_cert_prepare()); ctx->clr_cert_ready = true; }
    const ClrTables t = clearance_tables(ctx);
    const MvTracks trk = moving_tracks(ctx);
    const CertPlans p = {d_sx, d_sT, d_t_start, d_wait, d_hold};
    HIPCHK(ctx, clearance_cert_launch(t, &trk, p, B, margin, self_gap, n_start, n_rest, max_depth, d_out, d_cert, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_certified_timed_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, const double *t_start,
                                                     const double *wait_before, const double *hold_after, double margin, int self_gap, int n_start,
                                                     int n_rest, int max_depth, mpcmp_clearance *out, mpcmp_clearance_cert *cert) {
    if (int rc = clearance_cert_timed_check(ctx, B, sx, sT, margin, self_gap, n_start, n_rest, max_depth, out)) return rc;
    for (int b = 0; b < B; b++)
        if ((wait_before && wait_before[b] < 0.0) || (hold_after && hold_after[b] < 0.0)) {
            ctx->err = "mpcmp_clearance_certified_timed_batch: wait_before and hold_after must not be negative (problem " + std::to_string(b) + ")";
            return MPCMP_EINVAL;
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT, *dts, *dw, *dh;
    mpcmp_clearance *dout;
    mpcmp_clearance_cert *dcert = nullptr;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.in(&dts, t_start, B); sg.in(&dw, wait_before, B); sg.in(&dh, hold_after, B);
    sg.out(&dout, out, B);
    if (cert) sg.out(&dcert, cert, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_clearance_certified_timed_batch_device(ctx, B, dx, dT, dts, dw, dh, margin, self_gap, n_start, n_rest, max_depth, dout, dcert,
                                                              ctx->stream)) return rc;
    return sg.finish();
}

// ---- voxel worlds (include/mpcmp_field.h; the kernels are in field.hip, the rule in field_rule.hpp) ----
// the checks the four setters share; `given`: the occupancy or the points are there (or none are needed).  desc == NULL (clear) passes
static int field_set_check(mpcmp_ctx *ctx, const char *who, const mpcmp_field_desc *desc, bool given) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    if (!desc) return MPCMP_OK;
    if (!fld_desc_ok(*desc) || !given) {
        ctx->err = std::string(who) + ": 1 <= n[d] <= 1024 with at most 2^24 voxels, a finite origin, a finite h > 0 and the data required";
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}
// the three arrays of a grid of `desc` (the only allocation of this family): grown when the grid grows; the launches that read the old ones are waited for
static int field_reserve(mpcmp_ctx *ctx, const mpcmp_field_desc &desc) {
    const size_t want = (size_t)fld_voxels(desc);
    if (want <= ctx->fld_cap) return MPCMP_OK;
    void *q[3] = {nullptr, nullptr, nullptr};
    const size_t bytes[3] = {want, want * sizeof(unsigned), want * sizeof(unsigned)};
    for (int i = 0; i < 3; i++)
        if (hipMalloc(&q[i], bytes[i]) != hipSuccess) {
            for (int k = 0; k < i; k++) (void)hipFree(q[k]);
            ctx->err = "mpcmp_set_field: device allocation of " + std::to_string(want) + " voxels failed"; return MPCMP_ERUNTIME;
        }
    if (ctx->d_fld_occ) {
        HIPCHK(ctx, hipDeviceSynchronize());
        void *old[3] = {ctx->d_fld_occ, ctx->d_fld_d2, ctx->d_fld_tmp};
        for (void *o : old) { ctx->allocs.erase(std::find(ctx->allocs.begin(), ctx->allocs.end(), o)); (void)hipFree(o); }
    }
    for (void *p : q) ctx->allocs.push_back(p);
    ctx->d_fld_occ = (unsigned char *)q[0]; ctx->d_fld_d2 = (unsigned *)q[1]; ctx->d_fld_tmp = (unsigned *)q[2];
    ctx->fld_cap = want;
    ctx->fld_set = false;              // (the old field went with its arrays; the caller sets the new one)
    return MPCMP_OK;
}
static FldArrays field_arrays(const mpcmp_ctx *ctx, const mpcmp_field_desc &desc) {
    FldArrays f;
    f.desc = desc; f.d_occ = ctx->d_fld_occ; f.d_d2 = ctx->d_fld_d2; f.d_tmp = ctx->d_fld_tmp;
    return f;
}

extern "C" int mpcmp_set_field(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const unsigned char *occ) {
    if (int rc = field_set_check(ctx, "mpcmp_set_field", desc, occ != nullptr)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());          // (checks may be in flight on any stream of the caller: they read this field)
    if (!desc) { ctx->fld_set = false; return MPCMP_OK; }
    if (int rc = field_reserve(ctx, *desc)) return rc;
    const FldArrays f = field_arrays(ctx, *desc);
    ctx->fld_set = false;
    HIPCHK(ctx, hipMemcpy(f.d_occ, occ, (size_t)fld_voxels(*desc), hipMemcpyHostToDevice));
    HIPCHK(ctx, field_build_launch(f, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->fld_desc = *desc; ctx->fld_set = true;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_field_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const unsigned char *d_occ, void *hip_stream) {
    if (int rc = field_set_check(ctx, "mpcmp_set_field_device", desc, d_occ != nullptr)) return rc;
    if (!desc) { ctx->fld_set = false; return MPCMP_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = field_reserve(ctx, *desc)) return rc;
    const FldArrays f = field_arrays(ctx, *desc);
    ctx->fld_set = false;
    if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
            HIPCHK(ctx, hipMemcpyAsync(f.d_occ, d_occ, (size_t)fld_voxels(*desc), hipMemcpyDeviceToDevice, st));
            HIPCHK(ctx, field_build_launch(f, st));
            return MPCMP_OK;
        })) return rc;
    ctx->fld_desc = *desc; ctx->fld_set = true;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_field_points(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *points) {
    if (int rc = field_set_check(ctx, "mpcmp_set_field_points", desc, n_points >= 0 && (n_points == 0 || points))) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (!desc) { ctx->fld_set = false; return MPCMP_OK; }
    if (int rc = field_reserve(ctx, *desc)) return rc;
    const FldArrays f = field_arrays(ctx, *desc);
    ctx->fld_set = false;
    Stage sg(ctx);
    double *dp = nullptr;
    if (n_points > 0) sg.in(&dp, points, (size_t)3 * n_points);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, field_mark_launch(f, n_points, dp, ctx->stream));
    HIPCHK(ctx, field_build_launch(f, ctx->stream));
    if (int rc = sg.finish()) return rc;
    ctx->fld_desc = *desc; ctx->fld_set = true;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_field_points_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *d_points, void *hip_stream) {
    if (int rc = field_set_check(ctx, "mpcmp_set_field_points_device", desc, n_points >= 0 && (n_points == 0 || d_points))) return rc;
    if (!desc) { ctx->fld_set = false; return MPCMP_OK; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = field_reserve(ctx, *desc)) return rc;
    const FldArrays f = field_arrays(ctx, *desc);
    ctx->fld_set = false;
    if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
            HIPCHK(ctx, field_mark_launch(f, n_points, d_points, st));
            HIPCHK(ctx, field_build_launch(f, st));
            return MPCMP_OK;
        })) return rc;
    ctx->fld_desc = *desc; ctx->fld_set = true;
    return MPCMP_OK;
}

extern "C" int mpcmp_get_field(mpcmp_ctx *ctx, mpcmp_field_desc *desc_out, unsigned *d2_out) {
    if (!ctx) { g_err = "mpcmp_get_field: no context"; return MPCMP_EINVAL; }
    if (!ctx->fld_set || !desc_out) { ctx->err = "mpcmp_get_field: no field is set (mpcmp_set_field), or desc_out is NULL"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());          // (a device-side setter may have built it on any stream)
    *desc_out = ctx->fld_desc;
    if (d2_out) HIPCHK(ctx, hipMemcpy(d2_out, ctx->d_fld_d2, sizeof(unsigned) * (size_t)fld_voxels(ctx->fld_desc), hipMemcpyDeviceToHost));
    return MPCMP_OK;
}

static int clearance_field_check(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_pts, double margin, const mpcmp_clearance *out) {
    if (!ctx) { g_err = "mpcmp_clearance_field_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || n_pts < 1 || n_pts > CLR_MAX_PTS || !sx || !sT || !out || !std::isfinite(margin)) {
        ctx->err = "mpcmp_clearance_field_batch: B >= 1, 1 <= n_pts <= 4096, a finite margin and all pointers required"; return MPCMP_EINVAL;
    }
    if (!ctx->fld_set) { ctx->err = "mpcmp_clearance_field_batch: no field is set: see mpcmp_set_field"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_field_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, int n_pts, double margin,
                                                  mpcmp_clearance *d_out, void *hip_stream) {
    if (int rc = clearance_field_check(ctx, B, d_sx, d_sT, n_pts, margin, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const ClrTables t = clearance_tables(ctx);      // (the obstacle sets are not read)
    if (!ctx->fld_ready) { HIPCHK(ctx, field_prepare()); ctx->fld_ready = true; }
    HIPCHK(ctx, clearance_field_launch(t, field_arrays(ctx, ctx->fld_desc), B, d_sx, d_sT, n_pts, margin, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_field_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, int n_pts, double margin, mpcmp_clearance *out) {
    if (int rc = clearance_field_check(ctx, B, sx, sT, n_pts, margin, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT;
    mpcmp_clearance *dout;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_clearance_field_batch_device(ctx, B, dx, dT, n_pts, margin, dout, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_clearance_merge_batch_device(mpcmp_ctx *ctx, int B, const mpcmp_clearance *d_a, const mpcmp_clearance *d_b, mpcmp_clearance *d_out,
                                                  int *d_source, void *hip_stream) {
    if (!ctx) { g_err = "mpcmp_clearance_merge_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !d_a || !d_b || !d_out) { ctx->err = "mpcmp_clearance_merge_batch: B >= 1 and a, b and out required"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, clearance_merge_launch(B, d_a, d_b, d_out, d_source, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_merge_batch(mpcmp_ctx *ctx, int B, const mpcmp_clearance *a, const mpcmp_clearance *b, mpcmp_clearance *out,
                                           int *source) {
    if (!ctx) { g_err = "mpcmp_clearance_merge_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !a || !b || !out) { ctx->err = "mpcmp_clearance_merge_batch: B >= 1 and a, b and out required"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    mpcmp_clearance *da, *db, *dout;
    int *dsrc = nullptr;
    sg.in(&da, a, B); sg.in(&db, b, B); sg.out(&dout, out, B);
    if (source) sg.out(&dsrc, source, B);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, clearance_merge_launch(B, da, db, dout, dsrc, ctx->stream));
    return sg.finish();
}

// ---- camera frames as voxel worlds (include/mpcmp_frame.h; the kernels are in frame.hip, the rule in frame_rule.hpp) ----
// the checks the setters of the family share; `given`: the data of the call are there.  Nothing is changed before they have passed
static int frame_check(mpcmp_ctx *ctx, const char *who, const mpcmp_field_desc *desc, bool given, const double *q, double pad, int flags) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    bool q_ok = true;
    if (q) for (int j = 0; j < 7 * ctx->narm; j++) q_ok = q_ok && std::isfinite(q[j]);
    if (!desc || !fld_desc_ok(*desc) || !given || !q_ok || !frm_pad_ok(pad) || (flags & ~MPCMP_FRAME_KEEP)) {
        ctx->err = std::string(who) + ": a grid of 1 <= n[d] <= 1024 with at most 2^24 voxels, a finite origin and a finite h > 0, the data, a finite q, "
                   "a finite pad >= 0 and no flag but MPCMP_FRAME_KEEP required";
        return MPCMP_EINVAL;
    }
    if ((flags & MPCMP_FRAME_KEEP) && !(ctx->fld_set && frm_same_grid(ctx->fld_desc, *desc))) {
        ctx->err = std::string(who) + ": MPCMP_FRAME_KEEP needs a field in force with an identical desc"; return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}
// the filter table and the counts record (the family's own allocation, made by its first use)
static int frame_reserve(mpcmp_ctx *ctx) {
    if (ctx->d_frm_tab) return MPCMP_OK;
    void *p = nullptr;
    const size_t tab_bytes = sizeof(double) * 4 * FRM_MAX_SPH;
    if (hipMalloc(&p, tab_bytes + sizeof(mpcmp_frame_stats)) != hipSuccess) {
        ctx->err = "mpcmp_frame: device allocation of the filter table failed"; return MPCMP_ERUNTIME;
    }
    ctx->allocs.push_back(p);
    ctx->d_frm_tab = (double *)p;
    ctx->d_frm_stats = (mpcmp_frame_stats *)((char *)p + tab_bytes);
    return MPCMP_OK;
}
// the filter of one call, enqueued on st: the table of the sphere tables in force at q; none for q == NULL or empty tables
static int frame_filter(mpcmp_ctx *ctx, const double *q, double pad, hipStream_t st, FrmFilter *flt) {
    const ClrTables t = clearance_tables(ctx);
    flt->d_tab = ctx->d_frm_tab; flt->ns = 0;
    if (!q || t.n_sph[0] + t.n_sph[1] < 1) return MPCMP_OK;
    FrmPosture P = {};
    for (int j = 0; j < 7 * ctx->narm; j++) P.q[j] = q[j];
    HIPCHK(ctx, frame_spheres_launch(t, P, pad, ctx->d_frm_tab, st));
    flt->ns = t.n_sph[0] + t.n_sph[1];
    return MPCMP_OK;
}
// filter, mark, build: the device half of the four marking setters.  d_stats == NULL: the context's record
static int frame_mark_enqueue(mpcmp_ctx *ctx, const FldArrays &f, int src, int n, const void *d_src, const mpcmp_camera *cam, const double *q, double pad,
                              int flags, mpcmp_frame_stats *d_stats, hipStream_t st) {
    FrmFilter flt;
    if (int rc = frame_filter(ctx, q, pad, st, &flt)) return rc;
    HIPCHK(ctx, frame_mark_launch(f, src, n, d_src, cam, flt, (flags & MPCMP_FRAME_KEEP) != 0, d_stats ? d_stats : ctx->d_frm_stats, st));
    HIPCHK(ctx, field_build_launch(f, st));
    return MPCMP_OK;
}
// host variant: everything is waited for, the data go through the staging scratch
static int frame_mark_host(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int src, int n, const void *data, size_t bytes, const mpcmp_camera *cam,
                           const double *q, double pad, int flags, mpcmp_frame_stats *stats) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (int rc = frame_reserve(ctx)) return rc;
    if (int rc = field_reserve(ctx, *desc)) return rc;
    const FldArrays f = field_arrays(ctx, *desc);
    ctx->fld_set = false;
    Stage sg(ctx);
    unsigned char *dd = nullptr;
    mpcmp_frame_stats *ds = nullptr;
    if (n > 0) sg.in(&dd, static_cast<const unsigned char *>(data), bytes);
    if (stats) sg.out(&ds, stats, 1);
    if (int rc = sg.upload()) return rc;
    if (int rc = frame_mark_enqueue(ctx, f, src, n, dd, cam, q, pad, flags, ds, ctx->stream)) return rc;
    if (int rc = sg.finish()) return rc;
    ctx->fld_desc = *desc; ctx->fld_set = true;
    return MPCMP_OK;
}
static int frame_mark_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int src, int n, const void *d_data, const mpcmp_camera *cam, const double *q,
                             double pad, int flags, mpcmp_frame_stats *d_stats, void *hip_stream) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = frame_reserve(ctx)) return rc;
    if (int rc = field_reserve(ctx, *desc)) return rc;
    const FldArrays f = field_arrays(ctx, *desc);
    ctx->fld_set = false;
    if (int rc = with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int {
            return frame_mark_enqueue(ctx, f, src, n, d_data, cam, q, pad, flags, d_stats, st);
        })) return rc;
    ctx->fld_desc = *desc; ctx->fld_set = true;
    return MPCMP_OK;
}

extern "C" int mpcmp_set_field_points_filtered(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *points, const double *q,
                                               double pad, int flags, mpcmp_frame_stats *stats) {
    if (int rc = frame_check(ctx, "mpcmp_set_field_points_filtered", desc, n_points >= 0 && (n_points == 0 || points), q, pad, flags)) return rc;
    return frame_mark_host(ctx, desc, FRM_SRC_POINTS, n_points, points, sizeof(double) * 3 * (size_t)n_points, nullptr, q, pad, flags, stats);
}

extern "C" int mpcmp_set_field_points_filtered_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, int n_points, const double *d_points,
                                                      const double *q, double pad, int flags, mpcmp_frame_stats *d_stats, void *hip_stream) {
    if (int rc = frame_check(ctx, "mpcmp_set_field_points_filtered_device", desc, n_points >= 0 && (n_points == 0 || d_points), q, pad, flags)) return rc;
    return frame_mark_device(ctx, desc, FRM_SRC_POINTS, n_points, d_points, nullptr, q, pad, flags, d_stats, hip_stream);
}

static bool depth_args_ok(const mpcmp_camera *cam, const void *depth, int depth_type) {
    return cam && depth && frm_camera_ok(*cam) && (depth_type == MPCMP_DEPTH_U16 || depth_type == MPCMP_DEPTH_F32);
}

extern "C" int mpcmp_set_field_depth(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const mpcmp_camera *cam, const void *depth, int depth_type,
                                     const double *q, double pad, int flags, mpcmp_frame_stats *stats) {
    if (int rc = frame_check(ctx, "mpcmp_set_field_depth (a valid camera, an image and a known depth_type are data)", desc,
                             depth_args_ok(cam, depth, depth_type), q, pad, flags)) return rc;
    const int n = cam->width * cam->height;
    return frame_mark_host(ctx, desc, depth_type == MPCMP_DEPTH_U16 ? FRM_SRC_U16 : FRM_SRC_F32, n, depth,
                           (size_t)n * (depth_type == MPCMP_DEPTH_U16 ? 2 : 4), cam, q, pad, flags, stats);
}

extern "C" int mpcmp_set_field_depth_device(mpcmp_ctx *ctx, const mpcmp_field_desc *desc, const mpcmp_camera *cam, const void *d_depth, int depth_type,
                                            const double *q, double pad, int flags, mpcmp_frame_stats *d_stats, void *hip_stream) {
    if (int rc = frame_check(ctx, "mpcmp_set_field_depth_device (a valid camera, an image and a known depth_type are data)", desc,
                             depth_args_ok(cam, d_depth, depth_type), q, pad, flags)) return rc;
    return frame_mark_device(ctx, desc, depth_type == MPCMP_DEPTH_U16 ? FRM_SRC_U16 : FRM_SRC_F32, cam->width * cam->height, d_depth, cam, q, pad, flags,
                             d_stats, hip_stream);
}

static int frame_carve_check(mpcmp_ctx *ctx, const double *q, double pad) {
    if (!ctx) { g_err = "mpcmp_field_carve: no context"; return MPCMP_EINVAL; }
    if (!ctx->fld_set) { ctx->err = "mpcmp_field_carve: no field is set: see mpcmp_set_field"; return MPCMP_EINVAL; }
    return frame_check(ctx, "mpcmp_field_carve", &ctx->fld_desc, true, q, pad, 0);
}
static int frame_carve_enqueue(mpcmp_ctx *ctx, const FldArrays &f, const double *q, double pad, mpcmp_frame_stats *d_stats, hipStream_t st) {
    FrmFilter flt;
    if (int rc = frame_filter(ctx, q, pad, st, &flt)) return rc;
    HIPCHK(ctx, frame_carve_launch(f, flt, d_stats ? d_stats : ctx->d_frm_stats, st));
    HIPCHK(ctx, field_build_launch(f, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_field_carve(mpcmp_ctx *ctx, const double *q, double pad, mpcmp_frame_stats *stats) {
    if (int rc = frame_carve_check(ctx, q, pad)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    if (int rc = frame_reserve(ctx)) return rc;
    const FldArrays f = field_arrays(ctx, ctx->fld_desc);
    Stage sg(ctx);
    mpcmp_frame_stats *ds = nullptr;
    if (stats) sg.out(&ds, stats, 1);
    if (int rc = sg.upload()) return rc;
    if (int rc = frame_carve_enqueue(ctx, f, q, pad, ds, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_field_carve_device(mpcmp_ctx *ctx, const double *q, double pad, mpcmp_frame_stats *d_stats, void *hip_stream) {
    if (int rc = frame_carve_check(ctx, q, pad)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (int rc = frame_reserve(ctx)) return rc;
    const FldArrays f = field_arrays(ctx, ctx->fld_desc);
    return with_caller_stream(ctx, hip_stream, [&](hipStream_t st) -> int { return frame_carve_enqueue(ctx, f, q, pad, d_stats, st); });
}

// ---- certified clearance against the voxel world (include/mpcmp_field_cert.h; the kernels are in field_cert.hip, the rule in field_cert_rule.hpp) ----
static int clearance_cert_field_check(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, double margin, int n_start, int max_depth,
                                      const mpcmp_clearance *out) {
    if (!ctx) { g_err = "mpcmp_clearance_certified_field_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !sx || !sT || !out || !std::isfinite(margin) || n_start < 1 || n_start > MPCMP_CLR_CERT_CAPACITY ||
        ctx->nseg * n_start > MPCMP_CLR_CERT_CAPACITY || max_depth < 0 || max_depth > 16) {
        ctx->err = "mpcmp_clearance_certified_field_batch: B >= 1, n_start >= 1 with num_seg n_start <= 4096, max_depth in [0, 16], a finite margin "
                   "and all pointers (but cert) required";
        return MPCMP_EINVAL;
    }
    if (!ctx->fld_set) { ctx->err = "mpcmp_clearance_certified_field_batch: no field is set: see mpcmp_set_field"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_certified_field_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_sT, double margin, int n_start,
                                                            int max_depth, mpcmp_clearance *d_out, mpcmp_clearance_cert *d_cert, void *hip_stream) {
    if (int rc = clearance_cert_field_check(ctx, B, d_sx, d_sT, margin, n_start, max_depth, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const ClrTables t = clearance_tables(ctx);      // (the obstacle sets are not read)
    if (!ctx->fld_cert_ready) { HIPCHK(ctx, field_cert_prepare()); ctx->fld_cert_ready = true; }
    HIPCHK(ctx, clearance_cert_field_launch(t, field_arrays(ctx, ctx->fld_desc), B, d_sx, d_sT, margin, n_start, max_depth, d_out, d_cert,
                                            (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_certified_field_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *sT, double margin, int n_start,
                                                     int max_depth, mpcmp_clearance *out, mpcmp_clearance_cert *cert) {
    if (int rc = clearance_cert_field_check(ctx, B, sx, sT, margin, n_start, max_depth, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dx, *dT;
    mpcmp_clearance *dout;
    mpcmp_clearance_cert *dcert = nullptr;
    sg.in(&dx, sx, (size_t)ctx->nx * ctx->N * B); sg.in(&dT, sT, B); sg.out(&dout, out, B);
    if (cert) sg.out(&dcert, cert, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_clearance_certified_field_batch_device(ctx, B, dx, dT, margin, n_start, max_depth, dout, dcert, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_clearance_cert_merge_batch_device(mpcmp_ctx *ctx, int B, const mpcmp_clearance_cert *d_a, const mpcmp_clearance_cert *d_b,
                                                       mpcmp_clearance_cert *d_out, void *hip_stream) {
    if (!ctx) { g_err = "mpcmp_clearance_cert_merge_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !d_a || !d_b || !d_out) { ctx->err = "mpcmp_clearance_cert_merge_batch: B >= 1 and a, b and out required"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, clearance_cert_merge_launch(B, d_a, d_b, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_clearance_cert_merge_batch(mpcmp_ctx *ctx, int B, const mpcmp_clearance_cert *a, const mpcmp_clearance_cert *b,
                                                mpcmp_clearance_cert *out) {
    if (!ctx) { g_err = "mpcmp_clearance_cert_merge_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || !a || !b || !out) { ctx->err = "mpcmp_clearance_cert_merge_batch: B >= 1 and a, b and out required"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    mpcmp_clearance_cert *da, *db, *dout;
    sg.in(&da, a, B); sg.in(&db, b, B); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, clearance_cert_merge_launch(B, da, db, dout, ctx->stream));
    return sg.finish();
}

// `who`: the entry point's name; clr is required by mpcmp_select_clear_batch only
static int select_check(mpcmp_ctx *ctx, const char *who, bool need_clr, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                        const int *group, int n_groups, const int *chosen) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    if (B < 1 || n_groups < 0 || n_groups > ctx->max_batch || !sT || !info || (need_clr && !clr) || !group || (n_groups > 0 && !chosen)) {
        ctx->err = std::string(who) + ": B >= 1, n_groups in [0, max_batch] and all pointers required"; return MPCMP_EINVAL;
    }
    if (B > ctx->max_batch) { ctx->err = "batch exceeds the context capacity"; return MPCMP_ETOOBIG; }
    if (!ctx->d_sel_key) {            // first use
        HIPCHK(ctx, hipSetDevice(ctx->device));
        if (int rc = dalloc(ctx, &ctx->d_sel_key, (size_t)ctx->max_batch)) return rc;
    }
    return MPCMP_OK;
}

static int select_device(mpcmp_ctx *ctx, const char *who, bool need_clr, int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                         const mpcmp_limits *d_lim, int lim_mask, const int *d_group, int n_groups, int *d_chosen, void *hip_stream) {
    if (int rc = select_check(ctx, who, need_clr, B, d_sT, d_info, d_clr, d_group, n_groups, d_chosen)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, select_launch(B, d_sT, d_info, d_clr, d_lim, lim_mask, d_group, n_groups, ctx->d_sel_key, d_chosen, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

static int select_host(mpcmp_ctx *ctx, const char *who, bool need_clr, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                       const mpcmp_limits *lim, int lim_mask, const int *group, int n_groups, int *chosen) {
    if (int rc = select_check(ctx, who, need_clr, B, sT, info, clr, group, n_groups, chosen)) return rc;
    for (int i = 0; i < B; i++)
        if (group[i] < -1 || group[i] >= n_groups) {
            ctx->err = std::string(who) + ": group[" + std::to_string(i) + "] must be -1 or in [0, n_groups)"; return MPCMP_EINVAL;
        }
    if (n_groups == 0) return MPCMP_OK;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dT;
    mpcmp_info *di;
    mpcmp_clearance *dc;
    mpcmp_limits *dl;
    int *dg, *dch;
    sg.in(&dT, sT, B); sg.in(&di, info, B); sg.in(&dc, clr, B); sg.in(&dl, lim, B); sg.in(&dg, group, B); sg.out(&dch, chosen, n_groups);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, select_launch(B, dT, di, dc, dl, lim_mask, dg, n_groups, ctx->d_sel_key, dch, ctx->stream));
    return sg.finish();
}

extern "C" int mpcmp_select_clear_batch_device(mpcmp_ctx *ctx, int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                                               const int *d_group, int n_groups, int *d_chosen, void *hip_stream) {
    return select_device(ctx, "mpcmp_select_clear_batch", true, B, d_sT, d_info, d_clr, nullptr, 0, d_group, n_groups, d_chosen, hip_stream);
}

extern "C" int mpcmp_select_clear_batch(mpcmp_ctx *ctx, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr, const int *group,
                                        int n_groups, int *chosen) {
    return select_host(ctx, "mpcmp_select_clear_batch", true, B, sT, info, clr, nullptr, 0, group, n_groups, chosen);
}

// ------------------------------------------------------------------------------------------------
// limits between the nodes (limits.hpp; the kernel is in limits.hip)
static int limits_check(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_pts, const mpcmp_limits_spec *spec,
                        const mpcmp_limits *out) {
    if (!ctx) { g_err = "mpcmp_limits_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || B > ctx->max_batch || n_pts < 1 || n_pts > LIM_MAX_PTS || !sx || !su || !sT || !out) {
        ctx->err = "mpcmp_limits_batch: B in [1, max_batch], 1 <= n_pts <= 4096 and all pointers (but spec) required"; return MPCMP_EINVAL;
    }
    if (spec && !lim_spec_ok(*spec)) { ctx->err = "mpcmp_limits_batch: finite tolerances and tool maxima >= 0 (+inf: none) required"; return MPCMP_EINVAL; }
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    return rows_ok(ctx, B, PAYLOAD_ROWS);
}

static int limits_enqueue(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT, int n_pts, const mpcmp_limits_spec *spec,
                          mpcmp_limits *d_out, hipStream_t st) {
    mpcmp_bounds table;
    mpcmp_bounds_from_config(&ctx->cfg, &table);
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    HIPCHK(ctx, limits_launch(md, ms, ctx->narm, ctx->nseg, B, n_pts, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, table, d_sx, d_su, d_sT,
                              spec ? *spec : lim_default_spec(), d_out, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_limits_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT, int n_pts,
                                         const mpcmp_limits_spec *spec, mpcmp_limits *d_out, void *hip_stream) {
    if (int rc = limits_check(ctx, B, d_sx, d_su, d_sT, n_pts, spec, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return limits_enqueue(ctx, B, d_sx, d_su, d_sT, n_pts, spec, d_out, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_limits_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_pts,
                                  const mpcmp_limits_spec *spec, mpcmp_limits *out) {
    if (int rc = limits_check(ctx, B, sx, su, sT, n_pts, spec, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t NB = (size_t)ctx->N * B;
    Stage sg(ctx);
    double *dx, *du, *dT;
    mpcmp_limits *dout;
    sg.in(&dx, sx, ctx->nx * NB); sg.in(&du, su, ctx->nu * NB); sg.in(&dT, sT, B); sg.out(&dout, out, B);
    if (int rc = sg.upload()) return rc;
    if (int rc = limits_enqueue(ctx, B, dx, du, dT, n_pts, spec, dout, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_select_checked_batch_device(mpcmp_ctx *ctx, int B, const double *d_sT, const mpcmp_info *d_info, const mpcmp_clearance *d_clr,
                                                 const mpcmp_limits *d_lim, int lim_mask, const int *d_group, int n_groups, int *d_chosen,
                                                 void *hip_stream) {
    return select_device(ctx, "mpcmp_select_checked_batch", false, B, d_sT, d_info, d_clr, d_lim, lim_mask, d_group, n_groups, d_chosen, hip_stream);
}

extern "C" int mpcmp_select_checked_batch(mpcmp_ctx *ctx, int B, const double *sT, const mpcmp_info *info, const mpcmp_clearance *clr,
                                          const mpcmp_limits *lim, int lim_mask, const int *group, int n_groups, int *chosen) {
    return select_host(ctx, "mpcmp_select_checked_batch", false, B, sT, info, clr, lim, lim_mask, group, n_groups, chosen);
}

// ------------------------------------------------------------------------------------------------
// retiming of plans (retime.hpp; the kernels are in retime.hip).  A plan is a route of one leg: after its own checks a plan call goes through the
// enqueue helper of the route call with M = 0
static int retime_check(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_grid, const mpcmp_retime_spec *spec,
                        const double *prof, const mpcmp_retime *out) {
    if (!ctx) { g_err = "mpcmp_retime_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || B > ctx->max_batch || n_grid < 1 || n_grid > RT_MAX_GRID || !sx || !su || !sT || !prof || !out) {
        ctx->err = "mpcmp_retime_batch: B in [1, max_batch], 1 <= n_grid <= 4096 and all pointers (but spec) required"; return MPCMP_EINVAL;
    }
    if (spec && !rt_spec_ok(*spec)) {
        ctx->err = "mpcmp_retime_batch: tool maxima >= 0 (+inf: none), a finite rate_max > 0 and groups within MPCMP_RT_ALL_GROUPS required"; return MPCMP_EINVAL;
    }
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    return rows_ok(ctx, B, PAYLOAD_ROWS);
}

// the records go to d_route_out or, for plans (M = 0), to d_plan_out
static int retime_enqueue(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, int n_grid,
                          const mpcmp_retime_spec *spec, double *d_prof, double *d_legT, mpcmp_retime *d_plan_out, mpcmp_route_retime *d_route_out,
                          hipStream_t st) {
    mpcmp_bounds table;
    mpcmp_bounds_from_config(&ctx->cfg, &table);
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    HIPCHK(ctx, retime_launch(md, ms, ctx->narm, ctx->nseg, B, M, n_grid, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, table, d_sx, d_su, d_sT,
                              spec ? *spec : rt_default_spec(), d_prof, d_legT, d_plan_out, d_route_out, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_retime_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT, int n_grid,
                                         const mpcmp_retime_spec *spec, double *d_prof, mpcmp_retime *d_out, void *hip_stream) {
    if (int rc = retime_check(ctx, B, d_sx, d_su, d_sT, n_grid, spec, d_prof, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return retime_enqueue(ctx, B, 0, d_sx, d_su, d_sT, n_grid, spec, d_prof, nullptr, d_out, nullptr, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_retime_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_grid,
                                  const mpcmp_retime_spec *spec, double *prof, mpcmp_retime *out) {
    if (int rc = retime_check(ctx, B, sx, su, sT, n_grid, spec, prof, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = (size_t)ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *dprof;
    mpcmp_retime *dout;
    sg.in(&dx, sx, ctx->nx * NB); sg.in(&du, su, ctx->nu * NB); sg.in(&dT, sT, nb); sg.out(&dprof, prof, nb * (n_grid + 1) * 2); sg.out(&dout, out, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = retime_enqueue(ctx, B, 0, dx, du, dT, n_grid, spec, dprof, nullptr, dout, nullptr, ctx->stream)) return rc;
    return sg.finish();
}

static int sample_retimed_check(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_grid, const double *prof, int n_pts,
                                const double *out) {
    if (!ctx) { g_err = "mpcmp_sample_retimed_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || B > ctx->max_batch || n_grid < 1 || n_grid > RT_MAX_GRID || n_pts < 1 || !sx || !su || !sT || !prof || !out) {
        ctx->err = "mpcmp_sample_retimed_batch: B in [1, max_batch], 1 <= n_grid <= 4096, n_pts >= 1 and all pointers required"; return MPCMP_EINVAL;
    }
    return rows_ok(ctx, B, PAYLOAD_ROWS);
}

static int sample_retimed_enqueue(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, int n_grid,
                                  const double *d_prof, int n_pts, double *d_out, hipStream_t st) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    HIPCHK(ctx, sample_retimed_launch(md, ms, ctx->narm, ctx->nseg, B, M, n_grid, n_pts, d_sx, d_su, d_sT, d_prof, d_out, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_sample_retimed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT, int n_grid,
                                                 const double *d_prof, int n_pts, double *d_out, void *hip_stream) {
    if (int rc = sample_retimed_check(ctx, B, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, d_out)) return rc;
    return sample_retimed_enqueue(ctx, B, 0, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, d_out, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_sample_retimed_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_grid, const double *prof,
                                          int n_pts, double *out) {
    if (int rc = sample_retimed_check(ctx, B, sx, su, sT, n_grid, prof, n_pts, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = (size_t)ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *dprof, *dout;
    sg.in(&dx, sx, ctx->nx * NB); sg.in(&du, su, ctx->nu * NB); sg.in(&dT, sT, nb); sg.in(&dprof, prof, nb * (n_grid + 1) * 2);
    sg.out(&dout, out, nb * (n_pts + 1) * (1 + 28 * (size_t)ctx->narm));
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_sample_retimed_batch_device(ctx, B, dx, du, dT, n_grid, dprof, n_pts, dout, ctx->stream)) return rc;
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// route retiming (retime.hpp; the kernels are in retime.hip)
static int route_shape_check(mpcmp_ctx *ctx, const char *who, int B, int M, int n_grid, int *L) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    const long long l = (long long)B * ((long long)M + 1);
    if (B < 1 || M < 0 || l > ctx->max_batch || n_grid < 1 || n_grid > RT_MAX_GRID) {
        ctx->err = std::string(who) + ": B >= 1, M >= 0, B (M + 1) leg slots within max_batch and 1 <= n_grid <= 4096 required"; return MPCMP_EINVAL;
    }
    *L = (int)l;
    return MPCMP_OK;
}

static int retime_route_check(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_grid,
                              const mpcmp_retime_spec *spec, const double *prof, const mpcmp_route_retime *out, int *L) {
    if (int rc = route_shape_check(ctx, "mpcmp_retime_route_batch", B, M, n_grid, L)) return rc;
    if (!sx || !su || !sT || !prof || !out) { ctx->err = "mpcmp_retime_route_batch: all pointers (but spec and leg_T_new) required"; return MPCMP_EINVAL; }
    if (spec && !rt_spec_ok(*spec)) {
        ctx->err = "mpcmp_retime_route_batch: tool maxima >= 0 (+inf: none), a finite rate_max > 0 and groups within MPCMP_RT_ALL_GROUPS required"; return MPCMP_EINVAL;
    }
    if (int rc = rows_ok(ctx, *L, BOUND_ROWS)) return rc;
    return rows_ok(ctx, *L, PAYLOAD_ROWS);
}

extern "C" int mpcmp_retime_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, int n_grid,
                                               const mpcmp_retime_spec *spec, double *d_prof, double *d_legT, mpcmp_route_retime *d_out,
                                               void *hip_stream) {
    int L;
    if (int rc = retime_route_check(ctx, B, M, d_sx, d_su, d_sT, n_grid, spec, d_prof, d_out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return retime_enqueue(ctx, B, M, d_sx, d_su, d_sT, n_grid, spec, d_prof, d_legT, nullptr, d_out, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_retime_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_grid,
                                        const mpcmp_retime_spec *spec, double *prof, double *leg_T_new, mpcmp_route_retime *out) {
    int L;
    if (int rc = retime_route_check(ctx, B, M, sx, su, sT, n_grid, spec, prof, out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nl = L, NL = (size_t)ctx->N * nl;
    Stage sg(ctx);
    double *dx, *du, *dT, *dprof, *dleg = nullptr;
    mpcmp_route_retime *dout;
    sg.in(&dx, sx, ctx->nx * NL); sg.in(&du, su, ctx->nu * NL); sg.in(&dT, sT, nl); sg.out(&dprof, prof, nl * (n_grid + 1) * 2);
    if (leg_T_new) sg.out(&dleg, leg_T_new, nl);
    sg.out(&dout, out, (size_t)B);
    if (int rc = sg.upload()) return rc;
    if (int rc = retime_enqueue(ctx, B, M, dx, du, dT, n_grid, spec, dprof, dleg, nullptr, dout, ctx->stream)) return rc;
    return sg.finish();
}

static int sample_retimed_route_check(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_grid,
                                      const double *prof, int n_pts, const double *out, int *L) {
    if (int rc = route_shape_check(ctx, "mpcmp_sample_retimed_route_batch", B, M, n_grid, L)) return rc;
    if (n_pts < 1 || !sx || !su || !sT || !prof || !out) {
        ctx->err = "mpcmp_sample_retimed_route_batch: n_pts >= 1 and all pointers required"; return MPCMP_EINVAL;
    }
    return rows_ok(ctx, *L, PAYLOAD_ROWS);
}

extern "C" int mpcmp_sample_retimed_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT,
                                                       int n_grid, const double *d_prof, int n_pts, double *d_out, void *hip_stream) {
    int L;
    if (int rc = sample_retimed_route_check(ctx, B, M, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, d_out, &L)) return rc;
    return sample_retimed_enqueue(ctx, B, M, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, d_out, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_sample_retimed_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_grid,
                                                const double *prof, int n_pts, double *out) {
    int L;
    if (int rc = sample_retimed_route_check(ctx, B, M, sx, su, sT, n_grid, prof, n_pts, out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nl = L, NL = (size_t)ctx->N * nl;
    Stage sg(ctx);
    double *dx, *du, *dT, *dprof, *dout;
    sg.in(&dx, sx, ctx->nx * NL); sg.in(&du, su, ctx->nu * NL); sg.in(&dT, sT, nl); sg.in(&dprof, prof, nl * (n_grid + 1) * 2);
    sg.out(&dout, out, (size_t)B * (n_pts + 1) * (1 + 28 * (size_t)ctx->narm));
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_sample_retimed_route_batch_device(ctx, B, M, dx, du, dT, n_grid, dprof, n_pts, dout, ctx->stream)) return rc;
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// limits of retimed plans and routes, profile scaling (retimed_check.hpp; the kernels are in retimed_check.hip)
static int limits_retimed_check(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_grid, const double *prof, int n_pts,
                                const mpcmp_limits_spec *spec, const mpcmp_limits *out) {
    if (!ctx) { g_err = "mpcmp_limits_retimed_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || B > ctx->max_batch || n_grid < 1 || n_grid > RT_MAX_GRID || n_pts < 1 || n_pts > LIM_MAX_PTS || !sx || !su || !sT || !prof || !out) {
        ctx->err = "mpcmp_limits_retimed_batch: B in [1, max_batch], 1 <= n_grid <= 4096, 1 <= n_pts <= 4096 and all pointers (but spec and T_new) required";
        return MPCMP_EINVAL;
    }
    if (spec && !lim_spec_ok(*spec)) { ctx->err = "mpcmp_limits_retimed_batch: finite tolerances and tool maxima >= 0 (+inf: none) required"; return MPCMP_EINVAL; }
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    return rows_ok(ctx, B, PAYLOAD_ROWS);
}

static int limits_retimed_enqueue(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, int n_grid,
                                  const double *d_prof, int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *d_out, double *d_Tnew, hipStream_t st) {
    mpcmp_bounds table;
    mpcmp_bounds_from_config(&ctx->cfg, &table);
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    HIPCHK(ctx, limits_retimed_launch(md, ms, ctx->narm, ctx->nseg, B, M, n_grid, n_pts, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, table, d_sx, d_su,
                                      d_sT, d_prof, spec ? *spec : lim_default_spec(), d_out, d_Tnew, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_limits_retimed_batch_device(mpcmp_ctx *ctx, int B, const double *d_sx, const double *d_su, const double *d_sT, int n_grid,
                                                 const double *d_prof, int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *d_out,
                                                 double *d_Tnew, void *hip_stream) {
    if (int rc = limits_retimed_check(ctx, B, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, spec, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return limits_retimed_enqueue(ctx, B, 0, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, spec, d_out, d_Tnew, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_limits_retimed_batch(mpcmp_ctx *ctx, int B, const double *sx, const double *su, const double *sT, int n_grid, const double *prof,
                                          int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *out, double *T_new) {
    if (int rc = limits_retimed_check(ctx, B, sx, su, sT, n_grid, prof, n_pts, spec, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = (size_t)ctx->N * nb;
    Stage sg(ctx);
    double *dx, *du, *dT, *dprof, *dTn;
    mpcmp_limits *dout;
    sg.in(&dx, sx, ctx->nx * NB); sg.in(&du, su, ctx->nu * NB); sg.in(&dT, sT, nb); sg.in(&dprof, prof, nb * (n_grid + 1) * 2);
    sg.out(&dout, out, nb); sg.out(&dTn, T_new, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = limits_retimed_enqueue(ctx, B, 0, dx, du, dT, n_grid, dprof, n_pts, spec, dout, dTn, ctx->stream)) return rc;
    return sg.finish();
}

static int limits_retimed_route_check(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_grid,
                                      const double *prof, int n_pts, const mpcmp_limits_spec *spec, const mpcmp_limits *out, int *L) {
    if (int rc = route_shape_check(ctx, "mpcmp_limits_retimed_route_batch", B, M, n_grid, L)) return rc;
    if (n_pts < 1 || n_pts > LIM_MAX_PTS || !sx || !su || !sT || !prof || !out) {
        ctx->err = "mpcmp_limits_retimed_route_batch: 1 <= n_pts <= 4096 and all pointers (but spec and T_new) required"; return MPCMP_EINVAL;
    }
    if (spec && !lim_spec_ok(*spec)) {
        ctx->err = "mpcmp_limits_retimed_route_batch: finite tolerances and tool maxima >= 0 (+inf: none) required"; return MPCMP_EINVAL;
    }
    if (int rc = rows_ok(ctx, *L, BOUND_ROWS)) return rc;
    return rows_ok(ctx, *L, PAYLOAD_ROWS);
}

extern "C" int mpcmp_limits_retimed_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT,
                                                       int n_grid, const double *d_prof, int n_pts, const mpcmp_limits_spec *spec,
                                                       mpcmp_limits *d_out, double *d_Tnew, void *hip_stream) {
    int L;
    if (int rc = limits_retimed_route_check(ctx, B, M, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, spec, d_out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return limits_retimed_enqueue(ctx, B, M, d_sx, d_su, d_sT, n_grid, d_prof, n_pts, spec, d_out, d_Tnew, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_limits_retimed_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_grid,
                                                const double *prof, int n_pts, const mpcmp_limits_spec *spec, mpcmp_limits *out, double *T_new) {
    int L;
    if (int rc = limits_retimed_route_check(ctx, B, M, sx, su, sT, n_grid, prof, n_pts, spec, out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nl = L, NL = (size_t)ctx->N * nl;
    Stage sg(ctx);
    double *dx, *du, *dT, *dprof, *dTn;
    mpcmp_limits *dout;
    sg.in(&dx, sx, ctx->nx * NL); sg.in(&du, su, ctx->nu * NL); sg.in(&dT, sT, nl); sg.in(&dprof, prof, nl * (n_grid + 1) * 2);
    sg.out(&dout, out, (size_t)B); sg.out(&dTn, T_new, (size_t)B);
    if (int rc = sg.upload()) return rc;
    if (int rc = limits_retimed_enqueue(ctx, B, M, dx, du, dT, n_grid, dprof, n_pts, spec, dout, dTn, ctx->stream)) return rc;
    return sg.finish();
}

static int profile_scale_check(mpcmp_ctx *ctx, int L, int n_grid, const double *factor, const double *prof) {
    if (!ctx) { g_err = "mpcmp_profile_scale_batch: no context"; return MPCMP_EINVAL; }
    if (L < 1 || L > ctx->max_batch || n_grid < 1 || n_grid > RT_MAX_GRID || !factor || !prof) {
        ctx->err = "mpcmp_profile_scale_batch: L in [1, max_batch], 1 <= n_grid <= 4096 and both pointers required"; return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_profile_scale_batch_device(mpcmp_ctx *ctx, int L, int n_grid, const double *d_factor, double *d_prof, void *hip_stream) {
    if (int rc = profile_scale_check(ctx, L, n_grid, d_factor, d_prof)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, profile_scale_launch(L, n_grid, d_factor, d_prof, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_profile_scale_batch(mpcmp_ctx *ctx, int L, int n_grid, const double *factor, double *prof) {
    if (int rc = profile_scale_check(ctx, L, n_grid, factor, prof)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *df, *dprof;
    sg.in(&df, factor, (size_t)L); sg.inout(&dprof, prof, (size_t)L * (n_grid + 1) * 2);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, profile_scale_launch(L, n_grid, df, dprof, ctx->stream));
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// tool-line moves (toolpath.hpp; the kernels are in toolpath.hip, the single-problem host statements in model_host.cpp)
static int tool_line_check(mpcmp_ctx *ctx, int B, int arm, const double *q, const double *R1, const double *p1, const double *Tin,
                           const mpcmp_tool_line_spec *spec, const double *sx, const double *su, const double *sT) {
    if (!ctx) { g_err = "mpcmp_tool_line_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || B > ctx->max_batch) { ctx->err = "mpcmp_tool_line_batch: B must be in [1, max_batch]"; return MPCMP_EINVAL; }
    if (arm < 0 || arm >= ctx->narm) { ctx->err = "mpcmp_tool_line_batch: arm must be in [0, narm)"; return MPCMP_EINVAL; }
    if (!q || !R1 || !p1 || !sx || !su || !sT) { ctx->err = "mpcmp_tool_line_batch: q_start, R1, p1, sol_x, sol_u and sol_T are required"; return MPCMP_EINVAL; }
    if (ctx->narm > 1 && !Tin) { ctx->err = "mpcmp_tool_line_batch: a multi-arm plan needs T_in (the arms share T)"; return MPCMP_EINVAL; }
    if (spec && !mpcmp_tl::tl_spec_ok(*spec)) {
        ctx->err = "mpcmp_tool_line_batch: spec values finite and > 0 (the tool maxima may be +inf), n_sub in [1, 64] required"; return MPCMP_EINVAL;
    }
    return rows_ok(ctx, B, BOUND_ROWS);
}

extern "C" int mpcmp_tool_line_batch_device(mpcmp_ctx *ctx, int B, int arm, const double *d_q, const double *d_R1, const double *d_p1, const double *d_Tin,
                                            const mpcmp_tool_line_spec *spec, double *d_sx, double *d_su, double *d_sT, mpcmp_tool_line *d_out,
                                            void *hip_stream) {
    if (int rc = tool_line_check(ctx, B, arm, d_q, d_R1, d_p1, d_Tin, spec, d_sx, d_su, d_sT)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    mpcmp_bounds table;
    mpcmp_bounds_from_config(&ctx->cfg, &table);
    HIPCHK(ctx, mpcmp_tl::tool_line_launch(ctx->d_model + arm, ctx->nseg, B, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, table, ctx->nx, ctx->nu, 7 * arm,
                                           7 * ctx->narm + 7 * arm, 7 * arm, d_q, d_R1, d_p1, d_Tin, spec ? *spec : mpcmp_tl::tl_default_spec(), d_sx,
                                           d_su, d_sT, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_tool_line_batch(mpcmp_ctx *ctx, int B, int arm, const double *q, const double *R1, const double *p1, const double *Tin,
                                     const mpcmp_tool_line_spec *spec, double *sx, double *su, double *sT, mpcmp_tool_line *out) {
    if (int rc = tool_line_check(ctx, B, arm, q, R1, p1, Tin, spec, sx, su, sT)) return rc;
    const mpcmp_model *models = ctx->narm == 1 ? &ctx->model : nullptr;
    std::vector<mpcmp_model> hm;
    if (!models) {                              // (the host copy of the context holds arm 0 only)
        hm.resize(ctx->narm);
        HIPCHK(ctx, hipSetDevice(ctx->device));
        HIPCHK(ctx, hipMemcpy(hm.data(), ctx->d_model, sizeof(mpcmp_model) * ctx->narm, hipMemcpyDeviceToHost));
        models = hm.data();
    }
    for (int b = 0; b < B; b++)
        if (const char *why = mpcmp_tl::tl_check_problem(models[ctx->narm == 1 ? 0 : arm], q + 7 * (size_t)b, R1 + 9 * (size_t)b, p1 + 3 * (size_t)b, Tin ? Tin[b] : 0.0)) {
            ctx->err = "mpcmp_tool_line_batch: problem " + std::to_string(b) + ": " + why;
            return MPCMP_EINVAL;
        }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B, NB = (size_t)ctx->N * nb;
    Stage sg(ctx);
    double *dq, *dR, *dp, *dTi, *dx, *du, *dT;
    mpcmp_tool_line *dout;
    sg.in(&dq, q, 7 * nb); sg.in(&dR, R1, 9 * nb); sg.in(&dp, p1, 3 * nb); sg.in(&dTi, Tin, nb);
    if (ctx->narm > 1) { sg.inout(&dx, sx, ctx->nx * NB); sg.inout(&du, su, ctx->nu * NB); }      // the other arm's columns come back as they were
    else { sg.out(&dx, sx, ctx->nx * NB); sg.out(&du, su, ctx->nu * NB); }
    sg.out(&dT, sT, nb); sg.out(&dout, out, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_tool_line_batch_device(ctx, B, arm, dq, dR, dp, dTi, spec, dx, du, dT, dout, ctx->stream)) return rc;
    return sg.finish();
}

static int tool_deviation_check(mpcmp_ctx *ctx, int B, int arm, const double *sx, const double *R1, const double *p1, int n_pts, double tol_lin,
                                double tol_ang, const mpcmp_tool_dev *out) {
    if (!ctx) { g_err = "mpcmp_tool_deviation_batch: no context"; return MPCMP_EINVAL; }
    if (B < 1 || B > ctx->max_batch || arm < 0 || arm >= ctx->narm || n_pts < 1 || n_pts > mpcmp_tl::TD_MAX_PTS || !sx || !R1 || !p1 || !out ||
        !(tol_lin >= 0.0) || !(tol_ang >= 0.0)) {
        ctx->err = "mpcmp_tool_deviation_batch: B in [1, max_batch], arm in [0, narm), n_pts in [1, 65536], tolerances >= 0 and all pointers required";
        return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_tool_deviation_batch_device(mpcmp_ctx *ctx, int B, int arm, const double *d_sx, const double *d_R1, const double *d_p1, int n_pts,
                                                 double tol_lin, double tol_ang, mpcmp_tool_dev *d_out, void *hip_stream) {
    if (int rc = tool_deviation_check(ctx, B, arm, d_sx, d_R1, d_p1, n_pts, tol_lin, tol_ang, d_out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, mpcmp_tl::tool_deviation_launch(ctx->d_model + arm, ctx->nseg, B, ctx->nx, 7 * arm, d_sx, d_R1, d_p1, n_pts, tol_lin, tol_ang, d_out,
                                                (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_tool_deviation_batch(mpcmp_ctx *ctx, int B, int arm, const double *sx, const double *R1, const double *p1, int n_pts, double tol_lin,
                                          double tol_ang, mpcmp_tool_dev *out) {
    if (int rc = tool_deviation_check(ctx, B, arm, sx, R1, p1, n_pts, tol_lin, tol_ang, out)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nb = B;
    Stage sg(ctx);
    double *dx, *dR, *dp;
    mpcmp_tool_dev *dout;
    sg.in(&dx, sx, ctx->nx * (size_t)ctx->N * nb); sg.in(&dR, R1, 9 * nb); sg.in(&dp, p1, 3 * nb); sg.out(&dout, out, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_tool_deviation_batch_device(ctx, B, arm, dx, dR, dp, n_pts, tol_lin, tol_ang, dout, ctx->stream)) return rc;
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// via-point routes (route.hpp, route.hip): B routes with M vias = L = B (M + 1) leg slots
// the checks every route entry point shares; *L = the number of leg slots
static int route_check(mpcmp_ctx *ctx, const char *who, int B, int M, int *L) {
    if (!ctx) { g_err = std::string(who) + ": no context"; return MPCMP_EINVAL; }
    if (ctx->rh_B > 0) { ctx->err = std::string(who) + ": not available after mpcmp_rh_init (the receding-horizon driver plans single moves)"; return MPCMP_EINVAL; }
    if (B < 1 || M < 0) { ctx->err = std::string(who) + ": B >= 1 and M >= 0 required"; return MPCMP_EINVAL; }
    const long long l = (long long)B * ((long long)M + 1);
    if (l > ctx->max_batch) {
        ctx->err = std::string(who) + ": " + std::to_string(l) + " leg slots (B (M + 1)) exceed the context capacity (" + std::to_string(ctx->max_batch) + ")";
        return MPCMP_EINVAL;
    }
    *L = (int)l;
    return MPCMP_OK;
}
// the host-pointer variants' look at their values: finite states and vias, speed in [0, 1]
static int route_values_ok(mpcmp_ctx *ctx, const char *who, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed,
                           const double *xf) {
    const size_t nx = ctx->nx, nv = (size_t)B * M * (nx / 2);
    auto finite = [](const double *p, size_t n) { for (size_t i = 0; i < n; i++) if (!std::isfinite(p[i])) return false; return true; };
    if (!finite(x0, nx * B) || !finite(xf, nx * B) || (M > 0 && !finite(via, nv)) || (M > 0 && via_qd && !finite(via_qd, nv))) {
        ctx->err = std::string(who) + ": x0, xf, via and via_qd must be finite"; return MPCMP_EINVAL;
    }
    if (speed)
        for (int b = 0; b < B; b++)
            if (!(speed[b] >= 0.0 && speed[b] <= 1.0)) { ctx->err = std::string(who) + ": speed[" + std::to_string(b) + "] must lie in [0, 1]"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}
static int route_legs_enqueue(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                              const double *d_xf, double *d_l0, double *d_lf, double *d_vout, hipStream_t st) {
    mpcmp_bounds row;
    mpcmp_bounds_from_config(&ctx->cfg, &row);
    HIPCHK(ctx, route_legs_launch(B, M, ctx->narm, d_x0, d_via, d_vqd, d_speed, d_xf, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, row, d_l0, d_lf, d_vout, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_route_legs_device(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                                       const double *d_xf, double *d_l0, double *d_lf, double *d_vout, void *hip_stream) {
    int L;
    if (int rc = route_check(ctx, "mpcmp_route_legs", B, M, &L)) return rc;
    if (!d_x0 || !d_xf || !d_l0 || !d_lf || (M > 0 && !d_via)) { ctx->err = "mpcmp_route_legs: x0, xf, leg_x0, leg_xf (and via with M > 0) are required"; return MPCMP_EINVAL; }
    if (int rc = rows_ok(ctx, L, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return route_legs_enqueue(ctx, B, M, d_x0, d_via, d_vqd, d_speed, d_xf, d_l0, d_lf, d_vout, (hipStream_t)hip_stream);
}

extern "C" int mpcmp_route_legs(mpcmp_ctx *ctx, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed,
                                const double *xf, double *leg_x0, double *leg_xf, double *via_qd_out) {
    int L;
    if (int rc = route_check(ctx, "mpcmp_route_legs", B, M, &L)) return rc;
    if (!x0 || !xf || !leg_x0 || !leg_xf || (M > 0 && !via)) { ctx->err = "mpcmp_route_legs: x0, xf, leg_x0, leg_xf (and via with M > 0) are required"; return MPCMP_EINVAL; }
    if (int rc = route_values_ok(ctx, "mpcmp_route_legs", B, M, x0, via, via_qd, speed, xf)) return rc;
    if (int rc = rows_ok(ctx, L, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nx = ctx->nx, nv = (size_t)B * M * (nx / 2);
    Stage sg(ctx);
    double *d0, *df, *dv, *dq, *ds, *dl0, *dlf, *dvo;
    sg.in(&d0, x0, nx * B); sg.in(&df, xf, nx * B); sg.in(&dv, M > 0 ? via : nullptr, nv); sg.in(&dq, M > 0 ? via_qd : nullptr, nv); sg.in(&ds, speed, B);
    sg.out(&dl0, leg_x0, nx * L); sg.out(&dlf, leg_xf, nx * L); sg.out(&dvo, M > 0 ? via_qd_out : nullptr, nv);
    if (int rc = sg.upload()) return rc;
    if (int rc = route_legs_enqueue(ctx, B, M, d0, dv, dq, ds, df, dl0, dlf, dvo, ctx->stream)) return rc;
    return sg.finish();
}

static int route_join_check(mpcmp_ctx *ctx, int B, int M, const void *sx, const void *su, const void *sT, const void *info, const void *clr, const void *rT,
                            const void *rinfo, const void *seam, const void *rclr, int *L) {
    if (int rc = route_check(ctx, "mpcmp_route_join", B, M, L)) return rc;
    if (!sx || !su || !sT || !info || !rT || !rinfo || !seam || ((clr != nullptr) != (rclr != nullptr))) {
        ctx->err = "mpcmp_route_join: sol_x, sol_u, sol_T, info, route_T, route_info and seam are required; clr and route_clr both or neither"; return MPCMP_EINVAL;
    }
    return MPCMP_OK;
}

extern "C" int mpcmp_route_join_device(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, const mpcmp_info *d_info,
                                       const mpcmp_clearance *d_clr, double *d_rT, mpcmp_info *d_rinfo, mpcmp_route_seam *d_seam, mpcmp_clearance *d_rclr,
                                       void *hip_stream) {
    int L;
    if (int rc = route_join_check(ctx, B, M, d_sx, d_su, d_sT, d_info, d_clr, d_rT, d_rinfo, d_seam, d_rclr, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, route_join_launch(B, M, ctx->N, ctx->narm, d_sx, d_su, d_sT, d_info, d_clr, d_rT, d_rinfo, d_seam, d_rclr, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_route_join(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, const mpcmp_info *info,
                                const mpcmp_clearance *clr, double *rT, mpcmp_info *rinfo, mpcmp_route_seam *seam, mpcmp_clearance *rclr) {
    int L;
    if (int rc = route_join_check(ctx, B, M, sx, su, sT, info, clr, rT, rinfo, seam, rclr, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t NL = (size_t)ctx->N * L;
    Stage sg(ctx);
    double *dx, *du, *dT, *drT;
    mpcmp_info *di, *dri;
    mpcmp_clearance *dc, *drc;         // (clr and rclr: both given or neither, route_join_check)
    mpcmp_route_seam *ds;
    sg.in(&dx, sx, ctx->nx * NL); sg.in(&du, su, ctx->nu * NL); sg.in(&dT, sT, L); sg.in(&di, info, L); sg.in(&dc, clr, L);
    sg.out(&drT, rT, B); sg.out(&dri, rinfo, B); sg.out(&ds, seam, B); sg.out(&drc, rclr, B);
    if (int rc = sg.upload()) return rc;
    HIPCHK(ctx, route_join_launch(B, M, ctx->N, ctx->narm, dx, du, dT, di, dc, drT, dri, ds, drc, ctx->stream));
    return sg.finish();
}

// everything a route solve is refused for, and its scratch (first call only)
static int route_solve_check(mpcmp_ctx *ctx, int B, int M, const void *x0, const void *via, const void *xf, const double *jmax, const void *sx, const void *su,
                             const void *sT, const void *rT, const void *rinfo, const void *seam, int *L) {
    if (int rc = route_check(ctx, "mpcmp_solve_route_batch", B, M, L)) return rc;
    if (!x0 || !xf || (M > 0 && !via) || !sx || !su || !sT || !rT || !rinfo || !seam) {
        ctx->err = "mpcmp_solve_route_batch: x0, xf (and via with M > 0), sol_x, sol_u, sol_T, route_T, route_info and seam are required"; return MPCMP_EINVAL;
    }
    if (int rc = solve_rows_ok(ctx, *L)) return rc;
    if (ctx->narm == 2 && !jmax) { ctx->err = "mpcmp_solve_route_batch: multi-arm solves need the jerk-limited start guess (jmax)"; return MPCMP_EINVAL; }
    if (jmax) { JerkLimits lim; if (int rc = jerk_limits(ctx, nullptr, nullptr, jmax, lim)) return rc; }
    if (!ctx->d_rt_x0) {              // first use
        HIPCHK(ctx, hipSetDevice(ctx->device));
        const size_t Mx = ctx->max_batch, N = ctx->N, nx = ctx->nx, nu = ctx->nu;
        if (int rc = dalloc(ctx, &ctx->d_rt_xf, Mx * nx)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_wx, Mx * nx * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_wu, Mx * nu * N)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_wT, Mx)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_info, Mx)) return rc;
        if (int rc = dalloc(ctx, &ctx->d_rt_x0, Mx * nx)) return rc;      // (last: the mark of a complete scratch)
    }
    return MPCMP_OK;
}

// leg builder, start guess, one solve of the L legs, join: all on st, no host round trip
static int route_solve_enqueue(mpcmp_ctx *ctx, int B, int M, int L, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                               const double *d_xf, const double *jmax, double *d_sx, double *d_su, double *d_sT, mpcmp_info *d_info, double *d_rT,
                               mpcmp_info *d_rinfo, mpcmp_route_seam *d_seam, double *d_vout, hipStream_t st) {
    if (int rc = route_legs_enqueue(ctx, B, M, d_x0, d_via, d_vqd, d_speed, d_xf, ctx->d_rt_x0, ctx->d_rt_xf, d_vout, st)) return rc;
    SolveCall c;
    c.B = L; c.x0 = ctx->d_rt_x0; c.xf = ctx->d_rt_xf;
    if (jmax) {
        if (int rc = mpcmp_warm_start_jerk_batch_device(ctx, L, ctx->d_rt_x0, ctx->d_rt_xf, jmax, ctx->d_rt_wx, ctx->d_rt_wu, ctx->d_rt_wT, st)) return rc;
        c.wx = ctx->d_rt_wx; c.wu = ctx->d_rt_wu; c.wT = ctx->d_rt_wT;
    }
    c.sx = d_sx; c.su = d_su; c.sT = d_sT; c.info = d_info ? d_info : ctx->d_rt_info; c.stream = st;
    if (int rc = solve_dispatch(ctx, c)) return rc;
    HIPCHK(ctx, route_join_launch(B, M, ctx->N, ctx->narm, d_sx, d_su, d_sT, c.info, nullptr, d_rT, d_rinfo, d_seam, nullptr, st));
    return MPCMP_OK;
}

extern "C" int mpcmp_solve_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_x0, const double *d_via, const double *d_vqd, const double *d_speed,
                                              const double *d_xf, const double *jmax, double *d_sx, double *d_su, double *d_sT, mpcmp_info *d_info,
                                              double *d_rT, mpcmp_info *d_rinfo, mpcmp_route_seam *d_seam, double *d_vout, void *hip_stream) {
    int L;
    if (int rc = route_solve_check(ctx, B, M, d_x0, d_via, d_xf, jmax, d_sx, d_su, d_sT, d_rT, d_rinfo, d_seam, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return route_solve_enqueue(ctx, B, M, L, d_x0, d_via, d_vqd, d_speed, d_xf, jmax, d_sx, d_su, d_sT, d_info, d_rT, d_rinfo, d_seam, d_vout,
                               (hipStream_t)hip_stream);
}

extern "C" int mpcmp_solve_route_batch(mpcmp_ctx *ctx, int B, int M, const double *x0, const double *via, const double *via_qd, const double *speed,
                                       const double *xf, const double *jmax, double *sx, double *su, double *sT, mpcmp_info *info, double *rT,
                                       mpcmp_info *rinfo, mpcmp_route_seam *seam, double *via_qd_out) {
    int L;
    if (int rc = route_check(ctx, "mpcmp_solve_route_batch", B, M, &L)) return rc;
    if (!x0 || !xf || (M > 0 && !via)) { ctx->err = "mpcmp_solve_route_batch: x0, xf (and via with M > 0) are required"; return MPCMP_EINVAL; }
    if (int rc = route_values_ok(ctx, "mpcmp_solve_route_batch", B, M, x0, via, via_qd, speed, xf)) return rc;
    if (int rc = route_solve_check(ctx, B, M, x0, via, xf, jmax, sx, su, sT, rT, rinfo, seam, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t nx = ctx->nx, nv = (size_t)B * M * (nx / 2);
    hipStream_t st = ctx->stream;
    Stage sg(ctx);
    double *d0, *df, *dv, *dq, *ds, *drT, *dvo;
    mpcmp_info *dri;
    mpcmp_route_seam *dsm;
    sg.in(&d0, x0, nx * B); sg.in(&df, xf, nx * B); sg.in(&dv, M > 0 ? via : nullptr, nv); sg.in(&dq, M > 0 ? via_qd : nullptr, nv); sg.in(&ds, speed, B);
    sg.out(&drT, rT, B); sg.out(&dri, rinfo, B); sg.out(&dsm, seam, B); sg.out(&dvo, M > 0 ? via_qd_out : nullptr, nv);
    if (int rc = sg.upload()) return rc;
    if (int rc = route_solve_enqueue(ctx, B, M, L, d0, dv, dq, ds, df, jmax, ctx->d_sx, ctx->d_su, ctx->d_sT, ctx->d_info, drT, dri, dsm, dvo, st)) return rc;
    if (int rc = download_trajectories(ctx, L, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    return sg.finish();
}

static int route_sample_check(mpcmp_ctx *ctx, int B, int M, const void *sx, const void *su, const void *sT, int n_pts, const void *out, int *L) {
    if (int rc = route_check(ctx, "mpcmp_sample_route_batch", B, M, L)) return rc;
    if (n_pts < 1 || !sx || !su || !sT || !out) { ctx->err = "mpcmp_sample_route_batch: n_pts >= 1 and all pointers required"; return MPCMP_EINVAL; }
    SINGLE_ARM_ONLY(ctx);
    return rows_ok(ctx, *L, PAYLOAD_ROWS);
}

extern "C" int mpcmp_sample_route_batch_device(mpcmp_ctx *ctx, int B, int M, const double *d_sx, const double *d_su, const double *d_sT, int n_pts,
                                               double *d_out, void *hip_stream) {
    int L;
    if (int rc = route_sample_check(ctx, B, M, d_sx, d_su, d_sT, n_pts, d_out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    HIPCHK(ctx, route_sample_launch(md, ms, ctx->nseg, B, M, n_pts, d_sx, d_su, d_sT, d_out, (hipStream_t)hip_stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_sample_route_batch(mpcmp_ctx *ctx, int B, int M, const double *sx, const double *su, const double *sT, int n_pts, double *out) {
    int L;
    if (int rc = route_sample_check(ctx, B, M, sx, su, sT, n_pts, out, &L)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t NL = (size_t)ctx->N * L;
    Stage sg(ctx);
    double *dx, *du, *dT, *dout;
    sg.in(&dx, sx, 14 * NL); sg.in(&du, su, 7 * NL); sg.in(&dT, sT, L); sg.out(&dout, out, (size_t)B * (n_pts + 1) * 29);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_sample_route_batch_device(ctx, B, M, dx, du, dT, n_pts, dout, ctx->stream)) return rc;
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// batched tool-pose targets (ik_device.hpp): B problems x S starts of the DLS inverse kinematics, one start chosen per problem, xf columns of one arm
static int pose_targets_check(mpcmp_ctx *ctx, int B, int arm, const double *R, const double *p, int S, const double *seeds, const double *xf) {
    if (!ctx) { g_err = "mpcmp_pose_targets: no context"; return MPCMP_EINVAL; }
    if (B < 1) { ctx->err = "mpcmp_pose_targets: B must be >= 1"; return MPCMP_EINVAL; }
    if (S < 1 || S > 64) { ctx->err = "mpcmp_pose_targets: S must be in [1, 64]"; return MPCMP_EINVAL; }
    if (arm < 0 || arm >= ctx->narm) { ctx->err = "mpcmp_pose_targets: arm must be in [0, narm)"; return MPCMP_EINVAL; }
    if (!R || !p || !seeds || !xf) { ctx->err = "mpcmp_pose_targets: R, p, q_seeds and xf are required"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

extern "C" int mpcmp_pose_targets_batch_device(mpcmp_ctx *ctx, int B, int arm, const double *d_R, const double *d_p, const double *d_twist,
                                               int S, const double *d_seeds, const double *d_q_ref, double *d_xf, mpcmp_ik_info *d_info, void *hip_stream) {
    if (int rc = pose_targets_check(ctx, B, arm, d_R, d_p, S, d_seeds, d_xf)) return rc;
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    IkBounds bd;
    for (int j = 0; j < 7; j++) { bd.lq[j] = ctx->cfg.lbx[j]; bd.uq[j] = ctx->cfg.ubx[j]; bd.lv[j] = ctx->cfg.lbx[7 + j]; bd.uv[j] = ctx->cfg.ubx[7 + j]; }
    int P = 1;
    while (P < S) P <<= 1;
    const long threads = (long)B * P;
    hipLaunchKernelGGL(k_pose_targets, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, (hipStream_t)hip_stream, ctx->d_model + arm, bd, ctx->bnd_rows > 0 ? ctx->d_bnd : nullptr, B, S, P,
                       ctx->nx, 7 * arm, 7 * ctx->narm + 7 * arm, d_R, d_p, d_twist, d_seeds, d_q_ref, d_xf, d_info);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_pose_targets_batch(mpcmp_ctx *ctx, int B, int arm, const double *R, const double *p, const double *twist,
                                        int S, const double *seeds, const double *q_ref, double *xf, mpcmp_ik_info *info) {
    if (int rc = pose_targets_check(ctx, B, arm, R, p, S, seeds, xf)) return rc;
    if (int rc = rows_ok(ctx, B, BOUND_ROWS)) return rc;
    const size_t nb = B, nx = ctx->nx;
    const struct { const double *v; size_t n; } in[5] = {{R, 9 * nb}, {p, 3 * nb}, {twist, 6 * nb}, {seeds, 7 * nb * S}, {q_ref, 7 * nb}};
    for (const auto &a : in)
        if (a.v)
            for (size_t k = 0; k < a.n; k++)
                if (!std::isfinite(a.v[k])) { ctx->err = "mpcmp_pose_targets: an input value is not finite"; return MPCMP_EINVAL; }
    for (size_t b = 0; b < nb; b++) {
        const double *r = R + 9 * b;
        double dev = 0.0;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) {
                const double g = r[i] * r[j] + r[3 + i] * r[3 + j] + r[6 + i] * r[6 + j] - (i == j ? 1.0 : 0.0);
                dev = std::max(dev, std::fabs(g));
            }
        const double det = r[0] * (r[4] * r[8] - r[5] * r[7]) - r[1] * (r[3] * r[8] - r[5] * r[6]) + r[2] * (r[3] * r[7] - r[4] * r[6]);
        if (dev > 1e-6 || !(det > 0.0)) {
            std::ostringstream os;
            os << "mpcmp_pose_targets: R of problem " << b << " is not a rotation";
            ctx->err = os.str();
            return MPCMP_EINVAL;
        }
    }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    double *dR, *dp_, *dtw, *dsd, *dqr, *dxf;
    mpcmp_ik_info *dinfo;
    sg.in(&dR, R, 9 * nb); sg.in(&dp_, p, 3 * nb); sg.in(&dtw, twist, 6 * nb); sg.in(&dsd, seeds, 7 * nb * S); sg.in(&dqr, q_ref, 7 * nb);
    sg.inout(&dxf, xf, nx * nb);       // the other arm's columns come back as they were
    sg.out(&dinfo, info, nb);
    if (int rc = sg.upload()) return rc;
    if (int rc = mpcmp_pose_targets_batch_device(ctx, B, arm, dR, dp_, dtw, S, dsd, dqr, dxf, dinfo, ctx->stream)) return rc;
    return sg.finish();
}

// ------------------------------------------------------------------------------------------------
// receding-horizon driver (BASELINE config #5): B instances, every step = warm-started re-solve from the previous
// solution (re-guess rule of motionPlanner.cpp:199-207) + state advance along the new solution
// (get_MPC_point, motionPlanner.hpp:118-128).  The fixed launch sequence of one step is captured in a hipGraph.
extern "C" int mpcmp_reset_multipliers(mpcmp_ctx *ctx) {
    if (!ctx) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.lam, 0, sizeof(double) * ctx->lam_count, ctx->stream));
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.status, 0, sizeof(*ctx->ws.status) * ctx->max_batch, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_init(mpcmp_ctx *ctx, int B, const double *x0, const double *xf) {
    if (!ctx || !x0 || !xf || B < 1) return MPCMP_EINVAL;
    if (B > ctx->max_batch) return MPCMP_ETOOBIG;
    if (int rc = rows_ok(ctx, B, PAYLOAD_ROWS)) return rc;
    if (ctx->bnd_rows > 0) { ctx->err = "mpcmp_rh_init: the receding-horizon driver does not read bound rows (clear them: mpcmp_set_bounds(ctx, 0, NULL))"; return MPCMP_EINVAL; }
    if (ctx->tw_rows > 0) { ctx->err = "mpcmp_rh_init: the receding-horizon driver does not read final-time rows (clear them: mpcmp_set_time_windows(ctx, 0, NULL, NULL))"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.lam, 0, sizeof(double) * ctx->lam_count, st));       // new instances: no multipliers to carry, no failed solve behind them
    HIPCHK(ctx, hipMemsetAsync(ctx->ws.status, 0, sizeof(*ctx->ws.status) * ctx->max_batch, st));
    HIPCHK(ctx, hipMemsetAsync(ctx->d_retired, 0, sizeof(int) * ctx->max_batch, st));                       // nobody has arrived
    HIPCHK(ctx, hipMemsetAsync(ctx->d_rh_count, 0, 2 * sizeof(unsigned long long), st));
    if (int rc = upload_problems(ctx, B, x0, xf, nullptr, nullptr, nullptr, st)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(st));
    ctx->rh_B = B; ctx->rh_first = true;
    drop_rh_graph(ctx);
    return MPCMP_OK;
}

// capturing: st is being captured into the step graph
static int rh_enqueue_step(mpcmp_ctx *ctx, double dt, bool first, hipStream_t st, bool capturing) {
    const int B = ctx->rh_B;
    // The driver's start guess, every step, from every instance's current state: the jerk-limited time-synchronised trajectory the reference takes from
    // Ruckig for solve_trajectory(true) (motionPlanner.cpp:146-175), with the velocity / acceleration limits of the configuration and the jerk
    // margin every example of the reference uses (0.1 x max jerk: examples/offline_trajectory.cpp:9, benchmark.cpp).  It starts the first solve and
    // RE-starts an instance whose previous solve is no guess (hard failure, T outside its box, or a restart asked for by mpcmp_rh_update: k_init); the
    // other re-solves re-guess from the previous solution (solve_trajectory(false), motionPlanner.cpp:199-207).
    double jm[7];
    mpcmp_default_limits(nullptr, nullptr, nullptr, nullptr, jm, nullptr);
    for (int j = 0; j < 7; j++) jm[j] *= 0.1;
    // (after the first step only for the instances that restart: the generator costs ~ 0.15 ms per 512 instances, 4 % of a step)
    if (int rc = warm_start_jerk_device(ctx, B, ctx->d_x0, ctx->d_xf, nullptr, nullptr, nullptr, nullptr, jm, ctx->d_wx, ctx->d_wu, ctx->d_wT, st,
                                        first ? nullptr : ctx->ws.status, MPCMP_ST_NO_GUESS))
        return rc;
    SolveCall c = staged_call(ctx, B, true, st);
    if (!first) { c.wx = ctx->d_sx; c.wu = ctx->d_su; c.wT = ctx->d_sT; c.reguess = 1; }
    c.rh_step = true;              // the driver's defaults of the start flags (run_config) and the retired instances (WS::retired)
    c.capturing = capturing;
    if (int rc = solve_dispatch(ctx, c)) return rc;
    hipLaunchKernelGGL(k_advance, dim3((B + 255) / 256), dim3(256), 0, st, ctx->nseg, ctx->nx, B, dt, ctx->cfg.eps_target, ctx->d_sx, ctx->d_sT,
                       ctx->ws.status, ctx->d_xf, ctx->d_x0, ctx->d_retired, ctx->d_info, ctx->d_rh_count);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_run(mpcmp_ctx *ctx, int steps, double dt, int use_graph) {
    if (!ctx || steps < 1 || !(dt > 0.0) || ctx->rh_B < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    int done = 0;
    if (ctx->rh_first) {                       // first solve: built-in initialiser, not part of the graph
        if (int rc = rh_enqueue_step(ctx, dt, true, st, false)) return rc;
        ctx->rh_first = false; done = 1;
    }
    if (use_graph && steps - done > 0) {
        if (!ctx->rh_exec || ctx->rh_dt != dt) {
            drop_rh_graph(ctx);
            HIPCHK(ctx, hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal));
            const int rc = rh_enqueue_step(ctx, dt, false, st, true);
            hipError_t e = hipStreamEndCapture(st, &ctx->rh_graph);
            if (rc) return rc;
            HIPCHK(ctx, e);
            HIPCHK(ctx, hipGraphInstantiate(&ctx->rh_exec, ctx->rh_graph, nullptr, nullptr, 0));
            ctx->rh_dt = dt;
        }
        for (; done < steps; done++) HIPCHK(ctx, hipGraphLaunch(ctx->rh_exec, st));
    } else {
        for (; done < steps; done++)
            if (int rc = rh_enqueue_step(ctx, dt, false, st, false)) return rc;
    }
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

// Between two steps: new measured states and / or targets of listed instances (k_rh_update).  Only buffer contents change: a captured step graph
// stays valid, and the next step reads the new values through the pointers it was captured with.
static int rh_update_check(mpcmp_ctx *ctx, int n, const int *idx, const double *x, const double *xf, int flags) {
    if (!ctx) { g_err = "mpcmp_rh_update: no context"; return MPCMP_EINVAL; }
    if (ctx->rh_B < 1) { ctx->err = "mpcmp_rh_update: no receding-horizon loop (mpcmp_rh_init first)"; return MPCMP_EINVAL; }
    if (n < 1 || n > ctx->rh_B) { ctx->err = "mpcmp_rh_update: n must be in [1, B] of mpcmp_rh_init"; return MPCMP_EINVAL; }
    if (!idx && n != ctx->rh_B) { ctx->err = "mpcmp_rh_update: idx NULL needs n == B"; return MPCMP_EINVAL; }
    if (!x && !xf) { ctx->err = "mpcmp_rh_update: x and xf are both NULL"; return MPCMP_EINVAL; }
    if (flags & ~MPCMP_RH_RESTART) { ctx->err = "mpcmp_rh_update: unknown flag bits"; return MPCMP_EINVAL; }
    return MPCMP_OK;
}

static int rh_update_enqueue(mpcmp_ctx *ctx, int n, const int *d_idx, const double *d_x, const double *d_xf, int flags, hipStream_t st) {
    hipLaunchKernelGGL(k_rh_update, dim3((n + 255) / 256), dim3(256), 0, st, ctx->nx, n, d_idx, d_x, d_xf, (flags & MPCMP_RH_RESTART) ? 1 : 0,
                       ctx->d_x0, ctx->d_xf, ctx->d_retired, ctx->ws.status, ctx->d_info, ctx->d_rh_count);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_update(mpcmp_ctx *ctx, int n, const int *idx, const double *x, const double *xf, int flags) {
    if (int rc = rh_update_check(ctx, n, idx, x, xf, flags)) return rc;
    const int B = ctx->rh_B;
    const size_t nx = ctx->nx;
    if (idx) {
        std::vector<char> seen(B, 0);
        for (int i = 0; i < n; i++) {
            if (idx[i] < 0 || idx[i] >= B) { ctx->err = "mpcmp_rh_update: instance index out of range"; return MPCMP_EINVAL; }
            if (seen[idx[i]]++) { ctx->err = "mpcmp_rh_update: instance index repeated"; return MPCMP_EINVAL; }
        }
    }
    for (const double *v : {x, xf})
        if (v)
            for (size_t k = 0; k < n * nx; k++)
                if (!std::isfinite(v[k])) { ctx->err = "mpcmp_rh_update: a state or target value is not finite"; return MPCMP_EINVAL; }
    HIPCHK(ctx, hipSetDevice(ctx->device));
    Stage sg(ctx);
    int *di;
    double *dx, *dxf;
    sg.in(&di, idx, n); sg.in(&dx, x, n * nx); sg.in(&dxf, xf, n * nx);
    if (int rc = sg.upload()) return rc;
    if (int rc = rh_update_enqueue(ctx, n, di, dx, dxf, flags, ctx->stream)) return rc;
    return sg.finish();
}

extern "C" int mpcmp_rh_update_device(mpcmp_ctx *ctx, int n, const int *d_idx, const double *d_x, const double *d_xf, int flags, void *hip_stream) {
    if (int rc = rh_update_check(ctx, n, d_idx, d_x, d_xf, flags)) return rc;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    return with_caller_stream(ctx, hip_stream, [&](hipStream_t st) { return rh_update_enqueue(ctx, n, d_idx, d_x, d_xf, flags, st); });
}

extern "C" int mpcmp_rh_get(mpcmp_ctx *ctx, double *x0_now, double *sx, double *su, double *sT, mpcmp_info *info) {
    if (!ctx || ctx->rh_B < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t B = ctx->rh_B;
    hipStream_t st = ctx->stream;
    if (x0_now) HIPCHK(ctx, hipMemcpyAsync(x0_now, ctx->d_x0, sizeof(double) * ctx->nx * B, hipMemcpyDeviceToHost, st));
    if (int rc = download_trajectories(ctx, B, ctx->d_sx, ctx->d_su, ctx->d_sT, sx, su, sT, info, st)) return rc;
    HIPCHK(ctx, hipStreamSynchronize(st));
    return MPCMP_OK;
}

extern "C" int mpcmp_rh_stats(mpcmp_ctx *ctx, long long *resolves_done, long long *arrived) {
    if (!ctx || ctx->rh_B < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    unsigned long long c[2] = {0, 0};
    HIPCHK(ctx, hipMemcpyAsync(c, ctx->d_rh_count, sizeof(c), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    if (resolves_done) *resolves_done = (long long)c[0];
    if (arrived) *arrived = (long long)c[1];
    return MPCMP_OK;
}

// diagnostics: copy one workspace array of the last solve to the host (which: 0 z, 1 lambda, 2 c_eq, 3 g, 4 p, 5 y)
extern "C" int mpcmp_debug_fetch(mpcmp_ctx *ctx, int which, double *out, long count) {
    if (!ctx || !out || count < 1) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    const double *src = which == 0 ? ctx->ws.z : which == 1 ? ctx->ws.lam : which == 2 ? ctx->ws.ceq : which == 3 ? ctx->ws.g
                      : which == 4 ? ctx->ws.p : which == 5 ? ctx->ws.y : nullptr;
    if (!src) return MPCMP_EINVAL;
    HIPCHK(ctx, hipMemcpy(out, src, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost));
    return MPCMP_OK;
}

// diagnostics: raw phase stamps of the last k_qp launch (all zero unless built with -DMPCMP_STAMPS)
extern "C" int mpcmp_debug_stamps(mpcmp_ctx *ctx, int B, unsigned long long *out) {
    if (!ctx || !out || B < 1 || B > ctx->max_batch) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipDeviceSynchronize());
    HIPCHK(ctx, hipMemcpy(out, ctx->ws.dbg, sizeof(unsigned long long) * MPCMP_DBG_WORDS * B, hipMemcpyDeviceToHost));
    return MPCMP_OK;
}

extern "C" int mpcmp_kernel_timing(mpcmp_ctx *ctx, int reset, const char **name, double *ms_total, int *launches) {
    if (!ctx) return MPCMP_EINVAL;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    // fold finished event pairs into the accumulators (caller has synchronised the stream)
    for (size_t i = 0; i < ctx->sol.ev_used; i++) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ctx->sol.ev[i].e[0], ctx->sol.ev[i].e[1]) == hipSuccess) { ctx->qp_ms += ms; ctx->qp_launches++; }
    }
    ctx->sol.ev_used = 0;
    ctx->timing = true;            // event recording starts with the first call (bench.py calls it once before the timed region)
    if (name) *name = ctx->sol.loop_kernel;
    if (ms_total) *ms_total = ctx->qp_ms;
    if (launches) *launches = ctx->qp_launches;
    if (reset) { ctx->qp_ms = 0.0; ctx->qp_launches = 0; }
    return MPCMP_OK;
}
