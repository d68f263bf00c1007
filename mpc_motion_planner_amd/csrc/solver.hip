// solver.hip — the solver's translation unit: every register-bound kernel of the SQP chain that is not built with a scheduler strategy of its own
// (k_init, k_qp, k_qp2, k_qp3f, k_qp3, k_step, k_init_m, k_step_m, k_eval_constraints; qp3_n25.hip and qp5_n19.hip hold the others) is instantiated
// here and only here, together with the code that selects, prepares and launches them.  The C-ABI unit (mpcmp.hip) reaches it through the four
// functions of solver.hpp and reads none of the kernel headers, so an edit to an entry point neither recompiles these kernels nor shares a
// compilation with them.
// What else is in this unit is part of what these kernels compile to: the instantiation of k_qp makes the constant table c_D a global symbol for
// every kernel here (solver_kernels.hpp, at c_D), which is the form k_qp2<4>, k_step<4> and k_qp3<6, 2> were tuned and measured in.  So the
// kernels of the chain stay together in this file, k_qp among them, and nothing else is added to it; tests/test_kernel_resources.py compiles it.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "solver.hpp"
#include "solver_kernels.hpp"
#include "qp_kernel_v2.hpp"
#include "qp_kernel_v3.hpp"
#ifdef MPCMP_WITH_QP4      /* the measured two-OCPs-per-CU alternative for N = 13 (does not pay): tools/experiments/, built only on request (-DMPCMP_WITH_QP4 -Itools/experiments) */
#include "qp_kernel_v4.hpp"
#endif
#include "qp_kernel_v5.hpp"
#include "multi_kernels.hpp"


#ifdef MPCMP_SPLIT_N25
// the N = 25 kernels live in qp3_n25.hip (built with another scheduler strategy: see there)
namespace mpcmp {
extern template __global__ void k_qp3f<8, 1>(mpcmp_config, WS, const Qp3Pat *, Xch, int, double *);
extern template __global__ void k_qp3f<8, 2>(mpcmp_config, WS, const Qp3Pat *, Xch, int, double *);
extern template __global__ void k_qp3<8, 1>(mpcmp_config, WS, const Qp3Pat *, Xch, int, const double *);
extern template __global__ void k_qp3<8, 2>(mpcmp_config, WS, const Qp3Pat *, Xch, int, const double *);
}  // namespace mpcmp
#endif

#ifdef MPCMP_SPLIT_N19
// the N = 19 one-arm pair lives in qp5_n19.hip (its own scheduler strategy: see there)
namespace mpcmp {
extern template __global__ void k_qp3f<6, 1, 5>(mpcmp_config, WS, const Qp3Pat *, Xch, int, double *);
extern template __global__ void k_qp5<6>(mpcmp_config, WS, const Qp3Pat *, Xch, int, const double *);
}  // namespace mpcmp
#endif

using namespace mpcmp;

// the sizes the context's buffers are allocated and sliced with (dims_of, context.hpp) are the sizes the kernels index with, for every instantiated
// discretisation
template <int NSEG>
static constexpr bool dims_match() { constexpr Dims d = dims_of(NSEG, 1); using D = Dim<NSEG>; return d.N == D::N && d.n == D::n && d.meq == D::meq && d.m == D::m && d.mn == D::mn; }
template <int NSEG, int NARM>
static constexpr bool dims_match_m() { constexpr Dims d = dims_of(NSEG, NARM); using D = DimM<NSEG, NARM>; return d.N == D::N && d.n == D::n && d.meq == NARM * D::meq && d.m == D::m && d.mn == D::mn; }
static_assert(dims_match<1>() && dims_match<2>() && dims_match<4>() && dims_match<6>(), "Dim<NSEG> and the context's strides differ");
static_assert(dims_match_m<8, 1>() && dims_match_m<6, 2>() && dims_match_m<8, 2>(), "DimM<NSEG, NARM> and the context's strides differ");

// ------------------------------------------------------------------------------------------------
// launches
static hipEvent_t *next_events(mpcmp_ctx *ctx) {
    if (ctx->sol.ev_used == ctx->sol.ev.size()) {
        if (ctx->sol.ev.size() >= mpcmp_ctx::Solver::MAX_EV) return nullptr;      // bounded: untimed until the caller folds the pairs
        mpcmp_ctx::Solver::EvPair p;
        if (hipEventCreate(&p.e[0]) != hipSuccess) return nullptr;
        if (hipEventCreate(&p.e[1]) != hipSuccess) { (void)hipEventDestroy(p.e[0]); return nullptr; }
        ctx->sol.ev.push_back(p);
    }
    return ctx->sol.ev[ctx->sol.ev_used++].e;
}

// Kernel selection of a single-arm context (compile-time candidates, run-time choice by discretisation and the context's diagnostics)
template <int NSEG>
struct KSel {
    static constexpr bool V2C = (NSEG == 2 || NSEG == 4);      // role-specialised 1024-thread QP kernel
    static constexpr bool V3T = (NSEG >= 4);                   // k_qp3 instantiated (num_seg 4: diagnostics, MPCMP_QP13=3)
    static constexpr int N3 = V3T ? NSEG : 6, N2 = V2C ? NSEG : 4, N1 = (NSEG >= 6) ? 1 : NSEG;
    bool V3C, V4, V2, V5;
    explicit KSel(const mpcmp_ctx *ctx) {
        V3C = NSEG >= 6 || (NSEG == 4 && ctx->sol.qp13 == 3);      // k_qp3: T bordered out, E-free interior solve (N = 19, 25)
        V4 = NSEG == 4 && ctx->sol.qp13 == 4;                       // k_qp3f<4, 1, 4> + k_qp4: two OCPs per CU
        V2 = V2C && !ctx->sol.force_v1 && !V3C && !V4;
        V5 = NSEG == 6 && ctx->sol.qp19 == 5;
    }
    // the kernel that runs the ADMM loop, by the order of preference of solve_impl's launches
    const char *loop_kernel_name() const { return V4 ? "k_qp4" : V5 ? "k_qp5" : V3C ? "k_qp3" : V2 ? "k_qp2" : "k_qp"; }
};

// dynamic-LDS limits of every kernel a context of this discretisation can launch: set ONCE, in mpcmp_create
template <int NSEG>
static int prepare_impl(mpcmp_ctx *ctx) {
    using S = KSel<NSEG>;
    const S k(ctx);
    ctx->sol.loop_kernel = k.loop_kernel_name();
    if (int rc = set_lds(ctx, k_init<NSEG>, InitLds<NSEG>::size * sizeof(double))) return rc;
    if (int rc = set_lds(ctx, k_step<NSEG>, StepLds<NSEG>::size * sizeof(double))) return rc;
    if (k.V3C) {
        if (int rc = set_lds(ctx, k_qp3<S::N3, 1>, Qp3<S::N3>::sizeL * sizeof(double))) return rc;
        if (int rc = set_lds(ctx, k_qp3f<S::N3, 1>, Qp3<S::N3>::sizeF * sizeof(double))) return rc;
    }
    if (k.V5) {
        if (int rc = set_lds(ctx, k_qp5<6>, Qp5<6>::size5 * sizeof(double))) return rc;
        if (int rc = set_lds(ctx, k_qp3f<6, 1, 5>, Qp3<6>::sizeF * sizeof(double))) return rc;
    }
#ifdef MPCMP_WITH_QP4
    if (k.V4) {
        const size_t l_qp4 = Qp4<4>::size * sizeof(double);
        if (int rc = set_lds(ctx, k_qp4<4>, l_qp4)) return rc;
        if (int rc = set_lds(ctx, k_qp3f<4, 1, 4>, Qp3<4>::sizeF * sizeof(double))) return rc;
        if (ctx->sol.debug_occ) {
            int nb = -1;
            (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, k_qp4<4>, 384, l_qp4);
            std::fprintf(stderr, "k_qp4: %zu B of dynamic LDS, %d workgroups per CU\n", l_qp4, nb);
        }
    }
#endif
    if (k.V2) { if (int rc = set_lds(ctx, k_qp2<S::N2>, Qp2<S::N2>::size * sizeof(double))) return rc; }
    else if (!k.V3C && !k.V4) { if (int rc = set_lds(ctx, k_qp<S::N1>, QpLds<S::N1>::size * sizeof(double))) return rc; }
    return MPCMP_OK;
}

// ---- the parts of a solve ----
// A large batch is solved as parts on as many streams (why: solve_impl).  A part is a contiguous range of the call's problems with every per-problem
// pointer of the workspace, the exchange slots, the start guess and the outputs moved to its first problem
struct Part {
    int b0, B;
    hipStream_t stream;
    WS ws;
    Xch xch;
    const double *wx, *wu, *wT;
    double *sx, *su, *sT;
    mpcmp_info *info;
};
struct Parts {
    int n = 0;
    Part p[4];
    const Part *begin() const { return p; }
    const Part *end() const { return p + n; }
};

static Parts split(const mpcmp_ctx *ctx, const SolveCall &c, int nparts) {
    WS w = ctx->ws;
    w.x0 = c.x0; w.xf = c.xf;
    w.model = run_models(ctx, &w.mstride);
    w.retired = run_retired(ctx, c);
    w.tbox = run_rows(ctx, c);
    w.bnd = run_bounds(ctx, c);
    if (c.rh_step) { w.alt_x = ctx->d_wx; w.alt_u = ctx->d_wu; w.alt_T = ctx->d_wT; }
    const size_t nx = ctx->nx, nu = ctx->nu, N = ctx->N, n = ctx->n, mn = ctx->mn, meq = ctx->meq, narm = ctx->narm;
    const hipStream_t streams[4] = {c.stream, ctx->stream_x[0], ctx->stream_x[1], ctx->stream_x[2]};
    Parts ps;
    ps.n = nparts;
    for (int h = 0, acc = 0; h < nparts; h++) {
        Part &q = ps.p[h];
        q.b0 = acc; q.B = (c.B - acc + (nparts - h) - 1) / (nparts - h); q.stream = streams[h];
        acc += q.B;
        const size_t b0 = (size_t)q.b0;
        WS v = w;
        v.x0 += nx * b0; v.xf += nx * b0; v.z += n * b0; v.lam += mn * b0; v.ceq += meq * b0; v.g += 8 * N * narm * b0;
        v.Gk += 176 * N * narm * b0; v.p += n * b0; v.y += mn * b0; v.qpit += b0; v.perm += b0; v.okey += b0; v.done += h;
        v.qp_total += b0; v.status += b0; v.alpha += b0; v.dbg += (size_t)MPCMP_DBG_WORDS * b0;
        v.model += (size_t)v.mstride * b0;      // (the payload row is the problem's index in the whole batch, not in its part)
        if (v.retired) v.retired += b0;
        if (v.tbox) v.tbox += 2 * b0;
        if (v.bnd) v.bnd += b0;
        if (v.alt_x) { v.alt_x += nx * N * b0; v.alt_u += nu * N * b0; v.alt_T += b0; }
        q.ws = v;
        q.xch.buf = ctx->xch.buf ? ctx->xch.buf + (size_t)2 * MPCMP_XCH_STRIDE * b0 : nullptr;
        q.wx = c.wx ? c.wx + nx * N * b0 : nullptr; q.wu = c.wx ? c.wu + nu * N * b0 : nullptr; q.wT = c.wx ? c.wT + b0 : nullptr;
        q.sx = c.sx ? c.sx + nx * N * b0 : nullptr; q.su = c.su ? c.su + nu * N * b0 : nullptr;
        q.sT = c.sT ? c.sT + b0 : nullptr; q.info = c.info ? c.info + b0 : nullptr;
    }
    return ps;
}
// the further parts' streams start behind the work already on the call's stream (fork) and the call's stream goes on behind them (join); under stream
// capture the events carry the other streams into the graph
static int fork_parts(mpcmp_ctx *ctx, const Parts &ps) {
    if (ps.n > 1) HIPCHK(ctx, hipEventRecord(ctx->ev_fork, ps.p[0].stream));
    for (int h = 1; h < ps.n; h++) HIPCHK(ctx, hipStreamWaitEvent(ps.p[h].stream, ctx->ev_fork, 0));
    return MPCMP_OK;
}
static int join_parts(mpcmp_ctx *ctx, const Parts &ps) {
    for (int h = 1; h < ps.n; h++) { HIPCHK(ctx, hipEventRecord(ctx->ev_join[h - 1], ps.p[h].stream)); HIPCHK(ctx, hipStreamWaitEvent(ps.p[0].stream, ctx->ev_join[h - 1], 0)); }
    return MPCMP_OK;
}

template <int NSEG>
static int solve_impl(mpcmp_ctx *ctx, const SolveCall &c) {
    using D = Dim<NSEG>;
    using S = KSel<NSEG>;
    const S ks(ctx);
    const bool V3C = ks.V3C, V4 = ks.V4, V2 = ks.V2;
    const mpcmp_config cfg = run_config(ctx, c);
    const size_t l_init = InitLds<NSEG>::size * sizeof(double), l_qp = QpLds<S::N1>::size * sizeof(double),
                 l_step = StepLds<NSEG>::size * sizeof(double);
    const size_t l_qp3 = Qp3<S::N3>::sizeL * sizeof(double), l_qp3f = Qp3<S::N3>::sizeF * sizeof(double);
#ifdef MPCMP_WITH_QP4
    const size_t l_qp4 = Qp4<4>::size * sizeof(double);
#endif
    const size_t l_qp2 = Qp2<S::N2>::size * sizeof(double);
    // A large batch is solved as two half-batches on two streams.  Every SQP iteration is a chain of dependent launches
    // (QP -> order -> step), and a QP launch ends in a tail in which most CUs are idle (its problems run 25..700 ADMM
    // iterations, four workgroups per CU); with two independent chains in flight the tail of one half is filled by the other
    // half's next launch.  Replay of the bench workload's iteration counts: -5.8 % makespan.  Results are unaffected (problems
    // are independent); small batches stay on one stream.
    const bool dual = !ctx->sol.single_stream && !c.only_qp && c.B >= 512;      // (also under stream capture: see fork_parts)
    // parts: two; three for the N = 13 kernel from 1024 problems on (round 5, three repeats each: 15.74 - 15.77 k against 15.58 - 15.61 k traj/s on the
    // headline batch; 512 problems — the receding-horizon step — and N = 19 are faster with two: 135.7 k vs 130.0 k re-solves/s, 67.1 k vs 65.2 k traj/s)
    const int parts_auto = (NSEG == 4 && V2 && c.B >= 1024) ? 3 : 2;
    const Parts parts = split(ctx, c, dual ? (ctx->sol.parts_env < 1 ? parts_auto : (ctx->sol.parts_env > 4 ? 4 : ctx->sol.parts_env)) : 1);
    if (int rc = fork_parts(ctx, parts)) return rc;
    for (const Part &p : parts)
        hipLaunchKernelGGL(k_init<NSEG>, dim3(p.B), dim3(D::NT), l_init, p.stream, cfg, p.ws, p.wx, p.wu, p.wT, c.reguess);
    const int iters = c.only_qp ? 1 : cfg.sqp_iters;
    for (int it = 0; it < iters; it++) {
        for (const Part &p : parts) {
            hipEvent_t *ev = (ctx->timing && !c.capturing) ? next_events(ctx) : nullptr;
            if (ev) HIPCHK(ctx, hipEventRecord(ev[0], p.stream));
#ifdef MPCMP_WITH_QP4
            if (V4) {
                WS w3 = p.ws;
                w3.ext_of_int = ctx->sol.d3_ext_of_int; w3.entry_ptr = ctx->sol.d3_entry_ptr; w3.terms = ctx->sol.d3_terms;
                double *fh = ctx->sol.d_fac + (size_t)p.b0 * Qp4Fac<4>::FAC;
                hipLaunchKernelGGL((k_qp3f<4, 1, 4>), dim3(p.B), dim3(1024), Qp3<4>::sizeF * sizeof(double), p.stream, cfg, w3, ctx->sol.d_pat, ctx->xch, p.B, fh);
                hipLaunchKernelGGL((k_qp4<4>), dim3(p.B), dim3(384), l_qp4, p.stream, cfg, w3, (const uint32_t *)ctx->sol.d_lane4, p.B, (const double *)fh);
            }
#else
            if (V4) { ctx->err = "k_qp4 not built"; return MPCMP_EINVAL; }
#endif
            else if (ks.V5) {
                double *fh = ctx->sol.d_fac + (size_t)p.b0 * Qp5Fac<6>::FAC;
                hipLaunchKernelGGL((k_qp3f<6, 1, 5>), dim3(p.B), dim3(1024), Qp3<6>::sizeF * sizeof(double), p.stream, cfg, p.ws, ctx->sol.d_pat, ctx->xch, p.B, fh);
                hipLaunchKernelGGL((k_qp5<6>), dim3(p.B), dim3(768), Qp5<6>::size5 * sizeof(double), p.stream, cfg, p.ws, ctx->sol.d_pat, ctx->xch, p.B, (const double *)fh);
            }
            else if (V3C) {
                WS w3 = p.ws;
                if (NSEG == 4) { w3.ext_of_int = ctx->sol.d3_ext_of_int; w3.entry_ptr = ctx->sol.d3_entry_ptr; w3.terms = ctx->sol.d3_terms; }
                double *fh = ctx->sol.d_fac + (size_t)p.b0 * Qp3<S::N3>::FAC;
                hipLaunchKernelGGL((k_qp3f<S::N3, 1>), dim3(p.B), dim3(1024), l_qp3f, p.stream, cfg, w3, ctx->sol.d_pat, ctx->xch, p.B, fh);
                hipLaunchKernelGGL((k_qp3<S::N3, 1>), dim3(p.B), dim3(512), l_qp3, p.stream, cfg, w3, ctx->sol.d_pat, ctx->xch, p.B, (const double *)fh);
            }
            else if (V2) hipLaunchKernelGGL((k_qp2<S::N2>), dim3(p.B), dim3(1024), l_qp2, p.stream, cfg, p.ws, ctx->sol.streams);
            else hipLaunchKernelGGL((k_qp<S::N1>), dim3(p.B), dim3(Dim<S::N1>::NT), l_qp, p.stream, cfg, p.ws);
            if (ev) HIPCHK(ctx, hipEventRecord(ev[1], p.stream));
            if (c.only_qp) continue;
            hipLaunchKernelGGL(k_step<NSEG>, dim3(p.B), dim3(D::NT), l_step, p.stream, cfg, p.ws, it == iters - 1 ? 1 : 0, it,
                               p.sx, p.su, p.sT, p.info);
        }
    }
    if (int rc = join_parts(ctx, parts)) return rc;
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

template <int NSEG, int NARM>
static int prepare_impl_m(mpcmp_ctx *ctx) {
    using D = DimM<NSEG, NARM>;
    const size_t l_m = D::size * sizeof(double);
    ctx->sol.loop_kernel = "k_qp3";
    if (int rc = set_lds(ctx, k_init_m<NSEG, NARM>, l_m)) return rc;
    if (int rc = set_lds(ctx, k_step_m<NSEG, NARM>, l_m)) return rc;
    if (int rc = set_lds(ctx, k_qp3<NSEG, NARM>, Qp3<NSEG>::sizeL * sizeof(double))) return rc;
    if (int rc = set_lds(ctx, k_qp3f<NSEG, NARM>, Qp3<NSEG>::sizeF * sizeof(double))) return rc;
    return MPCMP_OK;
}

// dynamic-LDS limits of the context's kernels (hipFuncSetAttribute): once per context
static int prepare_kernels(mpcmp_ctx *ctx) {
    if (ctx->narm == 2) return ctx->nseg == 6 ? prepare_impl_m<6, 2>(ctx) : prepare_impl_m<8, 2>(ctx);
    switch (ctx->nseg) {
        case 1: return prepare_impl<1>(ctx);
        case 2: return prepare_impl<2>(ctx);
        case 4: return prepare_impl<4>(ctx);
        case 6: return prepare_impl<6>(ctx);
        case 8: return prepare_impl_m<8, 1>(ctx);
    }
    return MPCMP_EINVAL;
}

// N = 25 and multi-arm OCPs: k_init_m -> K x [k_qp3 (one workgroup per arm), k_step_m]
template <int NSEG, int NARM>
static int solve_impl_m(mpcmp_ctx *ctx, const SolveCall &c) {
    using D = DimM<NSEG, NARM>;
    const mpcmp_config cfg = run_config(ctx, c);
    const size_t l_m = D::size * sizeof(double), l_qp3 = Qp3<NSEG>::sizeL * sizeof(double), l_qp3f = Qp3<NSEG>::sizeF * sizeof(double);
    // two parts on two streams once one part alone fills the chip (one CU per arm): see solve_impl
    const bool dual = !ctx->sol.single_stream && !c.only_qp && c.B * NARM >= 512;
    const Parts parts = split(ctx, c, dual ? 2 : 1);
    if (int rc = fork_parts(ctx, parts)) return rc;
    for (const Part &p : parts)
        hipLaunchKernelGGL((k_init_m<NSEG, NARM>), dim3(p.B), dim3(D::NT), l_m, p.stream, cfg, p.ws.model, p.ws, p.xch, p.wx, p.wu, p.wT, c.reguess);
    const int iters = c.only_qp ? 1 : cfg.sqp_iters;
    for (int it = 0; it < iters; it++) {
        for (const Part &p : parts) {
            hipEvent_t *ev = (ctx->timing && !c.capturing) ? next_events(ctx) : nullptr;
            if (ev) HIPCHK(ctx, hipEventRecord(ev[0], p.stream));
            const int grid = NARM == 1 ? p.B : ((p.B + 7) / 8) * 16;       // arm workgroups of one OCP are 8 apart (k_qp3)
            double *fh = ctx->sol.d_fac + (size_t)p.b0 * NARM * Qp3<NSEG>::FAC;
            hipLaunchKernelGGL((k_qp3f<NSEG, NARM>), dim3(grid), dim3(1024), l_qp3f, p.stream, cfg, p.ws, ctx->sol.d_pat, p.xch, p.B, fh);
            hipLaunchKernelGGL((k_qp3<NSEG, NARM>), dim3(grid), dim3(512), l_qp3, p.stream, cfg, p.ws, ctx->sol.d_pat, p.xch, p.B, (const double *)fh);
            if (ev) HIPCHK(ctx, hipEventRecord(ev[1], p.stream));
            if (c.only_qp) continue;
            hipLaunchKernelGGL((k_step_m<NSEG, NARM>), dim3(p.B), dim3(D::NT), l_m, p.stream, cfg, p.ws.model, p.ws, p.xch,
                               it == iters - 1 ? 1 : 0, it, p.sx, p.su, p.sT, p.info);
        }
    }
    if (int rc = join_parts(ctx, parts)) return rc;
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}
int mpcmp::solver_run(mpcmp_ctx *ctx, const SolveCall &c) {
    if (ctx->narm == 2) return ctx->nseg == 6 ? solve_impl_m<6, 2>(ctx, c) : solve_impl_m<8, 2>(ctx, c);
    switch (ctx->nseg) {
        case 1: return solve_impl<1>(ctx, c);
        case 2: return solve_impl<2>(ctx, c);
        case 4: return solve_impl<4>(ctx, c);
        case 6: return solve_impl<6>(ctx, c);
        case 8: return solve_impl_m<8, 1>(ctx, c);
    }
    return MPCMP_EINVAL;
}

// ------------------------------------------------------------------------------------------------
// the solver's side of a new context
int mpcmp::solver_create(mpcmp_ctx *ctx) {
    const mpcmp_config *cfg = &ctx->cfg;
    const int narm = ctx->narm, max_batch = ctx->max_batch;
    // (the caller destroys the context on failure: mpcmp_destroy releases what was allocated so far)
#define TRY(x) do { int rc_ = (x); if (rc_) return rc_; } while (0)
#define HIPTRY(call) do { hipError_t e_ = (call); if (e_ != hipSuccess) { ctx->err = std::string(#call) + ": " + hipGetErrorString(e_); return MPCMP_ERUNTIME; } } while (0)
    StructureTables tab;
    // k_qp3 / k_qp4: per-arm tables with T bordered out (structure3.hpp), in ELL form
    auto build_v3 = [&](int nseg, StructureTables &tb, Qp3Pat &pat) -> bool {
        Tables3 t3;
        if (!build_tables3(nseg, t3)) return false;
        tb.nseg = t3.nseg; tb.ext_of_int = t3.ext_of_int; pat = t3.pat;
        // term lists in ELL form [term index][entry] (entry stride padded to 64): consecutive threads assemble consecutive entries,
        // so every load of a term word is one coalesced 256-byte request per wave (the per-entry lists of the CSR form cost a
        // cache line per 4-byte word, and every workgroup of the launch reads the same table: 0.47 M cycles per factorisation)
        const int E = (int)t3.entry_ptr.size() - 1, EP = (E + 63) / 64 * 64;
        // (kappa, the (T, T) entry, has one term per row of A: the kernel sums it by a workgroup reduction instead)
        const int e_kap = nseg * 1225 + 28 + nseg * 196 + nseg * 98 + 98 + 21 * (3 * nseg + 1);      // Dim3<nseg>::eKap
        int tmax = 0;
        for (int e = 0; e < E; e++) if (e != e_kap) tmax = std::max(tmax, t3.entry_ptr[e + 1] - t3.entry_ptr[e]);
        tb.entry_ptr.assign(EP, 0);
        tb.terms.assign((size_t)tmax * EP, 0xFFFFFFFFu);
        // Slots instead of entries: inside each of the two assembly calls' ranges ([0, EA): everything but K_II; [EA, E): K_II) the
        // entries are sorted by the length of their term lists, longest first, so that the 64 lanes of a wave (consecutive slots)
        // walk lists of (nearly) equal length.  In entry order a wave executed every step of its longest list for all of its 10 - 13
        // entries per lane: 140 term evaluations per lane for 32 terms.  tb.entry_ptr[slot] = count | entry << 8.
        const int EA = e_kap + 1;
        auto count_of = [&](int e) { return e == e_kap ? 0 : t3.entry_ptr[e + 1] - t3.entry_ptr[e]; };
        for (int part = 0; part < 2; part++) {
            const int lo = part ? EA : 0, hi = part ? E : EA;
            std::vector<int> order(hi - lo);
            for (int e = lo; e < hi; e++) order[e - lo] = e;
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return count_of(a) > count_of(b); });
            for (int k = 0; k < hi - lo; k++) {
                const int slot = lo + k, e = order[k], c = count_of(e);
                tb.entry_ptr[slot] = c | (e << 8);
                for (int t = 0; t < c; t++) tb.terms[(size_t)t * EP + slot] = t3.terms[t3.entry_ptr[e] + t];
            }
        }
        return true;
    };
    auto fac_doubles = [](int nseg) -> size_t { return nseg == 4 ? std::max<size_t>(Qp3<4>::FAC, Qp4Fac<4>::FAC) : (nseg == 6 ? std::max<size_t>(Qp3<6>::FAC, Qp5Fac<6>::FAC) : Qp3<8>::FAC); };
    if (cfg->num_seg == 6 && narm == 1) {
        if (const char *e = std::getenv("MPCMP_QP19")) ctx->sol.qp19 = std::atoi(e);
        if (ctx->sol.qp19 != 3 && ctx->sol.qp19 != 5) { ctx->err = "MPCMP_QP19 must be 3 (k_qp3) or 5 (k_qp5)"; return MPCMP_EINVAL; }
    }
    if (cfg->num_seg >= 6) {
        Qp3Pat pat;
        if (!build_v3(cfg->num_seg, tab, pat)) { ctx->err = "internal: structure table generation failed"; return MPCMP_EINVAL; }
        TRY(dalloc(ctx, &ctx->sol.d_fac, (size_t)max_batch * narm * fac_doubles(cfg->num_seg)));
        TRY(dalloc(ctx, &ctx->sol.d_pat, 1));
        HIPTRY(hipMemcpy(ctx->sol.d_pat, &pat, sizeof(Qp3Pat), hipMemcpyHostToDevice));
    } else if (!build_tables(cfg->num_seg, tab)) { ctx->err = "internal: structure table generation failed"; return MPCMP_EINVAL; }
    TRY(dalloc(ctx, &ctx->d_ext_of_int, tab.ext_of_int.size()));
    TRY(dalloc(ctx, &ctx->d_entry_ptr, tab.entry_ptr.size()));
    TRY(dalloc(ctx, &ctx->d_terms, tab.terms.size()));
    HIPTRY(hipMemcpy(ctx->d_ext_of_int, tab.ext_of_int.data(), tab.ext_of_int.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(ctx->d_entry_ptr, tab.entry_ptr.data(), tab.entry_ptr.size() * sizeof(int), hipMemcpyHostToDevice));
    HIPTRY(hipMemcpy(ctx->d_terms, tab.terms.data(), tab.terms.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    WS &w = ctx->ws;
    w.ext_of_int = ctx->d_ext_of_int; w.entry_ptr = ctx->d_entry_ptr; w.terms = ctx->d_terms;
    if (cfg->num_seg == 2 || cfg->num_seg == 4) {
        AsmStreams as;
        const int GS = cfg->num_seg == 4 ? Qp2<4>::GS : Qp2<2>::GS, RSv = Qp2<4>::RS;
        if (!build_streams(cfg->num_seg, 1024, Qp2<4>::HS, GS, RSv, as)) { ctx->err = "internal: assembly stream generation failed"; return MPCMP_EINVAL; }
        TRY(dalloc(ctx, &ctx->sol.d_stream, as.words.size()));
        HIPTRY(hipMemcpy(ctx->sol.d_stream, as.words.data(), as.words.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
        ctx->sol.streams.words = ctx->sol.d_stream; ctx->sol.streams.npass = as.npass;
        for (int p = 0; p < 8; p++) { ctx->sol.streams.off[p] = as.off[p]; ctx->sol.streams.W[p] = as.W[p]; }
        ctx->sol.streams.split_dst = as.split_dst; ctx->sol.streams.split_scr = as.split_scr; ctx->sol.streams.split_n = as.split_n;
    }
    if (cfg->num_seg == 4) {
        if (const char *e = std::getenv("MPCMP_QP13")) ctx->sol.qp13 = std::atoi(e);
        if (ctx->sol.qp13 != 2 && ctx->sol.qp13 != 3 && ctx->sol.qp13 != 4) { ctx->err = "MPCMP_QP13 must be 2 (k_qp2), 3 (k_qp3) or 4 (k_qp4, experimental: slower than k_qp2)"; return MPCMP_EINVAL; }
#ifndef MPCMP_WITH_QP4
        if (ctx->sol.qp13 == 4) { ctx->err = "MPCMP_QP13=4: this library was built without k_qp4 (experimental kernel: rebuild with -DMPCMP_WITH_QP4 -Itools/experiments)"; return MPCMP_EINVAL; }
#endif
        if (ctx->sol.qp13 != 2 && std::getenv("MPCMP_FORCE_V1")) { ctx->err = "MPCMP_FORCE_V1 and MPCMP_QP13 != 2 exclude each other"; return MPCMP_EINVAL; }
        if (ctx->sol.qp13 != 2) {
            StructureTables t4;
            Qp3Pat pat;
            if (!build_v3(4, t4, pat)) { ctx->err = "internal: structure table generation failed"; return MPCMP_EINVAL; }
            TRY(dalloc(ctx, &ctx->sol.d3_ext_of_int, t4.ext_of_int.size()));
            TRY(dalloc(ctx, &ctx->sol.d3_entry_ptr, t4.entry_ptr.size()));
            TRY(dalloc(ctx, &ctx->sol.d3_terms, t4.terms.size()));
            HIPTRY(hipMemcpy(ctx->sol.d3_ext_of_int, t4.ext_of_int.data(), t4.ext_of_int.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPTRY(hipMemcpy(ctx->sol.d3_entry_ptr, t4.entry_ptr.data(), t4.entry_ptr.size() * sizeof(int), hipMemcpyHostToDevice));
            HIPTRY(hipMemcpy(ctx->sol.d3_terms, t4.terms.data(), t4.terms.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
            TRY(dalloc(ctx, &ctx->sol.d_fac, (size_t)max_batch * fac_doubles(4)));
            TRY(dalloc(ctx, &ctx->sol.d_pat, 1));
            HIPTRY(hipMemcpy(ctx->sol.d_pat, &pat, sizeof(Qp3Pat), hipMemcpyHostToDevice));
#ifdef MPCMP_WITH_QP4
            std::vector<uint32_t> lane4((size_t)Qp4<4>::NF * Qp4<4>::NT);
            qp4_build_lanes<4>(pat, t4.ext_of_int.data(), lane4.data());
            TRY(dalloc(ctx, &ctx->sol.d_lane4, lane4.size()));
            HIPTRY(hipMemcpy(ctx->sol.d_lane4, lane4.data(), lane4.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
#endif
        }
    }
    // diagnostics (generic kernel everywhere, stream count, occupancy report): read here, per context
    ctx->sol.force_v1 = std::getenv("MPCMP_FORCE_V1") != nullptr;
    ctx->sol.single_stream = std::getenv("MPCMP_SINGLE_STREAM") != nullptr;
    ctx->sol.debug_occ = std::getenv("MPCMP_DEBUG_OCC") != nullptr;
    if (const char *e = std::getenv("MPCMP_STREAMS")) ctx->sol.parts_env = std::atoi(e);
    TRY(prepare_kernels(ctx));
#undef TRY
#undef HIPTRY
    return MPCMP_OK;
}

// k_init alone: the built-in initialiser writes the iterate z = [xs|us|T] of the staged problems (ctx->d_x0, d_xf) into ctx->ws.z
int mpcmp::solver_init_guess(mpcmp_ctx *ctx, int B, hipStream_t st) {
    const SolveCall plain;
    const mpcmp_config save = run_config(ctx, plain);
    WS w = ctx->ws; w.x0 = ctx->d_x0; w.xf = ctx->d_xf; w.tbox = run_rows(ctx, plain); w.bnd = run_bounds(ctx, plain);
#define LAUNCH_INIT(NS) { const size_t l = InitLds<NS>::size * sizeof(double); \
        hipLaunchKernelGGL(k_init<NS>, dim3(B), dim3(Dim<NS>::NT), l, st, save, w, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, 0); }
    switch (ctx->nseg) { case 1: LAUNCH_INIT(1) break; case 2: LAUNCH_INIT(2) break; case 4: LAUNCH_INIT(4) break; case 6: LAUNCH_INIT(6) break;
        case 8: { const size_t l = DimM<8, 1>::size * sizeof(double);
                  hipLaunchKernelGGL((k_init_m<8, 1>), dim3(B), dim3(512), l, st, save, ctx->d_model, w, ctx->xch, (const double *)nullptr, (const double *)nullptr, (const double *)nullptr, 0); } break; }
#undef LAUNCH_INIT
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}

// g [n][8] and G [n][8][22] of the path constraints at n points (x, u), all device pointers, on ctx->stream
int mpcmp::solver_eval_constraints(mpcmp_ctx *ctx, int n, const double *dx, const double *du, double *dg, double *dG) {
    constexpr int NS = 4;
    const size_t l = EvalLds<NS>::size * sizeof(double);
    if (int rc = set_lds(ctx, k_eval_constraints<NS>, l)) return rc;
    int ms;
    const mpcmp_model *md = run_models(ctx, &ms);
    const int per = ms ? 1 : Dim<NS>::N;           // points per workgroup: one with per-point models (k_eval_constraints)
    hipLaunchKernelGGL(k_eval_constraints<NS>, dim3((n + per - 1) / per), dim3(Dim<NS>::NT), l, ctx->stream, ctx->cfg, md, ms, n, dx, du, dg, dG);
    HIPCHK(ctx, hipGetLastError());
    return MPCMP_OK;
}
