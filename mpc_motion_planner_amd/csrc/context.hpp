// context.hpp — the context behind the opaque mpcmp_ctx of include/mpcmp.h and what the two units that work on it share: the C-ABI unit (mpcmp.hip)
// and the solver's unit (solver.hip).  No kernel and no kernel header is read here, so neither unit compiles the other's kernels.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/mpcmp.h"
#include "solver_types.hpp"
#include "clearance.hpp"
#include "model_host.hpp"

struct mpcmp_ctx {
    mpcmp_config cfg;
    int device = 0, max_batch = 0, nseg = 0, narm = 1;
    int N = 0, n = 0, meq = 0, m = 0, mn = 0;      // of the whole OCP (all arms): n = 21 N narm + 1, meq = 14 (N-1) narm, m = meq + 8 N narm
    int nx = 14, nu = 7;                           // state / control entries per node: 14 narm, 7 narm
    std::string err;
    hipStream_t stream = nullptr;
    hipStream_t stream_x[3] = {nullptr, nullptr, nullptr};   // further parts of a large solve (see solve_impl)
    hipEvent_t ev_fork = nullptr, ev_join[3] = {nullptr, nullptr, nullptr};
    // device buffers
    mpcmp_model *d_model = nullptr;   // [narm]
    mpcmp_model model;             // host copy: passed by value to the kernels that run the rigid-body recursions
    // per-problem payloads (mpcmp_set_payloads): d_pmodel [max_batch][narm] = the context's models with row b's payloads lumped in, written by
    // k_lump_payloads from d_pay [max_batch][narm]; both allocated by the first mpcmp_set_payloads.  pay_rows = 0: every problem reads d_model
    mpcmp_model *d_pmodel = nullptr;
    mpcmp_payload *d_pay = nullptr;
    int pay_rows = 0;
    // per-problem final-time windows (mpcmp_set_time_windows): d_tbox [max_batch][2] = (lbT, ubT), allocated by the first call; tw_rows = 0: cfg.lbT / ubT
    double *d_tbox = nullptr;
    int tw_rows = 0;
    // per-problem bounds (mpcmp_set_bounds): d_bnd [max_batch] rows of the six bound tables, allocated by the first setter call; bnd_rows = 0: the
    // tables of cfg for every problem
    mpcmp_bounds *d_bnd = nullptr;
    int bnd_rows = 0;
    // the synchronised solve's buffers (mpcmp_solve_batch_synced*), [max_batch] each, allocated by its first call: group keys, member counts and
    // times, the pass-2 mask (WS::retired of pass 2), the pass-1 status words, rows, T_new and stretched start guess
    int *d_sg_count = nullptr, *d_sg_skip = nullptr, *d_sg_status = nullptr;
    unsigned long long *d_sg_key = nullptr;
    double *d_sg_T = nullptr, *d_sg_rows = nullptr, *d_sg_Tn = nullptr, *d_sg_wx = nullptr, *d_sg_wu = nullptr, *d_sg_wT = nullptr;
    // clearance checks (mpcmp_clearance_batch*): the sphere tables of the arms (host copies; d_clr_sph [128] holds them arm-major, allocated by
    // mpcmp_create), the obstacle sets d_clr_obs [clr_sets][clr_nobs] (allocated and grown by mpcmp_set_obstacles*), the selection's keys
    // ([max_batch], allocated by its first call).  Read by no other entry point
    mpcmp_sphere clr_sph[2][mpcmp::CLR_MAX_SPH];
    int clr_nsph[2] = {0, 0};
    mpcmp::ClrSphere *d_clr_sph = nullptr;
    mpcmp_obstacle *d_clr_obs = nullptr;
    size_t clr_obs_cap = 0;
    int clr_sets = 0, clr_nobs = 0;
    bool clr_cert_ready = false;     // ... and the certified kernel's, with and without a timeline, by the first certified call
    bool clr_ready = false;          // the kernel's dynamic-LDS ceiling is set by the first check, so that a context that never checks never asks for it
    unsigned long long *d_sel_key = nullptr;
    // the track table of the obstacle sets (mpcmp_set_obstacle_tracks*, include/mpcmp_moving.h): d_mv_track_of [clr_sets][clr_nobs] and d_mv_off
    // [clr_sets][mv_tracks][mv_keys][3], allocated and grown by the setters; mv_tracks == 0: the world stands still.  Read by the checks of
    // mpcmp_moving.h only
    int *d_mv_track_of = nullptr;
    double *d_mv_off = nullptr;
    size_t mv_tof_cap = 0, mv_off_cap = 0;
    int mv_tracks = 0, mv_keys = 1;
    double mv_t0 = 0.0, mv_dt = 1.0;
    bool mv_ready = false;           // the dynamic-LDS ceilings of its kernels, by the first call of the family
    // the voxel world (mpcmp_set_field*, include/mpcmp_field.h): the grid in force, its occupancy, its squared distance field and the transform's
    // scratch, fld_cap entries each, allocated and grown by the setters and by nothing else; fld_set == false: no field.  Read by
    // mpcmp_clearance_field_batch* and mpcmp_get_field only
    mpcmp_field_desc fld_desc{};
    unsigned char *d_fld_occ = nullptr;
    unsigned *d_fld_d2 = nullptr, *d_fld_tmp = nullptr;
    size_t fld_cap = 0;
    bool fld_set = false;
    bool fld_ready = false;          // the dynamic-LDS ceiling of k_clearance_field, by the first field check
    bool fld_cert_ready = false;     // ... and of k_clearance_cert_field, by the first certified field check (include/mpcmp_field_cert.h)
    // camera frames (include/mpcmp_frame.h): the filter table [128][4] = c_s, R_s^2 of the last frame's posture and one counts record, one
    // allocation made by the family's first use.  Read by mpcmp_set_field_points_filtered*, mpcmp_set_field_depth* and mpcmp_field_carve* only
    double *d_frm_tab = nullptr;
    mpcmp_frame_stats *d_frm_stats = nullptr;
    // via-point routes (mpcmp_solve_route_batch*): [max_batch] rows each, allocated by its first call and never afterwards: the leg states and their
    // start guess, and the legs' records when the caller wants none
    double *d_rt_x0 = nullptr, *d_rt_xf = nullptr, *d_rt_wx = nullptr, *d_rt_wu = nullptr, *d_rt_wT = nullptr;
    mpcmp_info *d_rt_info = nullptr;
    int *d_ext_of_int = nullptr, *d_entry_ptr = nullptr;
    uint32_t *d_terms = nullptr;
    mpcmp::WS ws{};
    std::vector<void *> allocs;
    // host-API staging (device side)
    double *d_x0 = nullptr, *d_xf = nullptr, *d_wx = nullptr, *d_wu = nullptr, *d_wT = nullptr;
    double *d_sx = nullptr, *d_su = nullptr, *d_sT = nullptr;
    double *d_ax0 = nullptr, *d_axf = nullptr, *d_awx = nullptr, *d_awu = nullptr, *d_awT = nullptr;   // multi-arm warm start staging
    mpcmp_info *d_info = nullptr;
    mpcmp::Xch xch{nullptr};              // arm-to-arm exchange slots (multi-arm contexts)
    // what only the solver unit (solver.hip) reads and writes: set up by solver_create, released with the rest by mpcmp_destroy (the timing events are
    // folded and the kernel name reported by mpcmp_kernel_timing)
    struct Solver {
        uint32_t *d_stream = nullptr;
        mpcmp::Qp2Streams streams{};
        mpcmp::Qp3Pat *d_pat = nullptr;       // sparse K_JC pattern of k_qp3 (num_seg 6, 8), device copy
        double *d_fac = nullptr;       // factor workspace of k_qp3f -> k_qp3: [max_batch][narm][Qp3::FAC]
        // num_seg 4: second set of structure tables (structure3.hpp order, T bordered out) for the E-free QP kernels (k_qp3f + k_qp4 / k_qp3)
        int *d3_ext_of_int = nullptr, *d3_entry_ptr = nullptr;
        uint32_t *d3_terms = nullptr;
        uint32_t *d_lane4 = nullptr;   // lane-constant table of k_qp4 (qp4_build_lanes)
        int qp13 = 2;                  // QP kernel of num_seg 4: 2 = k_qp2, 3 = k_qp3f + k_qp3, 4 = k_qp3f + k_qp4 (env MPCMP_QP13)
        int qp19 = 5;                  // QP kernel of num_seg 6, one arm: 5 = k_qp3f<6, 1, 5> + k_qp5 (factor resident in registers), 3 = k_qp3f + k_qp3 (env MPCMP_QP19)
        // timing of the dominant kernel (k_qp)
        struct EvPair { hipEvent_t e[2]; };
        std::vector<EvPair> ev;          // at most MAX_EV pairs are ever created; launches beyond that are not timed until the
        size_t ev_used = 0;              // pairs have been folded by mpcmp_kernel_timing
        static constexpr size_t MAX_EV = 4096;
        const char *loop_kernel = "";    // its name: set with the kernels' LDS limits (solver_create)
        // diagnostics read from the environment ONCE PER CONTEXT, in mpcmp_create (never process-global state)
        bool force_v1 = false, single_stream = false, debug_occ = false;
        int parts_env = 0;                           // MPCMP_STREAMS: parts of a large batch (0 = automatic, see solve_impl)
    } sol;
    // timing of the dominant kernel: the folded event pairs of sol.ev
    double qp_ms = 0.0;
    int qp_launches = 0;
    bool timing = false;             // off until mpcmp_kernel_timing is first called: a plain solve records no events
    // growable device scratch of the host-pointer entry points (Stage: no hipMalloc per call once it is large enough)
    void *scratch = nullptr;
    size_t scratch_bytes = 0;
    // receding-horizon state (mpcmp_rh_*)
    int rh_B = 0;
    size_t lam_count = 0;          // doubles in ws.lam (max_batch x (m + n))
    bool rh_first = true;
    hipGraph_t rh_graph = nullptr;
    hipGraphExec_t rh_exec = nullptr;
    double rh_dt = 0.0;
    int *d_retired = nullptr;                    // [max_batch] arrived instances of the receding-horizon loop (k_advance); not re-solved
    unsigned long long *d_rh_count = nullptr;    // [2] re-solves executed, instances retired now (since mpcmp_rh_init)
    hipEvent_t ev_upd[2] = {nullptr, nullptr};   // with_caller_stream: the caller's stream -> ctx->stream, and back
};

#define HIPCHK(ctx, call)                                                                     \
    do {                                                                                      \
        hipError_t e_ = (call);                                                               \
        if (e_ != hipSuccess) {                                                               \
            std::ostringstream os_;                                                           \
            os_ << #call << " failed: " << hipGetErrorString(e_) << " (" << __FILE__ << ":" << __LINE__ << ")"; \
            if (ctx) (ctx)->err = os_.str();                                                  \
            mpcmp::g_err = os_.str();                                                         \
            return MPCMP_ERUNTIME;                                                            \
        }                                                                                     \
    } while (0)

namespace mpcmp {

// the sizes of one problem (all arms): the context's buffers are allocated with them (create_impl) and sliced by them (split)
struct Dims { int N, n, meq, m, mn; };
constexpr Dims dims_of(int nseg, int narm) {
    const int N = 3 * nseg + 1, n = 21 * N * narm + 1, meq = 14 * (N - 1) * narm, m = meq + 8 * N * narm;
    return {N, n, meq, m, m + n};
}

// One solve as the launch code sees it: B problems, device pointers, the stream it is enqueued on, and everything that makes it differ from a plain
// mpcmp_solve_batch_device.  A call is built where the solve is asked for and passed down by reference: the context holds no mode of a solve in flight
struct SolveCall {
    int B = 0;
    const double *x0 = nullptr, *xf = nullptr;                      // [B][nx]
    const double *wx = nullptr, *wu = nullptr, *wT = nullptr;       // start guess: all three or none (the built-in initialiser)
    double *sx = nullptr, *su = nullptr, *sT = nullptr;
    mpcmp_info *info = nullptr;
    hipStream_t stream = nullptr;
    int only_qp = 0, reguess = 0;
    bool rh_step = false;              // a step of the receding-horizon driver: its defaults of the start flags, its retired instances, no per-problem time / bound rows
    const double *tw_rows = nullptr;   // final-time rows that override the context's (the second pass of a synchronised solve)
    const int *skip = nullptr;         // problems that are not re-solved (the second pass of a synchronised solve)
    bool capturing = false;            // the stream is being captured into a graph: no timing events
};

// the configuration the kernels of a solve see: the two start flags resolved to 0 / 1.  0 = the library default (off for mpcmp_solve_batch, ON for
// the receding-horizon driver), 1 = on, -1 = off everywhere (include/mpcmp.h)
inline mpcmp_config run_config(const mpcmp_ctx *ctx, const SolveCall &c) {
    mpcmp_config cfg = ctx->cfg;
    cfg.qp_warm_start = c.rh_step ? (cfg.qp_warm_start >= 0) : (cfg.qp_warm_start > 0);
    cfg.carry_multipliers = c.rh_step ? (cfg.carry_multipliers >= 0) : (cfg.carry_multipliers > 0);
    return cfg;
}

// the models the dynamics of a call read: the context's [narm], or the per-problem copies [rows][narm] (problem b, arm a: base + b * stride + a)
inline const mpcmp_model *run_models(const mpcmp_ctx *ctx, int *stride) {
    *stride = ctx->pay_rows > 0 ? ctx->narm : 0;
    return ctx->pay_rows > 0 ? ctx->d_pmodel : ctx->d_model;
}
// the final-time rows a solve reads (WS::tbox): the call's own, the context's, or none (cfg.lbT / ubT; always none for the receding-horizon driver)
inline const double *run_rows(const mpcmp_ctx *ctx, const SolveCall &c) {
    if (c.tw_rows) return c.tw_rows;
    return (ctx->tw_rows > 0 && !c.rh_step) ? ctx->d_tbox : nullptr;
}
// the bound rows a solve reads (WS::bnd): the context's, or none (the tables of cfg; always none for the receding-horizon driver)
inline const mpcmp_bounds *run_bounds(const mpcmp_ctx *ctx, const SolveCall &c) { return (ctx->bnd_rows > 0 && !c.rh_step) ? ctx->d_bnd : nullptr; }
// the problems a solve leaves alone (WS::retired): the arrived instances of the receding-horizon loop, or the call's own mask
inline const int *run_retired(const mpcmp_ctx *ctx, const SolveCall &c) { return c.rh_step ? ctx->d_retired : c.skip; }

// device memory the context owns until mpcmp_destroy
template <typename T>
inline int dalloc(mpcmp_ctx *ctx, T **p, size_t count) {
    void *q = nullptr;
    HIPCHK(ctx, hipMalloc(&q, count * sizeof(T)));
    ctx->allocs.push_back(q);
    *p = (T *)q;
    return MPCMP_OK;
}

// the dynamic-LDS ceiling of a kernel
template <typename K>
inline int set_lds(mpcmp_ctx *ctx, K kern, size_t bytes) {
    HIPCHK(ctx, hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
    return MPCMP_OK;
}

}  // namespace mpcmp
