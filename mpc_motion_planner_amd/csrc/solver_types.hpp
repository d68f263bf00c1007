// solver_types.hpp — the small types, status bits and layout rules that the solver's kernels (solver_kernels.hpp, qp_kernel_v*.hpp,
// multi_kernels.hpp), the context (context.hpp) and the leaf kernels of the C-ABI unit share.  Nothing here is a kernel, so including this header
// does not change what any translation unit compiles to.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/mpcmp.h"

namespace mpcmp {

struct WS {
    const mpcmp_model *model;
    const int *ext_of_int;
    const int *entry_ptr;
    const uint32_t *terms;
    const double *x0, *xf;    // [B][14]
    double *z;                // [B][n]
    double *lam;              // [B][m+n]
    double *ceq;              // [B][meq]
    double *g;                // [B][8N]
    double *Gk;               // [B][N][8][22]
    double *p;                // [B][n]
    double *y;                // [B][m+n]
    int *qpit;                // [B] iterations of the last QP
    int *perm;                // [B] launch order of the QP kernel: workgroup g solves problem perm[g] (longest expected first)
    int *okey;                // [B] ordering key: decayed maximum of the problem's previous QP iteration counts
    int *done;                // [1] workgroups of the running step launch that have finished (the last one computes the next QP order)
    int *qp_total;            // [B]
    int *status;              // [B]
    double *alpha;            // [B]
    unsigned long long *dbg;  // [B][MPCMP_DBG_WORDS] phase cycle stamps (diagnostic builds with -DMPCMP_STAMPS only)
    const int *retired;       // [B] or null: receding-horizon instances that have arrived (k_advance) are not re-solved: every solve kernel returns at once (at N = 25 the QP kernels k_qp3f / k_qp3 still run, results discarded)
    const double *alt_x, *alt_u, *alt_T;   // or null: the receding-horizon driver's start guess (jerk-limited trajectory from the current state) for an instance
                                           // that cannot be re-guessed from its previous solve (k_init: reguess && prev_bad); null = the built-in initialiser
    int mstride;              // models per problem behind `model`: 0 = one model (per arm) for every problem; narm = per-problem models
                              // (mpcmp_set_payloads): problem b of the launch, arm a reads model + b * mstride + a
    const double *tbox;       // [B][2] or null: final-time window (lbT, ubT) of problem b (mpcmp_set_time_windows, the second pass of a synchronised
                              // solve); null = cfg.lbT / cfg.ubT for every problem.  Indexed by the problem (after perm), offset by a part's b0 like retired
    const mpcmp_bounds *bnd;  // [B] or null: the six bound tables of problem b (mpcmp_set_bounds); null = the configuration's for every problem.  Indexed
                              // and offset like tbox
};
// a retired instance of the receding-horizon loop: the whole workgroup leaves (uniform)
#define MPCMP_RETIRED(ws_, b_) ((ws_).retired != nullptr && (ws_).retired[b_] != 0)

// ws.status[b] while a solve runs: bits 0..6 = status bits of mpcmp_info (include/mpcmp.h), bits 8..30 = number of QPs that ran out of
// iterations (every QP kernel adds MPCMP_ST_CAP_ONE then); k_step / k_step_m fold it into the record.  Bit 7 (MPCMP_ST_RESTART) is set between two
// steps of the receding-horizon driver only (k_rh_update: new target, revival, MPCMP_RH_RESTART) and cleared by k_init / k_init_m with the whole word
#define MPCMP_ST_CAP_ONE 0x100
#define MPCMP_ST_RESTART 0x80
// the solve failed hard or left the box of T: there is no trajectory to follow (k_advance holds the state)
#define MPCMP_ST_FAILED (MPCMP_STATUS_NAN | MPCMP_STATUS_NOT_PD | MPCMP_STATUS_XCH_DEAD | MPCMP_STATUS_T_OUT_OF_BOX)
// the slot's previous solve is no start for the next one (neither a re-guess nor carried multipliers): it failed, or the caller asked for a restart
#define MPCMP_ST_NO_GUESS (MPCMP_ST_FAILED | MPCMP_ST_RESTART)
#define MPCMP_DBG_WORDS 160   /* 16 workgroup stamps + [16 waves][8] per-wave busy cycles of k_qp2 + 16 stamps of k_step */

// pass metadata of the assembly streams of k_qp2 (structure.hpp: build_streams)
struct Qp2Streams {
    const uint32_t *words;
    int npass;
    int off[8], W[8];
    int split_dst, split_scr, split_n;
};

// sparse K_JC pattern of k_qp3 (structure3.hpp): the context holds a device copy by pointer only
struct Qp3Pat;

// inter-workgroup exchange between the two arm workgroups of one OCP (NARM = 2): 8-byte data-tagged granules, agent-scope
// relaxed atomics on both sides (MI355X_MICROARCH.md, "Workgroup dispatch, XCD placement & inter-workgroup visibility": valid
// form for <= 8-byte hand-offs, placement independent).  Every slot is written once per launch; k_init_m / k_step_m reset the
// slots of their problem to XCH_EMPTY before the next QP launch.  Every spin is bounded (qp_kernel_v3.hpp: xch_post, xch_poll).
#define MPCMP_XCH_STRIDE 1024
#define MPCMP_XCH_EMPTY 0x7FF8DEADBEEF0001ull          /* a NaN payload no arithmetic produces */
struct Xch {
    unsigned long long *buf;        // [B][2][MPCMP_XCH_STRIDE]
};

// index of component r in [0,14) of arm a in an external state vector [q(7 NARM); qd(7 NARM)]
template <int NARM>
__device__ __forceinline__ int ext_x(int a, int r) { return r < 7 ? 7 * a + r : 7 * NARM + 7 * a + (r - 7); }

}  // namespace mpcmp
