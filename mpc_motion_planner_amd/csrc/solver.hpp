// solver.hpp — what the C-ABI unit (mpcmp.hip) calls of the solver's unit (solver.hip): four functions on a context.  The kernels of the SQP chain,
// their selection, their dynamic-LDS limits and their launch code live in solver.hip; nothing here is a kernel or reads a kernel header.
// Every function returns an mpcmp status and leaves the reason of a failure in ctx->err.
#pragma once
#include "context.hpp"

namespace mpcmp {

// The solver's side of mpcmp_create, on a context whose configuration, sizes, streams and device are set: reads the solver's environment knobs
// (MPCMP_QP13, MPCMP_QP19, MPCMP_FORCE_V1, MPCMP_SINGLE_STREAM, MPCMP_DEBUG_OCC, MPCMP_STREAMS), builds and uploads the structure and stream tables
// (ctx->d_ext_of_int / d_entry_ptr / d_terms and their pointers in ctx->ws, ctx->sol), allocates the factor workspace and sets the kernels' LDS limits.
// On failure the caller destroys the context, which releases what was allocated.
int solver_create(mpcmp_ctx *ctx);
// one solve (or one QP: c.only_qp) of c.B <= max_batch checked problems, enqueued on c.stream
int solver_run(mpcmp_ctx *ctx, const SolveCall &c);
// the built-in start guess of the B staged problems (ctx->d_x0, ctx->d_xf; single arm) into ctx->ws.z, enqueued on st
int solver_init_guess(mpcmp_ctx *ctx, int B, hipStream_t st);
// path constraints g [n][8] and their Jacobians G [n][8][22] at n points x [n][14], u [n][7] (device pointers), enqueued on ctx->stream
int solver_eval_constraints(mpcmp_ctx *ctx, int n, const double *d_x, const double *d_u, double *d_g, double *d_G);

}  // namespace mpcmp
