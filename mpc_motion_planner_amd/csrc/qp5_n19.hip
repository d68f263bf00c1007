// qp5_n19.hip — the kernel pair of the reference-as-shipped discretisation (N = 19, one arm): k_qp3f<6, 1, 5> + k_qp5<6>, as a translation unit of
// their own (like qp3_n25.hip: the machine scheduler's strategy is an option of the whole compilation).  The Makefile builds this file with the strategy
// named there; solver.hip (compiled with -DMPCMP_SPLIT_N19) only declares the two kernels.  A build of solver.hip without that macro still
// contains everything.
#include <hip/hip_runtime.h>
#include "../../include/mpcmp.h"
#include "qp_kernel_v3.hpp"
#include "qp_kernel_v5.hpp"

namespace mpcmp {
template __global__ void k_qp3f<6, 1, 5>(mpcmp_config, WS, const Qp3Pat *, Xch, int, double *);
template __global__ void k_qp5<6>(mpcmp_config, WS, const Qp3Pat *, Xch, int, const double *);
}  // namespace mpcmp
