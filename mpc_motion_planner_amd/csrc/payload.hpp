// payload.hpp — lumping rigid bodies into body 7 of a model (parallel-axis theorem), shared by the host and the device.
//
// One formula for three uses: mpcmp_default_model lumps the Panda's fixed children of link7 (link8, panda_tool) into body 7,
// mpcmp_model_add_payload adds a payload on the host, and k_lump_payloads writes the per-problem models of mpcmp_set_payloads[_device].
// FP contraction is off inside, so that the host and the device round every operation alike and the two agree bit for bit.
#pragma once
#include "../../include/mpcmp.h"

// (model_host.cpp is plain C++: it reads the two functions without the HIP runtime's header, and not the kernel)
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define MPCMP_PAYLOAD_HD __host__ __device__ inline
#else
#define MPCMP_PAYLOAD_HD inline
#endif

namespace mpcmp {

// body 7 of m := the nb bodies (masses mk, COMs ck and rotational inertias about their COMs Ik, all in the joint-7 frame) lumped into one
MPCMP_PAYLOAD_HD void lump_last_body(mpcmp_model *m, int nb, const double *mk, const double (*ck)[3], const double (*Ik)[9]) {
#pragma clang fp contract(off)
    double M = 0.0, c[3] = {0, 0, 0};
    for (int k = 0; k < nb; k++) M += mk[k];
    for (int k = 0; k < nb; k++) for (int d = 0; d < 3; d++) c[d] += mk[k] * ck[k][d];
    for (int d = 0; d < 3; d++) c[d] /= M;
    double It[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
    for (int k = 0; k < nb; k++) {
        const double d[3] = {ck[k][0] - c[0], ck[k][1] - c[1], ck[k][2] - c[2]};
        const double d2 = d[0] * d[0] + d[1] * d[1] + d[2] * d[2];
        for (int r = 0; r < 3; r++) for (int s = 0; s < 3; s++)
            It[3 * r + s] += Ik[k][3 * r + s] + mk[k] * ((r == s ? d2 : 0.0) - d[r] * d[s]);
    }
    m->mass[6] = M;
    for (int d = 0; d < 3; d++) m->com[6][d] = c[d];
    for (int q = 0; q < 9; q++) m->I[6][q] = It[q];
}

// out := m with the payload p added to body 7 (out may alias m).  A payload with mass 0 and I = 0 leaves the model as it is, bit for bit.
MPCMP_PAYLOAD_HD void add_payload(const mpcmp_model *m, const mpcmp_payload *p, mpcmp_model *out) {
    if (out != m) *out = *m;
    bool zero = p->mass == 0.0;
    for (int q = 0; q < 9; q++) zero = zero && p->I[q] == 0.0;
    if (zero) return;
    const double mk[2] = {out->mass[6], p->mass};
    const double ck[2][3] = {{out->com[6][0], out->com[6][1], out->com[6][2]}, {p->com[0], p->com[1], p->com[2]}};
    double Ik[2][9];
    for (int q = 0; q < 9; q++) { Ik[0][q] = out->I[6][q]; Ik[1][q] = p->I[q]; }
    lump_last_body(out, 2, mk, ck, Ik);
}

#ifdef __HIPCC__
// per-problem models of mpcmp_set_payloads[_device]: one thread per (row, arm), out[row][arm] = add_payload(base[arm], p[row][arm])
__global__ __launch_bounds__(256) void k_lump_payloads(const mpcmp_model *base, int narm, int rows, const mpcmp_payload *p, mpcmp_model *out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * narm) return;
    add_payload(base + i % narm, p + i, out + i);
}
#endif

}  // namespace mpcmp
