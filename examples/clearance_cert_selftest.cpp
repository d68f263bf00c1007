// Certified clearance (include/mpcmp_clearance_cert.h) from C++, in two parts, each printing one JSON line:
//   host   mpcmp_clearance_certified_one on a synthetic plan (a quintic swing of the first and fourth joint) past a thin pole: no context, no GPU.
//          With -DMPCMP_SELFTEST_HOST_ONLY this is the whole program, and it links against the host-only unit alone:
//            g++ -std=c++17 -DMPCMP_SELFTEST_HOST_ONLY -fsanitize=address,undefined -Iinclude examples/clearance_cert_selftest.cpp mpc_motion_planner_amd/csrc/model_host.cpp
//   shim   MotionPlanner::check_clearance_certified on a tool line (a lift of 15 cm) beside a pole, next to the sampled MotionPlanner::clearance
//            g++ -O2 -std=c++17 -Iinclude examples/clearance_cert_selftest.cpp -Lmpc_motion_planner_amd -lmpcmp -Wl,-rpath,$PWD/mpc_motion_planner_amd
#include <cmath>
#include <cstdio>
#include <iostream>
#include <vector>
#ifdef MPCMP_SELFTEST_HOST_ONLY
#include "mpcmp.h"
#else
#include "mpcmp_motion_planner.hpp"
#endif

static int host_part() {
    mpcmp_model m;
    mpcmp_default_model(&m);
    // three spheres: on the elbow, on the wrist and at the tool point
    mpcmp_sphere sph[3] = {};
    sph[0].joint = 3; sph[0].r = 0.06;
    sph[1].joint = 5; sph[1].r = 0.05;
    sph[2].joint = 6; sph[2].r = 0.03; sph[2].c[0] = m.tool[0]; sph[2].c[1] = m.tool[1]; sph[2].c[2] = m.tool[2];
    const int n_sph = 3;
    mpcmp_obstacle obs[2] = {};
    obs[0].type = MPCMP_OBS_HALFSPACE; obs[0].a[2] = 1.0; obs[0].b[0] = -0.05;                        // the floor
    obs[1].type = MPCMP_OBS_CAPSULE; obs[1].a[0] = 0.45; obs[1].a[1] = 0.35; obs[1].a[2] = 0.0;      // a pole of 1 cm
    obs[1].b[0] = 0.45; obs[1].b[1] = 0.35; obs[1].b[2] = 1.2; obs[1].r = 0.005;
    std::printf("{\"host\": [");
    bool first = true;
    for (int nseg = 1; nseg <= 8; nseg += 7) {
        const int N = 3 * nseg + 1;
        std::vector<double> tau(N), x((size_t)14 * N, 0.0);
        if (mpcmp_time_nodes(nseg, tau.data())) return 2;
        const double q0[7] = {-0.9, -0.4, 0.2, -2.0, 0.1, 1.8, 0.5}, q1[7] = {1.1, -0.4, 0.2, -1.4, 0.1, 1.8, 0.5};
        for (int k = 0; k < N; k++) {
            const double s = tau[k], sg = s * s * s * (10.0 - 15.0 * s + 6.0 * s * s);
            for (int j = 0; j < 7; j++) x[(size_t)14 * k + j] = q0[j] + (q1[j] - q0[j]) * sg;
        }
        for (int depth = 0; depth <= 12; depth += 6) {
            mpcmp_clearance r;
            mpcmp_clearance_cert c;
            if (mpcmp_clearance_certified_one(&m, 1, nseg, &n_sph, sph, 2, obs, x.data(), 2.0, 0.0, 2, 4, depth, &r, &c)) return 3;
            std::printf("%s[%d, %d, %d, %d, %.17g, %.17g, %.17g, %d, %d, %d, %d]", first ? "" : ", ", nseg, depth, r.status, r.n_hit, r.d_min, r.t_min, c.d_lower,
                        c.n_eval, c.n_clear, c.n_undecided, c.depth);
            first = false;
        }
    }
    // refused: nothing is written
    mpcmp_clearance r = {};
    r.n_hit = 77;
    std::vector<double> x((size_t)14 * 4, 0.0);
    if (mpcmp_clearance_certified_one(&m, 1, 1, &n_sph, sph, 2, obs, x.data(), 1.0, 0.0, 0, 4, 17, &r, nullptr) != MPCMP_EINVAL || r.n_hit != 77) return 4;
    std::printf("]}\n");
    return 0;
}

int main() {
    if (int rc = host_part()) return rc;
#ifndef MPCMP_SELFTEST_HOST_ONLY
    try {
        MotionPlanner planner("", 8, 2);                      // 25 nodes
        MotionPlanner::Vec7 q0, rest = MotionPlanner::Vec7::Zero();
        const double bent[7] = {0.3, -0.4, 0.2, -2.0, 0.1, 1.8, 0.5};
        for (int j = 0; j < 7; j++) q0(j) = bent[j];
        planner.set_current_state(q0, rest);
        double J[42], p0[3], R0[9];
        mpcmp_tool_jacobian(&planner.robot.model, bent, J, p0, R0);
        const double p1[3] = {p0[0], p0[1], p0[2] + 0.15};
        const mpcmp_tool_line tl = planner.plan_tool_line(R0, p1);
        // the floor, and a horizontal pole 20 cm in front of the tool's line
        mpcmp_obstacle obs[2] = {};
        obs[0].type = MPCMP_OBS_HALFSPACE; obs[0].a[2] = 1.0; obs[0].b[0] = -0.05;
        obs[1].type = MPCMP_OBS_CAPSULE; obs[1].r = 0.005;
        obs[1].a[0] = p0[0] + 0.2; obs[1].a[1] = p0[1] - 0.5; obs[1].a[2] = p0[2] + 0.07;
        obs[1].b[0] = p0[0] + 0.2; obs[1].b[1] = p0[1] + 0.5; obs[1].b[2] = p0[2] + 0.07;
        planner.set_obstacles(obs, 2);
        const mpcmp_clearance sampled = planner.clearance(200, 0.02);
        mpcmp_clearance_cert cert;
        const mpcmp_clearance certified = planner.check_clearance_certified(0.02, 0, 4, 10, &cert);
        const mpcmp_clearance coarse = planner.check_clearance_certified(0.02, 0, 1, 0);
        std::printf("{\"tl_status\": %d, \"sampled_status\": %d, \"sampled_d_min\": %.17g, \"status\": %d, \"d_min\": %.17g, \"d_lower\": %.17g, "
                    "\"n_eval\": %d, \"n_clear\": %d, \"n_undecided\": %d, \"depth\": %d, \"coarse_status\": %d}\n",
                    tl.status, sampled.status, sampled.d_min, certified.status, certified.d_min, cert.d_lower, cert.n_eval, cert.n_clear,
                    cert.n_undecided, cert.depth, coarse.status);
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
#endif
    return 0;
}
