// Certified clearance in a moving world (include/mpcmp_moving_cert.h) from C++, in two parts, each printing one JSON line:
//   host   mpcmp_clearance_certified_timed_one on synthetic plans (a quintic swing of the first and fourth joint) past a pole that drives through
//          the swing, with a wait before and a hold after the motion: no context, no GPU.  With -DMPCMP_SELFTEST_HOST_ONLY this is the whole program,
//          it calls nothing else of the library's checks, and it links against the host-only unit alone:
//            g++ -std=c++17 -DMPCMP_SELFTEST_HOST_ONLY -fsanitize=address,undefined -Iinclude examples/moving_cert_selftest.cpp mpc_motion_planner_amd/csrc/model_host.cpp
//   shim   MotionPlanner::check_clearance_certified_timed on a solved move, the same pole
//            g++ -O2 -std=c++17 -Iinclude examples/moving_cert_selftest.cpp -Lmpc_motion_planner_amd -lmpcmp -Wl,-rpath,$PWD/mpc_motion_planner_amd
#include <cmath>
#include <cstdio>
#include <iostream>
#include <vector>
#ifdef MPCMP_SELFTEST_HOST_ONLY
#include "mpcmp.h"
#else
#include "mpcmp_motion_planner.hpp"
#endif

// the floor, and a pole parked at x = 3 that drives to x = 0.45 and on to x = -2: offsets of one track, 5 keys from t0 = 0.5 every 0.5 s
static void scene(mpcmp_obstacle *obs, int *track_of, double *off) {
    obs[0] = mpcmp_obstacle{}; obs[1] = mpcmp_obstacle{};
    obs[0].type = MPCMP_OBS_HALFSPACE; obs[0].a[2] = 1.0; obs[0].b[0] = -0.05;
    obs[1].type = MPCMP_OBS_CAPSULE; obs[1].a[0] = 3.0; obs[1].a[1] = 0.35; obs[1].a[2] = 0.0;
    obs[1].b[0] = 3.0; obs[1].b[1] = 0.35; obs[1].b[2] = 1.2; obs[1].r = 0.05;
    track_of[0] = -1; track_of[1] = 0;
    const double x[5] = {0.0, -1.5, -2.55, -3.5, -5.0};
    for (int k = 0; k < 5; k++) { off[3 * k] = x[k]; off[3 * k + 1] = 0.0; off[3 * k + 2] = 0.0; }
}

static int host_part() {
    mpcmp_model m;
    mpcmp_default_model(&m);
    mpcmp_sphere sph[3] = {};
    sph[0].joint = 3; sph[0].r = 0.06;
    sph[1].joint = 5; sph[1].r = 0.05;
    sph[2].joint = 6; sph[2].r = 0.03; sph[2].c[0] = m.tool[0]; sph[2].c[1] = m.tool[1]; sph[2].c[2] = m.tool[2];
    const int n_sph = 3;
    mpcmp_obstacle obs[2];
    int track_of[2];
    double off[15];
    scene(obs, track_of, off);
    std::printf("{\"host\": [");
    bool first = true;
    for (int nseg = 1; nseg <= 8; nseg += 7) {
        const int N = 3 * nseg + 1;
        std::vector<double> tau(N), x((size_t)14 * N, 0.0);
        if (mpcmp_time_nodes(nseg, tau.data())) return 3;
        const double q0[7] = {-0.9, -0.4, 0.2, -2.0, 0.1, 1.8, 0.5}, q1[7] = {1.1, -0.4, 0.2, -1.4, 0.1, 1.8, 0.5};
        for (int k = 0; k < N; k++) {
            const double s = tau[k], sg = s * s * s * (10.0 - 15.0 * s + 6.0 * s * s);
            for (int j = 0; j < 7; j++) x[(size_t)14 * k + j] = q0[j] + (q1[j] - q0[j]) * sg;
        }
        // the world at rest; the swing that starts at 0.25 s and meets the pole; the swing that starts at 4 s, behind the pole, after a wait from
        // world time 0 during which the pole passes the start posture, and with a hold of 1 s
        mpcmp_clearance still, meet, late;
        mpcmp_clearance_cert c_still, c_meet, c_late;
        if (mpcmp_clearance_certified_timed_one(&m, 1, nseg, &n_sph, sph, 2, obs, nullptr, 0, 1, 0.0, 1.0, nullptr, x.data(), 2.0, 0.25, 0.0, 0.0, 0.02, 0, 4,
                                                2, 10, &still, &c_still)) return 4;
        if (mpcmp_clearance_certified_timed_one(&m, 1, nseg, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 2.0, 0.25, 0.0, 0.0, 0.02, 0, 4,
                                                2, 10, &meet, &c_meet)) return 4;
        if (mpcmp_clearance_certified_timed_one(&m, 1, nseg, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 2.0, 4.0, 4.0, 1.0, 0.02, 0, 4,
                                                2, 10, &late, &c_late)) return 4;
        std::printf("%s[%d, %d, %.17g, %.17g, %d, %d, %.17g, %.17g, %.17g, %d, %d, %d, %.17g, %.17g, %.17g, %d, %d]", first ? "" : ", ", nseg, still.status,
                    still.d_min, c_still.d_lower, c_still.n_eval, meet.status, meet.d_min, meet.t_min, c_meet.d_lower, c_meet.n_eval, c_meet.depth,
                    late.status, late.d_min, late.t_min, c_late.d_lower, c_late.n_eval, c_late.n_undecided);
        first = false;
    }
    // refused: nothing is written
    mpcmp_clearance r = {};
    r.n_hit = 77;
    std::vector<double> x((size_t)14 * 4, 0.0);
    if (mpcmp_clearance_certified_timed_one(&m, 1, 1, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 1.0, 0.0, -0.1, 0.0, 0.0, 0, 4, 2, 10, &r,
                                            nullptr) != MPCMP_EINVAL || r.n_hit != 77) return 6;
    if (mpcmp_clearance_certified_timed_one(&m, 1, 1, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 1.0, 0.0, 0.0, 0.0, 0.0, 0, 4, 0, 10, &r,
                                            nullptr) != MPCMP_EINVAL || r.n_hit != 77) return 6;
    std::printf("]}\n");
    return 0;
}

int main() {
    if (int rc = host_part()) return rc;
#ifndef MPCMP_SELFTEST_HOST_ONLY
    try {
        MotionPlanner planner("", 4, 2);
        MotionPlanner::Vec7 q0, q1, rest = MotionPlanner::Vec7::Zero();
        const double a[7] = {-0.9, -0.4, 0.2, -2.0, 0.1, 1.8, 0.5}, b[7] = {1.1, -0.4, 0.2, -1.4, 0.1, 1.8, 0.5};
        for (int j = 0; j < 7; j++) { q0(j) = a[j]; q1(j) = b[j]; }
        planner.set_current_state(q0, rest);
        planner.set_target_state(q1, rest);
        planner.solve_trajectory(true);
        mpcmp_obstacle obs[2];
        int track_of[2];
        double off[15];
        scene(obs, track_of, off);
        planner.set_obstacles(obs, 2);
        mpcmp_clearance_cert c_still, c_static, c_meet, c_late;
        const mpcmp_clearance still = planner.check_clearance_certified_timed(0.25, 0.0, 0.0, 0.02, 0, 4, 2, 10, &c_still);
        const mpcmp_clearance stat = planner.check_clearance_certified(0.02, 0, 4, 10, &c_static);
        planner.set_moving_obstacles(2, track_of, 1, 5, 0.5, 0.5, off);
        const mpcmp_clearance meet = planner.check_clearance_certified_timed(0.25, 0.0, 0.0, 0.02, 0, 4, 2, 10, &c_meet);
        const mpcmp_clearance late = planner.check_clearance_certified_timed(4.0, 4.0, 1.0, 0.02, 0, 4, 2, 10, &c_late);
        std::printf("{\"still_status\": %d, \"still_d_min\": %.17g, \"still_d_lower\": %.17g, \"static_status\": %d, \"static_d_min\": %.17g, "
                    "\"static_d_lower\": %.17g, \"static_n_eval\": %d, \"still_n_eval\": %d, \"meet_status\": %d, \"meet_d_min\": %.17g, "
                    "\"meet_d_lower\": %.17g, \"late_status\": %d, \"late_d_min\": %.17g, \"late_d_lower\": %.17g, \"late_t_min\": %.17g}\n",
                    still.status, still.d_min, c_still.d_lower, stat.status, stat.d_min, c_static.d_lower, c_static.n_eval, c_still.n_eval, meet.status,
                    meet.d_min, c_meet.d_lower, late.status, late.d_min, c_late.d_lower, late.t_min);
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
#endif
    return 0;
}
