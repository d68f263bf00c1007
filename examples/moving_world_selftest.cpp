// Clearance in a moving world (include/mpcmp_moving.h) from C++, in two parts, each printing one JSON line:
//   host   mpcmp_track_offset, mpcmp_clearance_timed_one and mpcmp_start_delay_one on synthetic plans (a quintic swing of the first and fourth
//          joint) past a pole that drives through the swing: no context, no GPU.  With -DMPCMP_SELFTEST_HOST_ONLY this is the whole program, and
//          it links against the host-only unit alone:
//            g++ -std=c++17 -DMPCMP_SELFTEST_HOST_ONLY -fsanitize=address,undefined -Iinclude examples/moving_world_selftest.cpp mpc_motion_planner_amd/csrc/model_host.cpp
//   shim   MotionPlanner::check_clearance_timed and MotionPlanner::first_clear_start on a solved move, the same pole
//            g++ -O2 -std=c++17 -Iinclude examples/moving_world_selftest.cpp -Lmpc_motion_planner_amd -lmpcmp -Wl,-rpath,$PWD/mpc_motion_planner_amd
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
    double off[15], p[3];
    scene(obs, track_of, off);
    // the offset at a key, between two keys, before the first and after the last
    const double taus[4] = {1.0, 1.25, -3.0, 9.0}, want[4] = {-1.5, -2.025, 0.0, -5.0};
    for (int i = 0; i < 4; i++)
        if (mpcmp_track_offset(5, 0.5, 0.5, off, taus[i], p) || std::fabs(p[0] - want[i]) > 1e-15 || p[1] != 0.0) return 2;
    if (mpcmp_track_offset(1, 0.5, 0.5, off + 3, 7.0, p) || p[0] != -1.5) return 2;
    if (mpcmp_track_offset(5, 0.5, 0.0, off, 1.0, p) != MPCMP_EINVAL) return 2;
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
        // a profile at half rate: t_k = 2 T k / n, x_k = 1 / 4
        const int n_grid = 8;
        double prof[2 * (8 + 1)];
        for (int k = 0; k <= n_grid; k++) { prof[2 * k] = 2.0 * 2.0 * k / n_grid; prof[2 * k + 1] = 0.25; }
        mpcmp_clearance still, moving, slow;
        if (mpcmp_clearance_timed_one(&m, 1, nseg, &n_sph, sph, 2, obs, nullptr, 0, 1, 0.0, 1.0, nullptr, x.data(), 2.0, 0, nullptr, 0.0, 100, 0.02, 0, &still))
            return 4;
        if (mpcmp_clearance_timed_one(&m, 1, nseg, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 2.0, 0, nullptr, 0.25, 100, 0.02, 0, &moving))
            return 4;
        if (mpcmp_clearance_timed_one(&m, 1, nseg, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 2.0, n_grid, prof, 0.25, 100, 0.02, 0, &slow))
            return 4;
        const double delays[6] = {0.0, 0.5, 1.0, 1.5, 2.0, 4.0};
        double d_all[6];
        mpcmp_start_delay sd, sdw;
        if (mpcmp_start_delay_one(&m, 1, nseg, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 2.0, 0, nullptr, 6, delays, 0, 100, 0.02, 0,
                                  d_all, &sd)) return 5;
        if (mpcmp_start_delay_one(&m, 1, nseg, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, 0.5, off, x.data(), 2.0, 0, nullptr, 6, delays, 1, 100, 0.02, 0,
                                  nullptr, &sdw)) return 5;
        std::printf("%s[%d, %d, %.17g, %d, %.17g, %.17g, %d, %.17g, %.17g, %d, %d, %.17g, %.17g, %d, %d, %.17g]", first ? "" : ", ", nseg, still.status,
                    still.d_min, moving.status, moving.d_min, moving.t_min, slow.status, slow.d_min, slow.t_min, sd.index, sd.n_clear, sd.delay, sd.d_min,
                    sdw.index, sdw.status, d_all[sd.index >= 0 ? sd.index : 0]);
        first = false;
    }
    // refused: nothing is written
    mpcmp_clearance r = {};
    r.n_hit = 77;
    std::vector<double> x((size_t)14 * 4, 0.0);
    if (mpcmp_clearance_timed_one(&m, 1, 1, &n_sph, sph, 2, obs, track_of, 1, 5, 0.5, -0.5, off, x.data(), 1.0, 0, nullptr, 0.0, 10, 0.0, 0, &r) != MPCMP_EINVAL ||
        r.n_hit != 77) return 6;
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
        const mpcmp_clearance still = planner.check_clearance_timed(0.0, 200, 0.02);
        planner.set_moving_obstacles(2, track_of, 1, 5, 0.5, 0.5, off);
        const mpcmp_clearance moving = planner.check_clearance_timed(0.25, 200, 0.02);
        const double delays[6] = {0.0, 0.5, 1.0, 1.5, 2.0, 4.0};
        const mpcmp_start_delay sd = planner.first_clear_start(delays, 6, true, 200, 0.02);
        const mpcmp_clearance again = planner.check_clearance_timed(sd.index >= 0 ? sd.delay : 0.0, 200, 0.02);
        planner.set_obstacles(obs, 2);                        // (the world stands still again)
        const mpcmp_clearance reset = planner.check_clearance_timed(0.25, 200, 0.02);
        std::printf("{\"still_status\": %d, \"still_d_min\": %.17g, \"moving_status\": %d, \"moving_d_min\": %.17g, \"index\": %d, \"delay\": %.17g, "
                    "\"n_clear\": %d, \"again_status\": %d, \"reset_d_min\": %.17g}\n",
                    still.status, still.d_min, moving.status, moving.d_min, sd.index, sd.delay, sd.n_clear, again.status, reset.d_min);
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
#endif
    return 0;
}
