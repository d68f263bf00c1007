// Drives the retimed-check members of the header-only MotionPlanner shim (check_retimed_limits, check_retimed_route_limits) and prints their records
// as one JSON line for tests/test_gpu_retimed_check.py: a move between states at rest, retimed and checked between its grid points, then the same
// move through one via point as a route.  Both members throw while no profile is present.
//   g++ -O2 -std=c++17 -Iinclude examples/retimed_check_selftest.cpp -Lmpc_motion_planner_amd -lmpcmp -Wl,-rpath,$PWD/mpc_motion_planner_amd
#include <cmath>
#include <cstdio>
#include <iostream>
#include <vector>
#include "mpcmp_motion_planner.hpp"

int main() {
    try {
        MotionPlanner planner("", 4, 3);
        MotionPlanner::Vec7 q0, qT, via, rest = MotionPlanner::Vec7::Zero();
        const double a[7] = {0.0, -0.4, 0.0, -2.0, 0.0, 1.6, 0.5}, b[7] = {0.8, 0.3, -0.5, -1.2, 0.4, 2.2, -0.3};
        for (int j = 0; j < 7; j++) { q0(j) = a[j]; qT(j) = b[j]; via(j) = 0.5 * (a[j] + b[j]) + (j == 1 ? 0.15 : 0.0); }
        planner.set_current_state(q0, rest);
        planner.set_target_state(qT, rest);
        int threw = 0;
        try { planner.check_retimed_limits(); } catch (const std::runtime_error &) { threw |= 1; }
        try { planner.check_retimed_route_limits(); } catch (const std::runtime_error &) { threw |= 2; }
        planner.solve_trajectory(true);
        try { planner.check_retimed_limits(); } catch (const std::runtime_error &) { threw |= 4; }
        mpcmp_limits_spec ls = {};
        for (int g = 0; g < MPCMP_LIM_GROUPS; g++) ls.tol[g] = 1e-6;
        ls.tool_lin_max = 1.7; ls.tool_ang_max = 2.5;
        mpcmp_retime_spec rs = {};
        rs.tool_lin_max = 1.7; rs.tool_ang_max = 2.5; rs.rate_max = 1.0; rs.groups = MPCMP_RT_ALL_GROUPS;
        const mpcmp_retime rt = planner.retime(50, &rs);
        double T_new = -1.0;
        const mpcmp_limits lim = planner.check_retimed_limits(200, &ls, &T_new);
        const mpcmp_limits lim0 = planner.check_retimed_limits(200, &ls);          // (T_new may be left out)
        auto fin = [](double x) { return std::isfinite(x) ? x : -1.0; };            // (JSON has no inf / nan)
        std::printf("{\"threw\": %d, \"rt_status\": %d, \"rt_T_new\": %.17g, \"T_new\": %.17g, \"status\": %d, \"same\": %d, \"stretch\": %.17g, "
                    "\"excess_qdd\": %.17g, \"t_at_qdd\": %.17g, \"channel_qdd\": %d, \"n_viol\": %d, ",
                    threw, rt.status, fin(rt.T_new), fin(T_new), lim.status, (int)(lim.status == lim0.status && lim.stretch == lim0.stretch),
                    lim.stretch, fin(lim.excess[MPCMP_LIM_QDD]), lim.t_at[MPCMP_LIM_QDD], lim.channel[MPCMP_LIM_QDD], lim.n_viol);
        planner.solve_route(std::vector<MotionPlanner::Vec7>{via});
        int route_threw = 0;
        try { planner.check_retimed_route_limits(); } catch (const std::runtime_error &) { route_threw = 1; }
        const mpcmp_route_retime rr = planner.retime_route(50, &rs);
        double route_T_new = -1.0;
        const mpcmp_limits rl = planner.check_retimed_route_limits(200, &ls, &route_T_new);
        std::printf("\"route_threw\": %d, \"route_rt_status\": %d, \"route_rt_T_new\": %.17g, \"route_T_new\": %.17g, \"route_status\": %d, "
                    "\"route_stretch\": %.17g, \"route_excess_qdd\": %.17g, \"route_t_at_qdd\": %.17g, \"route_n_viol\": %d}\n",
                    route_threw, rr.status, fin(rr.T_new), fin(route_T_new), rl.status, rl.stretch, fin(rl.excess[MPCMP_LIM_QDD]),
                    rl.t_at[MPCMP_LIM_QDD], rl.n_viol);
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
