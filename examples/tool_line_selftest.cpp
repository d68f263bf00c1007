// Drives the tool-line members of the header-only MotionPlanner shim (plan_tool_line, check_tool_line) and what applies to their plan afterwards
// (check_limits, retime, get_retimed_trajectory, get_MPC_trajectory), and prints the records as one JSON line for tests/test_gpu_toolpath.py:
// a lift of 15 cm straight up from a bent posture, planned by the duration rule, checked, retimed to its limits (rate_max 4) and sampled.
//   g++ -O2 -std=c++17 -Iinclude examples/tool_line_selftest.cpp -Lmpc_motion_planner_amd -lmpcmp -Wl,-rpath,$PWD/mpc_motion_planner_amd
#include <cmath>
#include <cstdio>
#include <iostream>
#include "mpcmp_motion_planner.hpp"

int main() {
    try {
        MotionPlanner planner("", 8, 2);                      // 25 nodes
        MotionPlanner::Vec7 q0, rest = MotionPlanner::Vec7::Zero();
        const double bent[7] = {0.3, -0.4, 0.2, -2.0, 0.1, 1.8, 0.5};
        for (int j = 0; j < 7; j++) q0(j) = bent[j];
        planner.set_current_state(q0, rest);
        // the start pose from the host kinematics, the goal 15 cm above it with the same orientation
        double J[42], p0[3], R0[9];
        mpcmp_tool_jacobian(&planner.robot.model, bent, J, p0, R0);
        const double p1[3] = {p0[0], p0[1], p0[2] + 0.15};
        const mpcmp_tool_line tl = planner.plan_tool_line(R0, p1);
        const mpcmp_tool_dev dev = planner.check_tool_line(200, 1e-4, 1e-4);
        mpcmp_limits_spec ls = {};
        ls.tool_lin_max = 1.7; ls.tool_ang_max = 2.5;
        const mpcmp_limits lim = planner.check_limits(200, &ls);
        mpcmp_retime_spec rs = {};
        rs.tool_lin_max = 1.7; rs.tool_ang_max = 2.5; rs.rate_max = 4.0; rs.groups = MPCMP_RT_ALL_GROUPS;
        const mpcmp_retime rt = planner.retime(200, &rs);
        mpcmp_shim::Mat<1, 51> t;
        mpcmp_shim::Mat<7, 51> q, v, a, tau;
        planner.get_retimed_trajectory<50>(t, q, v, a, tau);
        // the retimed samples stay on the line: the largest distance of their tool position from it
        double off = 0.0, rise = 0.0;
        for (int i = 0; i <= 50; i++) {
            double qi[7], p[3], R[9];
            for (int j = 0; j < 7; j++) qi[j] = q(j, i);
            mpcmp_tool_jacobian(&planner.robot.model, qi, J, p, R);
            off = std::fmax(off, std::hypot(p[0] - p0[0], p[1] - p0[1]));
            if (i == 50) rise = p[2] - p0[2];
        }
        planner.get_MPC_trajectory<50>(t, q, v, a, tau);
        std::printf("{\"T\": %.17g, \"tl_status\": %d, \"k_fail\": %d, \"err_max\": %.17g, \"manip_min\": %.17g, \"q_excess\": %.17g, "
                    "\"dev_lin\": %.17g, \"dev_perp\": %.17g, \"dev_ang\": %.17g, \"dev_n_over\": %d, \"dev_status\": %d, "
                    "\"lim_status\": %d, \"lim_tool_lin\": %.17g, \"rt_status\": %d, \"rt_T_new\": %.17g, \"rt_off_line\": %.17g, \"rt_rise\": %.17g, "
                    "\"t_last\": %.17g}\n",
                    planner.solution_T(), tl.status, tl.k_fail, tl.err_max, tl.manip_min, tl.q_excess, dev.lin_max, dev.perp_max, dev.ang_max,
                    dev.n_over, dev.status, lim.status, lim.excess[MPCMP_LIM_TOOL_LIN], rt.status, rt.T_new, off, rise, t(0, 50));
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
    return 0;
}
