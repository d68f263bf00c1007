// Camera frames as voxel worlds (include/mpcmp_frame.h) from C++, in two parts, each printing one JSON line:
//   host   mpcmp_frame_spheres, mpcmp_frame_points_one, mpcmp_frame_depth_one and mpcmp_frame_carve_one with mpcmp_field_edt on a 32 x 28 x 26 grid
//          and a three-sphere robot: the order of the classes, the count identity and both clearance guarantees; no context, no GPU.  With
//          -DMPCMP_SELFTEST_HOST_ONLY this is the whole program, and it links against the host-only unit alone:
//            g++ -std=c++17 -DMPCMP_SELFTEST_HOST_ONLY -fsanitize=address,undefined -Iinclude examples/frame_selftest.cpp mpc_motion_planner_amd/csrc/model_host.cpp
//   shim   MotionPlanner::set_point_cloud_filtered / set_depth_image / carve_robot on a solved move: a frame that sees the robot at the start
//          posture hits at t = 0 unfiltered and is clear there filtered
//            g++ -O2 -std=c++17 -Iinclude examples/frame_selftest.cpp -Lmpc_motion_planner_amd -lmpcmp -Wl,-rpath,$PWD/mpc_motion_planner_amd
#include <cmath>
#include <cstdio>
#include <iostream>
#include <vector>
#ifdef MPCMP_SELFTEST_HOST_ONLY
#include "mpcmp.h"
#else
#include "mpcmp_motion_planner.hpp"
#endif

static const double H = 0.05, MARGIN = 0.01;
static const double PAD_POINTS = 2.5 * 1.7320508075688772 * H + MARGIN + 1e-3, PAD_CARVE = 2.0 * 1.7320508075688772 * H + MARGIN + 1e-3;

static mpcmp_field_desc grid() {
    mpcmp_field_desc g = {};
    g.origin[0] = -0.813; g.origin[1] = -0.687; g.origin[2] = -0.031; g.h = H;
    g.n[0] = 32; g.n[1] = 28; g.n[2] = 26;
    return g;
}
// what a camera sees: a vertical pole at x = 0.45, y = 0.35 up to z = 0.6, and the shell of every sphere [ns][4] = c, R in 26 directions
static std::vector<double> frame_cloud(const std::vector<double> &sph) {
    std::vector<double> pts;
    for (int k = 0; k < 60; k++) { pts.push_back(0.45); pts.push_back(0.35); pts.push_back(0.005 + 0.01 * k); }
    for (size_t s = 0; s < sph.size() / 4; s++)
        for (int a = -1; a <= 1; a++)
            for (int b = -1; b <= 1; b++)
                for (int c = -1; c <= 1; c++) {
                    if (!a && !b && !c) continue;
                    const double l = std::sqrt((double)(a * a + b * b + c * c));
                    pts.push_back(sph[4 * s] + sph[4 * s + 3] * a / l);
                    pts.push_back(sph[4 * s + 1] + sph[4 * s + 3] * b / l);
                    pts.push_back(sph[4 * s + 2] + sph[4 * s + 3] * c / l);
                }
    return pts;
}

static int host_part() {
    const mpcmp_field_desc g = grid();
    const size_t nv = (size_t)g.n[0] * g.n[1] * g.n[2];
    mpcmp_model m;
    mpcmp_default_model(&m);
    mpcmp_sphere sph[3] = {};
    sph[0].joint = 3; sph[0].r = 0.06;
    sph[1].joint = 5; sph[1].r = 0.05;
    sph[2].joint = 6; sph[2].r = 0.03; sph[2].c[0] = m.tool[0]; sph[2].c[1] = m.tool[1]; sph[2].c[2] = m.tool[2];
    const int n_sph = 3;
    const double q[7] = {0.65, 0.3, 0.0, -1.6, 0.0, 1.9, 0.5};
    std::vector<double> body(12), filt(12);
    if (mpcmp_frame_spheres(&m, 1, &n_sph, sph, q, 0.0, body.data()) || mpcmp_frame_spheres(&m, 1, &n_sph, sph, q, PAD_POINTS, filt.data())) return 2;
    for (int s = 0; s < 3; s++) {
        if (filt[4 * s + 3] != sph[s].r + PAD_POINTS) return 3;
        for (int d = 0; d < 3; d++)                      // the guarantees' premise: centres inside the grid
            if (!(body[4 * s + d] > g.origin[d] && body[4 * s + d] < g.origin[d] + g.h * g.n[d])) return 3;
    }
    std::vector<unsigned char> occ(nv, 9);
    std::vector<unsigned> d2(nv);
    mpcmp_frame_stats st;
    // the order of the classes: a NaN that is also out of the grid, a point out of the grid, a sphere centre, a free point
    const double four[12] = {NAN, 9.0, 9.0, 9.0, 0.0, 0.0, body[0], body[1], body[2], -0.5, -0.5, 0.5};
    if (mpcmp_frame_points_one(&m, 1, &n_sph, sph, &g, 4, four, q, PAD_POINTS, 0, occ.data(), &st)) return 4;
    size_t marked = 0;
    for (size_t v = 0; v < nv; v++) marked += occ[v] != 0;
    const int order_wrong = (st.n_in != 4) + (st.n_invalid != 1) + (st.n_outside != 1) + (st.n_robot != 1) + (st.n_marked != 1) + (st.n_cleared != 0) +
                            (marked != 1);
    // the frame that sees the robot: unfiltered the posture is inside solid voxels, filtered it is clear by the bound
    std::vector<double> pts = frame_cloud(body);
    for (int k = 0; k < 6; k++) pts.push_back(four[k]);                      // (and the two points no class but the first two takes)
    const int np = (int)(pts.size() / 3);
    double d_raw, d_points, d_carve, d_depth;
    if (mpcmp_frame_points_one(nullptr, 0, nullptr, nullptr, &g, np, pts.data(), nullptr, 0.0, 0, occ.data(), nullptr)) return 5;
    const std::vector<unsigned char> seen = occ;
    if (mpcmp_field_edt(&g, occ.data(), d2.data()) || mpcmp_clearance_field_config(&m, 1, &n_sph, sph, &g, d2.data(), q, &d_raw, nullptr, nullptr)) return 5;
    if (mpcmp_frame_points_one(&m, 1, &n_sph, sph, &g, np, pts.data(), q, PAD_POINTS, 0, occ.data(), &st)) return 6;
    if (mpcmp_field_edt(&g, occ.data(), d2.data()) || mpcmp_clearance_field_config(&m, 1, &n_sph, sph, &g, d2.data(), q, &d_points, nullptr, nullptr)) return 6;
    // the unfiltered occupancy as a foreign grid, carved
    mpcmp_frame_stats sc;
    occ = seen;
    if (mpcmp_frame_carve_one(&m, 1, &n_sph, sph, &g, q, PAD_CARVE, occ.data(), &sc)) return 7;
    if (mpcmp_field_edt(&g, occ.data(), d2.data()) || mpcmp_clearance_field_config(&m, 1, &n_sph, sph, &g, d2.data(), q, &d_carve, nullptr, nullptr)) return 7;
    // a depth image from straight above the elbow sphere: a plane of constant depth through its centre
    mpcmp_camera cam = {};
    cam.R[0] = 1.0; cam.R[4] = -1.0; cam.R[8] = -1.0;
    cam.t[0] = body[0]; cam.t[1] = body[1]; cam.t[2] = body[2] + 0.6;
    cam.fx = cam.fy = 40.0; cam.cx = 23.5; cam.cy = 17.5; cam.depth_scale = 1.0; cam.z_min = 0.1; cam.z_max = 2.0; cam.width = 48; cam.height = 36;
    std::vector<float> depth(48 * 36, 0.6f);
    depth[0] = 0.0f; depth[1] = NAN; depth[2] = 5.0f;
    mpcmp_frame_stats sd;
    if (mpcmp_frame_depth_one(&m, 1, &n_sph, sph, &g, &cam, depth.data(), MPCMP_DEPTH_F32, q, PAD_POINTS, 0, occ.data(), &sd)) return 8;
    if (sd.n_invalid != 3 || sd.n_in != sd.n_invalid + sd.n_outside + sd.n_robot + sd.n_marked) return 8;
    if (mpcmp_field_edt(&g, occ.data(), d2.data()) || mpcmp_clearance_field_config(&m, 1, &n_sph, sph, &g, d2.data(), q, &d_depth, nullptr, nullptr)) return 8;
    // refused: nothing is written
    std::vector<unsigned char> keep(nv, 7);
    st.n_cleared = 77;
    if (mpcmp_frame_points_one(&m, 1, &n_sph, sph, &g, np, pts.data(), q, -1.0, 0, keep.data(), &st) != MPCMP_EINVAL || keep[0] != 7 || st.n_cleared != 77)
        return 9;
    std::printf("{\"host\": {\"order_wrong\": %d, \"n_in\": %d, \"n_invalid\": %d, \"n_outside\": %d, \"n_robot\": %d, \"n_marked\": %d, "
                "\"unfiltered_d\": %.17g, \"points_d\": %.17g, \"points_bound\": %.17g, \"carve_d\": %.17g, \"carve_bound\": %.17g, \"n_cleared\": %d, "
                "\"depth_n_in\": %d, \"depth_n_robot\": %d, \"depth_d\": %.17g}}\n",
                order_wrong, st.n_in, st.n_invalid, st.n_outside, st.n_robot, st.n_marked, d_raw, d_points,
                PAD_POINTS - 2.5 * 1.7320508075688772 * H, d_carve, PAD_CARVE - 2.0 * 1.7320508075688772 * H, sc.n_cleared, sd.n_in, sd.n_robot, d_depth);
    return 0;
}

int main() {
    if (int rc = host_part()) return rc;
#ifndef MPCMP_SELFTEST_HOST_ONLY
    try {
        MotionPlanner planner("", 4, 2);
        MotionPlanner::Vec7 q0, q1, rest = MotionPlanner::Vec7::Zero();
        const double a[7] = {0.65, 0.3, 0.0, -1.6, 0.0, 1.9, 0.5}, b[7] = {-0.4, 0.1, 0.2, -1.9, 0.1, 1.8, 0.3};
        for (int j = 0; j < 7; j++) { q0(j) = a[j]; q1(j) = b[j]; }
        planner.set_current_state(q0, rest);
        planner.set_target_state(q1, rest);
        planner.solve_trajectory(true);
        const mpcmp_field_desc g = grid();
        // the skeleton the shim installs, as the camera sees it at the start posture
        mpcmp_sphere sph[64];
        int n = 0;
        if (mpcmp_link_spheres(&planner.robot.model, 0.06, 0.08, 64, sph, &n)) return 10;
        std::vector<double> body(4 * (size_t)n);
        if (mpcmp_frame_spheres(&planner.robot.model, 1, &n, sph, a, 0.0, body.data())) return 10;
        const std::vector<double> pts = frame_cloud(body);
        const int np = (int)(pts.size() / 3);
        planner.set_point_cloud(g, np, pts.data());
        const mpcmp_clearance raw = planner.check_clearance_field(100, MARGIN);
        planner.set_point_cloud_filtered(g, np, pts.data(), a, PAD_POINTS);
        const mpcmp_frame_stats st = planner.frame_stats;
        const mpcmp_clearance filtered = planner.check_clearance_field(100, MARGIN);
        // the host statement marks the same voxels: the fields agree
        std::vector<unsigned char> occ((size_t)g.n[0] * g.n[1] * g.n[2]);
        std::vector<unsigned> ref(occ.size()), dev(occ.size());
        mpcmp_frame_stats hs;
        if (mpcmp_frame_points_one(&planner.robot.model, 1, &n, sph, &g, np, pts.data(), a, PAD_POINTS, 0, occ.data(), &hs)) return 11;
        if (mpcmp_field_edt(&g, occ.data(), ref.data())) return 11;
        mpcmp_field_desc back;
        planner.voxel_field(&back, dev.data());
        size_t differ = 0;
        for (size_t v = 0; v < occ.size(); v++) differ += dev[v] != ref[v];
        // the unfiltered cloud as a foreign grid, carved
        if (mpcmp_frame_points_one(nullptr, 0, nullptr, nullptr, &g, np, pts.data(), nullptr, 0.0, 0, occ.data(), nullptr)) return 12;
        planner.set_voxel_world(&g, occ.data());
        planner.carve_robot(a, PAD_CARVE);
        const int n_cleared = planner.frame_stats.n_cleared;
        const mpcmp_clearance carved = planner.check_clearance_field(100, MARGIN);
        // a depth image from above the elbow
        mpcmp_camera cam = {};
        cam.R[0] = 1.0; cam.R[4] = -1.0; cam.R[8] = -1.0;
        cam.t[0] = 0.3; cam.t[1] = 0.2; cam.t[2] = 1.2;
        cam.fx = cam.fy = 40.0; cam.cx = 23.5; cam.cy = 17.5; cam.depth_scale = 0.001; cam.z_min = 0.1; cam.z_max = 2.0; cam.width = 48; cam.height = 36;
        std::vector<unsigned short> depth(48 * 36, 1200);
        depth[5] = 0;
        planner.set_depth_image(g, cam, depth.data(), MPCMP_DEPTH_U16, a, PAD_POINTS);
        const mpcmp_frame_stats ds = planner.frame_stats;
        planner.set_voxel_world(nullptr, nullptr);
        std::printf("{\"raw_status\": %d, \"raw_t_first\": %.17g, \"raw_d_min\": %.17g, \"n_in\": %d, \"n_robot\": %d, \"n_marked\": %d, \"host_n_robot\": %d, "
                    "\"host_n_marked\": %d, \"differ\": %zu, \"filtered_t_first\": %.17g, \"filtered_status\": %d, \"n_cleared\": %d, \"carved_t_first\": %.17g, "
                    "\"depth_n_in\": %d, \"depth_n_invalid\": %d, \"depth_sum\": %d}\n",
                    raw.status, raw.t_first, raw.d_min, st.n_in, st.n_robot, st.n_marked, hs.n_robot, hs.n_marked, differ, filtered.t_first, filtered.status,
                    n_cleared, carved.t_first, ds.n_in, ds.n_invalid, ds.n_invalid + ds.n_outside + ds.n_robot + ds.n_marked);
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
#endif
    return 0;
}
