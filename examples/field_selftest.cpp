// Voxel worlds (include/mpcmp_field.h) from C++, in two parts, each printing one JSON line:
//   host   mpcmp_field_edt, mpcmp_field_sd and mpcmp_clearance_field_config on a 24 x 20 x 16 grid with a pole of occupied voxels: no context, no
//          GPU.  With -DMPCMP_SELFTEST_HOST_ONLY this is the whole program, and it links against the host-only unit alone:
//            g++ -std=c++17 -DMPCMP_SELFTEST_HOST_ONLY -fsanitize=address,undefined -Iinclude examples/field_selftest.cpp mpc_motion_planner_amd/csrc/model_host.cpp
//   shim   MotionPlanner::set_voxel_world / set_point_cloud / check_clearance_field on a solved move past the same pole, the field built on the GPU
//          and read back, next to the host transform
//            g++ -O2 -std=c++17 -Iinclude examples/field_selftest.cpp -Lmpc_motion_planner_amd -lmpcmp -Wl,-rpath,$PWD/mpc_motion_planner_amd
#include <cmath>
#include <cstdio>
#include <iostream>
#include <vector>
#ifdef MPCMP_SELFTEST_HOST_ONLY
#include "mpcmp.h"
#else
#include "mpcmp_motion_planner.hpp"
#endif

// a grid of 5 cm voxels around the robot and a vertical pole in it: the column of voxels that contains x = 0.45, y = 0.35, up to z = 0.6
static mpcmp_field_desc grid() {
    mpcmp_field_desc g = {};
    g.origin[0] = -0.613; g.origin[1] = -0.487; g.origin[2] = -0.031; g.h = 0.05;
    g.n[0] = 24; g.n[1] = 20; g.n[2] = 16;
    return g;
}
static std::vector<unsigned char> pole(const mpcmp_field_desc &g) {
    std::vector<unsigned char> occ((size_t)g.n[0] * g.n[1] * g.n[2], 0);
    const int i = (int)std::floor((0.45 - g.origin[0]) / g.h), j = (int)std::floor((0.35 - g.origin[1]) / g.h);
    for (int k = 0; k < g.n[2] && g.origin[2] + g.h * k < 0.6; k++) occ[((size_t)k * g.n[1] + j) * g.n[0] + i] = 1;
    return occ;
}

static int host_part() {
    const mpcmp_field_desc g = grid();
    const std::vector<unsigned char> occ = pole(g);
    const size_t nv = occ.size();
    std::vector<unsigned> d2(nv, 7u);
    if (mpcmp_field_edt(&g, occ.data(), d2.data())) return 2;
    // the transform against the definition, by brute force over the pole's voxels
    std::vector<int> w;
    for (size_t v = 0; v < nv; v++) if (occ[v]) w.push_back((int)v);
    size_t wrong = 0;
    unsigned d2_max = 0;
    for (size_t v = 0; v < nv; v++) {
        const int i = (int)(v % g.n[0]), j = (int)(v / g.n[0] % g.n[1]), k = (int)(v / g.n[0] / g.n[1]);
        unsigned best = MPCMP_FIELD_EMPTY;
        for (int u : w) {
            const int a = u % g.n[0] - i, b = u / g.n[0] % g.n[1] - j, c = u / g.n[0] / g.n[1] - k;
            const unsigned d = (unsigned)(a * a + b * b + c * c);
            if (d < best) best = d;
        }
        wrong += best != d2[v];
        if (d2[v] > d2_max) d2_max = d2[v];
    }
    // an empty world
    std::vector<unsigned char> none(nv, 0);
    std::vector<unsigned> e2(nv, 7u);
    if (mpcmp_field_edt(&g, none.data(), e2.data())) return 2;
    size_t not_empty = 0;
    for (size_t v = 0; v < nv; v++) not_empty += e2[v] != MPCMP_FIELD_EMPTY;
    // the distance inside the pole, beside it, outside the grid and on an empty field
    const double in_pole[3] = {0.45, 0.35, 0.3}, beside[3] = {0.2, 0.35, 0.3}, outside[3] = {0.45, 0.35, 5.0};
    double sd_in, sd_beside, sd_out, sd_none;
    int v_in, v_out;
    if (mpcmp_field_sd(&g, d2.data(), in_pole, &sd_in, &v_in) || mpcmp_field_sd(&g, d2.data(), beside, &sd_beside, nullptr) ||
        mpcmp_field_sd(&g, d2.data(), outside, &sd_out, &v_out) || mpcmp_field_sd(&g, e2.data(), beside, &sd_none, nullptr)) return 3;
    // one configuration of a three-sphere robot
    mpcmp_model m;
    mpcmp_default_model(&m);
    // three spheres: on the elbow, on the wrist and at the tool point
    mpcmp_sphere sph[3] = {};
    sph[0].joint = 3; sph[0].r = 0.06;
    sph[1].joint = 5; sph[1].r = 0.05;
    sph[2].joint = 6; sph[2].r = 0.03; sph[2].c[0] = m.tool[0]; sph[2].c[1] = m.tool[1]; sph[2].c[2] = m.tool[2];
    const int n_sph = 3;
    const double q[7] = {0.65, 0.3, 0.0, -1.6, 0.0, 1.9, 0.5};
    double d_min, d_none;
    int s_min, vox, s_none, vox_none;
    if (mpcmp_clearance_field_config(&m, 1, &n_sph, sph, &g, d2.data(), q, &d_min, &s_min, &vox)) return 5;
    if (mpcmp_clearance_field_config(&m, 1, &n_sph, sph, &g, e2.data(), q, &d_none, &s_none, &vox_none)) return 5;
    // refused: nothing is written
    mpcmp_field_desc bad = g;
    bad.n[1] = 1025;
    double keep = 77.0;
    if (mpcmp_field_edt(&bad, occ.data(), d2.data()) != MPCMP_EINVAL || mpcmp_field_sd(&bad, d2.data(), beside, &keep, nullptr) != MPCMP_EINVAL ||
        keep != 77.0) return 6;
    std::printf("{\"host\": {\"voxels\": %zu, \"occupied\": %zu, \"wrong\": %zu, \"d2_max\": %u, \"not_empty\": %zu, \"sd_in\": %.17g, \"v_in_occupied\": %d, "
                "\"sd_beside\": %.17g, \"sd_out\": %.17g, \"v_out\": %d, \"sd_none_is_inf\": %d, \"d_min\": %.17g, \"sphere\": %d, \"voxel\": %d, "
                "\"none_is_inf\": %d, \"none_sphere\": %d}}\n",
                nv, w.size(), wrong, d2_max, not_empty, sd_in, (int)occ[v_in], sd_beside, sd_out, v_out, (int)std::isinf(sd_none), d_min, s_min, vox,
                (int)std::isinf(d_none), s_none);
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
        const mpcmp_field_desc g = grid();
        const std::vector<unsigned char> occ = pole(g);
        planner.set_voxel_world(&g, occ.data());
        // the field the GPU built against the host transform
        std::vector<unsigned> dev(occ.size()), ref(occ.size());
        mpcmp_field_desc back;
        planner.voxel_field(&back, dev.data());
        if (mpcmp_field_edt(&g, occ.data(), ref.data())) return 7;
        size_t differ = 0;
        for (size_t v = 0; v < occ.size(); v++) differ += dev[v] != ref[v];
        const mpcmp_clearance field = planner.check_clearance_field(200, 0.02);
        // the same pole as a point cloud: one point in every occupied voxel
        std::vector<double> pts;
        for (size_t v = 0; v < occ.size(); v++)
            if (occ[v]) {
                pts.push_back(g.origin[0] + g.h * ((double)(v % g.n[0]) + 0.5));
                pts.push_back(g.origin[1] + g.h * ((double)(v / g.n[0] % g.n[1]) + 0.5));
                pts.push_back(g.origin[2] + g.h * ((double)(v / g.n[0] / g.n[1]) + 0.5));
            }
        planner.set_point_cloud(g, (int)(pts.size() / 3), pts.data());
        const mpcmp_clearance cloud = planner.check_clearance_field(200, 0.02);
        // merged with the floor as a primitive
        mpcmp_obstacle floor = {};
        floor.type = MPCMP_OBS_HALFSPACE; floor.a[2] = 1.0; floor.b[0] = -0.05;
        planner.set_obstacles(&floor, 1);
        int source = -1;
        const mpcmp_clearance merged = planner.check_clearance_field(200, 0.02, true, 0, &source);
        const mpcmp_clearance prim = planner.clearance(200, 0.02);
        planner.set_voxel_world(nullptr, nullptr);
        std::printf("{\"n\": [%d, %d, %d], \"differ\": %zu, \"status\": %d, \"d_min\": %.17g, \"t_min\": %.17g, \"sphere\": %d, \"voxel\": %d, "
                    "\"voxel_occupied_column\": %d, \"cloud_d_min\": %.17g, \"cloud_n_hit\": %d, \"n_hit\": %d, \"merged_d_min\": %.17g, "
                    "\"merged_n_hit\": %d, \"prim_d_min\": %.17g, \"prim_n_hit\": %d, \"source\": %d}\n",
                    back.n[0], back.n[1], back.n[2], differ, field.status, field.d_min, field.t_min, field.sphere, field.other,
                    (int)(field.other >= 0 && field.other < (int)occ.size()), cloud.d_min, cloud.n_hit, field.n_hit, merged.d_min, merged.n_hit,
                    prim.d_min, prim.n_hit, source);
    } catch (const std::exception &e) {
        std::cerr << "error: " << e.what() << std::endl;
        return 1;
    }
#endif
    return 0;
}
