// Drives the host-only part of the library (mpc_motion_planner_amd/csrc/model_host.cpp: URDF reader, default model) on its own, without a device and
// without the rest of the library, so that it can be run under the host sanitizers:
//   clang++ -g -O1 -std=c++17 -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude examples/urdf_selftest.cpp \
//       mpc_motion_planner_amd/csrc/model_host.cpp -o urdf_selftest && ./urdf_selftest tests/golden/panda_arm.urdf
// Reads the given URDF, copies of it cut off at every eighth of its length, a file that is not XML and a path that does not exist; checks the
// return codes, and the model of the whole file against mpcmp_default_model.  Exit status 0: every check passed.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include "mpcmp.h"
#include "../mpc_motion_planner_amd/csrc/model_host.hpp"      // (the message of a failed call without a context: mpcmp::g_err)

static int failures = 0;
static void check(bool ok, const char *what) {
    std::printf("%s: %s\n", ok ? "ok  " : "FAIL", what);
    if (!ok) failures++;
}

static bool write_file(const std::string &path, const std::string &text) {
    std::ofstream f(path, std::ios::binary);
    f << text;
    return (bool)f;
}

int main(int argc, char **argv) {
    const std::string urdf = argc > 1 ? argv[1] : "tests/golden/panda_arm.urdf";
    const std::string tmp = argc > 2 ? argv[2] : "/tmp";
    std::ifstream in(urdf, std::ios::binary);
    std::stringstream ss; ss << in.rdbuf();
    const std::string xml = ss.str();
    check(!xml.empty(), "the URDF can be read");

    // the whole file: one 7-joint chain, the numbers of the built-in model
    mpcmp_model m, d;
    check(mpcmp_model_from_urdf(urdf.c_str(), &m) == MPCMP_OK, "whole file: MPCMP_OK");
    check(mpcmp_default_model(&d) == MPCMP_OK, "default model");
    double worst = 0.0;
    for (int i = 0; i < 7; i++) {
        worst = std::fmax(worst, std::fabs(m.mass[i] - d.mass[i]));
        for (int k = 0; k < 3; k++) worst = std::fmax(worst, std::fabs(m.p[i][k] - d.p[i][k]));
        for (int k = 0; k < 9; k++) worst = std::fmax(worst, std::fabs(m.R0[i][k] - d.R0[i][k]));
    }
    check(worst <= 1e-9, "whole file: masses, joint placements and rotations of the default model");
    check(m.tool[2] == d.tool[2] && m.link8[2] == d.link8[2] && m.gravity[2] == -9.81, "whole file: tool and link8 frames, gravity");
    mpcmp_model two[2];
    int n = -1;
    check(mpcmp_models_from_urdf(urdf.c_str(), 2, two, &n) == MPCMP_OK && n == 1, "whole file: one chain");

    // cut off at every eighth: never a model of a chain the file does not hold, never a crash; the cut through the middle is refused with a reason
    for (int k = 1; k < 8; k++) {
        const std::string path = tmp + "/urdf_selftest_cut" + std::to_string(k) + ".urdf";
        check(write_file(path, xml.substr(0, xml.size() * k / 8)), "cut file written");
        mpcmp::g_err.clear();
        const int rc = mpcmp_model_from_urdf(path.c_str(), &m);
        std::printf("      cut at %d/8: rc = %d (%s)\n", k, rc, mpcmp::g_err.c_str());
        check(rc == MPCMP_EINVAL && !mpcmp::g_err.empty(), "cut file: MPCMP_EINVAL with a reason");
        std::remove(path.c_str());
    }

    // not XML at all, and no file
    const std::string junk = tmp + "/urdf_selftest_junk.urdf";
    check(write_file(junk, "this is not a robot description\n"), "junk file written");
    check(mpcmp_model_from_urdf(junk.c_str(), &m) == MPCMP_EINVAL && mpcmp::g_err == "URDF holds no links", "not XML: MPCMP_EINVAL, 'URDF holds no links'");
    check(mpcmp_models_from_urdf(junk.c_str(), 2, two, &n) == MPCMP_EINVAL && n == 0, "not XML: no chains");
    std::remove(junk.c_str());
    check(mpcmp_model_from_urdf((tmp + "/urdf_selftest_no_such_file.urdf").c_str(), &m) == MPCMP_EINVAL, "missing file: MPCMP_EINVAL");
    check(mpcmp_model_from_urdf(nullptr, &m) == MPCMP_EINVAL && mpcmp_model_from_urdf(urdf.c_str(), nullptr) == MPCMP_EINVAL, "null arguments: MPCMP_EINVAL");

    std::printf("%s (%d failed)\n", failures ? "FAILED" : "all checks passed", failures);
    return failures ? 1 : 0;
}
