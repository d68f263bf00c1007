"""Route retiming (include/mpcmp_route_retime.h), the part that needs no GPU: the ABI table, the record size, and the host statement of the rule
(mpcmp_retime_route_one) against the NumPy restatement of tests/route_retime_reference.py.

Inputs without a solve: the 16 rest-to-rest jerk-limited moves of tests/test_gpu_limits.py::moves (same seed), each cut into M + 1 legs of equal
duration.  q, qd and qdd of the move at every leg's time nodes come from oracle_py.sample with n_pts = 4 num_seg (M + 1) (the nodes of a leg lie at
multiples of 1 / (4 num_seg) of its length); each leg has T = T_move / (M + 1).  The junction states then agree bit for bit and are moving.  Rows:
tests/test_retime_host.py::rows per route, spread over the legs with Solver.repeat: odd routes tight, even routes loose; the tool maxima are the
batch medians of the routes' peak tool speeds.  The case builder below (case, check_route_against) is what tests/test_gpu_route_retime.py checks
the kernels with as well.

Bounds: those tests/test_retime_host.py derives.  1e-8 relative on x_k, t, leg_T_new and T_new; status, leg_fail and k_fail exact where the
reference's sets do not come within 1e-8 of empty (at most 1 route of the 16 may fall under that exemption); every case repeats the 1e-13
perturbation run on the reference and asserts an amplification <= 100 (the rule is chained over (M + 1) n_grid points).  For every case with
n_grid >= 50 and M >= 1 the reference must have at least 3 routes slowed (rate_min < 0.99), 2 untouched and 1 infeasible.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_py as o
import retime_reference as R
import route_retime_reference as RR
from test_gpu_limits import moves, robot
from test_retime_host import EPS, TIGHT, perturbation, rows

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 16
CASES = [(nseg, narm, M, n_grid) for nseg, narm in ((1, 1), (4, 1), (6, 2)) for M in (0, 1, 3) for n_grid in (1, 50, 70)]


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


@functools.lru_cache(maxsize=None)
def route_moves(narm, nseg, nvia):
    """the moves cut into nvia + 1 legs: sx [B][M+1][N][14 narm], su [B][M+1][N][7 narm], sT [B][M+1]"""
    import mpc_motion_planner_amd as M
    sx, su, sT = moves(narm, nseg, B)
    models = robot(M, narm)
    nl, N, nq, per = nvia + 1, 3 * nseg + 1, 7 * narm, 4 * nseg
    node = np.rint(o.time_nodes(nseg) * per).astype(int)
    assert (np.abs(o.time_nodes(nseg) * per - node) < 1e-12).all()
    lx, lu, lT = np.zeros((B, nl, N, 2 * nq)), np.zeros((B, nl, N, nq)), np.zeros((B, nl))
    for b in range(B):
        for a in range(narm):
            xa, ua = R.arm_nodes(sx[b], su[b], a)
            s = o.sample(nseg, xa, ua, sT[b], per * nl, model=R.omodel(models[a]))
            for m in range(nl):
                i = m * per + node
                lx[b, m, :, 7 * a:7 * a + 7], lx[b, m, :, nq + 7 * a:nq + 7 * a + 7], lu[b, m, :, 7 * a:7 * a + 7] = s[i, 1:8], s[i, 8:15], s[i, 15:22]
        lT[b] = sT[b] / nl
    for a in (lx, lu, lT):
        a.setflags(write=False)
    return lx, lu, lT


def route_rows(M, nseg, narm, nvia, n_grid=50):
    """BOUNDS_DTYPE [B][M+1]: the row of a route for each of its legs, from tests/test_retime_host.py::rows.  Two shapes have a tight row of their
    own (the conditions on the reference and the tool maxima stay as they are):
    num_seg 1 with M == 1: under a torque margin of 0.5 the reference amplifies the 1e-13 perturbation by 111 (n_grid 50) and 124 (n_grid 70),
    against the 100 the fair-test condition allows; a torque margin of 0.55 gives 6.1 and 7.1 (and 11 slowed, 3 untouched, 2 infeasible).
    num_seg 6 with two arms: only one of the 8 loose routes has both its peak tool speeds under the batch medians, and under the common tight row
    no odd route stays untouched (9 slowed, 1 untouched, 6 infeasible; 2 untouched are asked for).  The caps stay; a tight row with margins 1 on
    the velocity, 0.8 on the acceleration and 0.6 on the torque leaves route 3 untouched as well: 13 slowed, 2 untouched, 1 infeasible.  It is used
    where those counts are asserted (n_grid >= 50); at n_grid 1 the common tight row stays: under the other, the forward step of route 13 at M == 1
    lands on x == 0 at its end at rest by cancellation (7.8e-16 after the perturbation), where a relative deviation means nothing."""
    t = rows(M, B, nseg, narm)
    if (nseg, narm, nvia) == (1, 1, 1):
        t[1::2] = M.bounds_from_margins(*(TIGHT[:3] + (0.55,) + TIGHT[4:]))
    if (nseg, narm) == (6, 2) and n_grid >= 50:
        t[1::2] = M.bounds_from_margins(0.8, 1.0, 0.8, 0.6, 0.3)
    return M.Solver.repeat(t, nvia).reshape(B, nvia + 1)


def route_tool_maxima(P):
    """the batch medians of the routes' peak tool speeds; P: per route the list of its legs' path values"""
    return (float(np.median([max(p["vlin"].max() for p in legs) for legs in P])), float(np.median([max(p["vang"].max() for p in legs) for legs in P])))


def route_reference(table, sT, n_grid, lin_max, ang_max, P, rate_max=1.0, groups=R.ALL_GROUPS):
    out = []
    for b in range(sT.shape[0]):
        r = RR.retime_route_np(P[b], table[b], sT[b], n_grid, lin_max, ang_max, rate_max, groups)
        r["P"] = P[b]
        out.append(r)
    return out


def amplification(ref, ref2):
    amp = 0.0
    for r, r2 in zip(ref, ref2):
        if not r["status"] and not r2["status"] and not r["near"]:
            amp = max(amp, float((np.abs(r2["x"] - r["x"]) / np.maximum(r["x"], 1e-300)).max()) / EPS, abs(r2["T_new"] / r["T_new"] - 1.0) / EPS)
    return amp


@functools.lru_cache(maxsize=None)
def case(narm, nseg, nvia, n_grid):
    """(lin_max, ang_max, reference [B], amplification) for the common inputs; the amplification is max |x' - x| / x / EPS (and the same for T_new)
    over the feasible routes, x' from sampled q, v, a perturbed by EPS"""
    import mpc_motion_planner_amd as M
    sx, su, sT = route_moves(narm, nseg, nvia)
    models, table = robot(M, narm), route_rows(M, nseg, narm, nvia, n_grid)
    P = [RR.route_path_values(models, nseg, sx[b], su[b], sT[b], n_grid) for b in range(B)]
    lin_max, ang_max = route_tool_maxima(P)
    ref = route_reference(table, sT, n_grid, lin_max, ang_max, P)
    P2 = [RR.route_path_values(models, nseg, sx[b], su[b], sT[b], n_grid,
                               [perturbation(P[b][m]["q"].shape, b * (nvia + 1) + m) for m in range(nvia + 1)]) for b in range(B)]
    ref2 = route_reference(table, sT, n_grid, lin_max, ang_max, P2)
    return lin_max, ang_max, ref, amplification(ref, ref2)


def assert_reference_is_a_fair_test(ref, amp, counts=True):
    slowed = sum(1 for r in ref if not r["status"] and r["rate_min"] < 0.99)
    untouched = sum(1 for r in ref if not r["status"] and (r["x"] == 1.0).all())
    infeasible = sum(1 for r in ref if r["status"])
    near = sum(1 for r in ref if r["near"])
    if counts:
        assert slowed >= 3 and untouched >= 2 and infeasible >= 1, "reference: %d slowed, %d untouched, %d infeasible of %d" % (slowed, untouched, infeasible, len(ref))
    assert near <= 1, "reference: %d of %d routes within 1e-8 of an empty set" % (near, len(ref))
    assert amp <= 100.0, "reference: a relative input perturbation of %g is amplified by %.1f" % (EPS, amp)
    return slowed, untouched, infeasible


def check_route_against(ref, prof, leg_T, rec, rate_max=1.0, what="", worst=None):
    """prof [B][M+1][n + 1][2], leg_T [B][M+1], rec ROUTE_RETIME_DTYPE [B] against the reference dicts; returns the number of routes passed over
    because their reference sets come within 1e-8 of empty and the status differs"""
    exempt = 0
    for b, (r, g) in enumerate(zip(ref, rec)):
        tag = (what, b)
        assert g["pad"] == 0 and (g["status"] & ~(RR.INFEASIBLE | RR.NAN)) == 0, tag
        if not r["near"]:
            assert (g["status"], g["leg_fail"], g["k_fail"]) == (r["status"], r["leg_fail"], r["k_fail"]), (tag, g, r["status"], r["leg_fail"], r["k_fail"])
        elif g["status"] != r["status"]:
            exempt += 1
            continue
        if r["status"]:
            assert np.isposinf(g["T_new"]) and g["rate_min"] == 0.0 and g["s_slowest"] == -1.0 and g["leg_slowest"] == -1 and g["n_slowed"] == 0, (tag, g)
            assert np.isnan(prof[b]).all() and np.isposinf(leg_T[b]).all(), tag
            continue
        t, x = prof[b, :, :, 0], prof[b, :, :, 1]
        nl, n = x.shape[0], x.shape[1] - 1
        dx, dT = float((np.abs(x - r["x"]) / np.maximum(x, 1e-300)).max()), abs(g["T_new"] / r["T_new"] - 1.0)
        if worst is not None:
            worst[0], worst[1] = max(worst[0], dx), max(worst[1], dT)
        assert (np.abs(x - r["x"]) <= 1e-8 * x).all(), (tag, dx)
        assert (np.abs(t - r["t"]) <= 1e-8 * t[:, -1:]).all() and (t[:, 0] == 0.0).all(), tag
        assert (np.abs(leg_T[b] - r["leg_T_new"]) <= 1e-8 * leg_T[b]).all() and abs(g["T_new"] - r["T_new"]) <= 1e-8 * g["T_new"], (tag, g["T_new"], r["T_new"])
        # the junctions: one state, stored twice; the clock per leg and its sequential sum
        assert (x[:-1, n] == x[1:, 0]).all() and (leg_T[b] == t[:, n]).all(), tag
        total = leg_T[b, 0]
        for m in range(1, nl):
            total = total + leg_T[b, m]
        assert g["T_new"] == total, (tag, g["T_new"], total)
        assert abs(g["rate_min"] - r["rate_min"]) <= 1e-8 * g["rate_min"] and g["rate_min"] == np.sqrt(x.min()), (tag, g["rate_min"], r["rate_min"])
        lm, km = divmod(int(np.argmin(x)), n + 1)
        assert (g["leg_slowest"], g["s_slowest"]) == (lm, km / n) and r["x"][lm, km] <= r["x"].min() * (1.0 + 1e-8), (tag, g, lm, km)
        slowed = x < rate_max * rate_max
        assert g["n_slowed"] == int(slowed[0].sum() + slowed[1:, 1:].sum()), tag
        if not (np.abs(r["x"] - rate_max * rate_max) <= 1e-8).any() or (r["x"] == rate_max * rate_max).all():
            assert g["n_slowed"] == r["n_slowed"], (tag, g["n_slowed"], r["n_slowed"])
    return exempt


def check_route_limits_hold(P, table, T, x, lin_max, ang_max, groups=R.ALL_GROUPS, what=""):
    """one route: P, table, T per leg, x [M+1][n + 1].  The retimed motion of retime_reference.motion_np within its bounds by 1e-9 relative to the
    bound at every grid point; the acceleration and the torque of a junction are those of point 0 of the later leg: at the moving last point of a leg the rule has
    no row with w (include/mpcmp_retime.h, "Ends"), and tests/test_retime_host.py::check_limits_hold, which looks at a last point with the w of the
    interval before it, is written for ends at rest"""
    nl = len(P)
    for m in range(nl):
        mo = R.motion_np(P[m], T[m], x[m])
        narm = mo["vlin"].shape[1]
        t = lambda name, lo, hi: np.tile(np.asarray(table[m][name], dtype=np.float64)[lo:hi], narm)
        for g, val, lb, ub in ((R.QD, mo["qd"], t("lbx", 7, 14), t("ubx", 7, 14)), (R.QDD, mo["qdd"], t("lbu", 0, 7), t("ubu", 0, 7)),
                               (R.TAU, mo["tau"], t("lbg", 0, 7), t("ubg", 0, 7)), (R.TOOL_LIN, mo["vlin"], -np.inf, lin_max),
                               (R.TOOL_ANG, mo["vang"], -np.inf, ang_max)):
            if not groups >> g & 1:
                continue
            if g in (R.QDD, R.TAU) and m < nl - 1:
                val = val[:-1]
            with np.errstate(invalid="ignore"):
                over = np.maximum(val - ub - 1e-9 * np.abs(ub), lb - 1e-9 * np.abs(lb) - val)
            assert not (over > 0).any(), (what, m, "group %d over its bound by %.3e at grid point %d" % (g, over.max(), int(np.argmax(over.max(axis=1)))))


def retime_route_all(M, models, nseg, sx, su, sT, table, n_grid, spec):
    nb, nl = sT.shape
    prof, leg_T, rec = np.zeros((nb, nl, n_grid + 1, 2)), np.zeros((nb, nl)), np.zeros(nb, dtype=M.ROUTE_RETIME_DTYPE)
    for b in range(nb):
        prof[b], leg_T[b], rec[b] = M.retime_route_one(models, nseg, table[b], sx[b], su[b], sT[b], n_grid, spec)
    return prof, leg_T, rec


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_table_matches_the_route_retime_header_and_the_library(M):
    """capi.ABI_ROUTE_RETIME against include/mpcmp_route_retime.h the way tests/test_retime_host.py holds capi.ABI_RETIME: the same functions in the
    same order, the exact argument kinds, the exports and what lib() declared to ctypes"""
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_route_retime.h")).read(), flags=re.S)
    decl = []
    for name, args in re.findall(r"\bint\s+(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr):
        kinds = ""
        for a in [" ".join(a.split()) for a in args.split(",")]:
            kinds += "p" if "*" in a else {"int": "i", "double": "d"}[a.split(" ")[0]]
        decl.append((name, kinds))
    assert len(decl) == 5 and [d[0] for d in decl] == list(capi.ABI_ROUTE_RETIME)
    assert not set(capi.ABI_ROUTE_RETIME) & (set(capi.ABI) | set(capi.ABI_LIMITS) | set(capi.ABI_RETIME) | set(capi.ABI_TOOLPATH))
    ctype = {"p": C.c_void_p, "i": C.c_int, "d": C.c_double}
    for name, kinds in decl:
        assert kinds == capi.ABI_ROUTE_RETIME[name], (name, kinds)
        f = getattr(M.lib(), name)
        assert f.argtypes == [ctype[k] for k in kinds] and f.restype is C.c_int, name
    main = open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    assert '#include "mpcmp_route_retime.h"' in main and main.index('#include "mpcmp_route_retime.h"') > main.index("mpcmp_sample_route_batch_device")
    retime = open(os.path.join(ROOT, "include", "mpcmp_retime.h")).read()
    for name, _ in decl:
        assert not re.search(re.escape(name) + r"\s*\(", main) and not re.search(re.escape(name) + r"\s*\(", retime), name
    assert os.path.join(ROOT, "include", "mpcmp_route_retime.h") in capi.build_dependencies()
    for name in ("ROUTE_RETIME_DTYPE", "retime_route_one"):
        assert name in M.__all__ and hasattr(M, name), name
    for name in ("retime_route", "retime_route_device", "sample_retimed_route", "sample_retimed_route_device"):
        assert callable(getattr(M.Solver, name)), name
    for name in ("retime_route", "get_retimed_route_trajectory"):
        assert callable(getattr(M.BatchMotionPlanner, name)), name


def test_record_size(M, tmp_path):
    dt = M.ROUTE_RETIME_DTYPE
    assert dt.itemsize == 48 and [dt.fields[f][1] for f in ("leg_slowest", "leg_fail", "k_fail", "n_slowed", "status", "pad")] == [24, 28, 32, 36, 40, 44]
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(mpcmp_route_retime), offsetof(mpcmp_route_retime, leg_slowest), offsetof(mpcmp_route_retime, leg_fail), '
                   'offsetof(mpcmp_route_retime, k_fail), offsetof(mpcmp_route_retime, n_slowed), offsetof(mpcmp_route_retime, status), '
                   'offsetof(mpcmp_route_retime, pad)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    assert [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()] == [48, 24, 28, 32, 36, 40, 44]


def test_cpp_shim_members_compile(M, tmp_path):
    """MotionPlanner::retime_route and get_retimed_route_trajectory<NP> of the header-only planner, instantiated under -Wall -Werror and linked"""
    src = tmp_path / "route_retime_shim.cpp"
    src.write_text('#include "mpcmp_motion_planner.hpp"\n'
                   'int use(MotionPlanner &p) {\n'
                   '    mpcmp_route_retime r = p.retime_route(50, nullptr);\n'
                   '    mpcmp_shim::Mat<1, 11> t; mpcmp_shim::Mat<7, 11> q, v, a, tau;\n'
                   '    p.get_retimed_route_trajectory<10>(t, q, v, a, tau);\n'
                   '    return r.status + r.leg_fail + (int)p.route_leg_T_new.size();\n}\n'
                   'int main(int argc, char **) { return argc > 99 ? 1 : 0; }\n')
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp", "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"),
                           "-o", str(tmp_path / "route_retime_shim")])


@pytest.mark.parametrize("nseg,narm,nvia,n_grid", CASES)
def test_retime_route_one_against_the_numpy_reference(M, nseg, narm, nvia, n_grid):
    sx, su, sT = route_moves(narm, nseg, nvia)
    lin_max, ang_max, ref, amp = case(narm, nseg, nvia, n_grid)
    counts = assert_reference_is_a_fair_test(ref, amp, counts=n_grid >= 50 and nvia >= 1)
    prof, leg_T, rec = retime_route_all(M, robot(M, narm), nseg, sx, su, sT, route_rows(M, nseg, narm, nvia, n_grid), n_grid, M.retime_spec(lin_max, ang_max))
    worst = [0.0, 0.0]
    try:
        check_route_against(ref, prof, leg_T, rec, worst=worst)
    finally:
        print("host: nseg %d, arms %d, M %d, n_grid %d: slowed / untouched / infeasible %s, amplification %.1f, max |x / ref - 1| %.1e, |T_new / ref - 1| %.1e"
              % (nseg, narm, nvia, n_grid, counts, amp, worst[0], worst[1]))


@pytest.mark.parametrize("nseg,narm,nvia", [(4, 1, 3), (6, 2, 1)])
def test_the_limits_hold(M, nseg, narm, nvia):
    n_grid = 50
    sx, su, sT = route_moves(narm, nseg, nvia)
    lin_max, ang_max, ref, _ = case(narm, nseg, nvia, n_grid)
    table = route_rows(M, nseg, narm, nvia, n_grid)
    prof, leg_T, rec = retime_route_all(M, robot(M, narm), nseg, sx, su, sT, table, n_grid, M.retime_spec(lin_max, ang_max))
    assert (rec["status"] == 0).sum() >= 8
    for b in np.flatnonzero(rec["status"] == 0):
        check_route_limits_hold(ref[b]["P"], table[b], sT[b], prof[b, :, :, 1], lin_max, ang_max, what=b)


@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_one_leg_is_the_rule_of_a_single_plan(M, nseg, narm):
    """n_legs == 1: the whole profile and every field the two records share equal those of mpcmp_retime_one bit for bit: a plan is a route of one
    leg, and mpcmp_retime_one runs the host statement of mpcmp_retime_route_one"""
    n_grid = 50
    sx, su, sT = route_moves(narm, nseg, 0)
    models, table = robot(M, narm), route_rows(M, nseg, narm, 0)
    retimed = 0
    for b in range(B):
        prof, leg_T, rec = M.retime_route_one(models, nseg, table[b], sx[b], su[b], sT[b], n_grid, None)
        p1, r1 = M.retime_one(models, nseg, table[b, 0], sx[b, 0], su[b, 0], sT[b, 0], n_grid, None)
        assert np.ascontiguousarray(prof[0]).tobytes() == p1.tobytes(), b
        for f in ("T_new", "rate_min", "s_slowest", "k_fail", "n_slowed", "status"):
            assert np.asarray(rec[f]).tobytes() == np.asarray(r1[f]).tobytes(), (b, f)
        assert rec["leg_fail"] == (0 if r1["status"] and r1["k_fail"] >= 0 else -1), b
        if r1["status"]:
            assert np.isnan(p1).all(), b
            continue
        assert rec["leg_slowest"] == 0 and leg_T[0] == rec["T_new"], b
        retimed += 1
    assert retimed >= 1


def test_bad_inputs_and_arguments(M):
    nseg, n_grid, nvia, b = 4, 50, 1, 0
    sx, su, sT = route_moves(1, nseg, nvia)
    models, table = robot(M, 1), route_rows(M, nseg, 1, nvia)
    good = M.retime_route_one(models, nseg, table[b], sx[b], su[b], sT[b], n_grid, None)
    assert good[2]["status"] == 0
    x = sx[b].copy(); x[1, 3, 2] = np.nan                  # a NaN node in the second leg fails the whole route
    prof, leg_T, rec = M.retime_route_one(models, nseg, table[b], x, su[b], sT[b], n_grid, None)
    assert rec["status"] == RR.NAN and (rec["leg_fail"], rec["k_fail"]) == (-1, -1) and np.isnan(prof).all() and np.isposinf(leg_T).all() and np.isposinf(rec["T_new"])
    for T in (np.nan, np.inf, 0.0, -1.0):
        Tb = sT[b].copy(); Tb[1] = T
        assert M.retime_route_one(models, nseg, table[b], sx[b], su[b], Tb, n_grid, None)[2]["status"] == RR.NAN
    for spec in (M.retime_spec(rate_max=0.0), M.retime_spec(rate_max=np.nan), M.retime_spec(groups=1), M.retime_spec(-1.0)):
        with pytest.raises(M.MpcmpError):
            M.retime_route_one(models, nseg, table[b], sx[b], su[b], sT[b], n_grid, spec)
    for n in (0, 4097):
        with pytest.raises(M.MpcmpError):
            M.retime_route_one(models, nseg, table[b], sx[b], su[b], sT[b], n, None)
    arr = (M.Model * 1)(models[0])
    xx, uu, TT, rr = np.ascontiguousarray(sx[b]), np.ascontiguousarray(su[b]), np.ascontiguousarray(sT[b]), np.ascontiguousarray(table[b])
    prof = np.full((2, 51, 2), 7.0); leg_T = np.full(2, 7.0); rec = np.zeros(1, dtype=M.ROUTE_RETIME_DTYPE); rec["k_fail"] = 7
    args = dict(mdl=arr, narm=1, ns=nseg, nl=2, r=rr.ctypes.data, x=xx.ctypes.data, u=uu.ctypes.data, T=TT.ctypes.data, n=50, p=prof.ctypes.data,
                out=rec.ctypes.data)
    call = lambda mdl, narm, ns, nl, r, x, u, T, n, p, out: M.lib().mpcmp_retime_route_one(mdl, narm, ns, nl, r, None, x, u, T, n, p, leg_T.ctypes.data, out)
    for bad in (dict(mdl=None), dict(narm=0), dict(narm=3), dict(ns=0), dict(ns=9), dict(nl=0), dict(r=None), dict(x=None), dict(u=None), dict(T=None),
                dict(p=None), dict(out=None)):
        assert call(**dict(args, **bad)) == -1, bad
        assert (prof == 7.0).all() and (leg_T == 7.0).all() and rec["k_fail"][0] == 7, bad
    assert call(**args) == 0 and rec["status"][0] == 0 and prof.tobytes() == good[0].tobytes() and leg_T.tobytes() == good[1].tobytes()
    assert M.lib().mpcmp_retime_route_one(arr, 1, nseg, 2, rr.ctypes.data, None, xx.ctypes.data, uu.ctypes.data, TT.ctypes.data, 50, prof.ctypes.data, None,
                                          rec.ctypes.data) == 0        # leg_T_new may be NULL
