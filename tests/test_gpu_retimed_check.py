"""Limits of retimed plans and routes on the GPU (mpcmp_limits_retimed_batch*, mpcmp_limits_retimed_route_batch*, mpcmp_profile_scale_batch*) against
the NumPy reference of tests/retimed_check_reference.py, with the case builders, the bounds and the fair-test conditions of
tests/test_retimed_check_host.py (its docstring states them: 1e-9 on excess and stretch, T_new exact, the exact fields under the near-tol exemption).

Inputs: the 32 moves / 16 routes, rows and tool maxima of the retiming tests (no solve); tol = 1e-6 in every group.  The profile is the GPU's own,
from Solver.retime / Solver.retime_route, and the reference reads that same array.

Largest deviations seen (run with -s): see DESIGN.md, "Retimed plans between the grid points".
"""
import json
import os
import subprocess

import numpy as np
import pytest

import retimed_check_reference as RC
from test_gpu_limits import MARGINS, TOL, _case as limits_case, check_records, moves, robot, rows as limits_rows, select_np, solver
from test_gpu_route_retime import route_solver
from test_limits_host import GROUPS, QD, QDD, TAU, TOOL_LIN, TOOL_ANG
from test_retime_host import B, case, check_limits_hold, rows
from test_retimed_check_host import (KINEMATIC, assert_failed, assert_plans_are_a_fair_test, assert_routes_are_a_fair_test, check_retimed, counts,
                                     plan_references, report, route_references)
from test_route_retime_host import B as RB, case as route_case, route_moves, route_rows

pytestmark = pytest.mark.gpu
EINVAL = -1
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def plan_setup(M, nseg, narm, n_grid, nb=B):
    """the common plans retimed on the GPU: (solver with the rows set, models, sx, su, sT, table, lin_max, ang_max, prof, retime records)"""
    sx, su, sT = [a[:nb] for a in moves(narm, nseg)]
    lin_max, ang_max, _, _ = case(narm, nseg, n_grid)
    table = rows(M, B, nseg, narm)[:nb]
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    prof, rec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    return s, robot(M, narm), sx, su, sT, table, lin_max, ang_max, prof, rec


def route_setup(M, nseg, narm, nvia, n_grid):
    sx, su, sT = route_moves(narm, nseg, nvia)
    lin_max, ang_max, _, _ = route_case(narm, nseg, nvia, n_grid)
    table = route_rows(M, nseg, narm, nvia, n_grid)
    s = route_solver(M, narm, nseg, nvia, table)
    prof, _, rec = s.retime_route(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    return s, robot(M, narm), sx, su, sT, table, lin_max, ang_max, prof, rec


# ---- 1. parity, plans -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grid,n_pts", [(1, 1), (50, 200), (200, 50)])
@pytest.mark.parametrize("nseg,narm", [(1, 1), (4, 1), (6, 2), (8, 2)])
def test_parity_with_the_numpy_reference_plans(M, nseg, narm, n_grid, n_pts):
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid)
    ref = plan_references(models, nseg, sx, su, sT, prof, table, n_pts, lin_max, ang_max)
    c = assert_plans_are_a_fair_test(ref) if n_pts >= 50 else counts(ref)
    got, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    assert [r["failed"] for r in ref] == list(rrec["status"] != 0) and (T_new[rrec["status"] == 0] == rrec["T_new"][rrec["status"] == 0]).all()
    worst = np.zeros(GROUPS)
    try:
        check_retimed(M, got, T_new, ref, n_pts, what="plans", worst=worst)
    finally:
        report("plans, nseg %d, arms %d, n_grid %d, n_pts %d" % (nseg, narm, n_grid, n_pts), c, got, ref, worst)


def test_parity_on_the_strided_sample_loop(M):
    """n_pts = 300: the first 45 threads of a workgroup take two samples"""
    nseg, narm, n_grid, n_pts = 4, 1, 50, 300
    s, models, sx, su, sT, table, lin_max, ang_max, prof, _ = plan_setup(M, nseg, narm, n_grid)
    ref = plan_references(models, nseg, sx, su, sT, prof, table, n_pts, lin_max, ang_max)
    assert_plans_are_a_fair_test(ref)
    got, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    check_retimed(M, got, T_new, ref, n_pts, what="300")
    assert sum(1 for g, t, r in zip(got, T_new, ref) if not r["failed"] and round(g["t_at"][QDD] / t * n_pts) >= 256) >= 1      # a second-pass sample is named


def test_parity_at_the_full_bisection_depth(M):
    """n_grid = 4096, n_pts = 64: twelve bisection steps; one problem (a tight row)"""
    nseg, narm, n_grid, n_pts, b = 4, 1, 4096, 64, 1
    sx, su, sT = [a[b:b + 1] for a in moves(narm, nseg)]
    table = rows(M)[b:b + 1]
    lin_max, ang_max, _, _ = case(narm, nseg, 50)
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    prof, rrec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    assert rrec["status"][0] == 0 and rrec["rate_min"][0] < 0.99
    ref = plan_references(robot(M, narm), nseg, sx, su, sT, prof, table, n_pts, lin_max, ang_max)
    got, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    check_retimed(M, got, T_new, ref, n_pts, what="4096")


# ---- 2. parity, routes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm,nvia", [(4, 1, 0), (4, 1, 1), (6, 2, 3)])
def test_parity_with_the_numpy_reference_routes(M, nseg, narm, nvia):
    n_grid, n_pts = 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = route_setup(M, nseg, narm, nvia, n_grid)
    ref = route_references(models, nseg, sx, su, sT, prof, table, n_pts, lin_max, ang_max)
    c = assert_routes_are_a_fair_test(ref)
    got, T_new = s.limits_retimed_route(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    assert [r["failed"] for r in ref] == list(rrec["status"] != 0) and (T_new[rrec["status"] == 0] == rrec["T_new"][rrec["status"] == 0]).all()
    worst = np.zeros(GROUPS)
    try:
        check_retimed(M, got, T_new, ref, n_pts, what="routes", worst=worst)
    finally:
        report("routes, nseg %d, arms %d, M %d, n_grid %d, n_pts %d" % (nseg, narm, nvia, n_grid, n_pts), c, got, ref, worst)
    if nvia == 0:          # a route without vias is a plan: the plan call's record, bit for bit
        plan, plan_T = s.limits_retimed(sx[:, 0], su[:, 0], sT[:, 0], prof[:, 0], n_pts, TOL, lin_max, ang_max)
        assert plan.tobytes() == got.tobytes() and plan_T.tobytes() == T_new.tobytes()


# ---- 3. what the feature is for ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_the_limits_hold_at_the_grid_points_and_not_between_them(M, nseg, narm):
    n_grid, n_pts = 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid)
    _, _, rref, _ = case(narm, nseg, n_grid)
    got, _ = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    ok = np.flatnonzero(rrec["status"] == 0)
    for b in ok:
        check_limits_hold(dict(P=rref[b]["P"], T=sT[b]), table[b], prof[b, :, 1], lin_max, ang_max, what=b)
    over = [b for b in ok if got[b]["status"] >> QDD & 1]
    print("nseg %d, arms %d: %d of %d feasible plans over QDD between grid points, worst %.3f rad/s^2" % (nseg, narm, len(over), len(ok), got["excess"][ok, QDD].max()))
    assert len(over) >= 3, over


# ---- 4. identity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_a_profile_of_one_is_the_plan_as_solved(M, nseg, narm):
    """x == 1 with t_k = k / n_grid * T: the record of Solver.limits at the same n_pts"""
    n_grid, n_pts = 50, 200
    sx, su, sT = moves(narm, nseg)
    _, lin_max, ang_max, lref = limits_case(narm, nseg, n_pts)
    s = solver(M, narm, nseg)
    s.set_bounds(limits_rows(M, B, nseg))
    prof = np.ones((B, n_grid + 1, 2))
    prof[:, :, 0] = (np.arange(n_grid + 1) / n_grid)[None, :] * sT[:, None]
    plain = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    got, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    assert (T_new == sT).all()
    finite = np.isfinite(plain["excess"])
    assert (got["excess"][~finite] == plain["excess"][~finite]).all()
    assert np.abs(got["excess"][finite] - plain["excess"][finite]).max() <= 1e-9 and np.abs(got["stretch"] - plain["stretch"]).max() <= 1e-9
    for b in range(B):
        if not lref[b]["near"]:
            assert (got[b]["status"], got[b]["n_viol"]) == (plain[b]["status"], plain[b]["n_viol"]), b
            assert abs(got[b]["t_first"] - plain[b]["t_first"]) <= 1e-12 * sT[b], b
    check_records(got, lref, sT, n_pts, TOL, "identity")


# ---- 5. against the sampler -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_the_named_sample_of_the_sampler_reproduces_the_excess(M, nseg, narm):
    n_grid, n_pts = 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid)
    got, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    samples = s.sample_retimed(sx, su, sT, prof, n_pts)
    spec = M.limits_spec(TOL, lin_max, ang_max)
    worst = 0.0
    for b in np.flatnonzero(rrec["status"] == 0):
        for g in range(GROUPS):
            if got[b]["t_at"][g] < 0:          # (a group without bounds names no sample)
                continue
            ip = int(round(got[b]["t_at"][g] / T_new[b] * n_pts))
            assert got[b]["t_at"][g] == samples[b, ip, 0], (b, g)
            row = samples[b, ip]
            cat = lambda lo: np.concatenate([row[1 + 28 * a + lo:8 + 28 * a + lo] for a in range(narm)])
            ex, ch, _ = M.limits_config(models, table[b], cat(0), cat(7), cat(14), spec)
            worst = max(worst, abs(ex[g] - got[b]["excess"][g]))
            assert abs(ex[g] - got[b]["excess"][g]) <= 1e-9, (b, g, ex[g], got[b]["excess"][g])
    print("nseg %d, arms %d: max |excess - limits_config(sampler row)| %.1e" % (nseg, narm, worst))


# ---- 6. scale ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_scaling_by_the_stretch_cures_the_kinematic_groups(M, nseg, narm):
    n_grid, n_pts = 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid)
    got, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    ok = rrec["status"] == 0
    assert np.isfinite(got["stretch"][ok]).all() and (got["stretch"][ok] > 1 + 1e-6).sum() >= 3
    scaled = s.profile_scale(prof, got["stretch"])
    for b in range(B):          # the rule itself, and NaN profiles stay NaN
        assert np.array_equal(scaled[b], RC.scale_np(prof[b], got["stretch"][b]), equal_nan=True), b
    cured, T2 = s.limits_retimed(sx, su, sT, scaled, n_pts, TOL, lin_max, ang_max)
    print("nseg %d, arms %d: worst kinematic excess after scaling by the stretch %.1e, worst stretch - 1 %.1e" % (
        nseg, narm, cured["excess"][ok][:, KINEMATIC].max(), cured["stretch"][ok].max() - 1))
    assert cured["excess"][ok][:, KINEMATIC].max() <= 1e-9 and cured["stretch"][ok].max() <= 1 + 1e-9
    assert (np.abs(T2[ok] - got["stretch"][ok] * T_new[ok]) <= 1e-12 * T2[ok]).all()
    for b in np.flatnonzero(~ok):
        assert_failed(M, cured[b], T2[b], b)
    # a bad factor makes that slot's profile NaN and leaves its neighbours alone; the device variant works in place
    import torch
    f = np.ones(B); f[[1, 2, 3, 4]] = [0.0, -1.0, np.inf, np.nan]
    bad = s.profile_scale(prof, f)
    assert np.isnan(bad[1:5]).all() and np.array_equal(bad[5:], prof[5:], equal_nan=True) and np.array_equal(bad[0], prof[0], equal_nan=True)
    dprof, dfac = torch.from_numpy(prof.copy()).cuda(), torch.from_numpy(got["stretch"].copy()).cuda()
    s.profile_scale_device(B, n_grid, dfac.data_ptr(), dprof.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dprof.cpu().numpy().tobytes() == scaled.tobytes()


def test_scaling_a_route_with_one_factor_per_route(M):
    nseg, narm, nvia, n_grid, n_pts = 4, 1, 1, 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = route_setup(M, nseg, narm, nvia, n_grid)
    got, T_new = s.limits_retimed_route(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    ok = rrec["status"] == 0
    # (the ends of these routes are at rest, so no pinned end changes its speed)
    scaled = s.profile_scale(prof, M.Solver.repeat(got["stretch"], nvia))
    assert scaled.shape == prof.shape and (scaled[ok][:, :-1, -1, 1] == scaled[ok][:, 1:, 0, 1]).all()          # the rate stays continuous at the junctions
    cured, T2 = s.limits_retimed_route(sx, su, sT, scaled, n_pts, TOL, lin_max, ang_max)
    assert cured["excess"][ok][:, KINEMATIC].max() <= 1e-9 and cured["stretch"][ok].max() <= 1 + 1e-9
    assert (np.abs(T2[ok] - got["stretch"][ok] * T_new[ok]) <= 1e-12 * T2[ok]).all()


# ---- 7. selection -----------------------------------------------------------------------------------------------------------------------------
def test_selection_on_the_retimed_records(M):
    """select_checked reads the records as they stand, with T_new as its sol_T: per group of four candidates the fastest RETIMED plan that keeps
    its limits between the grid points; a failed profile (T_new +inf, MPCMP_LIM_NAN) is never chosen"""
    nseg, narm, n_grid, n_pts, K = 4, 1, 50, 200, 4
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid)
    got, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    group = (np.arange(B) // K).astype(np.int32)
    info = np.zeros(B, dtype=M.INFO_DTYPE)
    failed = rrec["status"] != 0
    assert failed.sum() >= 2 and np.isposinf(T_new[failed]).all()
    for mask in ((1 << QD) | (1 << QDD) | (1 << TOOL_LIN) | (1 << TOOL_ANG), 1 << QDD, 0, 0x7F):
        chosen = s.select_checked(T_new, info, group, None, got, mask, B // K)
        assert np.array_equal(chosen, select_np(T_new, info["status"], None, got["status"], mask, group, B // K)), mask
        assert not failed[chosen[chosen >= 0]].any(), mask
    # with no limit bit asked for, only the failed profiles are rejected: the fastest retimed plan of every group that has one
    chosen = s.select_checked(T_new, info, group, None, got, 0, B // K)
    for g in range(B // K):
        members = np.flatnonzero((group == g) & ~failed)
        assert chosen[g] == (members[np.argmin(T_new[members])] if len(members) else -1), g
    # ... and the limit record of the plans as solved selects differently: the gap this check closes
    plain = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    assert (plain["status"] != got["status"])[~failed].sum() >= 3
    # a group of failed profiles only
    only = np.flatnonzero(failed)[:2]
    assert list(s.select_checked(T_new[only], info[only], np.zeros(2, dtype=np.int32), None, got[only], 0, 1)) == [-1]


# ---- 8. remaining cases -----------------------------------------------------------------------------------------------------------------------
def test_payload_rows_change_the_torque_group(M):
    """1 kg and 3 kg on alternate problems: retimed and checked under the lumped models, as the reference with those models does"""
    nseg, narm, n_grid, n_pts = 4, 1, 50, 50
    sx, su, sT = moves(narm, nseg)
    lin_max, ang_max, _, _ = case(narm, nseg, n_grid)
    table = rows(M, B, nseg, narm)
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    prof, rrec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    plain, _ = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    mass = np.where(np.arange(B) % 2 == 0, 1.0, 3.0)
    s.set_payloads(mass)
    base = robot(M, narm)
    lumped = {m: [M.model_add_payload(bm, M.payload(m, bm.tool[:])) for bm in base] for m in (1.0, 3.0)}
    loaded, T_new = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)            # (the same profile: only the torque moves)
    ref = plan_references([lumped[m] for m in mass], nseg, sx, su, sT, prof, table, n_pts, lin_max, ang_max)
    check_retimed(M, loaded, T_new, ref, n_pts, what="payload")
    ok = rrec["status"] == 0
    assert (np.abs(loaded["excess"][ok, TAU] - plain["excess"][ok, TAU]) > 1e-3).sum() >= ok.sum() // 2
    for f in ("excess", "t_at", "channel"):
        assert np.delete(loaded[f], TAU, axis=1).tobytes() == np.delete(plain[f], TAU, axis=1).tobytes(), f
    assert loaded["stretch"].tobytes() == plain["stretch"].tobytes()
    s.clear_payloads()
    assert s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)[0].tobytes() == plain.tobytes()


def test_payload_rows_of_the_leg_slots(M):
    """a route whose legs carry 1 kg and 3 kg: every sample under the payload row of its leg slot"""
    nseg, narm, nvia, n_grid, n_pts = 4, 1, 1, 50, 50
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = route_setup(M, nseg, narm, nvia, n_grid)
    plain, _ = s.limits_retimed_route(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    s.set_payloads(np.tile([1.0, 3.0], RB))
    lumped = [[M.model_add_payload(models[0], M.payload(m, models[0].tool[:]))] for m in (1.0, 3.0)]
    loaded, T_new = s.limits_retimed_route(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    ref = route_references([lumped] * RB, nseg, sx, su, sT, prof, table, n_pts, lin_max, ang_max)
    check_retimed(M, loaded, T_new, ref, n_pts, what="leg payloads")
    ok = rrec["status"] == 0
    assert (np.abs(loaded["excess"][ok, TAU] - plain["excess"][ok, TAU]) > 1e-3).sum() >= ok.sum() // 2


@pytest.mark.parametrize("nseg,narm", [(4, 1), (8, 2)])
def test_a_record_does_not_depend_on_the_batch(M, nseg, narm):
    n_grid, n_pts = 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid)
    base, base_T = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    for b in (0, 17, 31):
        s.set_bounds(table[b:b + 1])
        one, one_T = s.limits_retimed(sx[b:b + 1], su[b:b + 1], sT[b:b + 1], prof[b:b + 1], n_pts, TOL, lin_max, ang_max)
        assert one[0].tobytes() == base[b].tobytes() and one_T.tobytes() == base_T[b:b + 1].tobytes(), b
    order = np.random.default_rng(5).permutation(B)
    s.set_bounds(table[order])
    moved, moved_T = s.limits_retimed(sx[order], su[order], sT[order], prof[order], n_pts, TOL, lin_max, ang_max)
    assert moved.tobytes() == base[order].tobytes() and moved_T.tobytes() == base_T[order].tobytes()


def test_a_route_record_does_not_depend_on_the_batch(M):
    nseg, narm, nvia, n_grid, n_pts = 6, 2, 3, 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = route_setup(M, nseg, narm, nvia, n_grid)
    base, base_T = s.limits_retimed_route(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    for b in (0, 7, 15):
        s.set_bounds(np.ascontiguousarray(table[b]))
        one, one_T = s.limits_retimed_route(sx[b:b + 1], su[b:b + 1], sT[b:b + 1], prof[b:b + 1], n_pts, TOL, lin_max, ang_max)
        assert one[0].tobytes() == base[b].tobytes() and one_T.tobytes() == base_T[b:b + 1].tobytes(), b


@pytest.mark.parametrize("nseg,narm", [(4, 1), (8, 2)])
def test_device_variants_equal_the_host_pointer_variants(M, nseg, narm):
    import torch
    n_grid, n_pts = 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid)
    host, host_T = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (sx, su, sT, prof)]
    dout = torch.zeros(B * M.LIMITS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dT = torch.full((B,), -7.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    spec = M.limits_spec(TOL, lin_max, ang_max)
    s.limits_retimed_device(B, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n_grid, dev[3].data_ptr(), n_pts, dout.data_ptr(), dT.data_ptr(), spec, stream=stream)
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == host.tobytes() and dT.cpu().numpy().tobytes() == host_T.tobytes()
    # T_new may be left out; a NULL spec is tol 0 and no tool limit
    dT.fill_(-7.0)
    s.limits_retimed_device(B, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n_grid, dev[3].data_ptr(), n_pts, dout.data_ptr(), 0, None, stream=stream)
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == s.limits_retimed(sx, su, sT, prof, n_pts)[0].tobytes() and (dT.cpu().numpy() == -7.0).all()


def test_route_device_variant_equals_the_host_pointer_variant(M):
    import torch
    nseg, narm, nvia, n_grid, n_pts = 4, 1, 1, 50, 200
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = route_setup(M, nseg, narm, nvia, n_grid)
    host, host_T = s.limits_retimed_route(sx, su, sT, prof, n_pts, TOL, lin_max, ang_max)
    dev = [torch.from_numpy(np.array(a)).cuda() for a in (sx, su, sT, prof)]
    dout = torch.zeros(RB * M.LIMITS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    dT = torch.zeros(RB, dtype=torch.float64, device="cuda")
    s.limits_retimed_route_device(RB, nvia, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), n_grid, dev[3].data_ptr(), n_pts, dout.data_ptr(),
                                  dT.data_ptr(), M.limits_spec(TOL, lin_max, ang_max), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == host.tobytes() and dT.cpu().numpy().tobytes() == host_T.tobytes()


def test_failed_profiles_and_non_finite_values_are_reported(M):
    nseg, narm, n_grid, n_pts = 4, 1, 50, 50
    s, models, sx, su, sT, table, lin_max, ang_max, prof, rrec = plan_setup(M, nseg, narm, n_grid, 16)
    sx, su, sT = np.array(sx), np.array(su), np.array(sT)
    good = np.flatnonzero(rrec["status"] == 0)
    assert len(good) >= 5 and (rrec["status"] != 0).any()
    a, b, c, d = good[:4]
    sx[a, 5, 3] = np.nan; su[b, 0, 6] = np.inf; sT[c] = np.nan
    p = prof.copy(); p[d] = np.nan
    got, T_new = s.limits_retimed(sx, su, sT, p, n_pts, TOL, lin_max, ang_max)
    for i in (a, b, c):          # a non-finite node value or sol_T under a finite profile: the finite T_new
        assert_failed(M, got[i], None, i)
        assert T_new[i] == prof[i, -1, 0], i
    for i in [d] + list(np.flatnonzero(rrec["status"] != 0)):
        assert_failed(M, got[i], T_new[i], i)
    rest = [i for i in good if i not in (a, b, c, d)]
    assert (got["status"][rest] & M.LIM_NAN == 0).all() and np.isfinite(got["excess"][rest][:, :4]).all() and np.isfinite(T_new[rest]).all()
    # a route fails as a whole when one leg's profile is not finite, and reports a NaN node of any leg
    s, models, rx, ru, rT, table, lin_max, ang_max, rprof, rrec = route_setup(M, 4, 1, 1, 50)
    good = np.flatnonzero(rrec["status"] == 0)
    a, b = good[:2]
    p = rprof.copy(); p[a, 1] = np.nan
    rx = np.array(rx); rx[b, 1, 2, 4] = np.nan
    got, T_new = s.limits_retimed_route(rx, ru, rT, p, n_pts, TOL, lin_max, ang_max)
    assert_failed(M, got[a], T_new[a], "route profile")
    assert_failed(M, got[b], None, "route node")
    assert np.isfinite(T_new[b]) and (got["status"][good[2:]] & M.LIM_NAN == 0).all()


def test_errors_write_nothing(M):
    n, n_grid, n_pts = 4, 20, 20
    sx, su, sT = [np.array(a[:n]) for a in moves(1, 4)]
    s = solver(M, 1, 4, 8)
    prof, _ = s.retime(sx, su, sT, n_grid)
    good, good_T = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, 1.0, 2.0)
    L, ctx = M.lib(), s._ctx
    big = [np.zeros((9,) + a.shape[1:]) for a in (sx, su, sT, prof)]
    ptr = lambda a: a.ctypes.data

    def call(B_=n, M_=None, sx_=ptr(sx), su_=ptr(su), sT_=ptr(sT), g_=n_grid, p_=ptr(prof), n_=n_pts, spec=M.limits_spec(TOL, 1.0, 2.0), out=True, device=False):
        o_ = np.zeros(9, dtype=M.LIMITS_DTYPE); o_["n_viol"] = -9
        t_ = np.full(9, -9.0)
        a = (ctx, B_) + (() if M_ is None else (M_,)) + (sx_, su_, sT_, g_, p_, n_, None if spec is None else spec.ctypes.data, ptr(o_) if out else None, ptr(t_))
        name = "mpcmp_limits_retimed_batch" if M_ is None else "mpcmp_limits_retimed_route_batch"
        rc = getattr(L, name + "_device")(*a, None) if device else getattr(L, name)(*a)
        assert np.all(o_["n_viol"] == -9) and np.all(t_ == -9.0)
        return rc
    bad = [dict(B_=0), dict(B_=-3), dict(B_=9, sx_=ptr(big[0]), su_=ptr(big[1]), sT_=ptr(big[2]), p_=ptr(big[3])), dict(n_=0), dict(n_=4097), dict(g_=0),
           dict(g_=4097), dict(sx_=None), dict(su_=None), dict(sT_=None), dict(p_=None), dict(out=False), dict(spec=M.limits_spec(np.nan)),
           dict(spec=M.limits_spec(np.inf)), dict(spec=M.limits_spec(0.0, np.nan)), dict(spec=M.limits_spec(0.0, 1.0, -1.0))]
    for kw in bad:
        for device in (False, True):          # (nothing is launched: the host addresses are never read)
            assert call(device=device, **kw) == EINVAL, kw
            assert call(device=device, M_=0, **kw) == EINVAL, kw
    for device in (False, True):
        assert call(device=device, B_=2, M_=-1) == EINVAL
        assert call(device=device, B_=3, M_=2) == EINVAL          # 9 leg slots above max_batch 8
    assert L.mpcmp_limits_retimed_batch(None, n, ptr(sx), ptr(su), ptr(sT), n_grid, ptr(prof), n_pts, None, ptr(good), None) == EINVAL
    # more problems (leg slots) than rows in force
    s.set_bounds(rows(M, 3))
    assert call() == EINVAL and call(B_=2, M_=1) == EINVAL
    s.clear_bounds()
    s.set_payloads(np.ones(2))
    assert call() == EINVAL and call(B_=2, M_=1) == EINVAL
    s.clear_payloads()
    # the scale call
    f = np.ones(n)
    for kw in (dict(L_=0), dict(L_=9), dict(g_=0), dict(g_=4097), dict(f_=None), dict(p_=None)):
        a = dict(L_=n, g_=n_grid, f_=ptr(f), p_=ptr(prof)); a.update(kw)
        before = prof.copy()
        assert L.mpcmp_profile_scale_batch(ctx, a["L_"], a["g_"], a["f_"], a["p_"]) == EINVAL, kw
        assert L.mpcmp_profile_scale_batch_device(ctx, a["L_"], a["g_"], a["f_"], a["p_"], None) == EINVAL, kw
        assert prof.tobytes() == before.tobytes()
    assert L.mpcmp_profile_scale_batch(None, n, n_grid, ptr(f), ptr(prof)) == EINVAL
    again, again_T = s.limits_retimed(sx, su, sT, prof, n_pts, TOL, 1.0, 2.0)
    assert again.tobytes() == good.tobytes() and again_T.tobytes() == good_T.tobytes()
    # a route of one leg through the route call, a maximum of 0 and one of +inf are values
    r, rT = s.limits_retimed_route(sx[:, None], su[:, None], sT[:, None], prof[:, None], n_pts, TOL, 1.0, 2.0)
    assert r.tobytes() == good.tobytes() and rT.tobytes() == good_T.tobytes()
    assert s.limits_retimed(sx, su, sT, prof, n_pts, TOL, 0.0, np.inf)[0].shape == (n,)


def test_the_calls_leave_the_solve_bit_for_bit(M):
    from mpc_motion_planner_amd import scenarios
    n = 64
    cfg = M.default_config(4, 2, margins=MARGINS)
    x0, xf = scenarios.make_batch(n, MARGINS)
    plain = M.Solver(cfg, n).solve(x0, xf)
    s = M.Solver(cfg, n)
    got = s.solve(x0, xf)
    prof, _ = s.retime(got[0], got[1], got[2], 50)
    rec, _ = s.limits_retimed(got[0], got[1], got[2], prof, 50, TOL, 1.0, 2.0)
    s.limits_retimed_route(got[0][:, None], got[1][:, None], got[2][:, None], prof[:, None], 50, TOL, 1.0, 2.0)
    s.profile_scale(prof, np.where(np.isfinite(rec["stretch"]), rec["stretch"], 1.0))
    again = s.solve(x0, xf)
    for a, b, c in zip(plain, got, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_planner_facade(M):
    from mpc_motion_planner_amd import scenarios
    from test_gpu_routes import _vias
    p = M.BatchMotionPlanner(max_batch=8, num_seg=2, sqp_iters=3)
    p.set_constraint_margins(*MARGINS)
    x0, xf = scenarios.make_batch(2, MARGINS)
    p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
    p.solve_trajectory()
    for call in (p.check_retimed_limits, p.check_retimed_route_limits):
        with pytest.raises(ValueError):
            call()
    spec = M.retime_spec(1.7, 2.5)
    prof, _ = p.retime(n_grid=60, spec=spec)
    rec, T_new = p.check_retimed_limits(n_pts=100, tol=TOL, tool_lin_max=1.7, tool_ang_max=2.5)
    sx, su, sT = p.solution()
    want = p._solver.limits_retimed(sx, su, sT, prof, 100, TOL, 1.7, 2.5)
    assert rec.dtype == M.LIMITS_DTYPE and rec.shape == (2,) and rec.tobytes() == want[0].tobytes() and T_new.tobytes() == want[1].tobytes()
    with pytest.raises(ValueError):
        p.check_retimed_route_limits()
    p.set_via_points(_vias(M, x0, xf, 2, 1))
    p.solve_trajectory()
    for call in (p.check_retimed_limits, p.check_retimed_route_limits):
        with pytest.raises(ValueError):
            call()
    prof, _, rrec = p.retime_route(n_grid=60, spec=spec)
    rec, T_new = p.check_retimed_route_limits(n_pts=100, tol=TOL, tool_lin_max=1.7, tool_ang_max=2.5)
    sx, su, sT = p.solution()
    want = p._solver.limits_retimed_route(sx, su, sT, prof, 100, TOL, 1.7, 2.5)
    assert rec.shape == (2,) and rec.tobytes() == want[0].tobytes() and T_new.tobytes() == want[1].tobytes()
    ok = rrec["status"] == 0
    assert (T_new[ok] == rrec["T_new"][ok]).all() and np.isposinf(T_new[~ok]).all()


def test_cpp_shim_members(M, tmp_path):
    """examples/retimed_check_selftest.cpp calls the header-only planner's check_retimed_limits and check_retimed_route_limits: they throw while no
    profile is present, and their records are consistent ones on the retimed clock"""
    exe = str(tmp_path / "retimed_check_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "examples", "retimed_check_selftest.cpp"),
                           "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp", "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"),
                           "-o", exe])
    r = json.loads(subprocess.check_output([exe]).decode())
    assert r["threw"] == 7 and r["route_threw"] == 1 and r["same"] == 1
    for pre in ("", "route_"):
        if r[pre + "rt_status"] == 0:
            assert r[pre + "T_new"] == r[pre + "rt_T_new"] > 0 and r[pre + "status"] & ~0x7F == 0 and r[pre + "stretch"] >= 1.0
            assert np.isfinite(r[pre + "excess_qdd"]) and 0.0 <= r[pre + "t_at_qdd"] <= r[pre + "T_new"]
            assert (r[pre + "n_viol"] > 0) == (r[pre + "status"] != 0)
        else:
            assert r[pre + "status"] == M.LIM_NAN and r[pre + "T_new"] == -1.0 and r[pre + "n_viol"] == 0
    assert r["rt_status"] == 0 and 0 <= r["channel_qdd"] < 7
