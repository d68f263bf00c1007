"""Retiming on the GPU (mpcmp_retime_batch*, mpcmp_sample_retimed_batch*) against the NumPy restatement of tests/retime_reference.py, with the case
builder, the bounds and the fair-test conditions of tests/test_retime_host.py (its docstring derives the 1e-8 parity bound).

Inputs: the 32 rest-to-rest jerk-limited moves of tests/test_gpu_limits.py::moves (same seed; no solve); (num_seg, arms) in (1, 1), (4, 1), (6, 1),
(6, 2), (8, 2); n_grid 1 (one interval), 50 (does not fill the 64-point chunk), 200 (crosses chunks), one problem at 4096.  Rows alternate between
the loose and the tight row of test_retime_host.rows; the tool maxima are the batch medians of the reference's peak tool speeds.

Largest deviations seen (run with -s): see DESIGN.md, "Retiming".
"""
import numpy as np
import pytest

import oracle_py as o
import retime_reference as R
from test_gpu_limits import moves, robot, solver
from test_retime_host import (B, KINEMATIC, assert_reference_is_a_fair_test, case, check_against, check_limits_hold, reference, rows, tool_maxima)

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_grid", [1, 50, 200])
@pytest.mark.parametrize("nseg,narm", [(1, 1), (4, 1), (6, 1), (6, 2), (8, 2)])
def test_parity_with_the_numpy_reference(M, nseg, narm, n_grid):
    sx, su, sT = moves(narm, nseg)
    lin_max, ang_max, ref, amp = case(narm, nseg, n_grid)
    counts = assert_reference_is_a_fair_test(ref, amp) if n_grid >= 50 else None
    s = solver(M, narm, nseg)
    s.set_bounds(rows(M, B, nseg, narm))
    prof, rec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    worst = [0.0, 0.0]
    try:
        check_against(ref, prof, rec, worst=worst)
    finally:
        print("nseg %d, arms %d, n_grid %d: slowed / untouched / infeasible %s, amplification %.1f, max |x / ref - 1| %.1e, |T_new / ref - 1| %.1e"
              % (nseg, narm, n_grid, counts, amp, worst[0], worst[1]))


def test_parity_at_the_largest_grid(M):
    """n_grid = 4096: 65 chunks; one problem (a tight row)"""
    nseg, narm, n_grid, b = 4, 1, 4096, 1
    sx, su, sT = [a[b:b + 1] for a in moves(narm, nseg)]
    table = rows(M)[b:b + 1]
    ref = reference(M, robot(M, narm), nseg, sx, su, sT, table, n_grid, np.inf, np.inf)
    lin_max, ang_max = 0.9 * ref[0]["P"]["vlin"].max(), 0.9 * ref[0]["P"]["vang"].max()
    ref = reference(M, robot(M, narm), nseg, sx, su, sT, table, n_grid, lin_max, ang_max, P=[ref[0]["P"]])
    assert ref[0]["status"] == 0 and ref[0]["rate_min"] < 0.99 and not ref[0]["near"]
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    prof, rec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    check_against(ref, prof, rec, what="4096")


# ---- 2. properties --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_the_limits_hold_and_the_gain_over_the_stretch(M, nseg, narm):
    """the GPU's profile of every feasible problem keeps every group within its bounds at every grid point (1e-9 relative to the bound); for the
    groups a stretch cures and rate_max 1, T <= T_new <= T * stretch (1 + 1e-9) with the stretch of mpcmp_limits_batch at n_pts = n_grid, and for at
    least 4 problems T_new < T * stretch - 1e-3 T: the gain the feature exists for.  T <= T_new is held to the rounding of the clock: T_new is a sum of
    n_grid terms, each within 2^-52 of T / n_grid where x == 1, so an untouched plan comes back within n_grid 2^-52 T of T on either side"""
    n_grid = 200
    sx, su, sT = moves(narm, nseg)
    table = rows(M, B, nseg, narm)
    lin_max, ang_max, ref, _ = case(narm, nseg, n_grid)
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    prof, rec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    assert (rec["status"] == 0).sum() >= 8
    for b in np.flatnonzero(rec["status"] == 0):
        check_limits_hold(dict(P=ref[b]["P"], T=sT[b]), table[b], prof[b, :, 1], lin_max, ang_max, what=b)
    prof, rec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max, 1.0, KINEMATIC))
    lim = s.limits(sx, su, sT, n_grid, None, lin_max, ang_max)
    gained = 0
    for b in range(B):
        stretch = lim[b]["stretch"]
        assert np.isfinite(stretch) and rec[b]["status"] == 0, (b, stretch, rec[b])
        assert sT[b] <= rec[b]["T_new"] * (1 + n_grid * 2.3e-16) and rec[b]["T_new"] <= sT[b] * stretch * (1 + 1e-9), (b, sT[b], rec[b]["T_new"], stretch)
        check_limits_hold(dict(P=ref[b]["P"], T=sT[b]), table[b], prof[b, :, 1], lin_max, ang_max, KINEMATIC, what=b)
        gained += rec[b]["T_new"] < sT[b] * stretch - 1e-3 * sT[b]
    print("nseg %d, arms %d: %d of %d plans gain over the stretch; median T_new / T %.3f beside median stretch %.3f"
          % (nseg, narm, gained, B, np.median(rec["T_new"] / sT), np.median(lim["stretch"])))
    assert gained >= 4, gained


# ---- 3. identity ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2), (8, 2)])
def test_no_group_or_no_bound_is_the_plan_as_solved(M, nseg, narm):
    n_grid, n_pts = 50, 40
    sx, su, sT = moves(narm, nseg)
    s = solver(M, narm, nseg)
    free = np.zeros(B, dtype=M.BOUNDS_DTYPE)
    for name in ("lbx", "lbu", "lbg"):
        free[name] = -np.inf
    for name in ("ubx", "ubu", "ubg"):
        free[name] = np.inf
    for table, spec in ((rows(M, B, nseg, narm), M.retime_spec(0.1, 0.1, 1.0, 0)), (free, None)):
        s.set_bounds(table)
        prof, rec = s.retime(sx, su, sT, n_grid, spec)
        assert (rec["status"] == 0).all() and (rec["n_slowed"] == 0).all() and (rec["rate_min"] == 1.0).all() and (rec["k_fail"] == -1).all()
        assert (prof[:, :, 1] == 1.0).all()
        assert (np.abs(prof[:, :, 0] - np.arange(n_grid + 1)[None, :] * sT[:, None] / n_grid) <= 1e-12).all()
        assert (np.abs(rec["T_new"] - sT) <= 1e-12).all()
    # the sampler then gives the rows of the plain sampler (one arm) and of the oracle's, arm by arm
    got = s.sample_retimed(sx, su, sT, prof, n_pts)
    assert got.shape == (B, n_pts + 1, 1 + 28 * narm)
    if narm == 1:
        assert np.abs(got - s.sample(sx, su, sT, n_pts)).max() <= 1e-10
    models = robot(M, narm)
    for b in range(0, B, 5):
        for a in range(narm):
            xa, ua = R.arm_nodes(sx[b], su[b], a)
            want = o.sample(nseg, xa, ua, sT[b], n_pts, model=R.omodel(models[a]))
            assert np.abs(got[b][:, 1 + 28 * a:29 + 28 * a] - want[:, 1:]).max() <= 1e-10, (b, a)
            assert np.abs(got[b][:, 0] - want[:, 0]).max() <= 1e-10, b


# ---- 4. the sampler under a slowed profile --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_sampler_under_a_slowed_profile(M, nseg, narm):
    n_grid, n_pts = 50, 37
    sx, su, sT = moves(narm, nseg)
    lin_max, ang_max, ref, _ = case(narm, nseg, n_grid)
    models = robot(M, narm)
    s = solver(M, narm, nseg)
    s.set_bounds(rows(M, B, nseg, narm))
    prof, rec = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max))
    got = s.sample_retimed(sx, su, sT, prof, n_pts)
    slowed = [b for b in range(B) if rec[b]["status"] == 0 and rec[b]["rate_min"] < 0.99][:4]
    failed = [b for b in range(B) if rec[b]["status"]][:2]
    assert len(slowed) == 4 and len(failed) == 2
    nq = 7 * narm
    for b in slowed:
        want = R.sample_retimed_np(models, nseg, sx[b], su[b], sT[b], prof[b], n_pts)
        assert np.abs(got[b] - want).max() <= 1e-9, (b, np.abs(got[b] - want).max())
        assert got[b][0, 0] == 0.0 and got[b][-1, 0] == rec[b]["T_new"]
        for a in range(narm):                     # the ends are the end nodes
            for i, node in ((0, 0), (n_pts, -1)):
                assert np.abs(got[b][i, 1 + 28 * a:8 + 28 * a] - sx[b][node, 7 * a:7 * a + 7]).max() <= 1e-12, (b, a, i)
                assert np.abs(got[b][i, 8 + 28 * a:15 + 28 * a] - np.sqrt(prof[b][node, 1]) * sx[b][node, nq + 7 * a:nq + 7 * a + 7]).max() <= 1e-12
    for b in failed:
        assert np.isnan(got[b]).all()
    # at t == t_k the q columns are the path at s_k: a hand-made symmetric profile over two intervals, whose t_1 is exactly T_new / 2
    T = sT[:4]
    hand = np.zeros((4, 3, 2))
    hand[:, :, 1] = [1.0, 0.25, 1.0]
    hand[:, 1, 0] = 2.0 * T * 0.5 / 1.5
    hand[:, 2, 0] = 2.0 * hand[:, 1, 0]
    mid = solver(M, narm, nseg, 4).sample_retimed(sx[:4], su[:4], T, hand, 2)
    for b in range(4):
        assert mid[b][1, 0] == hand[b, 1, 0]
        for a in range(narm):
            xa, ua = R.arm_nodes(sx[b], su[b], a)
            path = o.sample(nseg, xa, ua, T[b], 2, model=R.omodel(models[a]))[1]
            assert np.abs(mid[b][1, 1 + 28 * a:8 + 28 * a] - path[1:8]).max() <= 1e-12, (b, a)
            assert np.abs(mid[b][1, 8 + 28 * a:15 + 28 * a] - 0.5 * path[8:15]).max() <= 1e-12, (b, a)


# ---- 5. independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_a_record_does_not_depend_on_the_batch(M, nseg, narm):
    n_grid = 200
    sx, su, sT = moves(narm, nseg)
    table = rows(M, B, nseg, narm)
    lin_max, ang_max, _, _ = case(narm, nseg, 50)
    spec = M.retime_spec(lin_max, ang_max)
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    prof, rec = s.retime(sx, su, sT, n_grid, spec)
    perm = np.random.default_rng(5).permutation(B)
    s.set_bounds(table[perm])
    prof_p, rec_p = s.retime(sx[perm], su[perm], sT[perm], n_grid, spec)
    assert prof_p.tobytes() == prof[perm].tobytes() and rec_p.tobytes() == rec[perm].tobytes()
    for b in (0, 1, 7, 30):
        s.set_bounds(table[b:b + 1])
        prof_1, rec_1 = s.retime(sx[b:b + 1], su[b:b + 1], sT[b:b + 1], n_grid, spec)
        assert prof_1.tobytes() == prof[b:b + 1].tobytes() and rec_1.tobytes() == rec[b:b + 1].tobytes(), b


# ---- 6. rows, payloads, defaults, device pointers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_rows_payloads_and_defaults(M, nseg, narm):
    import torch
    n_grid = 50
    sx, su, sT = moves(narm, nseg)
    lin_max, ang_max, ref, _ = case(narm, nseg, n_grid)
    spec = M.retime_spec(lin_max, ang_max)
    s = solver(M, narm, nseg)
    base = robot(M, narm)
    P = [r["P"] for r in ref]
    # no rows set: the configuration's tables for everyone; a NULL spec is no tool limit, rate_max 1 and all groups
    table = np.repeat(M.bounds_from_config(s.cfg), B)
    plain = s.retime(sx, su, sT, n_grid, spec)
    check_against(reference(M, base, nseg, sx, su, sT, table, n_grid, lin_max, ang_max, P=P), *plain, what="defaults")
    null = s.retime(sx, su, sT, n_grid, None)
    assert null[0].tobytes() == s.retime(sx, su, sT, n_grid, M.retime_spec())[0].tobytes()
    check_against(reference(M, base, nseg, sx, su, sT, table, n_grid, np.inf, np.inf, P=P), *null, what="null spec")
    # rows, then cleared again
    s.set_bounds(rows(M, B, nseg, narm))
    with_rows = s.retime(sx, su, sT, n_grid, spec)
    assert with_rows[1].tobytes() != plain[1].tobytes()
    # the device entry points
    dx, du, dT = [torch.from_numpy(np.array(a)).cuda() for a in (sx, su, sT)]
    dprof = torch.zeros((B, n_grid + 1, 2), dtype=torch.float64, device="cuda")
    drec = torch.zeros(B * M.RETIME_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    s.retime_device(B, dx.data_ptr(), du.data_ptr(), dT.data_ptr(), n_grid, dprof.data_ptr(), drec.data_ptr(), spec, stream=stream)
    dout = torch.zeros((B, 11, 1 + 28 * narm), dtype=torch.float64, device="cuda")
    s.sample_retimed_device(B, dx.data_ptr(), du.data_ptr(), dT.data_ptr(), n_grid, dprof.data_ptr(), 10, dout.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert dprof.cpu().numpy().tobytes() == with_rows[0].tobytes() and drec.cpu().numpy().tobytes() == with_rows[1].tobytes()
    assert dout.cpu().numpy().tobytes() == s.sample_retimed(sx, su, sT, with_rows[0], 10).tobytes()
    s.clear_bounds()
    again = s.retime(sx, su, sT, n_grid, spec)
    assert again[0].tobytes() == plain[0].tobytes() and again[1].tobytes() == plain[1].tobytes()
    # payload rows: 1 kg and 6 kg on alternate problems (on every arm); the torque rows follow the lumped model, and the heavier load tips one
    mass = np.where(np.arange(B) % 2 == 0, 1.0, 6.0)
    s.set_payloads(mass if narm == 1 else np.repeat(mass[:, None], narm, axis=1))
    lumped = {m: [M.model_add_payload(bm, M.payload(m, bm.tool[:])) for bm in base] for m in (1.0, 6.0)}
    models = [lumped[m] for m in mass]
    want = reference(M, models, nseg, sx, su, sT, table, n_grid, lin_max, ang_max)
    bare = reference(M, base, nseg, sx, su, sT, table, n_grid, lin_max, ang_max, P=P)
    assert sum(1 for w, r in zip(want, bare) if w["status"] != r["status"] or (not w["status"] and w["rate_min"] < r["rate_min"] - 1e-3)) >= 2
    assert sum(w["near"] for w in want) == 0
    loaded = s.retime(sx, su, sT, n_grid, spec)
    check_against(want, *loaded, what="payloads")
    # ... and the sampled torque is that of the lumped model
    b = next(i for i in range(B) if loaded[1][i]["status"] == 0 and loaded[1][i]["rate_min"] < 0.99)
    got = s.sample_retimed(sx[b:b + 1], su[b:b + 1], sT[b:b + 1], loaded[0][b:b + 1], 12)[0]
    assert np.abs(got - R.sample_retimed_np(models[b], nseg, sx[b], su[b], sT[b], loaded[0][b], 12)).max() <= 1e-9
    s.clear_payloads()
    assert s.retime(sx, su, sT, n_grid, spec)[1].tobytes() == plain[1].tobytes()


# ---- 7. bad arguments and bad inputs --------------------------------------------------------------------------------------------------------
def test_bad_arguments_write_nothing(M):
    nseg, narm, n, n_grid = 4, 1, 4, 50
    sx, su, sT = [np.ascontiguousarray(a[:n]) for a in moves(narm, nseg)]
    s = solver(M, narm, nseg, max_batch=8)
    L, ctx = M.lib(), s._ctx
    prof = np.full((n, n_grid + 1, 2), 7.0); rec = np.zeros(n, dtype=M.RETIME_DTYPE); rec["k_fail"] = 7
    out = np.full((n, 11, 29), 7.0)
    good_spec = M.retime_spec(1.0, 2.0)

    def call(B=n, x=sx, u=su, T=sT, n_grid=n_grid, spec=good_spec, p=prof, r=rec, device=False):
        a = [ctx, B, x if x is None else x.ctypes.data, u if u is None else u.ctypes.data, T if T is None else T.ctypes.data, n_grid,
             spec if spec is None else spec.ctypes.data, p if p is None else p.ctypes.data, r if r is None else r.ctypes.data]
        return L.mpcmp_retime_batch_device(*a, None) if device else L.mpcmp_retime_batch(*a)

    bad = [dict(B=0), dict(B=9), dict(n_grid=0), dict(n_grid=4097), dict(x=None), dict(u=None), dict(T=None), dict(p=None), dict(r=None),
           dict(spec=M.retime_spec(rate_max=0.0)), dict(spec=M.retime_spec(rate_max=-2.0)), dict(spec=M.retime_spec(rate_max=np.inf)),
           dict(spec=M.retime_spec(rate_max=np.nan)), dict(spec=M.retime_spec(groups=1)), dict(spec=M.retime_spec(groups=1 << 4)),
           dict(spec=M.retime_spec(groups=0x16E)), dict(spec=M.retime_spec(-1e-3)), dict(spec=M.retime_spec(1.0, np.nan))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert call(device=True, **kw) == EINVAL, kw          # (nothing is launched: the host addresses are never read)
    assert L.mpcmp_retime_batch(None, n, sx.ctypes.data, su.ctypes.data, sT.ctypes.data, n_grid, None, prof.ctypes.data, rec.ctypes.data) == EINVAL

    def sample(B=n, x=sx, T=sT, n_grid=n_grid, p=prof, n_pts=10, o_=out, device=False):
        a = [ctx, B, x if x is None else x.ctypes.data, su.ctypes.data, T if T is None else T.ctypes.data, n_grid, p if p is None else p.ctypes.data,
             n_pts, o_ if o_ is None else o_.ctypes.data]
        return L.mpcmp_sample_retimed_batch_device(*a, None) if device else L.mpcmp_sample_retimed_batch(*a)

    for kw in (dict(B=0), dict(B=9), dict(n_grid=0), dict(n_grid=4097), dict(n_pts=0), dict(x=None), dict(T=None), dict(p=None), dict(o_=None)):
        assert sample(**kw) == EINVAL, kw
        assert sample(device=True, **kw) == EINVAL, kw
    # more problems than rows in force
    s.set_bounds(rows(M, 3))
    assert call() == EINVAL
    s.clear_bounds()
    s.set_payloads(np.ones(2))
    assert call() == EINVAL and sample() == EINVAL
    s.clear_payloads()
    assert (prof == 7.0).all() and (rec["k_fail"] == 7).all() and (out == 7.0).all()
    assert call() == 0 and (rec["k_fail"] == -1).all() and sample() == 0 and (out[:, 0, 0] == 0.0).all()


def test_bad_inputs(M):
    nseg, narm, n, n_grid = 4, 1, 6, 50
    sx, su, sT = [np.array(a[:n]) for a in moves(narm, nseg)]
    s = solver(M, narm, nseg, max_batch=8)
    table = np.repeat(M.bounds_from_margins(1, 1, 1, 1, -1), n)
    s.set_bounds(table)
    clean = s.retime(sx, su, sT, n_grid)
    assert (clean[1]["status"] == 0).all()
    sx[1, 3, 2] = np.nan; su[2, 7, 6] = np.inf; sT[3] = np.nan
    # a locked joint: lbx == ubx == 0 on a velocity channel that moves
    j = int(np.argmax(np.abs(sx[4][:, 7:]).max(axis=0)))
    table["lbx"][4, 7 + j] = table["ubx"][4, 7 + j] = 0.0
    s.set_bounds(table)
    prof, rec = s.retime(sx, su, sT, n_grid)
    assert list(rec["status"]) == [0, R.NAN, R.NAN, R.NAN, R.INFEASIBLE, 0]
    for b in (1, 2, 3, 4):
        assert np.isposinf(rec[b]["T_new"]) and rec[b]["rate_min"] == 0.0 and np.isnan(prof[b]).all() and rec[b]["n_slowed"] == 0
    assert (rec["k_fail"][[0, 1, 2, 3, 5]] == -1).all()
    want = R.retime_np(R.path_values(robot(M, narm), nseg, sx[4], su[4], sT[4], n_grid), table[4], sT[4], n_grid)
    assert (want["status"], want["k_fail"]) == (R.INFEASIBLE, rec[4]["k_fail"]) and 0 < rec[4]["k_fail"] < n_grid
    for b in (0, 5):
        assert prof[b].tobytes() == clean[0][b].tobytes() and rec[b].tobytes() == clean[1][b].tobytes()
    assert np.isnan(s.sample_retimed(sx, su, sT, prof, 8)[[1, 2, 3, 4]]).all()


# ---- 8. the planner facade and the C++ shim -------------------------------------------------------------------------------------------------
def test_planner_facade(M):
    from mpc_motion_planner_amd import scenarios
    margins = (0.9, 0.9, 0.5, 0.9, 0.1)
    p = M.BatchMotionPlanner(max_batch=8, num_seg=4, sqp_iters=2)
    p.set_constraint_margins(*margins)
    x0, xf = scenarios.make_batch(8, margins)
    p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
    p.solve_trajectory()
    spec = M.retime_spec(1.7, 2.5)
    prof, rec = p.retime(n_grid=100, spec=spec)
    sx, su, sT = p.solution()
    s = M.Solver(M.default_config(4, 2, margins=margins[:4]), 8)
    want = s.retime(sx, su, sT, 100, spec)
    assert prof.tobytes() == want[0].tobytes() and rec.tobytes() == want[1].tobytes()
    assert p.get_retimed_trajectory(30).tobytes() == s.sample_retimed(sx, su, sT, prof, 30).tobytes()


def test_cpp_shim_members(M, tmp_path):
    """examples/shim_selftest.cpp calls the header-only planner's retime and get_retimed_trajectory<N>; what they return is consistent"""
    import json, os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "shim_selftest.cpp"),
                           "-L" + os.path.join(root, "mpc_motion_planner_amd"), "-lmpcmp", "-Wl,-rpath," + os.path.join(root, "mpc_motion_planner_amd"),
                           "-o", exe])
    r = json.loads(subprocess.check_output([exe]).decode())
    assert r["rt_status"] == 0 and 0.0 < r["rt_rate_min"] <= 1.0 and 0 <= r["rt_n_slowed"] <= 201
    assert r["rt_stretch"] >= 1.0 and r["rt_T"] * (1 - 200 * 2.3e-16) <= r["rt_T_new"] <= r["rt_T"] * r["rt_stretch"] * (1 + 1e-9)
    assert r["rt_t_last"] == r["rt_T_new"] and r["rt_end_error"] <= 1e-12
    assert (r["rt_n_slowed"] > 0) == (r["rt_rate_min"] < 1.0)
