"""The readers of a finished plan on robots that are NOT the Panda, the part that needs no GPU: the cases of tests/test_gpu_general_robot_readers.py
are chosen and qualified here, the host statements of the rules (mpcmp_limits_config, mpcmp_retime_one, mpcmp_retime_route_one,
mpcmp_limits_retimed_one, mpcmp_clearance_certified_one, mpcmp_clearance_timed_one, mpcmp_start_delay_one, mpcmp_clearance_certified_timed_one) are
held to the NumPy references on them, and the builders below are what the GPU module checks the kernels with.

Every other test of these readers runs the compiled-in Panda (quarter-turn joint placements, p mostly zero, gravity on z only, the tool on the
flange axis), and the two-arm ones two copies of it.  The robots here come from tests/robots.py through models_from_urdf: general_11, tilted_14
(gravity (1.2, -2.3, -9.0)), dual_21 (two DIFFERENT chains) and general_12 under per-problem payload rows (the robot of
test_gpu_general_robot.PAYLOAD_CASE).

Rigid-body side of the references.  Torque, tool height and tool Jacobian come from oracle_py fed with the model, as in the references' own modules;
tests/test_rbd_reference_host.py pins oracle_py.rnea, fk and frame_jacobian to the energy-based rbd_reference.Reference on each of these chains (both
chains of dual_21 included).  clearance_cert_reference.frames is plain NumPy over R0 and p and is pinned to Reference.frames below.

Shapes: the smallest at which these readers can still go wrong.  One arm num_seg 4, two arms num_seg 6 (the smallest a two-arm context accepts);
B = 8 plans (12 in the moving certificate, whose builder draws 12); n_pts = n_grid = 20; routes of 2 legs; n_start 4, n_rest 3, max_depth 3, and one
case at max_depth 10 on plans the reference splits down to level 10; tracks of 8 keys.

Bounds: those of the modules the check functions come from, unchanged (1e-12 (1 + |x|) for the certificate records and mpcmp_limits_config, 1e-9 on
excesses, 1e-8 relative on profiles, 1e-10 on sampled clearances).  All of them hold on these robots.

Fairness.  Every condition is asserted on the reference alone and nothing is filtered at run time: the seeds, rows and scenes below were chosen
on the CPU so that EVERY plan passes (no decision gap under 1e-9, no value within 1e-8 of its tolerance, no sampled clearance within 1e-9 of the
margin: with zero problems exempt, where the Panda modules allow 2 %).
"""
import functools
import pathlib
import tempfile

import numpy as np
import pytest

import clearance_cert_reference as R
import moving_cert_reference as MC
import moving_reference as mr
import oracle_py as o
import rbd_reference as rr
import retime_reference as RT
import route_retime_reference as RR
import test_clearance_cert_host as H
import test_gpu_general_robot as g
import test_gpu_limits as GL
import test_limits_host as LH
import test_moving_cert_host as MH
import test_moving_world_host as MW
import test_retime_host as TH
import test_retimed_check_host as CH
import test_route_retime_host as RH
from robots import TILTED_GRAVITY, general_models

ROBOTS = {"general_11": (11, 1, None), "general_12": (12, 1, None), "tilted_14": (14, 1, TILTED_GRAVITY), "dual_21": (21, 2, None)}
READERS = ("general_11", "tilted_14", "dual_21")          # the robots of the limits / retime / certificate cases
MOVING = ("general_11", "dual_21")                        # ... of the route and moving-world cases
B, N_PTS, N_GRID, NVIA = 8, 20, 20, 1
TOL = GL.TOL


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


@functools.lru_cache(maxsize=None)
def models(name):
    """name -> ctypes array of the robot's Models, written as a URDF and read back through models_from_urdf once"""
    import mpc_motion_planner_amd as M
    M.build_library()          # (tests that take no M fixture get here first when they run alone)
    seed, n_chains, gravity = ROBOTS[name]
    with tempfile.TemporaryDirectory() as d:
        return general_models(M, pathlib.Path(d), seed, n_chains, gravity=gravity)[0]


def shape(name):
    """(arms, num_seg)"""
    narm = ROBOTS[name][1]
    return narm, 6 if narm == 2 else 4


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 1. the references' forward kinematics
@pytest.mark.parametrize("name", list(ROBOTS))
def test_certificate_reference_frames_vs_rbd_reference(name):
    """clearance_cert_reference.frames against Reference.frames at 50 random postures per chain, to the 1e-11 tests/test_rbd_reference_host.py
    holds the oracle's frames to"""
    rng = np.random.default_rng(ROBOTS[name][0])
    lim = o.default_limits()
    for a, m in enumerate(models(name)):
        q = rng.uniform(lim["qmin"], lim["qmax"], (50, 7))
        Rw, pw = rr.Reference.from_model(m).frames(q)
        arr = R.model_arrays(m)
        worst = 0.0
        for i in range(50):
            Rs, ps = R.frames(arr, q[i])
            worst = max(worst, np.abs(Rs - Rw[i]).max(), np.abs(ps - pw[i]).max())
        print("%s chain %d: max |frames - Reference.frames| = %.1e" % (name, a, worst))
        assert worst < rr.TAU_TOL, (name, a, worst)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 2. limits, retiming, retimed limits: cases
# (torque margin, minimum tool height) of the tight rows and the torque margin of the loose rows, per robot.  The torques of these robots are about
# a fifth of the Panda limits the rows scale, and their bases stand at z = 1: the Panda rows (0.3, 0.3) would leave TAU and HEIGHT without a
# violating problem.  The values lie inside the spread of the moves' peak |tau| / tau_max (0.18 .. 0.28, 0.11 .. 0.21, 0.29 .. 0.56, 0.10 .. 0.22)
# and lowest tool heights.
ROW_PARAMS = {"general_11": (0.2, 0.85, 1.0), "tilted_14": (0.14, 0.6, 0.19), "dual_21": (0.4, 0.7, 1.0), "general_12": (0.15, 0.72, 1.0)}
# (robot, payload rows) -> seed of test_gpu_limits.moves where it is not that module's own: under the loads, the common moves leave general_12
# without an untouched plan (4 slowed, 4 infeasible) and dual_21 with one slowed plan (2 untouched, 5 infeasible)
MOVE_SEED = {("general_12", True): 3, ("dual_21", True): 3}


def reader_rows(M, name, n=B):
    """even problems under the tight row (0.8 of the position range, 0.8 / 0.5 of the velocity and acceleration limits, ROW_PARAMS), odd ones under
    the loose row of the Panda modules"""
    t = np.zeros(n, dtype=M.BOUNDS_DTYPE)
    t[0::2] = M.bounds_from_margins(0.8, 0.8, 0.5, ROW_PARAMS[name][0], min_height=ROW_PARAMS[name][1])
    t[1::2] = M.bounds_from_margins(1, 1, 1, ROW_PARAMS[name][2], min_height=-1)
    return t


def check_rows(M, name, n=B):
    """the rows the RETIMED plans are checked under: the tight rows a little tighter than the rows they were retimed under (0.7 / 0.4 of the velocity
    and acceleration limits, 0.8 of the torque margin), so that a feasible plan of an even problem is over in every group a retiming holds; under
    the rows it was retimed with, a retimed plan leaves QDD and TAU within tol at these shapes and the two groups would have no violating problem.
    The loose rows take the tight rows' minimum tool height: few tight plans stay feasible, and HEIGHT would be left without one over"""
    t = reader_rows(M, name, n)
    t[0::2] = M.bounds_from_margins(0.8, 0.7, 0.4, 0.8 * ROW_PARAMS[name][0], min_height=ROW_PARAMS[name][1])
    t[1::2] = M.bounds_from_margins(1, 1, 1, ROW_PARAMS[name][2], min_height=ROW_PARAMS[name][1])
    return t


PAYLOAD_KINDS = np.resize(np.array(g.PAYLOAD_CASE[4]), B)          # rows of test_gpu_payload.PAYLOADS, per problem (arm 0)


def payload_table(name):
    """(mass [B][narm], com [B][narm][3], inertia [B][narm][3][3]): arm a of problem b carries row (PAYLOAD_KINDS[b] + a) % 4"""
    from test_gpu_payload import PAYLOADS
    narm = ROBOTS[name][1]
    kind = (PAYLOAD_KINDS[:, None] + np.arange(narm)[None, :]) % len(PAYLOADS)
    pick = lambda i: np.array([[PAYLOADS[k][i] for k in row] for row in kind], dtype=np.float64)
    return pick(0), pick(1), pick(2)


def lumped_models(M, name):
    """per problem the list of the arms' Models with that problem's payloads lumped in by the host helper"""
    mass, com, inertia = payload_table(name)
    return [[M.model_add_payload(m, M.payload(mass[b, a], com[b, a], inertia[b, a])) for a, m in enumerate(models(name))] for b in range(B)]


@functools.lru_cache(maxsize=None)
def reader_case(name, payload=False):
    """the limits / retime case of a robot, with the references computed once: dict of narm, nseg, models (one list, or one per problem under
    payload rows), sx, su, sT, table, vals, lin_max, ang_max (the batch medians of the reference's peak tool speeds), lim_ref (record_np per
    problem), P, rt_ref, amp (tests/test_retime_host.py::case)"""
    import mpc_motion_planner_amd as M
    narm, nseg = shape(name)
    sx, su, sT = GL.moves(narm, nseg, B, MOVE_SEED.get((name, payload), GL.SEED))
    ms = lumped_models(M, name) if payload else GL.robot(M, narm, models(name))
    per = lambda b: ms[b] if payload else ms
    table = reader_rows(M, name)
    vals = GL.sampled(ms, nseg, sx, su, sT, N_PTS)
    lin_max, ang_max = GL.tool_maxima(vals)
    lim_ref = GL.records(vals, table, sT, N_PTS, TOL, lin_max, ang_max)
    P = [RT.path_values(per(b), nseg, sx[b], su[b], sT[b], N_GRID) for b in range(B)]
    rt_ref = TH.reference(M, ms, nseg, sx, su, sT, table, N_GRID, lin_max, ang_max, P=P)
    P2 = [RT.path_values(per(b), nseg, sx[b], su[b], sT[b], N_GRID, TH.perturbation(P[b]["q"].shape, b)) for b in range(B)]
    rt_ref2 = TH.reference(M, ms, nseg, sx, su, sT, table, N_GRID, lin_max, ang_max, P=P2)
    return dict(narm=narm, nseg=nseg, models=ms, sx=sx, su=su, sT=sT, table=table, vals=vals, lin_max=lin_max, ang_max=ang_max, lim_ref=lim_ref,
                P=P, rt_ref=rt_ref, amp=RH.amplification(rt_ref, rt_ref2))


def assert_limits_case_is_fair(ref, what=""):
    """no problem within 1e-8 of a tolerance; every group has a violating and a clean problem"""
    assert not any(r["near"] for r in ref), ("reference: a value within 1e-8 of its tolerance", what)
    for k in range(LH.GROUPS):
        n = sum((r["status"] >> k) & 1 for r in ref)
        assert 0 < n < len(ref), ("reference: %d of %d problems violate %s" % (n, len(ref), GL.NAMES[k]), what)


def assert_retime_case_is_fair(ref, amp, what=""):
    """no controllable set within 1e-8 of empty; slowed, untouched and infeasible plans all occur; the 1e-13 perturbation is amplified by <= 100"""
    slowed = sum(1 for r in ref if not r["status"] and r["rate_min"] < 0.99)
    untouched = sum(1 for r in ref if not r["status"] and (r["x"] == 1.0).all())
    infeasible = sum(1 for r in ref if r["status"])
    assert not any(r["near"] for r in ref), ("reference: a set within 1e-8 of empty", what)
    assert slowed >= 2 and untouched >= 1 and infeasible >= 1, ("reference: %d slowed, %d untouched, %d infeasible" % (slowed, untouched, infeasible), what)
    assert amp <= 100.0, ("reference: amplification %.1f" % amp, what)
    return slowed, untouched, infeasible


def assert_retimed_case_is_fair(ref, what=""):
    """no feasible plan within 1e-8 of a tolerance; every group has a violating and a clean plan among the feasible ones"""
    c = CH.counts(ref)
    assert c["near"] == 0 and c["feasible"] >= 3, ("reference: %d near, %d feasible" % (c["near"], c["feasible"]), what)
    assert all(0 < n < c["feasible"] for n in c["over"]), ("reference: %s over, per group, of %d feasible" % (c["over"], c["feasible"]), what)
    return c


def z_only(m, gz=None):
    """a copy of the Model with gravity (0, 0, gz), by default (0, 0, -|g|): what a reader that assumed gravity along z would compute with"""
    import mpc_motion_planner_amd as M
    out = M.Model.from_buffer_copy(m)
    norm = float(np.linalg.norm(m.gravity[:]))
    out.gravity[0], out.gravity[1], out.gravity[2] = 0.0, 0.0, -norm if gz is None else gz
    return out


CASES_23 = [(n, False) for n in READERS] + [("general_12", True), ("dual_21", True)]
IDS_23 = ["%s%s" % (n, "-payloads" if p else "") for n, p in CASES_23]


@pytest.mark.parametrize("name,payload", CASES_23, ids=IDS_23)
def test_limits_config_vs_reference(M, name, payload):
    """mpcmp_limits_config at every sample of every move against groups_np / ratios_np of tests/test_limits_host.py at that file's 1e-12, and the
    fairness of the GPU case (records over the same samples)"""
    c = reader_case(name, payload)
    assert_limits_case_is_fair(c["lim_ref"], name)
    spec = M.limits_spec(TOL, c["lin_max"], c["ang_max"])
    worst = np.zeros(LH.GROUPS)
    for b in range(B):
        v, mb = c["vals"][b], (c["models"][b] if payload else c["models"])
        for i in range(N_PTS + 1):
            ex, ch, r = M.limits_config(mb, c["table"][b], v["q"][i], v["qd"][i], v["qdd"][i], spec)
            one = {k: a[i:i + 1] for k, a in v.items()}
            E = LH.groups_np(one, c["table"][b], c["lin_max"], c["ang_max"])
            for k in range(LH.GROUPS):
                ref = E[k][0].max()
                if np.isneginf(ref):
                    assert np.isneginf(ex[k]) and ch[k] == -1, (name, b, i, k)
                    continue
                worst[k] = max(worst[k], abs(ex[k] - ref))
                assert abs(ex[k] - ref) <= 1e-12 and abs(E[k][0][ch[k]] - ref) <= 1e-12, (name, b, i, k, ex[k], ref)
            assert np.abs(r - LH.ratios_np(one, c["table"][b], c["lin_max"], c["ang_max"])).max() <= 1e-12, (name, b, i)
    print("%s: violating per group %s; max |excess - reference| per group %s" % (
        name, [sum((r["status"] >> k) & 1 for r in c["lim_ref"]) for k in range(LH.GROUPS)], " ".join("%.1e" % w for w in worst)))


@pytest.mark.parametrize("name,payload", CASES_23, ids=IDS_23)
def test_retime_one_vs_reference(M, name, payload):
    c = reader_case(name, payload)
    counts = assert_retime_case_is_fair(c["rt_ref"], c["amp"], name)
    prof, rec = host_profiles(M, c)
    worst = [0.0, 0.0]
    try:
        TH.check_against(c["rt_ref"], prof, rec, worst=worst)
    finally:
        print("%s: slowed / untouched / infeasible %s, amplification %.1f, max |x / ref - 1| %.1e, |T_new / ref - 1| %.1e"
              % (name, counts, c["amp"], worst[0], worst[1]))
    for b in np.flatnonzero(rec["status"] == 0):
        TH.check_limits_hold(dict(P=c["P"][b], T=c["sT"][b]), c["table"][b], prof[b, :, 1], c["lin_max"], c["ang_max"], what=(name, b))


def host_profiles(M, c):
    """mpcmp_retime_one on every plan of a reader case: (prof [B][n_grid + 1][2], RETIME_DTYPE [B])"""
    per = isinstance(c["models"][0], (list, tuple))
    prof, rec = np.zeros((B, N_GRID + 1, 2)), np.zeros(B, dtype=M.RETIME_DTYPE)
    spec = M.retime_spec(c["lin_max"], c["ang_max"])
    for b in range(B):
        prof[b], rec[b] = M.retime_one(c["models"][b] if per else c["models"], c["nseg"], c["table"][b], c["sx"][b], c["su"][b], c["sT"][b], N_GRID, spec)
    return prof, rec


def test_the_tilted_case_sees_a_z_only_gravity_term():
    """on tilted_14 the gravity torque of every plan differs, at some grid point, by more than 100 x TAU_TOL (by a tenth of a newton metre, in
    fact) from the torque under (0, 0, -9.81), the vector the condition is stated with, and from the torque under (0, 0, -|g|), |g| = 9.37, which
    is what a reader that kept the magnitude and assumed the direction would use; and a retiming reference fed the latter model gives other
    profiles: a split that is right for gravity along z only cannot pass the retime tests of this robot"""
    c = reader_case("tilted_14")
    flat, nominal = [z_only(m) for m in c["models"]], [z_only(m, -9.81) for m in c["models"]]
    moved = 0
    for b in range(B):
        Pz = RT.path_values(flat, c["nseg"], c["sx"][b], c["su"][b], c["sT"][b], N_GRID)
        d = np.abs(Pz["c"] - c["P"][b]["c"]).max()
        dn = np.abs(RT.path_values(nominal, c["nseg"], c["sx"][b], c["su"][b], c["sT"][b], N_GRID)["c"] - c["P"][b]["c"]).max()
        assert min(d, dn) > 100.0 * rr.TAU_TOL and min(d, dn) > 0.1, (b, d, dn)
        rz = RT.retime_np(Pz, c["table"][b], c["sT"][b], N_GRID, c["lin_max"], c["ang_max"])
        r = c["rt_ref"][b]
        moved += rz["status"] != r["status"] or (not r["status"] and np.abs(rz["x"] - r["x"]).max() > 1e-6)
    print("tilted_14: a z-only gravity term changes the reference's record of %d of %d plans" % (moved, B))
    assert moved >= 2, moved


@pytest.mark.parametrize("name,payload", CASES_23, ids=IDS_23)
def test_limits_retimed_one_vs_reference(M, name, payload):
    """the profiles are those mpcmp_retime_one wrote; both sides read that array"""
    c = reader_case(name, payload)
    prof, rrec = host_profiles(M, c)
    table = check_rows(M, name)
    ref = CH.plan_references(c["models"], c["nseg"], c["sx"], c["su"], c["sT"], prof, table, N_PTS, c["lin_max"], c["ang_max"])
    cnt = assert_retimed_case_is_fair(ref, name)
    got, T_new = host_limits_retimed(M, c, prof, table)
    assert [r["failed"] for r in ref] == list(rrec["status"] != 0)
    worst = np.zeros(LH.GROUPS)
    try:
        CH.check_retimed(M, got, T_new, ref, N_PTS, what=name, worst=worst)
    finally:
        CH.report(name, cnt, got, ref, worst)


def host_limits_retimed(M, c, prof, table):
    """mpcmp_limits_retimed_one on every plan of a reader case under the rows `table`: (LIMITS_DTYPE [B], T_new [B])"""
    per = isinstance(c["models"][0], (list, tuple))
    rec, T_new = np.zeros(B, dtype=M.LIMITS_DTYPE), np.zeros(B)
    spec = M.limits_spec(TOL, c["lin_max"], c["ang_max"])
    for b in range(B):
        rec[b], T_new[b] = M.limits_retimed_one(c["models"][b] if per else c["models"], c["nseg"], table[b], c["sx"][b], c["su"][b], c["sT"][b],
                                                prof[b], N_PTS, spec)
    return rec, T_new


def test_payload_rows_are_felt():
    """the payload cases differ from the bare robot by newton metres, and the two arms of dual_21 carry different loads"""
    for name in ("general_12", "dual_21"):
        bare, loaded = reader_case(name), reader_case(name, True)
        d = [np.abs(loaded["vals"][b]["tau"] - bare["vals"][b]["tau"]).max() for b in range(B)]
        assert sum(x > 0.1 for x in d) >= B // 2, (name, d)
    mass = payload_table("dual_21")[0]
    assert (mass[:, 0] != mass[:, 1]).all()


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 3. routes of two legs
@functools.lru_cache(maxsize=None)
def route_case(name):
    """the first B routes of tests/test_route_retime_host.py::route_moves (the moves cut into two legs: robot-independent node arrays) on a general
    robot: dict of narm, nseg, models, sx [B][2][N][..], su, sT [B][2], table [B][2] (reader_rows per route), check [B][2] (check_rows per route:
    the rows the retimed routes are checked under), P, lin_max, ang_max, ref, amp"""
    import mpc_motion_planner_amd as M
    narm, nseg = shape(name)
    sx, su, sT = [np.ascontiguousarray(a[:B]) for a in RH.route_moves(narm, nseg, NVIA)]
    ms = GL.robot(M, narm, models(name))
    table = M.Solver.repeat(reader_rows(M, name), NVIA).reshape(B, NVIA + 1)
    P = [RR.route_path_values(ms, nseg, sx[b], su[b], sT[b], N_GRID) for b in range(B)]
    lin_max, ang_max = RH.route_tool_maxima(P)
    ref = RH.route_reference(table, sT, N_GRID, lin_max, ang_max, P)
    P2 = [RR.route_path_values(ms, nseg, sx[b], su[b], sT[b], N_GRID, [TH.perturbation(P[b][m]["q"].shape, b * (NVIA + 1) + m) for m in range(NVIA + 1)])
          for b in range(B)]
    amp = RH.amplification(ref, RH.route_reference(table, sT, N_GRID, lin_max, ang_max, P2))
    check = M.Solver.repeat(check_rows(M, name), NVIA).reshape(B, NVIA + 1)
    return dict(narm=narm, nseg=nseg, models=ms, sx=sx, su=su, sT=sT, table=table, check=check, P=P, lin_max=lin_max, ang_max=ang_max, ref=ref, amp=amp)


def assert_route_case_is_fair(ref, amp, what=""):
    slowed = sum(1 for r in ref if not r["status"] and r["rate_min"] < 0.99)
    untouched = sum(1 for r in ref if not r["status"] and (r["x"] == 1.0).all())
    assert not any(r["near"] for r in ref), ("reference: a set within 1e-8 of empty", what)
    assert slowed >= 2 and untouched >= 1, ("reference: %d slowed, %d untouched" % (slowed, untouched), what)
    assert amp <= 100.0, ("reference: amplification %.1f" % amp, what)


@pytest.mark.parametrize("name", MOVING)
def test_route_readers_vs_reference(M, name):
    """mpcmp_retime_route_one against route_retime_reference, and mpcmp_limits_retimed_one on the routes it retimed against retimed_check_reference"""
    c = route_case(name)
    assert_route_case_is_fair(c["ref"], c["amp"], name)
    prof, leg_T, rec = RH.retime_route_all(M, c["models"], c["nseg"], c["sx"], c["su"], c["sT"], c["table"], N_GRID, M.retime_spec(c["lin_max"], c["ang_max"]))
    assert RH.check_route_against(c["ref"], prof, leg_T, rec, what=name) == 0
    ref = CH.route_references(c["models"], c["nseg"], c["sx"], c["su"], c["sT"], prof, c["check"], N_PTS, c["lin_max"], c["ang_max"])
    cnt = assert_retimed_case_is_fair(ref, name)
    got, T_new = CH.limits_retimed_all(M, c["models"], c["nseg"], c["sx"], c["su"], c["sT"], c["check"], prof, N_PTS, M.limits_spec(TOL, c["lin_max"], c["ang_max"]))
    CH.check_retimed(M, got, T_new, ref, N_PTS, what=name)
    print("%s routes: feasible %d, over tol per group %s" % (name, cnt["feasible"], cnt["over"]))


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 4. the certificate
SCENE = tuple(g.WORLD)          # the scene of tests/test_gpu_general_robot.py: a floor at z = 0.55, a sphere, a capsule and a box around the first base
MARGIN = 0.02
# name -> (self_gap, sphere radius, n_start, max_depth, seed of the plans).  The radii are those of test_gpu_general_robot.CLEARANCE_CASES (see RADIUS
# there: on these short links spheres of the Panda's 0.06 m three joints apart touch in every posture).  The seeds were chosen on the CPU.
CERT_CASES = {"general_11": (3, g.RADIUS, 4, 3, 31), "tilted_14": (3, g.RADIUS, 4, 3, 33), "dual_21": (0, 0.05, 4, 3, 33)}
DEEP = ("dual_21", 32, 10)      # the case at max_depth 10: (robot, seed of the plans, max_depth); three of its plans split down to level 10


@functools.lru_cache(maxsize=None)
def cert_tables(name):
    """per arm the skeleton of mpcmp_link_spheres (radius + 0.01 arm, spacing 0.08 + 0.03 arm: the tables of the arms differ) without the sphere at
    the origin of joints 1 .. 6, which coincides with the last sphere of the link before it (tests/test_clearance_cert_host.py::robot)"""
    import mpc_motion_planner_amd as M
    out = []
    for a, m in enumerate(models(name)):
        t = M.link_spheres(m, CERT_CASES[name][1] + 0.01 * a, 0.08 + 0.03 * a)
        out.append(np.ascontiguousarray(t[(t["joint"] == 0) | (np.abs(t["c"]).max(axis=1) > 0.0)]))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def cert_robot(name):
    """(Models, their arrays for the reference, the sphere tables), computed once"""
    return H.robot(ROBOTS[name][1], list(models(name)), list(cert_tables(name)))


def cert_world(name):
    return H.world(ROBOTS[name][1], SCENE)


def cert_plans(name, seed=None):
    narm, nseg = shape(name)
    return H.plans(narm, nseg, CERT_CASES[name][4] if seed is None else seed, B)


@functools.lru_cache(maxsize=None)
def cert_reference(name, seed=None, max_depth=None):
    _, arrays, tables = cert_robot(name)
    narm, nseg = shape(name)
    self_gap, _, n_start, depth, _ = CERT_CASES[name]
    x, T = cert_plans(name, seed)
    return [R.certified_np(arrays, tables, cert_world(name), nseg, x[b], T[b], MARGIN, self_gap, n_start, depth if max_depth is None else max_depth)
            for b in range(B)]


def assert_cert_case_is_fair(ref, what=""):
    gaps = [r["gap"] for r in ref]
    assert min(gaps) > H.GAP, ("reference: a decision within 1e-9 of the margin", what, gaps)
    st = [r["clr"]["status"] for r in ref]
    assert any(s & 1 for s in st) and any(s == 0 for s in st), ("reference: hits and certificates must both occur", what, st)
    assert any(r["cert"]["depth"] >= 1 for r in ref), ("reference: no plan splits below level 0", what)


@pytest.mark.parametrize("name", READERS)
def test_sphere_tables_have_no_tie(name):
    """the care of tests/test_clearance_cert_host.py::robot, checked instead of argued: over 200 random postures no two spheres of the pair set
    coincide, and none sits at a constant distance under the sum of the radii plus the margin (such a pair would decide every record alike)"""
    _, arrays, tables = cert_robot(name)
    narm = ROBOTS[name][1]
    self_gap = CERT_CASES[name][0]
    lim = o.default_limits()
    q = np.random.default_rng(5).uniform(np.tile(lim["qmin"], narm), np.tile(lim["qmax"], narm), (200, 7 * narm))
    cen, rad, arm, jnt = [], [], [], []
    for a in range(narm):
        fr = [R.frames(arrays[a], q[i, 7 * a:7 * a + 7]) for i in range(200)]
        for s in tables[a]:
            j = int(s["joint"])
            cen.append(np.array([ps[j] + Rs[j] @ s["c"] for Rs, ps in fr])); rad.append(float(s["r"])); arm.append(a); jnt.append(j)
    n_pairs = 0
    for s in range(len(cen)):
        for t in range(s + 1, len(cen)):
            if arm[s] != arm[t] or (self_gap > 0 and abs(jnt[s] - jnt[t]) >= self_gap):
                d = np.linalg.norm(cen[s] - cen[t], axis=1)
                n_pairs += 1
                assert d.min() > 1e-6, (name, s, t)
                assert d.max() - d.min() > 1e-3 or d.min() > rad[s] + rad[t] + MARGIN, (name, s, t, d.min(), d.max())
    assert n_pairs > 0 and (narm == 1 or not np.array_equal(tables[0]["r"][:4], tables[1]["r"][:4]))


@pytest.mark.parametrize("name", READERS)
def test_certified_one_vs_reference(M, name):
    ref = cert_reference(name)
    assert_cert_case_is_fair(ref, name)
    models_, _, tables = cert_robot(name)
    narm, nseg = shape(name)
    self_gap, _, n_start, depth, _ = CERT_CASES[name]
    x, T = cert_plans(name)
    for b in range(B):
        clr, cert = H.one(M, narm, nseg, cert_world(name), x[b], T[b], MARGIN, self_gap, n_start, depth, tables=tables, models=models_)
        H.check_records(clr, cert, ref[b], (name, b))
        assert clr["d_min"] >= cert["d_lower"]
    print("%s: status %s, depth %s, n_eval %s, smallest decision gap %.1e" % (name, [r["clr"]["status"] for r in ref], [r["cert"]["depth"] for r in ref],
                                                                               [r["cert"]["n_eval"] for r in ref], min(r["gap"] for r in ref)))


def test_certified_one_at_depth_ten(M):
    """the plans of DEEP at max_depth 10: the reference splits some of them down to level 10, and the host statement follows it leaf by leaf"""
    name, seed, depth = DEEP
    ref = cert_reference(name, seed, depth)
    assert min(r["gap"] for r in ref) > H.GAP and sum(r["cert"]["depth"] == depth for r in ref) >= 2
    models_, _, tables = cert_robot(name)
    narm, nseg = shape(name)
    self_gap, _, n_start, _, _ = CERT_CASES[name]
    x, T = cert_plans(name, seed)
    for b in range(B):
        clr, cert = H.one(M, narm, nseg, cert_world(name), x[b], T[b], MARGIN, self_gap, n_start, depth, tables=tables, models=models_)
        H.check_records(clr, cert, ref[b], (name, "deep", b))


@pytest.mark.parametrize("name", MOVING)
def test_static_lower_bound_is_sound(M, name):
    """tests/test_clearance_cert_host.py::test_lower_bound_is_sound on these robots, with its 20,001 uniform samples of mpcmp_clearance_config per
    plan: nothing lies below d_lower, and a certified plan has nothing below the margin"""
    models_, _, tables = cert_robot(name)
    narm, nseg = shape(name)
    self_gap = CERT_CASES[name][0]
    x, T = cert_plans(name)
    n_cert = 0
    for b in range(3):
        dmin, _ = H.dense_min(M, narm, nseg, cert_world(name), x[b], self_gap, tables=tables, models=models_)
        for margin in (MARGIN, dmin - 0.01):
            clr, cert = H.one(M, narm, nseg, cert_world(name), x[b], T[b], margin, self_gap, 4, 10, tables=tables, models=models_)
            assert dmin >= cert["d_lower"] - 1e-12 and clr["d_min"] >= cert["d_lower"], (name, b, dmin, clr, cert)
            assert clr["d_min"] >= dmin - 1e-4
            if clr["status"] == 0:
                n_cert += 1
                assert dmin >= margin, (name, b, dmin, margin)
    assert n_cert >= 3


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 5. the moving world
N_KEY = 8
# The margins of these cases: negative, as in tests/test_moving_world_host.py (see MV_MARGIN there: a hit is then a penetration, the margin is any
# finite number and the comparison is the same code).  The skeletons dip into SCENE's floor and box in most of the moves, so at a margin near 0
# every plan would hit; at these, 1 of the 8 plans hits the world at rest, 1 to 5 hit the moving one, and no sampled minimum lies within 1 mm.
MV_MARGINS = {"general_11": -0.045, "dual_21": -0.105}
DELAYS_K = 9


def moving_robot(name):
    """(Models, the whole skeleton of every arm with spheres of 0.03 m (+ 0.01 m per arm): the timed checks compare pairs tie-robustly)"""
    import mpc_motion_planner_amd as M
    ms = list(models(name))
    return ms, [M.link_spheres(m, 0.03 + 0.01 * a, 0.08 + 0.03 * a) for a, m in enumerate(ms)]


def moving_plans(name):
    """the first B moves of tests/test_moving_world_host.py::plans (robot-independent node arrays)"""
    narm, nseg = shape(name)
    return [np.ascontiguousarray(a[:B]) for a in MW.plans(narm, nseg)]


def moving_world(M, name, window, press=False, shift_y=0.0):
    """tests/test_moving_world_host.py::moving_world around robots whose bases stand at z = 1: SCENE at rest, and four obstacles PARKED out of reach
    that their tracks of N_KEY keys carry through the cell: a ball along x above the bases, a pole (capsule) along y, a box coming back along x with
    a sideways wobble, and a ceiling (half-space) that comes down (press: down to a flat bottom and up again, from t = 0).  shift_y: the ball, the pole and the box pass
    that much further along y (one world per problem).  -> (obstacle records [8], (track_of, offsets [4][N_KEY][3], t0, dt))"""
    narm = ROBOTS[name][1]
    cx = 0.0 if narm == 1 else 0.35
    side = 0.25 if narm == 1 else 0.35
    fr = np.arange(N_KEY) / (N_KEY - 1)
    ball = np.stack([cx - 0.9 + 1.8 * fr, np.full_like(fr, side), np.full_like(fr, 1.3)], axis=1)
    pole = np.stack([np.full_like(fr, cx + 0.3), -0.9 + 1.8 * fr, np.full_like(fr, 0.6)], axis=1)
    box = np.stack([cx + 0.9 - 1.2 * fr, -side + 0.1 * np.sin(2 * np.pi * fr), np.full_like(fr, 0.8)], axis=1)
    h0, h1 = (2.2, 1.35) if press else (1.9, 1.45)
    ceil = np.stack([np.zeros_like(fr), np.zeros_like(fr), h0 + (h1 - h0) * (np.minimum(1.0, 2.5 * np.sin(np.pi * fr)) if press else fr)], axis=1)
    rows = [(M.OBS_SPHERE, tuple(MW.PARK), (0, 0, 0), 0.10), (M.OBS_CAPSULE, tuple(MW.PARK), tuple(MW.PARK + [0, 0, 0.8]), 0.05),
            (M.OBS_BOX, tuple(MW.PARK), (0.10, 0.20, 0.10), 0.0), (M.OBS_HALFSPACE, (0.0, 0.0, -1.0), (-MW.PARK[2], 0, 0), 0.0)]
    obs = np.concatenate([H.world(narm, SCENE), MW.scene(M, rows)])
    offsets = np.stack([ball - MW.PARK, pole - MW.PARK, box - MW.PARK, ceil - MW.PARK])
    offsets[:3, :, 1] += shift_y
    track_of = np.array([-1, -1, -1, -1, 0, 1, 2, 3], dtype=np.int32)
    return obs, (track_of, np.ascontiguousarray(offsets), 0.0 if press else 0.25 * window, window / (N_KEY - 1))


def assert_moving_case_is_fair(ref, tracks, what=""):
    """both outcomes occur, no per-sample minimum within 1e-9 of the margin, the tracks change an outcome, and obstacles of both kinds are there"""
    n_hit = sum(r["status"] for r in ref)
    assert not any(r["near"] for r in ref), ("reference: a sample within 1e-9 of the margin", what)
    assert 0 < n_hit < len(ref), ("reference: %d of %d problems hit" % (n_hit, len(ref)), what)
    assert sum(r["status"] != r["status_rest"] for r in ref) >= 1, ("reference: the tracks change no status", what)
    assert (tracks[0] >= 0).any() and (tracks[0] < 0).any()


@functools.lru_cache(maxsize=None)
def moving_profiles(name):
    """the plans retimed by mpcmp_retime_one under rows at 45 % of the velocity limits (tests/test_moving_world_host.py::host_profiles)"""
    import mpc_motion_planner_amd as M
    narm, nseg = shape(name)
    sx, su, sT = moving_plans(name)
    return MW.host_profiles(M, moving_robot(name)[0], nseg, sx, su, sT, N_GRID)


def moving_worlds(M, name, window, per_problem, press=False):
    """per plan (obstacle records, tracks): one world for all, or the tracked obstacles of plan b passing up to 0.1 m further along y"""
    shift = np.linspace(-0.1, 0.1, B) if per_problem else np.zeros(B)
    return [moving_world(M, name, window, press, shift[b]) for b in range(B)]


@pytest.mark.parametrize("per_problem", [False, True], ids=["one-world", "world-per-problem"])
@pytest.mark.parametrize("name", MOVING)
def test_timed_one_and_start_delay_one_vs_reference(M, name, per_problem):
    narm, nseg = shape(name)
    ms, tables = moving_robot(name)
    sx, su, sT = moving_plans(name)
    w, ts, margin = MW.window_of(sT), MW.start_times(sT), MV_MARGINS[name]
    worlds = moving_worlds(M, name, w, per_problem)
    for prof, t_start in ((None, None), (moving_profiles(name), ts)):
        ref = [MW.timed_references(ms, tables, mr.World(*worlds[b]), nseg, sx[b:b + 1], su[b:b + 1], sT[b:b + 1], None if prof is None else prof[b:b + 1],
                                   None if t_start is None else t_start[b:b + 1], N_PTS, margin)[0] for b in range(B)]
        assert_moving_case_is_fair(ref, worlds[0][1], (name, per_problem, prof is not None))
        got = [M.clearance_timed_one(ms, nseg, tables, worlds[b][0], worlds[b][1], sx[b], sT[b], None if prof is None else prof[b],
                                     0.0 if t_start is None else t_start[b], N_PTS, margin) for b in range(B)]
        MW.check_timed_records(got, ref, sT if prof is None else prof[:, -1, 0], N_PTS, (name, per_problem, prof is not None))
        print("%s, retimed %s: %d of %d hit, %d changed by the tracks" % (name, prof is not None, sum(r["status"] for r in ref), B,
                                                                         sum(r["status"] != r["status_rest"] for r in ref)))
    presses = moving_worlds(M, name, w, per_problem, press=True)
    delays = MW.delay_grid(DELAYS_K, w)
    for cw in (False, True):
        ref = [MW.delay_references(ms, tables, mr.World(*presses[b]), nseg, sx[b:b + 1], su[b:b + 1], sT[b:b + 1], None, N_PTS, delays, cw, margin)[0]
               for b in range(B)]
        assert_delay_case_is_fair(ref, (name, per_problem, cw))
        got = [M.start_delay_one(ms, nseg, tables, presses[b][0], presses[b][1], sx[b], sT[b], delays, None, cw, N_PTS, margin) for b in range(B)]
        MW.check_delay_records([x[0] for x in got], np.array([x[1] for x in got]), ref, delays, (name, per_problem, cw))
        print("%s, check_wait %s: index %s" % (name, cw, [r["index"] for r in ref]))


def assert_delay_case_is_fair(ref, what=""):
    """no sample within 1e-9 of the margin; a plan that may start at once, and one that has to wait or finds no clear delay"""
    assert not any(r["near"] for r in ref), ("reference: a sample within 1e-9 of the margin", what)
    idx = [r["index"] for r in ref]
    assert any(i == 0 for i in idx) and any(i != 0 for i in idx), ("reference: delays", what, idx)


# ---------------------------------------------------------------------------------------------------------------------------------------------
# 6. the certificate in the moving world
# tests/test_moving_cert_host.py::case_data on these robots: SCENE at rest, the tracked paths lifted by 0.75 m to the height of the arms; one world for
# every plan (general_11) and one per problem (dual_21); wait and hold positive; 8 keys; n_start 4, n_rest 3, max_depth 3.  self_gap and the tables are
# those of CERT_CASES.  The seeds were chosen on the CPU (seed 202 of dual_21 fails the resting-plan condition of assert_mcert_case_is_fair).
MCERT_CASES = {"general_11": MH.Case("general_11", 1, 4, 3, 4, 3, 3, 8, 4, False, True, True, 1, (-1.5, 4.5), MARGIN, 201),
               "dual_21": MH.Case("dual_21", 2, 6, 0, 4, 3, 3, 8, 4, True, True, True, -1, (0.3, 0.9), MARGIN, 206)}
LIFT = (0.0, 0.0, 0.75)


def mcert_data(name):
    return MH.case_data(MCERT_CASES[name], SCENE, LIFT)


@functools.lru_cache(maxsize=None)
def mcert_reference(name):
    case, d = MCERT_CASES[name], mcert_data(name)
    _, arrays, tables = cert_robot(name)
    return [MC.certified_timed_np(arrays, tables, d["obs"][b], d["tracks"][b], case.nseg, d["x"][b], d["T"][b], d["ts"][b], d["w"][b], d["h"][b],
                                  case.margin, case.self_gap, case.n_start, case.n_rest, case.max_depth) for b in range(MH.NP)]


def mcert_one(M, name, b, margin=None, n_start=None, n_rest=None, max_depth=None):
    case, d = MCERT_CASES[name], mcert_data(name)
    ms, _, tables = cert_robot(name)
    return MH.one(M, case.narm, case.nseg, d["obs"][b], d["tracks"][b], d["x"][b], d["T"][b], d["ts"][b], d["w"][b], d["h"][b],
                  case.margin if margin is None else margin, case.self_gap, case.n_start if n_start is None else n_start,
                  case.n_rest if n_rest is None else n_rest, case.max_depth if max_depth is None else max_depth, tables=tables, models=ms)


def assert_mcert_case_is_fair(name, ref):
    MH.assert_fair(MCERT_CASES[name], ref)
    assert any(r["cert"]["depth"] >= 1 for r in ref), ("reference: no plan splits below level 0", name)
    d = mcert_data(name)
    assert all((t[0] >= 0).any() and (t[0] < 0).any() for t in d["tracks"])
    # a plan that rests (amplitude 0) keeps one distance to everything that stands still for all of its intervals: its t_min is then decided by the
    # last bit of the interpolation weights.  Its closest obstacle must be one that rides a track (seed 202 of dual_21 fails this)
    for b in np.flatnonzero(d["amp"] == 0.0):
        other = ref[b]["clr"]["other"]
        assert other >= 0 and d["tracks"][b][0][other] >= 0, ("reference: the resting plan is closest to something at rest", name, b, other)


@pytest.mark.parametrize("name", MOVING)
def test_certified_timed_one_vs_reference(M, name):
    ref = mcert_reference(name)
    assert_mcert_case_is_fair(name, ref)
    for b in range(MH.NP):
        clr, cert = mcert_one(M, name, b)
        H.check_records(clr, cert, ref[b], (name, b))
        assert clr["d_min"] >= cert["d_lower"]


@pytest.mark.parametrize("name", MOVING)
def test_moving_lower_bound_is_sound(M, name):
    """tests/test_moving_cert_host.py::test_lower_bound_is_sound on these robots, with its sample counts (20,001 of the motion, 5,001 of each rest),
    at max_depth 10: nothing lies below d_lower, and nothing below the margin where the record says clear"""
    case, d = MCERT_CASES[name], mcert_data(name)
    ms, _, tables = cert_robot(name)
    ref = mcert_reference(name)
    picks = [b for b in range(MH.NP) if ref[b]["clr"]["status"] == 0][:2] + [b for b in range(MH.NP) if ref[b]["clr"]["status"] != 0][:1]
    n_cert = 0
    for b in picks:
        clr, cert = mcert_one(M, name, b, max_depth=10)
        dmin = MH.dense_minimum(M, case.narm, case.nseg, d["obs"][b], d["tracks"][b], d["x"][b], d["T"][b], d["ts"][b], d["w"][b], d["h"][b],
                                case.self_gap, tables=tables, n_motion=20000, n_rest=5000, models=ms)
        assert dmin >= cert["d_lower"] - 1e-12 and clr["d_min"] >= cert["d_lower"], (name, b, dmin, clr, cert)
        if clr["status"] == 0:
            n_cert += 1
            assert dmin >= case.margin, (name, b, dmin)
    assert n_cert >= 2
