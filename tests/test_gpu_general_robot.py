"""The GPU rigid-body path on robots that are NOT the Panda.  Run with -m gpu.

Every other GPU test runs the compiled-in Panda, whose constants are full of structural zeros (joint placements that are quarter turns about x, p
mostly zero, small off-diagonal inertia, gravity on z only, the tool on the flange axis), and every two-arm test runs two copies of it.  Here the
models come from URDFs with everything rotated, oblique joint axes, a fixed intermediate link and full inertia tensors (robots.general_models), one of
them under a gravity vector with all three components, and the two-arm robot has two DIFFERENT chains.

Leaf kernels (rnea, eval_constraints, the torque columns of sample / mpc_point / jerk_point, the tool-velocity flags of traj_stats, clearance) are
checked against the energy-based reference of tests/rbd_reference.py, not against the oracle: the oracle is a Newton-Euler recursion like the kernels.
Every QP path runs end to end against the oracle on the same model (the oracle itself is pinned to the reference off the Panda by
tests/test_rbd_reference_host.py).

Choice of robots and problems for the solves (made on the CPU with the oracle alone, nothing is filtered at run time).  A (robot seed, num_seg,
SQP depth, batch, problem stream) qualifies if every problem of the batch returns finite outputs, has no hard-failure bit (1 | 2 | 4) in its status
and keeps its qp_iters_total when every constant of the model (R0, p, mass, com, I, tool, link8, gravity) is perturbed by 1e-12 relative with
random signs, three perturbations each: no termination test sits on a knife edge where rounding differences would turn into iteration differences.
tests/test_general_robot_cases_host.py re-runs this qualification on the case tables below (SOLVE_CASES, DUAL_CASES, PAYLOAD_CASE) without a GPU.
All of these qualified at the first stream tried (offset 100 for one arm, 50 for two, the offsets of the Panda parity tests):
    one arm, robot 11:            num_seg 4 / 3 SQP / B 3;  num_seg 6 / 2 / B 2 (both N = 19 loop kernels);  num_seg 8 / 2 / B 2;
                                  num_seg 2 / 3 / B 2 (k_qp2 at N = 7, and the generic k_qp under MPCMP_FORCE_V1)
    one arm, robot 14 (tilted):   num_seg 4 / 2 / B 2
    two arms, robot 21 (2 chains): num_seg 6 / 2 / B 2 (also the swap test);  num_seg 8 / 2 / B 2
    payload rows on robot 12:     num_seg 4 / 2 / B 3

The other choices made on the CPU, asserted by the same CPU module on the helpers the GPU tests call:
    clearance: one scene (WORLD) for all robots, link spheres of 0.01 m for one arm and 0.05 / 0.06 m for two; 12 moves each, of which 10 (robot
        11), 11 (robot 12), 8 (robot 14) and 10 (robot 21) hit, none within 1e-9 of the margin.
    tool-velocity flags: the aimed speed ratios are 0.995 / 1.005; the ratio that a problem does not aim lies between 0.25 and 0.49 (linear) or
        between 1.5 and 3.9 (angular), nowhere within 1e-3 of 1.
    pose targets: 4 starts per target within +-0.3 rad of the generating configuration.  With the host DLS loop (the kernel's step) 63 of 64 starts
        of arm 0 and 64 of 64 of arm 1 converge, in 81 .. 828 iterations (median 225 and 145) of the 1000 allowed; every target keeps at least 3.
        The scenario streams of the targets were chosen for that: on stream 300 one target of arm 0 converges from none of its 4 starts and on
        stream 350 one target of arm 1 from 1 of 4 (slow convergence into the iteration cap, as on the Panda, where about 9 % of targets fail), so
        arm 0 takes stream 500 and arm 1 stream 300.
"""
import numpy as np
import pytest

import oracle_py as o
import rbd_reference as rr
from robots import general_models, tilted_gravity_models
from test_clearance_host import scene, sd_np
from test_gpu_clearance import check_records, moves, sampled_q

pytestmark = pytest.mark.gpu

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
SINGLE = ("general_11", "general_12", "tilted_14")           # two general single-arm robots and the tilted-gravity robot
DUAL_SEED = 21
_CACHE = {}


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def robot(M, tmp_path_factory, name):
    """name -> ctypes Model array (general_<seed>, tilted_<seed>: one chain; dual_<seed>: two different chains), read from its URDF once"""
    if name not in _CACHE:
        kind, seed = name.split("_")
        d = tmp_path_factory.mktemp(name)
        if kind == "tilted":
            _CACHE[name] = tilted_gravity_models(M, d, int(seed))[0]
        else:
            _CACHE[name] = general_models(M, d, int(seed), 2 if kind == "dual" else 1)[0]
    return _CACHE[name]


def omodels(arr):
    out = (o.Model * len(arr))()
    for a in range(len(arr)):
        out[a] = o.Model.from_buffer_copy(arr[a])
    return out


def _cfgs(M, nseg, sqp, **kw):
    return M.default_config(nseg, sqp, margins=MARGINS, **kw), o.default_config(nseg, sqp, margins=MARGINS, **kw)


def leaf_samples(n, seed):
    rng = np.random.default_rng(seed)
    lim = o.default_limits()
    q = rng.uniform(lim["qmin"], lim["qmax"], (n, 7))
    return q, rng.uniform(-1, 1, (n, 7)) * lim["vmax"], rng.uniform(-1, 1, (n, 7)) * lim["amax"]


def leaf_reference(M, tmp_path_factory, name, n):
    """the reference's answers on the leaf samples of (robot, n), computed once and shared by the tests that need them"""
    key = ("leaf", name, n)
    if key not in _CACHE:
        r = rr.Reference.from_model(robot(M, tmp_path_factory, name)[0])
        q, v, a = leaf_samples(n, 100 + n)
        x = np.concatenate([q, v], axis=1)
        g, G, est = r.constraints(x, a, quirk=1)
        _CACHE[key] = dict(q=q, v=v, a=a, x=x, g=g, G=G, est=est)
    return _CACHE[key]


# ---- 1. leaf kernels against the reference ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SINGLE)
def test_rnea_vs_reference(M, tmp_path_factory, name):
    s = M.Solver(_cfgs(M, 4, 1)[0], 8, model=robot(M, tmp_path_factory, name)[0])
    for n in (1, 13, 67):
        ref = leaf_reference(M, tmp_path_factory, name, n)
        tau = s.rnea(ref["q"], ref["v"], ref["a"])
        d = np.abs(tau - ref["g"][:, :7]).max()
        print("%s rnea n = %d: max |tau - reference| = %.2e (|tau| <= %.1f)" % (name, n, d, np.abs(tau).max()))
        assert d < rr.TAU_TOL, (name, n, d)


@pytest.mark.parametrize("quirk", [1, 0])
@pytest.mark.parametrize("name", SINGLE)
def test_eval_constraints_vs_reference(M, tmp_path_factory, name, quirk):
    s = M.Solver(M.default_config(4, 1, margins=MARGINS, quirk_dtau_dT=quirk), 8, model=robot(M, tmp_path_factory, name)[0])
    for n in (1, 13, 67):
        ref = leaf_reference(M, tmp_path_factory, name, n)
        g, G = s.eval_constraints(ref["x"], ref["a"])
        G_ref = ref["G"].copy()
        assert np.abs(G_ref[:, :7, 21]).max() > 1e-3          # (the flag changes the Jacobian)
        if not quirk:
            G_ref[:, :, 21] = 0.0
        print("%s eval_constraints quirk %d n = %d: max |g - ref| = %.2e, max |G - ref| = %.2e (|G| <= %.1f, Richardson estimate <= %.1e)"
              % (name, quirk, n, np.abs(g - ref["g"]).max(), np.abs(G - G_ref).max(), np.abs(G_ref).max(), ref["est"].max()))
        for i in range(n):
            rr.assert_constraints_close(g[i], G[i], ref["g"][i], G_ref[i], ref["est"][i], (name, quirk, n, i))


def test_inertia_is_read_row_by_row_vs_oracle(M, tmp_path_factory):
    """A rigid body's inertia tensor is symmetric, so no physical model and no energy can tell I[1] from I[3]: swapped off-diagonal indices in the
    kernels' I * omega are invisible to everything above.  The struct of include/mpcmp.h holds nine numbers per body, row-major; this pins that
    convention with a tensor made asymmetric on purpose (upper off-diagonal entries x 1.5), against the oracle, which multiplies the nine numbers
    the same way.  The energy-based reference cannot serve here: it sees only the symmetric part"""
    model = M.Model.from_buffer_copy(robot(M, tmp_path_factory, "general_12")[0])
    for i in range(7):
        for k in (1, 2, 5):
            model.I[i][k] *= 1.5
    om = o.Model.from_buffer_copy(model)
    s = M.Solver(_cfgs(M, 4, 1)[0], 8, model=model)
    q, v, a = leaf_samples(13, 31)
    x = np.concatenate([q, v], axis=1)
    tau = s.rnea(q, v, a)
    g, G = s.eval_constraints(x, a)
    sym = np.stack([o.rnea(q[i], v[i], a[i], model=o.Model.from_buffer_copy(robot(M, tmp_path_factory, "general_12")[0])) for i in range(13)])
    assert np.abs(tau - sym).max() > 1e-3                  # (the asymmetry is felt)
    for i in range(13):
        assert np.abs(tau[i] - o.rnea(q[i], v[i], a[i], model=om)).max() < rr.TAU_TOL, i
        g0, G0 = o.eval_constraints(x[i], a[i], quirk=1, model=om)
        assert np.abs(g[i] - g0).max() < rr.TAU_TOL and np.abs(G[i] - G0).max() < rr.jac_tol(G0), i


def lagrange_sample(nseg, xs, us, t):
    """q, qd, qdd [7] each of the node polynomials (cubic Lagrange on the local nodes -1, -1/2, 1/2, 1 of every segment) at normalised time t"""
    xi = np.array([-1.0, -0.5, 0.5, 1.0])
    s = min(max(int(np.floor(t * nseg)), 0), nseg - 1)
    x = 2.0 * (t * nseg - s) - 1.0
    L = np.array([np.prod([(x - xi[k]) / (xi[j] - xi[k]) for k in range(4) if k != j]) for j in range(4)])
    return L @ xs[3 * s:3 * s + 4, :7], L @ xs[3 * s:3 * s + 4, 7:], L @ us[3 * s:3 * s + 4]


def single_arm_moves(nseg, B, seed):
    """jerk-limited moves between random states (oracle_py.warm_start_jerk): node states, node accelerations, durations, and the end states"""
    from mpc_motion_planner_amd import scenarios
    lim = o.default_limits()
    x0, xf = scenarios.make_batch(B, MARGINS, stream_offset=seed)
    N = 3 * nseg + 1
    xs, us, T = np.zeros((B, N, 14)), np.zeros((B, N, 7)), np.zeros(B)
    for b in range(B):
        xs[b], us[b], T[b] = o.warm_start_jerk(nseg, MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"], x0[b], xf[b])
    return x0, xf, xs, us, T


TOOL_AIMS = (0.995, 0.995, 1.005, 1.005, 0.995, 1.005)          # reference's largest tool speed / threshold, per problem


def tool_velocity_case(r, nseg, B, n_pts):
    """CPU side of the sampled-torque test: B jerk-limited moves whose node velocities are scaled so that the reference's largest linear (even
    problems) or angular (odd problems) tool speed over the sample grid lies 0.5 % below or above its threshold.  J(q) qd is linear in qd and q
    is not scaled, so the aimed ratio is exact; the other ratio of each problem falls where it falls and is asserted clear of its threshold"""
    x0, xf, xs, us, T = single_arm_moves(nseg, B, 640)

    def grid(xs):
        pts = np.array([[np.concatenate(lagrange_sample(nseg, xs[b], us[b], ip / n_pts)) for ip in range(n_pts + 1)] for b in range(B)])
        q, v, a = pts[..., :7], pts[..., 7:14], pts[..., 14:]
        twist = np.einsum("...ij,...j->...i", r.fk(q)["J"], v)
        return q, v, a, np.linalg.norm(twist[..., :3], axis=-1).max(axis=1), np.linalg.norm(twist[..., 3:], axis=-1).max(axis=1)
    _, _, _, lin, ang = grid(xs)
    k = np.where(np.arange(B) % 2 == 0, np.array(TOOL_AIMS) * 1.7 / lin, np.array(TOOL_AIMS) * 2.5 / ang)
    xs = xs.copy(); xs[:, :, 7:] *= k[:, None, None]
    q, v, a, lin, ang = grid(xs)
    assert np.abs(lin / 1.7 - 1.0).min() > 1e-3 and np.abs(ang / 2.5 - 1.0).min() > 1e-3         # (no flag rests on a rounding)
    want_lin, want_ang = (lin <= 1.7).astype(float), (ang <= 2.5).astype(float)
    assert 0 < want_lin.sum() < B and 0 < want_ang.sum() < B
    return dict(x0=x0, xf=xf, xs=xs, us=us, T=T, q=q, v=v, a=a, lin=lin, ang=ang, want_lin=want_lin, want_ang=want_ang)


@pytest.mark.parametrize("name", SINGLE)
def test_sampled_torques_and_tool_velocity_flags_vs_reference(M, tmp_path_factory, name):
    """sample, mpc_point, jerk_point: q, qd, qdd are the node polynomials (restated here), the torque columns the reference's tau there.
    traj_stats: torque extrema over the same grid.  It reports the tool velocities only as flags (linear <= 1.7 m/s, angular <= 2.5 rad/s), so
    the extrema themselves cannot be compared; the flags are what J(q) qd of the reference says on trajectories scaled to 0.5 % either side of
    the threshold (tool_velocity_case): a task velocity wrong by more than that flips one"""
    nseg, B, n_pts = 4, 6, 20
    model = robot(M, tmp_path_factory, name)[0]
    r = rr.Reference.from_model(model)
    s = M.Solver(_cfgs(M, nseg, 1)[0], B, model=model)
    c = tool_velocity_case(r, nseg, B, n_pts)
    x0, xf, xs, us, T, q, v, a, lin, ang = (c[k] for k in ("x0", "xf", "xs", "us", "T", "q", "v", "a", "lin", "ang"))
    tau = r.tau(q, v, a)
    out = s.sample(xs, us, T, n_pts)
    assert np.abs(out[..., 0] - np.arange(n_pts + 1) / n_pts * T[:, None]).max() < 1e-12
    assert np.abs(out[..., 1:8] - q).max() < 1e-12 and np.abs(out[..., 8:15] - v).max() < 1e-12 and np.abs(out[..., 15:22] - a).max() < 1e-11
    print("%s sample: max |tau - reference| = %.2e (|tau| <= %.1f)" % (name, np.abs(out[..., 22:] - tau).max(), np.abs(tau).max()))
    assert np.abs(out[..., 22:] - tau).max() < rr.TAU_TOL
    # one point per problem, at a grid time
    ip = np.array([3, 7, 11, 13, 17, 19])
    pt = s.mpc_point(xs, us, T, ip / n_pts * T)
    b = np.arange(B)
    assert np.abs(pt[:, :7] - q[b, ip]).max() < 1e-11 and np.abs(pt[:, 7:14] - v[b, ip]).max() < 1e-11 and np.abs(pt[:, 14:21] - a[b, ip]).max() < 1e-10
    assert np.abs(pt[:, 21:] - r.tau(pt[:, :7], pt[:, 7:14], pt[:, 14:21])).max() < rr.TAU_TOL
    jmax = MARGINS[4] * M.default_limits()["jmax"]
    jp, jT = s.jerk_point(x0, xf, jmax, 0.37 * T)
    assert np.abs(jp[:, 21:] - r.tau(jp[:, :7], jp[:, 7:14], jp[:, 14:21])).max() < rr.TAU_TOL and np.abs(jp[:, 14:21]).max() > 0.1
    # traj_stats on the same grid
    st = s.traj_stats(xs, us, T, xf, n_pts)
    assert np.abs(st[:, 21:28] - tau.min(axis=1)).max() < rr.TAU_TOL and np.abs(st[:, 49:56] - tau.max(axis=1)).max() < rr.TAU_TOL
    print("%s traj_stats: reference max linear %s, angular %s" % (name, np.round(lin, 4), np.round(ang, 4)))
    assert np.array_equal(st[:, 71], c["want_lin"]) and np.array_equal(st[:, 72], c["want_ang"])
    assert np.array_equal(st[:, 73], (r.fk(q)["tool"][..., 2].min(axis=1) >= 0.0).astype(float))


def clearances_ref(refs, tables, obstacles, q, self_gap):
    """test_clearance_host.clearances_np with the sphere centres from the reference's forward kinematics"""
    cen, rad, arm, jnt = [], [], [], []
    for a, (r, t) in enumerate(zip(refs, tables)):
        Rw, pw = r.frames(q[..., 7 * a:7 * a + 7])
        for k in range(t.shape[0]):
            j = int(t["joint"][k])
            cen.append(pw[..., j, :] + np.einsum("...ij,j->...i", Rw[..., j, :, :], t["c"][k]))
            rad.append(float(t["r"][k])); arm.append(a); jnt.append(j)
    cen, rad = np.stack(cen, axis=-2), np.array(rad)
    S, ns = cen.shape[0], cen.shape[1]
    dob = np.full((S, ns, obstacles.shape[0]), np.inf)
    for k in range(obstacles.shape[0]):
        dob[:, :, k] = sd_np(obstacles[k], cen) - rad[None, :]
    drb = np.full((S, ns, ns), np.inf)
    for s in range(ns):
        for t in range(s + 1, ns):
            if arm[s] != arm[t] or (self_gap > 0 and abs(jnt[s] - jnt[t]) >= self_gap):
                drb[:, s, t] = np.linalg.norm(cen[:, s] - cen[:, t], axis=-1) - rad[s] - rad[t]
    return dob, drb


def clearance_reference(M, models, nseg, B, n_pts, margin, self_gap, world, radius):
    """CPU side of a clearance case: per-arm sphere tables that differ, the scene, the moves and the reference records; asserted on the
    reference: both outcomes occur and no per-sample minimum lies on the margin"""
    narm = len(models)
    tables = [M.link_spheres(models[a], radius + 0.01 * a, 0.08 + 0.03 * a) for a in range(narm)]
    obs = scene(M, world)
    sx, sT = moves(narm, nseg, B)
    q = sampled_q(narm, nseg, sx, sT, n_pts)
    refs = [rr.Reference.from_model(models[a]) for a in range(narm)]
    ref = []
    for b in range(B):
        dob, drb = clearances_ref(refs, tables, obs, q[b], self_gap)
        smin = np.minimum(dob.reshape(n_pts + 1, -1).min(axis=1), drb.reshape(n_pts + 1, -1).min(axis=1, initial=np.inf))
        hit = smin < margin
        first = int(np.argmax(hit)) if hit.any() else -1
        ref.append(dict(dob=dob, drb=drb, smin=smin, d_min=smin.min(), n_hit=int(hit.sum()), t_first=(first / n_pts) * sT[b] if first >= 0 else -1.0,
                        status=int(hit.any()), near=bool((np.abs(smin - margin) <= 1e-9).any())))
    n_hit = sum(x["status"] for x in ref)
    print("clearance, %d arm(s): %d of %d hit, d_min %.3f .. %.3f" % (narm, n_hit, B, min(x["d_min"] for x in ref), max(x["d_min"] for x in ref)))
    assert not any(x["near"] for x in ref) and 0 < n_hit < B
    return tables, obs, sx, sT, ref


def clearance_case(M, models, nseg, B, n_pts, margin, self_gap, world, radius):
    narm = len(models)
    tables, obs, sx, sT, ref = clearance_reference(M, models, nseg, B, n_pts, margin, self_gap, world, radius)
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B, model=models[0]) if narm == 1 else M.Solver(M.default_config(nseg, 1, margins=MARGINS), B, models=models)
    for a in range(narm):
        s.set_robot_spheres(tables[a], arm=a)
    s.set_obstacles(obs)
    check_records(s.clearance(sx, sT, n_pts, margin, self_gap), ref, sT, n_pts)


# the links of these robots are short (lengths x 0.5): on robot 12, spheres of 0.025 m three joints apart come within the margin on every one of the
# moves, so that all hit; with 0.01 m every robot has moves that hit an obstacle, moves that hit through a pair inside the arm, and clear ones
RADIUS = 0.01
# the bases stand at z = 1: a floor at z = 0.55 that a stretched arm reaches, a sphere, a capsule and a box around the first base
WORLD = [(3, (0.0, 0.0, 1.0), (0.55, 0, 0), 0.0), (0, (0.35, 0.2, 1.25), (0, 0, 0), 0.08), (1, (-0.3, -0.3, 0.7), (-0.3, 0.3, 1.4), 0.04),
         (2, (0.3, -0.4, 0.8), (0.08, 0.08, 0.1), 0.01)]
# name -> arguments of clearance_case after the models (both qualified on the CPU: tests/test_general_robot_cases_host.py)
CLEARANCE_CASES = {name: (4, 12, 20, 0.02, 3, WORLD, RADIUS) for name in SINGLE}
CLEARANCE_CASES["dual_%d" % DUAL_SEED] = (6, 12, 20, 0.02, 0, WORLD, 0.05)


@pytest.mark.parametrize("name", SINGLE)
def test_clearance_vs_reference_kinematics(M, tmp_path_factory, name):
    clearance_case(M, robot(M, tmp_path_factory, name), *CLEARANCE_CASES[name])


def test_two_different_arms_clearance_with_per_arm_tables(M, tmp_path_factory):
    name = "dual_%d" % DUAL_SEED
    clearance_case(M, robot(M, tmp_path_factory, name), *CLEARANCE_CASES[name])


# ---- 2. every QP path end to end against the oracle on the same model ---------------------------------------------------------------------------
def solve_states(B, off):
    from mpc_motion_planner_amd import scenarios
    return scenarios.make_batch(B, MARGINS, stream_offset=off)


def dual_states(B, off):
    a0, af = solve_states(B, off)
    b0, bf = solve_states(B, off + 7919)
    return (np.stack([o.merge_arm_states([a0[b], b0[b]]) for b in range(B)]), np.stack([o.merge_arm_states([af[b], bf[b]]) for b in range(B)]))


def single_problems(ocfg, B):
    """x0, xf and the oracle's start guess of the one-arm solve cases"""
    x0, xf = solve_states(B, SOLVE_OFFSET)
    N = 3 * ocfg.num_seg + 1
    wx = np.zeros((B, N, 14)); wu = np.zeros((B, N, 7)); wT = np.zeros(B)
    for b in range(B):
        wx[b], wu[b], wT[b] = o.warm_start(ocfg, x0[b], xf[b])
    return x0, xf, wx, wu, wT


def assert_solve_parity(sx, su, sT, info, xs, us, T, oi, tag):
    """the bars of test_gpu_parity.py::test_solve_vs_oracle"""
    assert (oi.status & 7) == 0 and info["status"] == oi.status, (tag, info["status"], oi.status)
    assert abs(sT - T) <= 1e-6 * abs(T), (tag, sT, T)
    assert np.abs(sx - xs).max() <= 1e-6, (tag, np.abs(sx - xs).max())
    assert np.abs(su - us).max() <= 1e-5, (tag, np.abs(su - us).max())
    assert info["qp_iters_total"] == oi.qp_iters_total and info["qp_capped"] == oi.qp_capped and info["last_alpha"] == oi.last_alpha, tag
    assert abs(info["viol_l1"] - oi.viol_l1) < 1e-6 and abs(info["defect_inf"] - oi.defect_inf) < 1e-6, (tag, info["viol_l1"], oi.viol_l1)
    assert abs(info["term_err_inf"] - oi.term_err_inf) < 1e-6, (tag, info["term_err_inf"], oi.term_err_inf)          # (the final linearisation counts)


# (robot, num_seg, SQP iterations, B, environment at mpcmp_create, loop kernel reported by mpcmp_kernel_timing).  num_seg 2 runs the N = 7
# instantiation of k_qp2 by default and the generic k_qp under MPCMP_FORCE_V1: both are run, on the same qualified problems
SOLVE_CASES = [("general_11", 4, 3, 3, "", "k_qp2"), ("tilted_14", 4, 2, 2, "", "k_qp2"), ("general_11", 6, 2, 2, "", "k_qp5"),
               ("general_11", 6, 2, 2, "qp19=3", "k_qp3"), ("general_11", 8, 2, 2, "", "k_qp3"), ("general_11", 2, 3, 2, "", "k_qp2"),
               ("general_11", 2, 3, 2, "force_v1=1", "k_qp")]
SOLVE_OFFSET, DUAL_OFFSET = 100, 50
DUAL_CASES = [(6, 2, 2), (8, 2, 2)]          # (num_seg, SQP iterations, B) of the two-arm robot; the swap test runs the first
PAYLOAD_CASE = ("general_12", 4, 2, 3, (2, 0, 3, 1, 2))          # (robot, num_seg, SQP iterations, B, rows of test_gpu_payload.PAYLOADS)


@pytest.mark.parametrize("name,nseg,sqp,B,kern,loop", SOLVE_CASES)
def test_one_qp_and_solve_vs_oracle(M, tmp_path_factory, monkeypatch, name, nseg, sqp, B, kern, loop):
    if kern:
        monkeypatch.setenv("MPCMP_" + kern.split("=")[0].upper(), kern.split("=")[1])
    cfg, ocfg = _cfgs(M, nseg, sqp)
    model = robot(M, tmp_path_factory, name)[0]; om = o.Model.from_buffer_copy(model)
    x0, xf, wx, wu, wT = single_problems(ocfg, B)
    s = M.Solver(cfg, B, model=model)
    assert s.kernel_timing()[0] == loop
    p, y, it = s.qp(x0, xf, wx, wu, wT)                    # one QP (bars of test_gpu_parity.py::_qp_case)
    for b in range(B):
        p0, y0, it0 = o.debug_qp(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b], model=om)
        assert it[b] == it0, (b, it[b], it0)
        assert np.abs(p[b] - p0).max() < 1e-7 * (1 + np.abs(p0).max()) and np.abs(y[b] - y0).max() < 1e-6 * (1 + np.abs(y0).max()), b
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
    for b in range(B):
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b], model=om)
        assert_solve_parity(sx[b], su[b], sT[b], info[b], xs, us, T, oi, (name, nseg, b))
    # the general model is what was solved: the Panda gives another answer
    xs, _, T, _ = o.solve(ocfg, x0[0], xf[0], wx[0], wu[0], wT[0])
    assert abs(T - sT[0]) > 1e-4 * T or np.abs(xs - sx[0]).max() > 1e-4


def dual_warm(nseg, x0, xf):
    lim = o.default_limits()
    B, N = x0.shape[0], 3 * nseg + 1
    wx = np.zeros((B, N, 28)); wu = np.zeros((B, N, 14)); wT = np.zeros(B)
    for b in range(B):
        wx[b], wu[b], wT[b] = o.warm_start_jerk_multi(nseg, MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"], x0[b], xf[b])
    return wx, wu, wT


@pytest.mark.parametrize("nseg,sqp,B", DUAL_CASES)
def test_two_different_arms_solve_vs_oracle(M, tmp_path_factory, nseg, sqp, B):
    """the jerk warm start of the two-arm robot and the solve, against the oracle fed the same two models"""
    cfg, ocfg = _cfgs(M, nseg, sqp)
    models = robot(M, tmp_path_factory, "dual_%d" % DUAL_SEED); om = omodels(models)
    x0, xf = dual_states(B, DUAL_OFFSET)
    wx, wu, wT = dual_warm(nseg, x0, xf)
    s = M.Solver(cfg, B, models=models)
    assert s.kernel_timing()[0] == "k_qp3"
    gx, gu, gT = s.warm_start_jerk(x0, xf, MARGINS[4] * M.default_limits()["jmax"])
    assert np.abs(gT - wT).max() <= 1e-9 * wT.max() and np.abs(gx - wx).max() <= 1e-8 and np.abs(gu - wu).max() <= 1e-6
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))            # (mpcmp_qp_batch is a single-arm entry point: the QPs run inside the solve)
    for b in range(B):
        xs, us, T, oi = o.solve_multi(om, ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert_solve_parity(sx[b], su[b], sT[b], info[b], xs, us, T, oi, (nseg, b))


def test_two_different_arms_swapped(M, tmp_path_factory):
    """the two-iteration solve of the two-arm robot (DUAL_CASES[0]) against the oracle, and again with the model order and the per-arm halves of
    x0, xf and the guess swapped: the second result is the first with the arm halves swapped.  Two iterations, because the step kernel reads the
    per-arm model in its line-search trials and in the linearisation for the NEXT iteration: after one iteration a mix-up there leaves the
    iterate untouched.  A kernel that mixes up arm indices fails this whatever the oracle says"""
    nseg, sqp, B = DUAL_CASES[0]
    cfg, ocfg = _cfgs(M, nseg, sqp)
    models = robot(M, tmp_path_factory, "dual_%d" % DUAL_SEED)
    swapped = (M.Model * 2)(); swapped[0] = models[1]; swapped[1] = models[0]
    x0, xf = dual_states(B, DUAL_OFFSET)
    wx, wu, wT = dual_warm(nseg, x0, xf)
    px = np.r_[7:14, 0:7, 21:28, 14:21]; pu = np.r_[7:14, 0:7]
    s = M.Solver(cfg, B, models=models)
    assert s.kernel_timing()[0] == "k_qp3"
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
    tx, tu, tT, tinfo = M.Solver(cfg, B, models=swapped).solve(x0[:, px], xf[:, px], (wx[:, :, px], wu[:, :, pu], wT))
    assert np.abs(tT - sT).max() <= 1e-6 * np.abs(sT).max() and np.abs(tx[:, :, px] - sx).max() <= 1e-6 and np.abs(tu[:, :, pu] - su).max() <= 1e-5
    assert np.array_equal(tinfo["qp_iters_total"], info["qp_iters_total"]) and np.array_equal(tinfo["status"], info["status"])
    assert np.array_equal(tinfo["last_alpha"], info["last_alpha"])
    for k in ("viol_l1", "defect_inf", "term_err_inf"):
        assert np.abs(tinfo[k] - info[k]).max() < 1e-6, k
    assert np.abs(sx[:, :, px] - sx).max() > 1e-2          # (the halves differ: the swap is visible)
    for b in range(B):
        xs, us, T, oi = o.solve_multi(omodels(models), ocfg, x0[b], xf[b], wx[b], wu[b], wT[b])
        assert_solve_parity(sx[b], su[b], sT[b], info[b], xs, us, T, oi, b)
    # the two arms are two robots: with arm 0's model in both places the oracle gives another answer
    same = (o.Model * 2)(); same[0] = same[1] = o.Model.from_buffer_copy(models[0])
    xs, _, T, _ = o.solve_multi(same, ocfg, x0[0], xf[0], wx[0], wu[0], wT[0])
    assert abs(T - sT[0]) > 1e-5 * T or np.abs(xs - sx[0]).max() > 1e-4


def log6_norm(R, p):
    """||log6|| of the rigid motion (R, p): [V^-1 p; omega]"""
    c = np.clip(0.5 * (np.trace(R) - 1.0), -1.0, 1.0)
    th = np.arccos(c)
    w = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])       # sin(th) axis
    w = w * (th / np.sin(th)) if th > 1e-7 else w
    W = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    k = 1.0 / 12.0 if th < 1e-3 else (1.0 - th * np.sin(th) / (2.0 * (1.0 - np.cos(th)))) / th ** 2
    v = (np.eye(3) - 0.5 * W + k * W @ W) @ p
    return float(np.sqrt(v @ v + w @ w))


IK_B, IK_STARTS, IK_SPREAD = 16, 4, 0.3
IK_OFFSETS = (500, 300)          # scenario streams of the generating configurations, per arm (chosen on the CPU: module docstring)


def pose_target_case(models, arm):
    """CPU side of the pose-target test for one arm: the reference of that arm's chain, forward kinematics of IK_B random in-bounds
    configurations as targets, and IK_STARTS starts per target within +-IK_SPREAD rad of the generating configuration (the spread of
    tests/test_gpu_pose_targets.py)"""
    from mpc_motion_planner_amd import scenarios
    r = rr.Reference.from_model(models[arm])
    qt = scenarios.sample_states(IK_B, MARGINS, stream_offset=IK_OFFSETS[arm])[:, :7]
    f = r.fk(qt)
    seeds = qt[:, None, :] + np.random.default_rng(3 + arm).uniform(-IK_SPREAD, IK_SPREAD, (IK_B, IK_STARTS, 7))
    return r, f, seeds


def test_two_different_arms_pose_targets(M, tmp_path_factory):
    """pose_targets for arm 0 and arm 1 of the two-arm robot: forward kinematics of the returned q through the reference of THAT arm's chain hits the
    target pose within the tolerance of the inverse kinematics (1e-4 on ||log6|| of the pose error in the target frame: tests/test_gpu_pose_targets.py)"""
    cfg = M.default_config(6, 1, margins=MARGINS)
    models = robot(M, tmp_path_factory, "dual_%d" % DUAL_SEED)
    s = M.Solver(cfg, IK_B, models=models)
    xf = np.zeros((IK_B, 28))
    targets = []
    for arm in range(2):
        r, f, seeds = pose_target_case(models, arm)
        _, info = s.pose_targets(f["R"][:, 6], f["tool"], seeds, arm=arm, xf=xf)
        print("arm %d: DLS iterations of the chosen start %d .. %d" % (arm, info["iters"].min(), info["iters"].max()))
        assert np.all(info["status"] & M.IK_NOT_CONVERGED == 0) and np.all(info["err"] < 1e-4), (arm, info)
        targets.append((r, f))
    for arm, (r, f) in enumerate(targets):
        g = r.fk(xf[:, 7 * arm:7 * arm + 7])
        errs = [log6_norm(f["R"][b, 6].T @ g["R"][b, 6], f["R"][b, 6].T @ (g["tool"][b] - f["tool"][b])) for b in range(IK_B)]
        print("arm %d: largest pose error through the reference %.2e" % (arm, max(errs)))
        assert max(errs) < 1e-4, (arm, errs)
        other = targets[1 - arm][0].fk(xf[:, 7 * arm:7 * arm + 7])          # (through the OTHER arm's chain the pose is somewhere else)
        assert np.abs(other["tool"] - f["tool"]).max() > 1e-2
    assert np.all(xf[:, 14:] == 0.0)


# ---- 3. payload rows on a general model ---------------------------------------------------------------------------------------------------------
def test_payload_rows_on_a_general_model(M, tmp_path_factory):
    """set_payloads with a mixed table on a general robot: the leaf calls against the reference and the solve against the oracle, both fed
    model_add_payload of that model"""
    from test_gpu_payload import PAYLOADS
    name, nseg, sqp, B, kinds = PAYLOAD_CASE
    model = robot(M, tmp_path_factory, name)[0]
    cfg, ocfg = _cfgs(M, nseg, sqp)
    kinds = np.array(kinds)
    lumped = [M.model_add_payload(model, M.payload(*PAYLOADS[k])) for k in kinds]
    s = M.Solver(cfg, 8, model=model)
    s.set_payloads(np.array([PAYLOADS[k][0] for k in kinds]), np.array([PAYLOADS[k][1] for k in kinds]), np.array([PAYLOADS[k][2] for k in kinds]))
    q, v, a = leaf_samples(5, 77)
    x = np.concatenate([q, v], axis=1)
    tau = s.rnea(q, v, a)
    g, G = s.eval_constraints(x, a)
    for i in range(5):
        g0, G0, est = rr.Reference.from_model(lumped[i]).constraints(x[i], a[i], quirk=1)
        assert np.abs(tau[i] - g0[:7]).max() < rr.TAU_TOL, i
        rr.assert_constraints_close(g[i], G[i], g0, G0, est, ("payload", i))
    assert np.abs(tau[0] - rr.Reference.from_model(model).tau(q[0], v[0], a[0])).max() > 0.1          # (the load is felt)
    x0, xf, wx, wu, wT = single_problems(ocfg, B)
    assert s.kernel_timing()[0] == "k_qp2"
    sx, su, sT, info = s.solve(x0, xf, (wx, wu, wT))
    for b in range(B):
        xs, us, T, oi = o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b], model=o.Model.from_buffer_copy(lumped[b]))
        assert_solve_parity(sx[b], su[b], sT[b], info[b], xs, us, T, oi, ("payload", b))
