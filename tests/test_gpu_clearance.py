"""Clearance checks on the GPU (mpcmp_clearance_batch*, mpcmp_select_clear_batch*, the setters) against the NumPy restatement of
tests/test_clearance_host.py: forward kinematics from the Model fields (pinned to the oracle there), sample positions from oracle_py.sample, the
four distance formulas written out.

Bounds.  d_min: 1e-10, the project's GPU-to-oracle bound for kinematic quantities (the kernel contracts FMAs, the reference does not).  The pair and
the sample a record names are checked tie-robustly: in the reference that pair at that sample lies within the same 1e-10 of the reference minimum
(the kernel orders values that may each differ from the reference's by that much).  n_hit, t_first and status are exact for every problem whose
reference per-sample minima all keep 1e-9 away from the margin; every case asserts ON THE REFERENCE that at most 2 % of its problems fall under that
exemption and that at least a quarter of them hit and a quarter are clear.
"""
import ctypes as C

import numpy as np
import pytest

import oracle_py as o
from test_clearance_host import clearances_np, named_pair_value, scene

pytestmark = pytest.mark.gpu

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
SEED = 20261016
MARGIN = 0.02
EINVAL = -1


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def world(M, narm):
    """the scene of the parity cases: one of each primitive.  Two arms share the floor and the capsule; the sphere and the box stand beside the line
    between the bases so that about half of the two-arm moves stay clear"""
    if narm == 1:
        return scene(M, [(M.OBS_SPHERE, (0.55, 0.0, 0.75), (0, 0, 0), 0.10), (M.OBS_BOX, (0.6, -0.5, 0.15), (0.1, 0.1, 0.15), 0.0),
                         (M.OBS_CAPSULE, (-0.5, 0.5, 0.2), (-0.5, 0.5, 1.0), 0.04), (M.OBS_HALFSPACE, (0.0, 0.0, 1.0), (-0.05, 0, 0), 0.0)])
    return scene(M, WORLD2)


WORLD2 = [(0, (0.5, 0.75, 0.9), (0, 0, 0), 0.05), (2, (0.5, -0.8, 0.15), (0.1, 0.1, 0.15), 0.0),
          (1, (-0.6, 0.6, 0.2), (-0.6, 0.6, 1.0), 0.04), (3, (0.0, 0.0, 1.0), (-0.05, 0, 0), 0.0)]


def moves(narm, nseg, B, seed=SEED):
    """B rest-to-rest jerk-limited moves (oracle_py.warm_start_jerk[_multi]) between random configurations inside 90 % of the joint ranges:
    all starts drawn first, then all targets.  Returns sx [B][N][14 narm], sT [B]"""
    lim = o.default_limits()
    vmax, amax, jmax = MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"]
    rng = np.random.default_rng(seed)
    span = np.tile(lim["qmax"] - lim["qmin"], narm)
    q0 = np.tile(lim["qmin"], narm) + (0.05 + 0.9 * rng.random((B, 7 * narm))) * span
    q1 = np.tile(lim["qmin"], narm) + (0.05 + 0.9 * rng.random((B, 7 * narm))) * span
    N = 3 * nseg + 1
    sx, sT = np.zeros((B, N, 14 * narm)), np.zeros(B)
    for b in range(B):
        x0, xf = np.concatenate([q0[b], np.zeros(7 * narm)]), np.concatenate([q1[b], np.zeros(7 * narm)])
        if narm == 1:
            sx[b], _, sT[b] = o.warm_start_jerk(nseg, vmax, amax, jmax, x0, xf)
        else:
            sx[b], _, sT[b] = o.warm_start_jerk_multi(nseg, vmax, amax, jmax, x0, xf)
    return sx, sT


def sampled_q(narm, nseg, sx, sT, n_pts):
    """joint positions [B][n_pts + 1][7 narm] at the uniform samples, arm by arm from oracle_py.sample"""
    B, N = sx.shape[0], sx.shape[1]
    q = np.zeros((B, n_pts + 1, 7 * narm))
    for b in range(B):
        for a in range(narm):
            xa = np.concatenate([sx[b][:, 7 * a:7 * a + 7], sx[b][:, 7 * narm + 7 * a:7 * narm + 7 * a + 7]], axis=1)
            q[b, :, 7 * a:7 * a + 7] = o.sample(nseg, xa, np.zeros((N, 7)), sT[b], n_pts)[:, 1:8]
    return q


def reference(models, tables, obs, q, sT, n_pts, margin, self_gap):
    """per problem: (dob [S, nsph, n_obs], drb [S, nsph, nsph], per-sample minimum [S]) and the record fields that follow from them"""
    out = []
    for b in range(q.shape[0]):
        dob, drb = clearances_np(models, tables, obs, q[b], self_gap)
        S = q.shape[1]
        smin = np.minimum(dob.reshape(S, -1).min(axis=1, initial=np.inf), drb.reshape(S, -1).min(axis=1, initial=np.inf))
        hit = smin < margin
        first = int(np.argmax(hit)) if hit.any() else -1
        out.append(dict(dob=dob, drb=drb, smin=smin, d_min=smin.min(), n_hit=int(hit.sum()), t_first=(first / n_pts) * sT[b] if first >= 0 else -1.0,
                        status=int(hit.any()), near=bool((np.abs(smin - margin) <= 1e-9).any())))
    return out


def assert_reference_is_a_fair_test(ref):
    B = len(ref)
    n_near, n_hit = sum(r["near"] for r in ref), sum(r["status"] for r in ref)
    assert n_near <= 0.02 * B, "reference: %d of %d problems within 1e-9 of the margin" % (n_near, B)
    assert n_hit >= B / 4 and B - n_hit >= B / 4, "reference: %d of %d problems hit" % (n_hit, B)


def check_records(got, ref, sT, n_pts, what=""):
    for b, (g, r) in enumerate(zip(got, ref)):
        tag = (what, b)
        assert abs(g["d_min"] - r["d_min"]) <= 1e-10, (tag, g["d_min"], r["d_min"])
        ip = int(round(g["t_min"] / sT[b] * n_pts))
        assert 0 <= ip <= n_pts and g["t_min"] == (ip / n_pts) * sT[b], (tag, g["t_min"])
        assert 0 <= g["sphere"] < r["dob"].shape[1], tag
        assert abs(named_pair_value(r["dob"], r["drb"], ip, int(g["sphere"]), int(g["other"])) - r["d_min"]) <= 1e-10, (tag, ip, g["sphere"], g["other"])
        if not r["near"]:
            assert g["n_hit"] == r["n_hit"] and g["t_first"] == r["t_first"] and g["status"] == r["status"], (tag, g, r["n_hit"], r["t_first"])


def setup(M, narm, nseg, B, spheres=True, obstacles=True):
    models = M.arm_models(M.DUAL_BASES) if narm == 2 else None
    s = M.Solver(M.default_config(nseg, 1, margins=MARGINS), B, models=models)
    mlist = list(models) if narm == 2 else [M.default_model()]
    tables = [M.link_spheres(m, 0.06, 0.08) for m in mlist]
    obs = world(M, narm)
    if spheres:
        for a in range(narm):
            s.set_robot_spheres(tables[a], arm=a)
    if obstacles:
        s.set_obstacles(obs)
    return s, mlist, tables, obs


# ---- 3. parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", [1, 50, 200, 1000])
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 1), (8, 1), (6, 2), (8, 2)])
def test_parity_with_the_numpy_reference(M, nseg, narm, n_pts):
    B = 64
    s, models, tables, obs = setup(M, narm, nseg, B)
    sx, sT = moves(narm, nseg, B)
    q = sampled_q(narm, nseg, sx, sT, n_pts)
    ref = reference(models, tables, obs, q, sT, n_pts, MARGIN, 0)
    assert_reference_is_a_fair_test(ref)
    got = s.clearance(sx, sT, n_pts, MARGIN, 0)
    print("nseg %d, arms %d, n_pts %d: %d of %d hit, d_min %.3f .. %.3f, max |d_min - ref| = %.2e" % (
        nseg, narm, n_pts, sum(r["status"] for r in ref), B, min(r["d_min"] for r in ref), max(r["d_min"] for r in ref),
        max(abs(g["d_min"] - r["d_min"]) for g, r in zip(got, ref))))
    check_records(got, ref, sT, n_pts)


@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 1), (8, 1), (6, 2), (8, 2)])
def test_parity_with_pairs_inside_one_arm(M, nseg, narm):
    """self_gap = 3.  With the 0.06 m spheres of the other cases the skeleton's fixed pairs (joint origins 0.088 m apart, three joints on) overlap in every
    configuration and every problem hits; spheres of radius 0.03 m leave those pairs 0.028 m clear, above the margin, so that hitting depends on the
    move.  The three conditions on the reference hold for this case as for the others, and the within-arm pairs decide d_min for at least a quarter
    of the problems (asserted on the reference: its d_min with self_gap = 3 lies below its d_min with self_gap = 0)."""
    B, n_pts, radius = 64, 50, 0.03
    s, models, _, obs = setup(M, narm, nseg, B)
    tables = [M.link_spheres(m, radius, 0.08) for m in models]
    for a in range(narm):
        s.set_robot_spheres(tables[a], arm=a)
    sx, sT = moves(narm, nseg, B)
    q = sampled_q(narm, nseg, sx, sT, n_pts)
    ref = reference(models, tables, obs, q, sT, n_pts, MARGIN, 3)
    ref0 = reference(models, tables, obs, q, sT, n_pts, MARGIN, 0)
    assert_reference_is_a_fair_test(ref)
    decided = sum(r["d_min"] < r0["d_min"] - 1e-9 for r, r0 in zip(ref, ref0))
    assert decided >= B / 4, decided
    got = s.clearance(sx, sT, n_pts, MARGIN, 3)
    print("nseg %d, arms %d, self_gap 3: %d of %d hit, within-arm pairs decide %d, max |d_min - ref| = %.2e" % (
        nseg, narm, sum(r["status"] for r in ref), B, decided, max(abs(g["d_min"] - r["d_min"]) for g, r in zip(got, ref))))
    check_records(got, ref, sT, n_pts, "self_gap 3")
    assert sum(int(g["other"]) < 0 and int(g["sphere"]) // tables[0].shape[0] == (-1 - int(g["other"])) // tables[0].shape[0] for g in got) >= B / 4


def test_parity_on_solved_trajectories(M):
    from mpc_motion_planner_amd import scenarios
    B, nseg, n_pts = 64, 4, 200
    s, models, tables, obs = setup(M, 1, nseg, B)
    s.set_config(M.default_config(nseg, 3, margins=MARGINS))
    x0, xf = scenarios.make_batch(B, MARGINS)
    sx, su, sT, info = s.solve(x0, xf)
    ok = (info["status"] & 1) == 0
    assert ok.sum() >= B // 2
    sx, sT = np.ascontiguousarray(sx[ok]), np.ascontiguousarray(sT[ok])
    ref = reference(models, tables, obs, sampled_q(1, nseg, sx, sT, n_pts), sT, n_pts, MARGIN, 0)
    assert sum(r["near"] for r in ref) <= 0.02 * len(ref)
    check_records(s.clearance(sx, sT, n_pts, MARGIN, 0), ref, sT, n_pts, "solved")


# ---- 4. batch independence ------------------------------------------------------------------------------------------------------------------
def test_a_record_does_not_depend_on_the_batch(M):
    nseg, n_pts = 4, 200
    s, _, _, _ = setup(M, 1, nseg, 1024)
    sx, sT = moves(1, nseg, 64)
    order = np.random.default_rng(5).permutation(1024)          # problem order[i] % 64 at position i
    big = s.clearance(sx[order % 64], sT[order % 64], n_pts, MARGIN, 3)
    base = s.clearance(sx, sT, n_pts, MARGIN, 3)
    for i in range(1024):
        assert big[i].tobytes() == base[order[i] % 64].tobytes(), i
    for b in (0, 17, 63):
        assert s.clearance(sx[b:b + 1], sT[b:b + 1], n_pts, MARGIN, 3)[0].tobytes() == base[b].tobytes()


# ---- 5. per-problem obstacle sets -----------------------------------------------------------------------------------------------------------
def test_per_problem_obstacle_sets(M):
    nseg, n_pts, B = 4, 50, 48
    s, models, tables, obs = setup(M, 1, nseg, B)
    sx, sT = moves(1, nseg, B)
    shared = s.clearance(sx, sT, n_pts, MARGIN, 0)
    s.set_obstacles(np.tile(obs, (B, 1)))
    assert s.clearance(sx, sT, n_pts, MARGIN, 0).tobytes() == shared.tobytes()
    # set i = the shared world moved by (0.01 i, 0, 0): problem i against its own world, then the sets permuted with the problems
    sets = np.tile(obs, (B, 1))
    for i in range(B):
        sets[i]["a"][:3, 0] += 0.01 * i                        # (the half-space's normal stays)
    s.set_obstacles(sets)
    own = s.clearance(sx, sT, n_pts, MARGIN, 0)
    q = sampled_q(1, nseg, sx, sT, n_pts)
    for i in (0, 5, B - 1):
        check_records(own[i:i + 1], reference(models, tables, sets[i], q[i:i + 1], sT[i:i + 1], n_pts, MARGIN, 0), sT[i:i + 1], n_pts, "own set %d" % i)
    perm = np.random.default_rng(3).permutation(B)
    s.set_obstacles(sets[perm])
    assert s.clearance(sx[perm], sT[perm], n_pts, MARGIN, 0).tobytes() == own[perm].tobytes()
    # more problems than sets: MPCMP_EINVAL, nothing written
    s.set_obstacles(sets[:B - 1])
    out = np.zeros(B, dtype=M.CLEARANCE_DTYPE); out["n_hit"] = -9
    rc = M.lib().mpcmp_clearance_batch(s._ctx, B, sx.ctypes.data, sT.ctypes.data, n_pts, MARGIN, 0, out.ctypes.data)
    assert rc == EINVAL and np.all(out["n_hit"] == -9)
    assert s.clearance(sx[:B - 1], sT[:B - 1], n_pts, MARGIN, 0).tobytes() == own[:B - 1].tobytes()
    s.clear_obstacles()
    none = s.clearance(sx, sT, n_pts, MARGIN, 0)
    assert np.all(none["d_min"] == np.inf) and np.all(none["sphere"] == -1) and np.all(none["status"] == 0) and np.all(none["t_min"] == -1.0)


# ---- 6. two arms driven through each other ---------------------------------------------------------------------------------------------------
def test_dual_arm_reports_the_partner_sphere(M):
    nseg, n_pts, B = 6, 100, 8
    s, models, tables, obs = setup(M, 2, nseg, B)
    lim = o.default_limits()
    vmax, amax, jmax = MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"]
    # targets: of 4,000 random two-arm configurations the B whose arms overlap most (a search on the reference alone)
    rng = np.random.default_rng(11)
    span = np.tile(lim["qmax"] - lim["qmin"], 2)
    cand = np.tile(lim["qmin"], 2) + (0.05 + 0.9 * rng.random((4000, 14))) * span
    _, drb = clearances_np(models, tables, None, cand, 0)
    pair_min = drb.reshape(4000, -1).min(axis=1)
    pick = np.argsort(pair_min)[:B]
    assert pair_min[pick].max() < -0.02
    rest = np.tile(0.5 * (lim["qmin"] + lim["qmax"]), 2)
    sx, sT = np.zeros((B, 3 * nseg + 1, 28)), np.zeros(B)
    for b in range(B):
        sx[b], _, sT[b] = o.warm_start_jerk_multi(nseg, vmax, amax, jmax, np.concatenate([rest, np.zeros(14)]), np.concatenate([cand[pick[b]], np.zeros(14)]))
    q = sampled_q(2, nseg, sx, sT, n_pts)
    s.clear_obstacles()
    ref = reference(models, tables, None, q, sT, n_pts, MARGIN, 0)
    got = s.clearance(sx, sT, n_pts, MARGIN, 0)
    check_records(got, ref, sT, n_pts, "arms only")
    n0 = tables[0].shape[0]
    assert np.all(got["other"] < 0) and np.all(got["sphere"] < n0) and np.all(-1 - got["other"] >= n0) and np.all(got["status"] == M.CLR_HIT)
    # arm 1 without spheres: obstacle pairs only
    s.set_obstacles(obs)
    s.set_robot_spheres(None, arm=1)
    got = s.clearance(sx, sT, n_pts, MARGIN, 0)
    check_records(got, reference(models, [tables[0], tables[1][:0]], obs, q, sT, n_pts, MARGIN, 0), sT, n_pts, "arm 1 cleared")
    assert np.all(got["other"] >= 0)


# ---- 7. device variants ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("narm,nseg", [(1, 4), (2, 8)])
def test_device_variants_equal_the_host_pointer_variants(M, narm, nseg):
    import torch
    B, n_pts = 64, 200
    s, models, tables, obs = setup(M, narm, nseg, B)
    sx, sT = moves(narm, nseg, B)
    host = s.clearance(sx, sT, n_pts, MARGIN, 3)
    dx, dT = torch.from_numpy(sx).cuda(), torch.from_numpy(sT).cuda()
    dout = torch.zeros(B * M.CLEARANCE_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    s.clearance_device(B, dx.data_ptr(), dT.data_ptr(), n_pts, MARGIN, 3, dout.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == host.tobytes()
    # obstacles from device memory: another world (the floor raised by 0.15 m), so that the call is seen to take effect
    host0 = s.clearance(sx, sT, n_pts, MARGIN, 0)
    obs2 = obs.copy(); obs2["b"][3, 0] = 0.1
    s.set_obstacles(obs2)
    host2 = s.clearance(sx, sT, n_pts, MARGIN, 0)
    assert np.all(host2["d_min"] <= host0["d_min"]) and (host2["d_min"] < host0["d_min"] - 0.1).sum() >= B // 8
    s.set_obstacles(obs)
    dobs = torch.from_numpy(obs2.view(np.uint8).copy()).cuda()
    s.set_obstacles_device(1, obs2.shape[0], dobs.data_ptr(), stream=stream)
    s.clearance_device(B, dx.data_ptr(), dT.data_ptr(), n_pts, MARGIN, 0, dout.data_ptr(), stream=stream)
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == host2.tobytes()


# ---- 8. the choice -------------------------------------------------------------------------------------------------------------------------
def select_np(sT, status, clr_status, group, n_groups):
    bad = 1 | 2 | 4 | 16 | 32
    chosen = np.full(n_groups, -1, dtype=np.int32)
    for g in range(n_groups):
        best = None
        for i in range(len(sT)):
            if group[i] == g and (status[i] & bad) == 0 and clr_status[i] == 0 and (best is None or sT[i] < sT[best]):
                best = i
        chosen[g] = -1 if best is None else best
    return chosen


def test_select_clear(M):
    import torch
    B, G = 40, 7
    s = M.Solver(M.default_config(4, 1, margins=MARGINS), 64)
    rng = np.random.default_rng(2)
    sT = np.round(rng.uniform(0.5, 3.0, B), 1)                                        # (one decimal: ties in T)
    group = rng.integers(-1, G - 1, B).astype(np.int32)                               # ids -1 .. G - 2: group G - 1 is empty
    info = np.zeros(B, dtype=M.INFO_DTYPE); clr = np.zeros(B, dtype=M.CLEARANCE_DTYPE)
    info["status"] = rng.choice([0, 0, 0, 8, 64, 1, 2, 4, 16, 32, 8 | 16], B)        # (QP_CAPPED and ARRIVED do not exclude)
    clr["status"] = rng.choice([0, 0, 0, 1, 2], B)
    group[:4] = 0; sT[:4] = 0.4; info["status"][:4] = (16, 0, 0, 0); clr["status"][:4] = (0, 1, 0, 0)      # a tie: the lowest admissible index, 2
    group[group == 3] = -1; group[4:7] = 3; info["status"][4:7] = 1                   # group 3 has members, none admissible
    exp = select_np(sT, info["status"], clr["status"], group, G)
    assert exp[0] == 2 and exp[3] == -1 and exp[G - 1] == -1 and (exp >= 0).sum() >= 3
    got = s.select_clear(sT, info, clr, group, G)
    assert np.array_equal(got, exp), (got, exp)
    dev = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in (sT, info, clr, group)]
    dch = torch.full((G,), 77, dtype=torch.int32, device="cuda")
    s.select_clear_device(B, *[t.data_ptr() for t in dev], G, dch.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dch.cpu().numpy(), exp)
    # the device variant treats ids outside [-1, n_groups) as -1; the host variant rejects them and writes nothing
    g2 = group.copy(); g2[10] = G + 3; g2[11] = -5
    e2 = select_np(sT, info["status"], clr["status"], np.where((g2 < 0) | (g2 >= G), -1, g2), G)
    d2 = torch.from_numpy(g2).cuda()
    s.select_clear_device(B, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), d2.data_ptr(), G, dch.data_ptr(), stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert np.array_equal(dch.cpu().numpy(), e2)
    ch = np.full(G, 55, dtype=np.int32)
    rc = M.lib().mpcmp_select_clear_batch(s._ctx, B, sT.ctypes.data, info.ctypes.data, clr.ctypes.data, g2.ctypes.data, G, ch.ctypes.data)
    assert rc == EINVAL and np.all(ch == 55)
    assert s.select_clear(sT, info, clr, np.full(B, -1, dtype=np.int32), 0).shape == (0,)


# ---- 9. the tables change no solve -----------------------------------------------------------------------------------------------------------
def test_tables_leave_the_solve_bit_for_bit(M):
    from mpc_motion_planner_amd import scenarios
    B = 256
    cfg = M.default_config(4, 2, margins=MARGINS)
    x0, xf = scenarios.make_batch(B, MARGINS)
    plain = M.Solver(cfg, B).solve(x0, xf)
    s, _, _, _ = setup(M, 1, 4, B)
    s.set_config(cfg)
    got = s.solve(x0, xf)
    s.clearance(got[0], got[2], 50, MARGIN, 3)
    again = s.solve(x0, xf)
    for a, b, c in zip(plain, got, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


# ---- 10. error paths ------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(M):
    B, n_pts = 4, 20
    s, models, tables, obs = setup(M, 1, 4, 8)
    sx, sT = moves(1, 4, B)
    good = s.clearance(sx, sT, n_pts, MARGIN, 0)
    L, ctx = M.lib(), s._ctx

    def call(B_=B, sx_=sx.ctypes.data, sT_=sT.ctypes.data, n=n_pts, margin=MARGIN, gap=0, out=True):
        o_ = np.zeros(B, dtype=M.CLEARANCE_DTYPE); o_["n_hit"] = -9
        rc = L.mpcmp_clearance_batch(ctx, B_, sx_, sT_, n, margin, gap, o_.ctypes.data if out else None)
        assert np.all(o_["n_hit"] == -9)
        return rc
    for kw in (dict(B_=0), dict(sx_=None), dict(sT_=None), dict(n=0), dict(n=4097), dict(margin=float("nan")), dict(margin=float("inf")),
               dict(gap=-1), dict(out=False)):
        assert call(**kw) == EINVAL, kw
    assert L.mpcmp_clearance_batch_device(ctx, B, None, None, n_pts, MARGIN, 0, None, None) == EINVAL
    assert L.mpcmp_clearance_batch(None, B, sx.ctypes.data, sT.ctypes.data, n_pts, MARGIN, 0, good.ctypes.data) == EINVAL
    # spheres: a bad table changes nothing
    for field, idx, val in (("joint", 2, 7), ("joint", 0, -1), ("r", 1, 0.0), ("r", 1, -0.1), ("r", 3, np.nan), ("c", 0, np.inf)):
        bad = tables[0].copy()
        if field == "c":
            bad["c"][idx, 1] = val
        else:
            bad[field][idx] = val
        assert L.mpcmp_set_robot_spheres(ctx, 0, bad.shape[0], bad.ctypes.data) == EINVAL, (field, val)
    assert L.mpcmp_set_robot_spheres(ctx, 1, 1, tables[0].ctypes.data) == EINVAL          # (a one-arm context)
    assert L.mpcmp_set_robot_spheres(ctx, 0, 65, tables[0].ctypes.data) == EINVAL
    assert L.mpcmp_set_robot_spheres(ctx, 0, 3, None) == EINVAL
    # obstacles: a bad set changes nothing
    def bad_obs(i, **kw):
        b = obs.copy()
        for k, v in kw.items():
            if k == "type" or k == "r":
                b[k][i] = v
            else:
                b[k][i] = v
        return b
    for b in (bad_obs(0, type=4), bad_obs(0, type=-1), bad_obs(0, r=-0.01), bad_obs(2, r=np.nan), bad_obs(1, b=(0.1, 0.0, 0.1)), bad_obs(1, a=(np.inf, 0, 0)),
              bad_obs(3, a=(0.0, 0.0, 1.0 + 1e-8))):
        assert L.mpcmp_set_obstacles(ctx, 1, b.shape[0], b.ctypes.data) == EINVAL
    assert L.mpcmp_set_obstacles(ctx, 1, 257, obs.ctypes.data) == EINVAL
    assert L.mpcmp_set_obstacles(ctx, 9, 4, obs.ctypes.data) == EINVAL                     # (more sets than max_batch = 8)
    assert L.mpcmp_set_obstacles(ctx, -1, 4, obs.ctypes.data) == EINVAL
    assert L.mpcmp_set_obstacles(ctx, 1, 4, None) == EINVAL
    assert L.mpcmp_set_obstacles_device(ctx, 1, 300, None, None) == EINVAL
    assert s.clearance(sx, sT, n_pts, MARGIN, 0).tobytes() == good.tobytes()
    # a half-space normal within 1e-9 of unit length is accepted
    okn = obs.copy(); okn["a"][3] = (0.0, 0.0, 1.0 + 5e-10)
    s.set_obstacles(okn)
    # selection
    info = np.zeros(B, dtype=M.INFO_DTYPE); grp = np.zeros(B, dtype=np.int32); ch = np.full(2, 55, dtype=np.int32)
    args = [sT.ctypes.data, info.ctypes.data, good.ctypes.data, grp.ctypes.data]
    assert L.mpcmp_select_clear_batch(ctx, 0, *args, 1, ch.ctypes.data) == EINVAL
    assert L.mpcmp_select_clear_batch(ctx, B, *args, -1, ch.ctypes.data) == EINVAL
    assert L.mpcmp_select_clear_batch(ctx, B, *args, 9, ch.ctypes.data) == EINVAL
    assert L.mpcmp_select_clear_batch(ctx, B, *args, 1, None) == EINVAL
    for k in range(4):
        a2 = list(args); a2[k] = None
        assert L.mpcmp_select_clear_batch(ctx, B, *a2, 1, ch.ctypes.data) == EINVAL
        assert L.mpcmp_select_clear_batch_device(ctx, B, *a2, 1, ch.ctypes.data, None) == EINVAL
    assert np.all(ch == 55)


def test_non_finite_sample_is_reported(M):
    s, _, _, _ = setup(M, 1, 4, 4)
    sx, sT = moves(1, 4, 4)
    sx[2, 5, 3] = np.nan
    got = s.clearance(sx, sT, 50, MARGIN, 0)
    assert got["status"][2] == M.CLR_NAN and np.isnan(got["d_min"][2]) and got["n_hit"][2] == 0 and got["t_first"][2] == -1.0
    assert np.all(got["status"][[0, 1, 3]] != M.CLR_NAN) and np.all(np.isfinite(got["d_min"][[0, 1, 3]]))


def test_cpp_shim_members(M, tmp_path):
    """examples/shim_selftest.cpp calls the header-only planner's set_obstacles / clearance; its record is a consistent one"""
    import json, os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "shim_selftest.cpp"),
                           "-L" + os.path.join(root, "mpc_motion_planner_amd"), "-lmpcmp", "-Wl,-rpath," + os.path.join(root, "mpc_motion_planner_amd"),
                           "-o", exe])
    r = json.loads(subprocess.check_output([exe]).decode())
    assert np.isfinite(r["clr_d_min"]) and 0 <= r["clr_sphere"] < 24 and r["clr_other"] in (0, 1) and 0 <= r["clr_t_min"]
    assert r["clr_status"] == (1 if r["clr_n_hit"] > 0 else 0) and (r["clr_d_min"] < MARGIN) == (r["clr_n_hit"] > 0)


def test_planner_facade(M):
    p = M.BatchMotionPlanner(max_batch=8, num_seg=4, sqp_iters=2)
    p.set_constraint_margins(*MARGINS)
    from mpc_motion_planner_amd import scenarios
    x0, xf = scenarios.make_batch(8, MARGINS)
    p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
    p.solve_trajectory()
    p.set_obstacles(world(M, 1))
    rec = p.check_clearance(n_pts=100, margin=MARGIN)
    sx, _, sT = p.solution()
    s, _, _, _ = setup(M, 1, 4, 8)
    assert rec.tobytes() == s.clearance(sx, sT, 100, MARGIN, 0).tobytes()
