"""Between-node limit checks on the GPU (mpcmp_limits_batch*, mpcmp_select_checked_batch*) against the NumPy restatement of
tests/test_limits_host.py: per arm oracle_py.sample (q, qd, qdd and the torque with that arm's model, the payload lumped by the host helper where
rows are set), oracle_py.fk and oracle_py.frame_jacobian, the formulas of include/mpcmp_limits.h written out.

Inputs: the 32 rest-to-rest jerk-limited moves of tests/test_gpu_clearance.py::moves (same seed, with the accelerations that function drops), so
that the check does not depend on a solve.  Even problems run under bounds_from_margins(0.8, 0.9, 0.5, 0.3, min_height=0.3), odd ones under
bounds_from_margins(1, 1, 1, 1, min_height=-1) (num_seg 1: see rows); tol = 1e-6 in every group; the tool maxima are the batch medians of the reference's own peak speeds.

Bounds.  |excess - reference| <= 1e-9 in every group: the bound test_sample_vs_oracle holds for the rows these values are differences of.
|stretch - reference| <= 1e-9: ratios of such values over bounds >= 1.5.  The sample and channel a record names are checked tie-robustly: the
reference's value at the named place lies within 1e-9 of the reference maximum.  status, n_viol and t_first are exact for every problem none of
whose reference per-sample group excesses lies within 1e-8 of its tol; every case with n_pts >= 50 asserts ON THE REFERENCE that at most 2 % of its
problems fall under that exemption and that every group has at least 4 of 32 problems violating and at least 4 clean.

Largest deviations seen (run with -s): see DESIGN.md, "Limits between the nodes".
"""
import functools

import numpy as np
import pytest

import oracle_py as o
from test_gpu_clearance import MARGINS, SEED
from test_limits_host import GROUPS, QD, QDD, TAU, TOOL_LIN, TOOL_ANG, omodel, record_np, values_np

pytestmark = pytest.mark.gpu

B = 32
TOL = 1e-6
EINVAL = -1
KINEMATIC = (QD, QDD, TOOL_LIN, TOOL_ANG)
NAMES = ("Q", "QD", "QDD", "TAU", "HEIGHT", "TOOL_LIN", "TOOL_ANG")


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


@functools.lru_cache(maxsize=None)
def moves(narm, nseg, n=B, seed=SEED):
    """tests/test_gpu_clearance.py::moves, with the accelerations: sx [n][N][14 narm], su [n][N][7 narm], sT [n]; seed: another stream of moves"""
    lim = o.default_limits()
    vmax, amax, jmax = MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"]
    rng = np.random.default_rng(seed)
    span = np.tile(lim["qmax"] - lim["qmin"], narm)
    q0 = np.tile(lim["qmin"], narm) + (0.05 + 0.9 * rng.random((n, 7 * narm))) * span
    q1 = np.tile(lim["qmin"], narm) + (0.05 + 0.9 * rng.random((n, 7 * narm))) * span
    N = 3 * nseg + 1
    sx, su, sT = np.zeros((n, N, 14 * narm)), np.zeros((n, N, 7 * narm)), np.zeros(n)
    for b in range(n):
        x0, xf = np.concatenate([q0[b], np.zeros(7 * narm)]), np.concatenate([q1[b], np.zeros(7 * narm)])
        sx[b], su[b], sT[b] = (o.warm_start_jerk if narm == 1 else o.warm_start_jerk_multi)(nseg, vmax, amax, jmax, x0, xf)
    for a in (sx, su, sT):
        a.setflags(write=False)
    return sx, su, sT


def rows(M, n=B, nseg=4):
    """even / odd problems' rows.  num_seg 1 has its own: one cubic through four nodes overshoots the generator's velocity limit in 30 of the 32
    moves (peaks up to 1.2 x vmax) and its node accelerations are almost all zero (peaks 0, 0.01 .. 0.02 or 0.51 x amax), so the common rows leave
    2 problems clean in QD and 3 violating in QDD; a velocity margin of 1.5 on the odd rows and an acceleration margin of 0.005 on the even ones
    give 16 and 7 (the condition on the reference stays as it is)"""
    t = np.zeros(n, dtype=M.BOUNDS_DTYPE)
    t[0::2] = M.bounds_from_margins(0.8, 0.9, 0.5 if nseg > 1 else 0.005, 0.3, min_height=0.3)
    t[1::2] = M.bounds_from_margins(1, 1 if nseg > 1 else 1.5, 1, 1, min_height=-1)
    return t


def robot(M, narm, models=None):
    """the Panda(s) of narm, or the models given"""
    if models is not None:
        return list(models)
    return list(M.arm_models(M.DUAL_BASES)) if narm == 2 else [M.default_model()]


def sampled(models, nseg, sx, su, sT, n_pts):
    """per problem the dict of values_np at the n_pts + 1 uniform samples; models: one list of Models, or one list per problem"""
    narm = sx.shape[2] // 14; nq = 7 * narm
    out = []
    for b in range(sx.shape[0]):
        mb = models[b] if isinstance(models[0], (list, tuple)) else models
        cols = []
        for a in range(narm):
            xa = np.concatenate([sx[b][:, 7 * a:7 * a + 7], sx[b][:, nq + 7 * a:nq + 7 * a + 7]], axis=1)
            cols.append(o.sample(nseg, xa, su[b][:, 7 * a:7 * a + 7], sT[b], n_pts, model=omodel(mb[a])))
        cat = lambda lo: np.concatenate([c[:, lo:lo + 7] for c in cols], axis=1)
        out.append(values_np(mb, cat(1), cat(8), cat(15), tau=cat(22)))
    return out


def tool_maxima(vals):
    """the batch medians of the peak tool speeds"""
    return float(np.median([v["vlin"].max() for v in vals])), float(np.median([v["vang"].max() for v in vals]))


def records(vals, table, sT, n_pts, tol, lin_max, ang_max):
    return [record_np(v, table[b], sT[b], n_pts, tol, lin_max, ang_max) for b, v in enumerate(vals)]


@functools.lru_cache(maxsize=None)
def _case(narm, nseg, n_pts):
    import mpc_motion_planner_amd as M
    sx, su, sT = moves(narm, nseg)
    vals = sampled(robot(M, narm), nseg, sx, su, sT, n_pts)
    lin_max, ang_max = tool_maxima(vals)
    return vals, lin_max, ang_max, records(vals, rows(M, B, nseg), sT, n_pts, TOL, lin_max, ang_max)


def assert_reference_is_a_fair_test(ref):
    n_near = sum(r["near"] for r in ref)
    assert n_near <= 0.02 * len(ref), "reference: %d of %d problems within 1e-8 of a tolerance" % (n_near, len(ref))
    for g in range(GROUPS):
        n = sum((r["status"] >> g) & 1 for r in ref)
        assert n >= 4 and len(ref) - n >= 4, "reference: %d of %d problems violate %s" % (n, len(ref), NAMES[g])


def check_records(got, ref, sT, n_pts, tol, what="", worst=None):
    tol = np.broadcast_to(np.asarray(tol, dtype=np.float64), (GROUPS,))
    for b, (g, r) in enumerate(zip(got, ref)):
        tag = (what, b)
        assert g["pad"] == 0 and (g["status"] & ~0x7F) == 0, tag
        for k in range(GROUPS):
            if np.isneginf(r["excess"][k]):
                assert np.isneginf(g["excess"][k]) and g["t_at"][k] == -1.0 and g["channel"][k] == -1, (tag, k)
                continue
            dev = abs(g["excess"][k] - r["excess"][k])
            if worst is not None:
                worst[k] = max(worst[k], dev)
            assert dev <= 1e-9, (tag, NAMES[k], g["excess"][k], r["excess"][k])
            ip = int(round(g["t_at"][k] / sT[b] * n_pts))
            assert 0 <= ip <= n_pts and g["t_at"][k] == (ip / n_pts) * sT[b], (tag, k, g["t_at"][k])
            ch = int(g["channel"][k])
            assert 0 <= ch < r["E"][k].shape[1] and abs(r["E"][k][ip, ch] - r["excess"][k]) <= 1e-9, (tag, NAMES[k], ip, ch)
        assert abs(g["stretch"] - r["stretch"]) <= 1e-9 and g["stretch"] >= 1.0, (tag, g["stretch"], r["stretch"])
        if not r["near"]:
            assert g["status"] == r["status"] and g["n_viol"] == r["n_viol"] and g["t_first"] == r["t_first"], (tag, g, r["status"], r["n_viol"], r["t_first"])


def solver(M, narm, nseg, max_batch=B, sqp=1, models=None):
    """a context of the Panda(s) of narm, or of the models given (a ctypes array of narm Models)"""
    if models is not None:
        cfg = M.default_config(nseg, sqp, margins=MARGINS)
        return M.Solver(cfg, max_batch, models=models) if narm == 2 else M.Solver(cfg, max_batch, model=models[0])
    return M.Solver(M.default_config(nseg, sqp, margins=MARGINS), max_batch, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)


# ---- 1. parity ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_pts", [1, 50, 200])
@pytest.mark.parametrize("nseg,narm", [(1, 1), (2, 1), (4, 1), (6, 1), (6, 2), (8, 2)])
def test_parity_with_the_numpy_reference(M, nseg, narm, n_pts):
    sx, su, sT = moves(narm, nseg)
    vals, lin_max, ang_max, ref = _case(narm, nseg, n_pts)
    if n_pts >= 50:
        assert_reference_is_a_fair_test(ref)
    s = solver(M, narm, nseg)
    s.set_bounds(rows(M, B, nseg))
    got = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    worst = np.zeros(GROUPS)
    try:
        check_records(got, ref, sT, n_pts, TOL, worst=worst)
    finally:
        print("nseg %d, arms %d, n_pts %d: violating %s, stretch %.3f .. %.3f, max |excess - ref| per group %s, max |stretch - ref| %.1e" % (
            nseg, narm, n_pts, [sum((r["status"] >> g) & 1 for r in ref) for g in range(GROUPS)], min(r["stretch"] for r in ref),
            max(r["stretch"] for r in ref), " ".join("%.1e" % w for w in worst), max(abs(g["stretch"] - r["stretch"]) for g, r in zip(got, ref))))


def test_parity_on_the_strided_sample_loop(M):
    """n_pts = 4096: every thread takes seventeen samples; one problem (the odd row)"""
    nseg, narm, n_pts, b = 4, 1, 4096, 1
    sx, su, sT = [a[b:b + 1] for a in moves(narm, nseg)]
    vals = sampled(robot(M, narm), nseg, sx, su, sT, n_pts)
    lin_max, ang_max = 0.9 * vals[0]["vlin"].max(), 0.9 * vals[0]["vang"].max()
    table = rows(M)[b:b + 1]
    ref = records(vals, table, sT, n_pts, TOL, lin_max, ang_max)
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    check_records(s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max), ref, sT, n_pts, TOL, "4096")


# ---- 2. rows, payloads, defaults ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_rows_payloads_and_defaults(M, nseg, narm):
    n_pts = 50
    sx, su, sT = moves(narm, nseg)
    vals, lin_max, ang_max, _ = _case(narm, nseg, n_pts)
    s = solver(M, narm, nseg)
    # no rows set: the configuration's tables for everyone
    table = np.repeat(M.bounds_from_config(s.cfg), B)
    plain = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    check_records(plain, records(vals, table, sT, n_pts, TOL, lin_max, ang_max), sT, n_pts, TOL, "defaults")
    # rows, then cleared again
    s.set_bounds(rows(M))
    assert s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max).tobytes() != plain.tobytes()
    s.clear_bounds()
    assert s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max).tobytes() == plain.tobytes()
    # a NULL spec is tol 0 and infinite maxima
    null = s.limits(sx, su, sT, n_pts)
    assert null.tobytes() == s.limits(sx, su, sT, n_pts, 0.0).tobytes()
    assert np.isneginf(null["excess"][:, TOOL_LIN:]).all() and (null["channel"][:, TOOL_LIN:] == -1).all() and (null["t_at"][:, TOOL_LIN:] == -1).all()
    check_records(null, records(vals, table, sT, n_pts, 0.0, np.inf, np.inf), sT, n_pts, 0.0, "null spec")
    # payload rows: 1 kg and 3 kg on alternate problems (on every arm); the torque group follows the lumped model, the others do not move
    mass = np.where(np.arange(B) % 2 == 0, 1.0, 3.0)
    s.set_payloads(mass if narm == 1 else np.repeat(mass[:, None], narm, axis=1))
    base = robot(M, narm)
    lumped = {m: [M.model_add_payload(bm, M.payload(m, bm.tool[:])) for bm in base] for m in (1.0, 3.0)}
    lvals = sampled([lumped[m] for m in mass], nseg, sx, su, sT, n_pts)
    loaded = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    check_records(loaded, records(lvals, table, sT, n_pts, TOL, lin_max, ang_max), sT, n_pts, TOL, "payload")
    assert (np.abs(loaded["excess"][:, TAU] - plain["excess"][:, TAU]) > 1e-3).sum() >= B // 2
    for f in ("excess", "t_at", "channel"):
        assert np.delete(loaded[f], TAU, axis=1).tobytes() == np.delete(plain[f], TAU, axis=1).tobytes(), f
    assert loaded["stretch"].tobytes() == plain["stretch"].tobytes()
    s.clear_payloads()
    assert s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max).tobytes() == plain.tobytes()


# ---- 3. the stretch cures the kinematic groups ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (6, 2)])
def test_stretch_cures(M, nseg, narm):
    n_pts = 200
    sx, su, sT = moves(narm, nseg)
    _, lin_max, ang_max, ref = _case(narm, nseg, n_pts)
    s = solver(M, narm, nseg)
    s.set_bounds(rows(M))
    first = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    st = first["stretch"]
    assert np.isfinite(st).all() and (st > 1 + 1e-6).sum() >= 8
    x0, xf = np.ascontiguousarray(sx[:, 0]), np.ascontiguousarray(sx[:, -1])          # (states at rest: pinning the end nodes changes nothing)
    ox, ou, oT = s.time_scale(x0, xf, sx, su, sT, sT * st * (1 + 1e-12))
    cured = s.limits(ox, ou, oT, n_pts, TOL, lin_max, ang_max)
    assert cured["excess"][:, KINEMATIC].max() <= 1e-10, cured["excess"][:, KINEMATIC].max(axis=0)
    assert np.abs(cured["stretch"] - 1.0).max() <= 1e-9
    ox, ou, oT = s.time_scale(x0, xf, sx, su, sT, sT * st * (1 - 1e-6))
    short = s.limits(ox, ou, oT, n_pts, TOL, lin_max, ang_max)
    need = st > 1 + 1e-6
    assert (short["excess"][need][:, KINEMATIC].max(axis=1) > 0).all()
    # positions and height are where they were: a stretch does not cure them
    for g in (0, 4):
        assert np.abs(cured["excess"][:, g] - first["excess"][:, g]).max() <= 1e-12


# ---- 4. independence ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (8, 2)])
def test_a_record_does_not_depend_on_the_batch(M, nseg, narm):
    n_pts = 200
    sx, su, sT = moves(narm, nseg)
    _, lin_max, ang_max, _ = _case(narm, nseg, n_pts)
    table = rows(M)
    s = solver(M, narm, nseg)
    s.set_bounds(table)
    base = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    for b in (0, 17, 31):
        s.set_bounds(table[b:b + 1])
        assert s.limits(sx[b:b + 1], su[b:b + 1], sT[b:b + 1], n_pts, TOL, lin_max, ang_max)[0].tobytes() == base[b].tobytes(), b
    order = np.random.default_rng(5).permutation(B)
    s.set_bounds(table[order])
    moved = s.limits(sx[order], su[order], sT[order], n_pts, TOL, lin_max, ang_max)
    for i in range(B):
        assert moved[i].tobytes() == base[order[i]].tobytes(), i


# ---- 5. solved plans ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm,n,sqp", [(2, 1, 8, 3), (6, 2, 2, 1)])
def test_parity_on_solved_plans(M, nseg, narm, n, sqp):
    n_pts = 200
    mv = moves(narm, nseg)
    s = solver(M, narm, nseg, n, sqp)
    table = rows(M, n)
    s.set_bounds(table)
    x0, xf = np.ascontiguousarray(mv[0][:n, 0]), np.ascontiguousarray(mv[0][:n, -1])
    sx, su, sT, info = s.solve(x0, xf, (mv[0][:n], mv[1][:n], mv[2][:n]))
    assert np.isfinite(sx).all() and np.isfinite(su).all() and (sT > 0).all()
    vals = sampled(robot(M, narm), nseg, sx, su, sT, n_pts)
    lin_max, ang_max = tool_maxima(vals)
    ref = records(vals, table, sT, n_pts, TOL, lin_max, ang_max)
    got = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    print("solved, nseg %d, arms %d: excess per group %s" % (nseg, narm, np.array2string(got["excess"].max(axis=0), precision=3)))
    check_records(got, ref, sT, n_pts, TOL, "solved")


# ---- 6. device variant, non-finite values -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,narm", [(4, 1), (8, 2)])
def test_device_variant_equals_the_host_pointer_variant(M, nseg, narm):
    import torch
    n_pts = 200
    sx, su, sT = moves(narm, nseg)
    _, lin_max, ang_max, _ = _case(narm, nseg, n_pts)
    s = solver(M, narm, nseg)
    s.set_bounds(rows(M))
    host = s.limits(sx, su, sT, n_pts, TOL, lin_max, ang_max)
    dx, du, dT = [torch.from_numpy(np.array(a)).cuda() for a in (sx, su, sT)]
    dout = torch.zeros(B * M.LIMITS_DTYPE.itemsize, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    s.limits_device(B, dx.data_ptr(), du.data_ptr(), dT.data_ptr(), n_pts, dout.data_ptr(), M.limits_spec(TOL, lin_max, ang_max), stream=stream)
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == host.tobytes()
    s.limits_device(B, dx.data_ptr(), du.data_ptr(), dT.data_ptr(), n_pts, dout.data_ptr(), None, stream=stream)
    torch.cuda.synchronize()
    assert dout.cpu().numpy().tobytes() == s.limits(sx, su, sT, n_pts).tobytes()


def test_non_finite_sample_is_reported(M):
    sx, su, sT = [np.array(a[:4]) for a in moves(1, 4)]
    sx[1, 5, 3] = np.nan; su[2, 0, 6] = np.inf
    s = solver(M, 1, 4)
    got = s.limits(sx, su, sT, 50, TOL, 1.0, 1.0)
    for b in (1, 2):
        assert got["status"][b] == M.LIM_NAN and np.isnan(got["excess"][b]).all() and (got["t_at"][b] == -1).all() and (got["channel"][b] == -1).all()
        assert got["n_viol"][b] == 0 and got["t_first"][b] == -1.0 and got["stretch"][b] == 1.0
    assert np.all(got["status"][[0, 3]] & M.LIM_NAN == 0) and np.isfinite(got["excess"][[0, 3]]).all()


# ---- 7. the choice --------------------------------------------------------------------------------------------------------------------------
def select_np(sT, status, clr_status, lim_status, lim_mask, group, n_groups):
    bad = 1 | 2 | 4 | 16 | 32
    chosen = np.full(n_groups, -1, dtype=np.int32)
    for g in range(n_groups):
        best = None
        for i in range(len(sT)):
            ok = group[i] == g and (status[i] & bad) == 0 and (clr_status is None or clr_status[i] == 0) and \
                (lim_status is None or (lim_status[i] & (lim_mask | 128)) == 0)
            if ok and (best is None or sT[i] < sT[best]):
                best = i
        chosen[g] = -1 if best is None else best
    return chosen


def test_select_checked(M):
    import torch
    G, K = 12, 4                                                  # groups of four candidates
    n = G * K
    s = M.Solver(M.default_config(4, 1, margins=MARGINS), 64)
    group = np.repeat(np.arange(G, dtype=np.int32), K)
    sT = np.tile([1.0, 2.0, 3.0, 4.0], G)
    info = np.zeros(n, dtype=M.INFO_DTYPE); clr = np.zeros(n, dtype=M.CLEARANCE_DTYPE); lim = np.zeros(n, dtype=M.LIMITS_DTYPE)
    mask = (1 << M.LIM_QD) | (1 << M.LIM_TAU)
    # group g: its fastest member made inadmissible for one reason each (so member 1 is chosen), then the special groups
    info["status"][0 * K] = M.STATUS_NAN; info["status"][1 * K] = M.STATUS_OUTSIDE_TOL; info["status"][2 * K] = M.STATUS_T_OUT_OF_BOX
    clr["status"][3 * K] = M.CLR_HIT; clr["status"][4 * K] = M.CLR_NAN
    lim["status"][5 * K] = 1 << M.LIM_QD; lim["status"][6 * K] = (1 << M.LIM_TAU) | (1 << M.LIM_Q); lim["status"][7 * K] = M.LIM_NAN
    lim["status"][8 * K] = (1 << M.LIM_Q) | (1 << M.LIM_QDD) | (1 << M.LIM_TOOL_ANG)          # bits outside the mask: still admissible
    info["status"][9 * K] = M.STATUS_QP_CAPPED                                               # does not exclude
    lim["status"][10 * K:11 * K] = 1 << M.LIM_QD                                             # nobody admissible
    sT[11 * K:12 * K] = 2.5; clr["status"][11 * K] = 1; lim["status"][11 * K + 1] = 1 << M.LIM_TAU      # a tie among members 2 and 3: the lower index
    exp = select_np(sT, info["status"], clr["status"], lim["status"], mask, group, G)
    assert list(exp) == [1, 5, 9, 13, 17, 21, 25, 29, 32, 36, -1, 46]
    got = s.select_checked(sT, info, group, clr, lim, mask, G)
    assert np.array_equal(got, exp), (got, exp)
    # another mask, no mask
    for m in (0, 0x7F, 1 << M.LIM_Q):
        assert np.array_equal(s.select_checked(sT, info, group, clr, lim, m, G), select_np(sT, info["status"], clr["status"], lim["status"], m, group, G)), m
    # lim = NULL is select_clear exactly; clr = NULL skips the clearance test
    assert np.array_equal(s.select_checked(sT, info, group, clr, None, mask, G), s.select_clear(sT, info, clr, group, G))
    assert np.array_equal(s.select_checked(sT, info, group, clr, None, mask, G), select_np(sT, info["status"], clr["status"], None, 0, group, G))
    e3 = select_np(sT, info["status"], None, lim["status"], mask, group, G)
    assert e3[3] == 12 and e3[4] == 16 and e3[11] == 44
    assert np.array_equal(s.select_checked(sT, info, group, None, lim, mask, G), e3)
    assert np.array_equal(s.select_checked(sT, info, group, None, None, mask, G), select_np(sT, info["status"], None, None, 0, group, G))
    # the device variant equals the host one
    dev = [torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).cuda() for a in (sT, info, clr, lim, group)]
    dch = torch.full((G,), 77, dtype=torch.int32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    s.select_checked_device(n, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(), mask, dev[4].data_ptr(), G, dch.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(dch.cpu().numpy(), exp)
    s.select_checked_device(n, dev[0].data_ptr(), dev[1].data_ptr(), 0, dev[3].data_ptr(), mask, dev[4].data_ptr(), G, dch.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(dch.cpu().numpy(), e3)
    s.select_checked_device(n, dev[0].data_ptr(), dev[1].data_ptr(), dev[2].data_ptr(), 0, mask, dev[4].data_ptr(), G, dch.data_ptr(), stream=st)
    torch.cuda.synchronize()
    assert np.array_equal(dch.cpu().numpy(), s.select_clear(sT, info, clr, group, G))
    # errors write nothing
    L, ctx = M.lib(), s._ctx
    ch = np.full(G, 55, dtype=np.int32)
    args = [sT.ctypes.data, info.ctypes.data, clr.ctypes.data, lim.ctypes.data, mask, group.ctypes.data]
    assert L.mpcmp_select_checked_batch(ctx, 0, *args, G, ch.ctypes.data) == EINVAL
    assert L.mpcmp_select_checked_batch(ctx, n, *args, -1, ch.ctypes.data) == EINVAL
    assert L.mpcmp_select_checked_batch(ctx, n, *args, 65, ch.ctypes.data) == EINVAL
    assert L.mpcmp_select_checked_batch(ctx, n, *args, G, None) == EINVAL
    for k in (0, 1, 5):
        a2 = list(args); a2[k] = None
        assert L.mpcmp_select_checked_batch(ctx, n, *a2, G, ch.ctypes.data) == EINVAL
        assert L.mpcmp_select_checked_batch_device(ctx, n, *a2, G, ch.ctypes.data, None) == EINVAL
    g2 = group.copy(); g2[3] = G
    assert L.mpcmp_select_checked_batch(ctx, n, *args[:5], g2.ctypes.data, G, ch.ctypes.data) == EINVAL
    assert L.mpcmp_select_checked_batch(None, n, *args, G, ch.ctypes.data) == EINVAL
    assert np.all(ch == 55)


# ---- 8. error paths -------------------------------------------------------------------------------------------------------------------------
def test_errors_write_nothing(M):
    n, n_pts = 4, 20
    sx, su, sT = [np.array(a[:n]) for a in moves(1, 4)]
    s = solver(M, 1, 4, 8)
    good = s.limits(sx, su, sT, n_pts, TOL, 1.0, 2.0)
    L, ctx = M.lib(), s._ctx
    big = [np.zeros((9,) + a.shape[1:]) for a in (sx, su, sT)]

    def call(B_=n, sx_=sx.ctypes.data, su_=su.ctypes.data, sT_=sT.ctypes.data, n_=n_pts, spec=M.limits_spec(TOL, 1.0, 2.0), out=True, device=False):
        o_ = np.zeros(9, dtype=M.LIMITS_DTYPE); o_["n_viol"] = -9
        a = (ctx, B_, sx_, su_, sT_, n_, None if spec is None else spec.ctypes.data, o_.ctypes.data if out else None)
        rc = L.mpcmp_limits_batch_device(*a, None) if device else L.mpcmp_limits_batch(*a)
        assert np.all(o_["n_viol"] == -9)
        return rc
    bad = [dict(B_=0), dict(B_=-3), dict(B_=9, sx_=big[0].ctypes.data, su_=big[1].ctypes.data, sT_=big[2].ctypes.data), dict(n_=0), dict(n_=4097),
           dict(sx_=None), dict(su_=None), dict(sT_=None), dict(out=False), dict(spec=M.limits_spec(np.nan)), dict(spec=M.limits_spec(np.inf)),
           dict(spec=M.limits_spec([0, 0, 0, -np.inf, 0, 0, 0])), dict(spec=M.limits_spec(0.0, np.nan)), dict(spec=M.limits_spec(0.0, 1.0, np.nan)),
           dict(spec=M.limits_spec(0.0, -1e-3)), dict(spec=M.limits_spec(0.0, 1.0, -1.0))]
    for kw in bad:
        assert call(**kw) == EINVAL, kw
        assert call(device=True, **kw) == EINVAL, kw          # (nothing is launched: the host addresses are never read)
    assert L.mpcmp_limits_batch(None, n, sx.ctypes.data, su.ctypes.data, sT.ctypes.data, n_pts, None, good.ctypes.data) == EINVAL
    # more problems than rows in force
    s.set_bounds(rows(M, 3))
    assert call() == EINVAL
    s.clear_bounds()
    s.set_payloads(np.ones(2))
    assert call() == EINVAL
    s.clear_payloads()
    assert s.limits(sx, su, sT, n_pts, TOL, 1.0, 2.0).tobytes() == good.tobytes()
    assert s.limits(sx, su, sT, n_pts, TOL, 0.0, np.inf).shape == (n,)          # a maximum of 0 and one of +inf are values


# ---- 9. nothing else changes ----------------------------------------------------------------------------------------------------------------
def test_the_check_leaves_the_solve_bit_for_bit(M):
    from mpc_motion_planner_amd import scenarios
    n = 64
    cfg = M.default_config(4, 2, margins=MARGINS)
    x0, xf = scenarios.make_batch(n, MARGINS)
    plain = M.Solver(cfg, n).solve(x0, xf)
    s = M.Solver(cfg, n)
    got = s.solve(x0, xf)
    s.limits(got[0], got[1], got[2], 50, TOL, 1.0, 2.0)
    again = s.solve(x0, xf)
    for a, b, c in zip(plain, got, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()


def test_planner_facade(M):
    from mpc_motion_planner_amd import scenarios
    p = M.BatchMotionPlanner(max_batch=8, num_seg=4, sqp_iters=2)
    p.set_constraint_margins(*MARGINS)
    x0, xf = scenarios.make_batch(8, MARGINS)
    p.set_current_state(x0[:, :7], x0[:, 7:]); p.set_target_state(xf[:, :7], xf[:, 7:])
    p.solve_trajectory()
    rec = p.check_limits(n_pts=100, tol=TOL, tool_lin_max=1.7, tool_ang_max=2.5)
    sx, su, sT = p.solution()
    s = M.Solver(M.default_config(4, 2, margins=MARGINS[:4]), 8)
    assert rec.tobytes() == s.limits(sx, su, sT, 100, TOL, 1.7, 2.5).tobytes()


def test_cpp_shim_member(M, tmp_path):
    """examples/shim_selftest.cpp calls the header-only planner's check_limits; its record is a consistent one"""
    import json, os, subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "shim_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-I" + os.path.join(root, "include"), os.path.join(root, "examples", "shim_selftest.cpp"),
                           "-L" + os.path.join(root, "mpc_motion_planner_amd"), "-lmpcmp", "-Wl,-rpath," + os.path.join(root, "mpc_motion_planner_amd"),
                           "-o", exe])
    r = json.loads(subprocess.check_output([exe]).decode())
    assert r["lim_stretch"] >= 1.0 and np.isfinite(r["lim_excess_qd"]) and 0 <= r["lim_channel_qd"] < 7 and r["lim_status"] & ~0x7F == 0
    assert (r["lim_n_viol"] > 0) == (r["lim_status"] != 0)
