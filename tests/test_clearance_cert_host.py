"""Certified clearance (include/mpcmp_clearance_cert.h), the part that needs no GPU: the ABI table and record sizes, and the host statement of the
rule (mpcmp_clearance_certified_one) against the NumPy restatement of tests/clearance_cert_reference.py, with the properties the feature exists
for.  The builders below (robot, world, plans, CASES, case_reference, check_records, thin_capsule_case) are what tests/test_gpu_clearance_cert.py
checks the kernel with as well.

Plans are synthetic node arrays: a quintic rest-to-rest swing between two seeded postures inside the middle 80 % of the joint ranges with a seeded
ripple of 0.05 rad with a seeded phase on top (so that the cubics of the segments are not all alike and the plan has no symmetry); the velocity columns are not read and stay 0.

Bounds.  Doubles within 1e-12 (1 + |x|): every quantity is a sum of a few dozen products of magnitudes of order 1 (m, rad), each rounded to 1.1e-16.
Integer fields and leaf counts are compared exactly, which is fair only while no decision of the reference lies within rounding of the margin: every
case asserts ON THE REFERENCE that its smallest decision gap is above 1e-9, for every plan (no plan is left out: the seeds are chosen for it).
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import clearance_cert_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 0.02
NP = 12                 # plans per case
TOL = 1e-12
GAP = 1e-9


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


@functools.lru_cache(maxsize=None)
def _panda(narm):
    import mpc_motion_planner_amd as M
    return robot(narm, list(M.arm_models(M.DUAL_BASES)) if narm == 2 else [M.default_model()])


def robot(narm, models=None, tables=None):
    """(ctypes Models [narm], their arrays for the reference, the sphere table of every arm).  The table is the skeleton of mpcmp_link_spheres without
    the sphere at the origin of joints 1 .. 6: that one lies exactly where the last sphere of the link before it lies, so the two would tie in
    every clearance, and which of them a record names would be decided by the last bit of the forward kinematics.
    models: the Panda(s) of narm, computed once, unless given; tables: that skeleton of every model unless given"""
    import mpc_motion_planner_amd as M
    if models is None:
        return _panda(narm)
    models = list(models)
    if tables is not None:
        return models, [R.model_arrays(m) for m in models], list(tables)
    tables = []
    for m in models:
        t = M.link_spheres(m, 0.06, 0.08)
        tables.append(np.ascontiguousarray(t[(t["joint"] == 0) | (np.abs(t["c"]).max(axis=1) > 0.0)]))
    return models, [R.model_arrays(m) for m in models], tables


@functools.lru_cache(maxsize=None)
def world(narm, rows=None):
    """one of each primitive, near the workspace; rows: (type, a, b, r) tuples of another scene"""
    import mpc_motion_planner_amd as M
    if rows is not None:
        return np.array([M.obstacle(*r) for r in rows], dtype=M.OBSTACLE_DTYPE)
    rows = [(M.OBS_SPHERE, (0.55, 0.0, 0.75), (0, 0, 0), 0.10), (M.OBS_BOX, (0.6, -0.5, 0.15), (0.1, 0.1, 0.15), 0.01),
            (M.OBS_CAPSULE, (-0.5, 0.5, 0.2), (-0.5, 0.5, 1.0), 0.04), (M.OBS_HALFSPACE, (0.0, 0.0, 1.0), (-0.05, 0, 0), 0.0)]
    if narm == 2:
        rows[0] = (M.OBS_SPHERE, (0.5, 0.75, 0.9), (0, 0, 0), 0.05)
        rows[1] = (M.OBS_BOX, (0.5, -0.8, 0.15), (0.1, 0.1, 0.15), 0.01)
    return np.array([M.obstacle(*r) for r in rows], dtype=M.OBSTACLE_DTYPE)


def swing(nseg, q0, q1, ripple=None):
    """x [N][2 nq]: q0 + (q1 - q0) sigma(tau_k) + a_j sin(3.1 tau_k + phi_j) at the collocation nodes, sigma the quintic, ripple = (a, phi);
    velocities 0.  The ripple also breaks the point symmetry of the swing about its middle, which would make mirrored intervals tie in dev"""
    import mpc_motion_planner_amd as M
    tau = M.time_nodes(nseg)
    sg = tau ** 3 * (10.0 - 15.0 * tau + 6.0 * tau ** 2)
    nq = q0.shape[0]
    x = np.zeros((tau.shape[0], 2 * nq))
    x[:, :nq] = q0[None] + (q1 - q0)[None] * sg[:, None]
    if ripple is not None:
        x[:, :nq] += ripple[0][None] * np.sin(3.1 * tau[:, None] + ripple[1][None])
    return x


@functools.lru_cache(maxsize=None)
def plans(narm, nseg, seed, n=NP):
    """(x [n][N][14 narm], T [n])"""
    import mpc_motion_planner_amd as M
    lim = M.default_limits()
    lo, span = np.tile(lim["qmin"], narm), np.tile(lim["qmax"] - lim["qmin"], narm)
    rng = np.random.default_rng(seed)
    q0 = lo + (0.1 + 0.8 * rng.random((n, 7 * narm))) * span
    q1 = lo + (0.1 + 0.8 * rng.random((n, 7 * narm))) * span
    rip, phase = 0.05 * rng.uniform(-1.0, 1.0, (n, 7 * narm)), rng.uniform(0.0, 6.28, (n, 7 * narm))
    return np.stack([swing(nseg, q0[b], q1[b], (rip[b], phase[b])) for b in range(n)]), 1.0 + 2.0 * rng.random(n)


# (narm, num_seg, self_gap, n_start, max_depth, seed): one arm at num_seg 1 and 4, two arms at 6 (the smallest a multi-arm context accepts); every
# case runs in the world of all four obstacle types; self_gap on and off, n_start 1 and 4, max_depth 0, 3 and 10 for every robot
# (self_gap 4 where it is on: at 3 the skeleton has sphere pairs at a constant distance below the sum of their radii, the last sphere of link 3 and the
# first of link 6, 88 mm apart in every posture, so every interval would be a hit with the same clearance)
CASES = [(1, 1, 0, 1, 0, 11), (1, 1, 4, 4, 3, 12), (1, 1, 0, 4, 10, 13), (1, 4, 4, 1, 10, 14), (1, 4, 0, 4, 3, 15), (1, 4, 5, 4, 0, 16),
         (2, 6, 0, 1, 3, 17), (2, 6, 4, 4, 10, 18), (2, 6, 0, 4, 0, 19)]


@functools.lru_cache(maxsize=None)
def case_reference(narm, nseg, self_gap, n_start, max_depth, seed):
    """the reference's answer for the plans of a case, computed once and shared: [dict(clr, cert, gap)]"""
    _, arrays, tables = robot(narm)
    x, T = plans(narm, nseg, seed)
    return [R.certified_np(arrays, tables, world(narm), nseg, x[b], T[b], MARGIN, self_gap, n_start, max_depth) for b in range(x.shape[0])]


def close(a, b):
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    return a == b or abs(a - b) <= TOL * (1.0 + abs(b))


def check_records(clr, cert, ref, what=""):
    """one CLEARANCE_DTYPE and one CLEARANCE_CERT_DTYPE record against a reference dict (or against records of the same dtypes)"""
    rc, rt = ref["clr"], ref["cert"]
    for f in ("sphere", "other", "n_hit", "status"):
        assert int(clr[f]) == int(rc[f]), (what, f, clr, rc)
    for f in ("d_min", "t_min", "t_first"):
        assert close(float(clr[f]), float(rc[f])), (what, f, clr, rc)
    for f in ("n_eval", "n_clear", "n_undecided", "depth"):
        assert int(cert[f]) == int(rt[f]), (what, f, cert, rt)
    for f in ("d_lower", "t_lower"):
        assert close(float(cert[f]), float(rt[f])), (what, f, cert, rt)


def one(M, narm, nseg, obstacles, x, T, margin, self_gap, n_start, max_depth, tables=None, models=None):
    models, _, tabs = robot(narm, models, tables)
    return M.clearance_certified_one(models, nseg, tabs if tables is None else tables, obstacles, x, T, margin, self_gap, n_start, max_depth)


def dense_min(M, narm, nseg, obstacles, x, self_gap, n=20000, tables=None, models=None):
    """the smallest clearance over n + 1 uniform samples by mpcmp_clearance_config (called directly: the tables are marshalled once): (minimum,
    per-sample values)"""
    from mpc_motion_planner_amd.capi import host
    models, _, tabs = robot(narm, models, tables)
    tabs = tabs if tables is None else tables
    arr = (M.Model * narm)(*[M.Model.from_buffer_copy(m) for m in models])
    cnt = np.array([t.shape[0] for t in tabs], dtype=np.int32)
    tab = np.ascontiguousarray(np.concatenate(tabs))
    t = np.arange(n + 1) / n
    seg = np.minimum(np.floor(t * nseg).astype(int), nseg - 1)
    xx = 2.0 * (t * nseg - seg) - 1.0
    w = np.stack([np.prod([(xx - R.XI[k]) / (R.XI[j] - R.XI[k]) for k in range(4) if k != j], axis=0) for j in range(4)], axis=1)       # [n + 1][4]
    q = np.ascontiguousarray(sum(w[:, j, None] * x[3 * seg + j, :7 * narm] for j in range(4)))
    d, out = np.zeros(n + 1), C.c_double(0)
    f, pa, pc, pt, po = M.lib().mpcmp_clearance_config, C.addressof(arr), host(cnt), host(tab), host(obstacles)
    for i in range(n + 1):
        assert f(pa, narm, pc, pt, obstacles.shape[0], po, self_gap, q[i].ctypes.data, C.addressof(out), None, None) == 0
        d[i] = out.value
    return d.min(), d


def thin_capsule_case(nseg=4):
    """The motivating case: one arm whose only sphere is a wrist sphere of 5 mm, a swing of the first and fourth joint, and a capsule of radius 1 mm
    and length 2 cm that the sphere's centre crosses at t = 0.37, between samples 7 and 8 of n_pts = 20, at right angles to its velocity.
    Returns (x [N][14], T, the sphere table, the obstacle, the crossing time)."""
    import mpc_motion_planner_amd as M
    _, arrays, _ = robot(1)
    x = swing(nseg, np.array([-0.9, -0.4, 0.2, -2.0, 0.1, 1.8, 0.5]), np.array([1.1, -0.4, 0.2, -1.4, 0.1, 1.8, 0.5]))
    table = M.spheres([6], [[0.0, 0.0, 0.05]], 0.005)

    def centre(t):
        Rs, ps = R.frames(arrays[0], R.position(nseg, x, t))
        return ps[6] + Rs[6] @ np.array([0.0, 0.0, 0.05])
    ts = 0.37
    c, v = centre(ts), centre(ts + 1e-6) - centre(ts - 1e-6)
    u = np.cross(v, [0.0, 0.0, 1.0]); u /= np.linalg.norm(u)
    ob = np.array([M.obstacle(M.OBS_CAPSULE, c - 0.01 * u, c + 0.01 * u, 0.001)], dtype=M.OBSTACLE_DTYPE)
    return x, 2.0, table, ob, ts


def test_abi_table_and_record_sizes(M):
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_clearance_cert.h")).read(), flags=re.S)
    decl = re.findall(r"\bint\s+(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr)
    assert [d[0] for d in decl] == list(capi.ABI_CLEARANCE_CERT) and len(decl) == 3
    for name, args in decl:
        kinds = ""
        for a in [" ".join(a.split()) for a in args.split(",")]:
            kinds += "p" if "*" in a else {"int": "i", "double": "d"}[a.split(" ")[0]]
        assert kinds == capi.ABI_CLEARANCE_CERT[name], (name, kinds)
        assert getattr(M.lib(), name).argtypes == [{"p": C.c_void_p, "i": C.c_int, "d": C.c_double}[k] for k in kinds]
    assert not set(capi.ABI_CLEARANCE_CERT) & set(capi.SYMBOLS)
    assert '#include "mpcmp_clearance_cert.h"' in open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    assert capi.CLEARANCE_CERT_DTYPE.itemsize == 32 and capi.CLEARANCE_DTYPE.itemsize == 40 and M.CLR_UNDECIDED == 4 == R.UNDECIDED
    assert "#define MPCMP_CLR_UNDECIDED 4" in hdr and "#define MPCMP_CLR_CERT_CAPACITY 4096" in hdr and R.CAPACITY == 4096


def test_reference_pieces():
    """the reference's own parts against closed forms: the Bernstein form reproduces the cubic, its hull bounds it, and the reach bounds the motion
    of a sphere centre under a change of one joint"""
    rng = np.random.default_rng(3)
    nodes = rng.normal(size=4)
    ctrl, mid = R.bezier_of_interval(nodes, -0.3, 0.45)
    ctrl, mid = ctrl[:, 0], mid[0]
    u = np.linspace(0.0, 1.0, 101)
    bern = sum(ctrl[k] * [1, 3, 3, 1][k] * u ** k * (1 - u) ** (3 - k) for k in range(4))
    lag = np.array([R.position(1, nodes[:, None], (xi + 1.0) / 2.0)[0] for xi in -0.3 + 0.75 * u])
    assert np.abs(bern - lag).max() <= 1e-14 and abs(mid - lag[50]) <= 1e-14
    assert bern.max() <= ctrl.max() + 1e-15 and bern.min() >= ctrl.min() - 1e-15
    _, arrays, tables = robot(1)
    q = rng.uniform(-1.0, 1.0, 7)
    plen = np.linalg.norm(arrays[0][1], axis=1)
    for s in tables[0][::5]:
        j = int(s["joint"])
        for i in range(j + 1):
            dq = np.zeros(7); dq[i] = 0.3
            Ra, pa = R.frames(arrays[0], q); Rb, pb = R.frames(arrays[0], q + dq)
            moved = np.linalg.norm(pb[j] + Rb[j] @ s["c"] - pa[j] - Ra[j] @ s["c"])
            assert moved <= (np.linalg.norm(s["c"]) + plen[i + 1:j + 1].sum()) * 0.3 + 1e-15


@pytest.mark.parametrize("narm,nseg,self_gap,n_start,max_depth,seed", CASES)
def test_host_statement_matches_reference(M, narm, nseg, self_gap, n_start, max_depth, seed):
    ref = case_reference(narm, nseg, self_gap, n_start, max_depth, seed)
    gaps = [r["gap"] for r in ref]
    assert min(gaps) > GAP, ("reference: a decision within 1e-9 of the margin", gaps)
    x, T = plans(narm, nseg, seed)
    kinds = {"hit": 0, "clear": 0, "undecided": 0}
    for b in range(x.shape[0]):
        clr, cert = one(M, narm, nseg, world(narm), x[b], T[b], MARGIN, self_gap, n_start, max_depth)
        check_records(clr, cert, ref[b], (narm, nseg, b))
        assert clr["d_min"] >= cert["d_lower"]
        kinds["hit" if clr["status"] & 1 else "undecided" if clr["status"] & 4 else "clear"] += 1
    print("arms %d num_seg %d self_gap %d n_start %d max_depth %d: %s; n_eval %d .. %d; smallest decision gap %.2e"
          % (narm, nseg, self_gap, n_start, max_depth, kinds, min(r["cert"]["n_eval"] for r in ref), max(r["cert"]["n_eval"] for r in ref), min(gaps)))


def test_the_cases_see_every_kind_of_leaf():
    """over the cases the reference produces hit, certified and undecided plans, splits below level 0 and robot pairs at d_min"""
    refs = [r for c in CASES for r in case_reference(*c)]
    st = [r["clr"]["status"] for r in refs]
    assert any(s & 1 for s in st) and any(s == 0 for s in st) and any(s & 4 for s in st)
    assert any(r["cert"]["depth"] == 10 for r in refs) and any(r["clr"]["other"] < 0 for r in refs) and any(r["clr"]["other"] >= 0 for r in refs)


@pytest.mark.parametrize("narm,nseg,self_gap,seed", [(1, 4, 0, 15), (2, 6, 4, 18)])
def test_lower_bound_is_sound(M, narm, nseg, self_gap, seed):
    """against 20,001 uniform samples of mpcmp_clearance_config: nothing lies below d_lower, and a certified plan has nothing below the margin"""
    x, T = plans(narm, nseg, seed)
    n_cert = 0
    for b in range(3):
        dmin, _ = dense_min(M, narm, nseg, world(narm), x[b], self_gap)
        for margin in (MARGIN, dmin - 0.01):          # (the second margin lies below the plan's minimum: it can be certified)
            clr, cert = one(M, narm, nseg, world(narm), x[b], T[b], margin, self_gap, 4, 10)
            assert dmin >= cert["d_lower"] - 1e-12 and clr["d_min"] >= cert["d_lower"], (b, dmin, clr, cert)
            assert clr["d_min"] >= dmin - 1e-4           # (midpoints are configurations of the plan too: d_min cannot lie far below the dense minimum)
            if clr["status"] == 0:
                n_cert += 1
                assert dmin >= margin, (b, dmin, margin)
    assert n_cert >= 3


def test_a_crossing_between_samples_is_found(M):
    """a wrist sphere crosses a capsule of radius 1 mm between samples 7 and 8 of n_pts = 20: every one of the 21 samples is clear, the certified
    record is a hit with t_min strictly inside that sample interval"""
    x, T, table, ob, ts = thin_capsule_case()
    models = robot(1)[0]
    d = [M.clearance_config(models, [table], ob, R.position(4, x[:, :7], i / 20), 0)[0] for i in range(21)]
    assert min(d) >= 0.0, d
    clr, cert = one(M, 1, 4, ob, x, T, 0.0, 0, 4, 10, tables=[table])
    assert clr["status"] & M.CLR_HIT and clr["n_hit"] >= 1 and clr["d_min"] < 0.0
    assert 7 / 20 * T < clr["t_min"] < 8 / 20 * T and 7 / 20 * T < clr["t_first"] < 8 / 20 * T
    assert abs(clr["t_min"] / T - ts) <= 1e-2 and cert["d_lower"] <= clr["d_min"] and clr["sphere"] == 0 and clr["other"] == 0


def test_depth_limit_leaves_a_graze_undecided(M):
    x, T, table, ob, _ = thin_capsule_case()
    clr, cert = one(M, 1, 4, ob, x, T, 0.0, 0, 1, 0, tables=[table])
    assert clr["status"] == M.CLR_UNDECIDED and cert["n_undecided"] >= 1 and cert["depth"] == 0 and cert["n_eval"] == 4
    assert clr["n_hit"] == 0 and clr["t_first"] == -1.0 and cert["d_lower"] < 0.0 <= clr["d_min"]


def test_capacity_rule_on_a_long_graze(M):
    """n0 = 4096: a sphere slides 1e-5 above the margin over a floor during a linear sweep, so that every level-0 interval wants to be split:
    the first 2048 are, the others and the whole of level 1 (max_depth 1) end undecided, as in the reference"""
    _, arrays, _ = robot(1)
    nseg, n_start = 4, 1024
    q0 = np.array([-1.0, -0.5, 0.0, -2.0, 0.0, 1.6, 0.0]); q1 = q0.copy(); q1[0] = 1.0; q1[1] = -0.5 + 1e-5
    tau = M.time_nodes(nseg)
    x = np.zeros((tau.shape[0], 14)); x[:, :7] = q0[None] + (q1 - q0)[None] * tau[:, None]
    table = M.spheres([3], [[0.0, 0.0, 0.0]], 0.05)
    z = [R.frames(arrays[0], R.position(nseg, x, t))[1][3][2] for t in np.linspace(0.0, 1.0, 2001)]
    floor = min(z) - 0.05 - MARGIN - 1e-5
    ob = np.array([M.obstacle(M.OBS_HALFSPACE, (0.0, 0.0, 1.0), (floor, 0, 0), 0.0)], dtype=M.OBSTACLE_DTYPE)
    ref = R.certified_np(arrays, [table], ob, nseg, x, 2.0, MARGIN, 0, n_start, 1)
    assert ref["gap"] > GAP and ref["cert"]["n_eval"] == 8192 and ref["cert"]["n_undecided"] == 2048 + 4096 and ref["cert"]["n_clear"] == 0
    clr, cert = one(M, 1, nseg, ob, x, 2.0, MARGIN, 0, n_start, 1, tables=[table])
    check_records(clr, cert, ref, "capacity")
    assert clr["status"] == M.CLR_UNDECIDED


def test_edge_records(M):
    x, T = plans(1, 4, 15)
    # no pair: no obstacle, one arm, self_gap 0
    clr, cert = one(M, 1, 4, None, x[0], T[0], MARGIN, 0, 4, 10)
    assert clr["status"] == 0 and clr["d_min"] == np.inf and clr["t_min"] == -1.0 and clr["sphere"] == -1 and clr["other"] == 0 and clr["n_hit"] == 0
    assert cert["d_lower"] == np.inf and cert["n_eval"] == 16 and cert["n_clear"] == 16 and cert["n_undecided"] == 0 and cert["depth"] == 0
    assert cert["t_lower"] == T[0] / 32
    check_records(clr, cert, R.certified_np(robot(1)[1], robot(1)[2], None, 4, x[0], T[0], MARGIN, 0, 4, 10), "no pair")
    # a plan at rest: every deviation is 0 up to the rounding of the weights, so level 0 decides and the bound is the clearance itself
    rest = np.repeat(x[0][:1], x.shape[1], axis=0)
    d0 = M.clearance_config(robot(1)[0], robot(1)[2], world(1), rest[0, :7], 3)[0]
    clr, cert = one(M, 1, 4, world(1), rest, 1.0, d0 - 1e-6, 3, 4, 10)
    assert clr["status"] == 0 and cert["depth"] == 0 and cert["n_eval"] == 16 == cert["n_clear"]
    assert abs(clr["d_min"] - d0) <= 1e-12 and 0.0 <= clr["d_min"] - cert["d_lower"] <= 1e-12
    # a NaN node
    bad = x[0].copy(); bad[5, 3] = np.nan
    clr, cert = one(M, 1, 4, world(1), bad, T[0], MARGIN, 0, 4, 10)
    assert clr["status"] == M.CLR_NAN and np.isnan(clr["d_min"]) and clr["t_min"] == -1.0 and clr["t_first"] == -1.0 and clr["sphere"] == -1
    assert clr["other"] == 0 and clr["n_hit"] == 0
    assert np.isnan(cert["d_lower"]) and cert["t_lower"] == -1.0 and cert["n_eval"] == 0 and cert["n_clear"] == 0 and cert["n_undecided"] == 0
    check_records(clr, cert, R.certified_np(robot(1)[1], robot(1)[2], world(1), 4, bad, T[0], MARGIN, 0, 4, 10), "nan")
    # a NaN in a velocity column is not read
    vel = x[0].copy(); vel[5, 9] = np.nan
    assert one(M, 1, 4, world(1), vel, T[0], MARGIN, 0, 4, 10)[0]["status"] != M.CLR_NAN


def test_argument_validation(M):
    from mpc_motion_planner_amd.capi import host
    models, _, tables = robot(1)
    arr = (M.Model * 1)(*[M.Model.from_buffer_copy(m) for m in models])
    x, T = plans(1, 4, 15)
    xb = np.ascontiguousarray(x[0]); tab = np.ascontiguousarray(tables[0]); obs = world(1); cnt = np.array([tab.shape[0]], dtype=np.int32)
    f = M.lib().mpcmp_clearance_certified_one

    def call(**kw):
        rec, cert = np.zeros(1, dtype=M.CLEARANCE_DTYPE), np.zeros(1, dtype=M.CLEARANCE_CERT_DTYPE)
        rec["n_hit"] = 77; cert["n_eval"] = 77
        a = dict(models=arr, narm=1, nseg=4, cnt=host(cnt), tab=host(tab), n_obs=obs.shape[0], obs=host(obs), x=host(xb), T=float(T[0]), margin=MARGIN,
                 self_gap=0, n_start=4, max_depth=10, out=host(rec), cert=host(cert))
        a.update(kw)
        rc = f(a["models"], a["narm"], a["nseg"], a["cnt"], a["tab"], a["n_obs"], a["obs"], a["x"], a["T"], a["margin"], a["self_gap"], a["n_start"],
               a["max_depth"], a["out"], a["cert"])
        return rc, bool(rec["n_hit"][0] == 77 and cert["n_eval"][0] == 77)
    assert call() == (0, False)
    rc, _ = call(cert=None)
    assert rc == 0
    bad_cnt = np.array([65], dtype=np.int32)
    bad_tab = tab.copy(); bad_tab["joint"][2] = 7
    for what, kw in (("no models", dict(models=None)), ("narm 0", dict(narm=0)), ("narm 3", dict(narm=3)), ("num_seg 0", dict(nseg=0)),
                     ("no counts", dict(cnt=None)), ("no spheres", dict(tab=None)), ("65 spheres", dict(cnt=host(bad_cnt))),
                     ("joint 7", dict(tab=host(bad_tab))), ("n_obs -1", dict(n_obs=-1)), ("n_obs 257", dict(n_obs=257)), ("no obstacles", dict(obs=None)),
                     ("no plan", dict(x=None)), ("margin NaN", dict(margin=float("nan"))), ("margin inf", dict(margin=float("inf"))),
                     ("self_gap -1", dict(self_gap=-1)), ("n_start 0", dict(n_start=0)), ("n0 4100", dict(n_start=1025)),
                     ("n_start overflow", dict(n_start=2 ** 30)), ("max_depth -1", dict(max_depth=-1)), ("max_depth 17", dict(max_depth=17)),
                     ("no record", dict(out=None))):
        assert call(**kw) == (-1, True), what
    assert call(n_start=1024, max_depth=0)[0] == 0 and call(max_depth=16, margin=-10.0)[0] == 0


def test_selftest_under_the_sanitizers(M, tmp_path):
    """examples/clearance_cert_selftest.cpp, host part alone (its own main, the host-only unit model_host.cpp, nothing of the GPU) under ASan and
    UBSan; what it prints is a consistent set of records: deeper searches decide more, and the bound never passes the minimum"""
    import json
    exe = str(tmp_path / "clearance_cert_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMPCMP_SELFTEST_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "clearance_cert_selftest.cpp"), os.path.join(ROOT, "mpc_motion_planner_amd", "csrc", "model_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rows = json.loads(r.stdout)["host"]
    assert [(row[0], row[1]) for row in rows] == [(1, 0), (1, 6), (1, 12), (8, 0), (8, 6), (8, 12)]
    for nseg, depth, status, n_hit, d_min, t_min, d_lower, n_eval, n_clear, n_und, deepest in rows:
        assert d_lower <= d_min and deepest <= depth and n_eval >= 4 * nseg and (status & 4) == (4 if n_und else 0) and 0.0 < t_min < 2.0
    assert rows[0][2] == 4 and rows[2][2] == 0 and rows[5][2] == 0 and rows[2][6] > 0.0
