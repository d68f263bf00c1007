"""Certified clearance against a voxel world (include/mpcmp_field_cert.h), the part that needs no GPU: the ABI table and record sizes, and the host
statement of the rule (mpcmp_clearance_certified_field_one) against the NumPy restatement of tests/field_cert_reference.py, with the properties the
feature exists for.  The robot, the world, the plans and the nine CASES are those of tests/test_clearance_cert_host.py (self_gap is ignored: the
field check knows no robot pairs); the world is rasterised by field_reference.rasterise at ORIGIN on the two GRIDS.  The builders below
(voxel_world, case_reference, one, one_voxel_case, capacity_case) are what tests/test_gpu_field_cert.py checks the kernel with as well.

Bounds.  Doubles within 1e-12 (1 + |x|), the bound of tests/test_clearance_cert_host.py.  Integer fields and leaf counts are compared exactly, which is
fair only while no decision of the reference lies within rounding of the margin and no evaluated centre within rounding of a voxel face (where
sd_field jumps): every case asserts ON THE REFERENCE, for every plan, a smallest decision gap above 1e-9 and a smallest face distance above 1e-9.
The seeds are those of CASES: the conditions hold for all of them on both grids.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import clearance_cert_reference as R
import field_cert_reference as FC
import field_reference as F
from test_clearance_cert_host import CASES, GAP, check_records, plans, robot, thin_capsule_case, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORIGIN = (-1.013, -0.987, -0.131)
GRIDS = {0.04: ((50, 50, 36), -0.05), 0.02: ((100, 100, 72), 0.0)}          # h: (n, margin)
FACE = 1e-9


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


@functools.lru_cache(maxsize=None)
def voxel_world(narm, h):
    """(occupancy, field) of the world of tests/test_clearance_cert_host.py on the grid of edge h"""
    occ = F.rasterise(ORIGIN, h, GRIDS[h][0], world(narm))
    return occ, F.edt(occ)


@functools.lru_cache(maxsize=None)
def case_reference(h, narm, nseg, self_gap, n_start, max_depth, seed):
    """the reference's answer for the plans of a case on the grid of edge h, computed once and shared: [dict(clr, cert, gap, face)]"""
    _, arrays, tables = robot(narm)
    x, T = plans(narm, nseg, seed)
    n, margin = GRIDS[h]
    d2 = voxel_world(narm, h)[1]
    return [FC.certified_field_np(arrays, tables, ORIGIN, h, n, d2, nseg, x[b], T[b], margin, n_start, max_depth) for b in range(x.shape[0])]


def assert_reference_is_fair(ref):
    gaps, faces = [r["gap"] for r in ref], [r["face"] for r in ref]
    assert min(gaps) > GAP, ("reference: a decision within 1e-9 of the margin", gaps)
    assert min(faces) > FACE, ("reference: an evaluated centre within 1e-9 of a voxel face", faces)


def one(M, narm, nseg, desc, d2, x, T, margin, n_start, max_depth, tables=None):
    models, _, tabs = robot(narm)
    return M.clearance_certified_field_one(models, nseg, tabs if tables is None else tables, desc, d2, x, T, margin, n_start, max_depth)


def one_voxel_case():
    """What sampling misses: the plan and the wrist sphere of thin_capsule_case(), a 32^3 grid of 4 mm voxels of which only the centre voxel
    (16, 16, 16) is occupied, placed so that the sphere's centre at the normalised time 0.37 lies in it (at 0.37 of its edge on every axis).
    Returns (x, T, the sphere table, origin, h, n, occ)"""
    x, T, table, _, ts = thin_capsule_case()
    _, arrays, _ = robot(1)
    Rs, ps = R.frames(arrays[0], R.position(4, x[:, :7], ts))
    p = ps[6] + Rs[6] @ np.array([0.0, 0.0, 0.05])
    h, n = 0.004, (32, 32, 32)
    occ = np.zeros((32, 32, 32), dtype=np.uint8)
    occ[16, 16, 16] = 1
    return x, T, table, tuple(p - h * (16 + 0.37)), h, n, occ


def capacity_case(M):
    """n0 = 4096 and max_depth = 1 with a grazing wall.  A sphere of 5 cm on joint 3 swings about the vertical first axis alone, so its height does not
    change (the swing speeds up from 1 to 1.4 rad per unit time, so that the bounds of no two intervals of a level tie); the grid is a wall of
    occupied voxels (the plane i = 0 of a 6 x 5 x 4 grid of 5 cm voxels) that lies wholly on the low side of the swing in x and in y, so both are clamped onto the grid's edge all the way and sd_field reads ONE voxel at one offset: the clearance is the same
    at every time up to rounding, 1e-5 above the margin, while the bound of a level-0 interval lies 1e-4 and that of a level-1 interval 5e-5 below
    the clearance.  So every level-0 interval wants to be split, the first 2048 are, and everything else ends undecided.
    Returns (x, T, table, origin, h, n, occ, margin)"""
    _, arrays, _ = robot(1)
    nseg = 4
    q0 = np.array([0.2, -0.5, 0.0, -2.0, 0.0, 1.6, 0.0])
    tau = M.time_nodes(nseg)
    x = np.zeros((tau.shape[0], 14)); x[:, :7] = q0[None]
    x[:, 0] += tau + 0.2 * tau ** 2
    table = M.spheres([3], [[0.0, 0.0, 0.0]], 0.05)
    c = np.array([R.frames(arrays[0], R.position(nseg, x[:, :7], t))[1][3] for t in np.linspace(0.0, 1.0, 201)])
    h, n = 0.05, (6, 5, 4)
    origin = (c[:, 0].min() - 0.03 - h * n[0], c[:, 1].min() - 0.03 - h * n[1], c[0, 2] - h * 2.3)
    occ = np.zeros(n[::-1], dtype=np.uint8)
    occ[:, :, 0] = 1
    d = F.sd_field(origin, h, n, F.edt(occ), c)[0] - 0.05
    assert d.max() - d.min() <= 1e-13 and d.min() > 0.1
    return x, 2.0, table, origin, h, n, occ, float(d.min()) - 1e-5


def cropped_world():
    """the world of one arm at h = 0.04 cropped to x >= 0: the columns whose low face lies at x >= 0 (plans leave this box on the low side)"""
    h = 0.04
    occ, _ = voxel_world(1, h)
    i0 = int(np.ceil((0.0 - ORIGIN[0]) / h))
    crop = np.ascontiguousarray(occ[:, :, i0:])
    return (ORIGIN[0] + h * i0, ORIGIN[1], ORIGIN[2]), h, crop.shape[::-1], crop


def test_abi_table_and_record_sizes(M):
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_field_cert.h")).read(), flags=re.S)
    decl = re.findall(r"\bint\s+(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr)
    assert [d[0] for d in decl] == list(capi.ABI_FIELD_CERT) and len(decl) == 5
    for name, args in decl:
        kinds = ""
        for a in [" ".join(a.split()) for a in args.split(",")]:
            kinds += "p" if "*" in a else {"int": "i", "double": "d"}[a.split(" ")[0]]
        assert kinds == capi.ABI_FIELD_CERT[name], (name, kinds)
        assert getattr(M.lib(), name).argtypes == [{"p": C.c_void_p, "i": C.c_int, "d": C.c_double}[k] for k in kinds]
    others = set(capi.ABI) | set(capi.ABI_CLEARANCE_CERT) | set(capi.ABI_FIELD) | set(capi.ABI_MOVING_CERT)
    assert not set(capi.ABI_FIELD_CERT) & others
    main = open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    inc = [main.index('#include "mpcmp_%s.h"' % nm) for nm in ("clearance_cert", "field", "field_cert")]
    assert inc[0] < inc[2] and inc[1] < inc[2]
    assert capi.CLEARANCE_CERT_DTYPE.itemsize == 32 == FC.CERT_DTYPE.itemsize and capi.CLEARANCE_DTYPE.itemsize == 40
    assert [capi.CLEARANCE_CERT_DTYPE.fields[k][1] for k in FC.CERT_DTYPE.names] == [FC.CERT_DTYPE.fields[k][1] for k in FC.CERT_DTYPE.names]
    assert "mpcmp_field_cert.h" in open(os.path.join(ROOT, "include", "mpcmp_field.h")).read()


@pytest.mark.parametrize("h", sorted(GRIDS))
@pytest.mark.parametrize("narm,nseg,self_gap,n_start,max_depth,seed", CASES)
def test_host_statement_matches_reference(M, h, narm, nseg, self_gap, n_start, max_depth, seed):
    ref = case_reference(h, narm, nseg, self_gap, n_start, max_depth, seed)
    assert_reference_is_fair(ref)
    x, T = plans(narm, nseg, seed)
    n, margin = GRIDS[h]
    desc, d2 = M.field_desc(ORIGIN, h, n), voxel_world(narm, h)[1]
    kinds = {"hit": 0, "clear": 0, "undecided": 0}
    for b in range(x.shape[0]):
        clr, cert = one(M, narm, nseg, desc, d2, x[b], T[b], margin, n_start, max_depth)
        check_records(clr, cert, ref[b], (h, narm, nseg, b))
        assert clr["d_min"] >= cert["d_lower"]
        kinds["hit" if clr["status"] & 1 else "undecided" if clr["status"] & 4 else "clear"] += 1
    if max_depth >= 3:
        assert kinds["hit"] >= 1 and kinds["clear"] >= 1, kinds
    print("h %.2f arms %d num_seg %d n_start %d max_depth %d: %s; n_eval %d .. %d; smallest gap %.2e, smallest face distance %.2e"
          % (h, narm, nseg, n_start, max_depth, kinds, min(r["cert"]["n_eval"] for r in ref), max(r["cert"]["n_eval"] for r in ref),
             min(r["gap"] for r in ref), min(r["face"] for r in ref)))


@pytest.mark.parametrize("case", [CASES[3], CASES[7]])
def test_lower_bound_is_sound_against_the_exact_world(M, case):
    """against field_reference.true_distance (the distance to the union of the occupied cubes) at 401 uniform times: nothing lies below d_lower, and
    a certified plan has nothing below the margin"""
    narm, nseg, _, n_start, max_depth, seed = case
    h = 0.04
    n, margin = GRIDS[h]
    _, arrays, tables = robot(narm)
    occ, d2 = voxel_world(narm, h)
    desc = M.field_desc(ORIGIN, h, n)
    x, T = plans(narm, nseg, seed)
    arm = [a for a in range(narm) for _ in range(len(tables[a]))]
    sph = [s for a in range(narm) for s in tables[a]]
    rad = np.array([s["r"] for s in sph])
    n_clear = 0
    for b in range(x.shape[0]):
        cen = np.zeros((401, len(sph), 3))
        for k, t in enumerate(np.arange(401) / 400.0):
            q = R.position(nseg, x[b][:, :7 * narm], t)
            fr = [R.frames(arrays[a], q[7 * a:7 * a + 7]) for a in range(narm)]
            for s, rec in enumerate(sph):
                Rs, ps = fr[arm[s]]
                cen[k, s] = ps[int(rec["joint"])] + Rs[int(rec["joint"])] @ rec["c"]
        true_min = float((F.true_distance(ORIGIN, h, occ, cen.reshape(-1, 3)).reshape(401, -1) - rad[None]).min())
        clr, cert = one(M, narm, nseg, desc, d2, x[b], T[b], margin, n_start, max_depth)
        assert cert["d_lower"] <= true_min + 1e-9, (b, cert, true_min)
        if clr["status"] == 0:
            n_clear += 1
            assert true_min >= margin - 1e-9, (b, true_min)
    assert n_clear >= 3, n_clear


def test_a_voxel_between_samples_is_found(M):
    """one occupied voxel of 4 mm that the wrist sphere's centre crosses at t = 0.37, between samples 7 and 8 of n_pts = 20: the field clearance is
    positive at every one of the 21 samples, the certificate has a HIT leaf with d_min < 0 and t_min strictly inside that sample interval; on the
    reference and on the host statement"""
    x, T, table, origin, h, n, occ = one_voxel_case()
    models, arrays, _ = robot(1)
    d2 = F.edt(occ)
    desc = M.field_desc(origin, h, n)
    ref_s, host_s = [], []
    for i in range(21):
        q = R.position(4, x[:, :7], i / 20)
        Rs, ps = R.frames(arrays[0], q)
        ref_s.append(float(F.sd_field(origin, h, n, d2, ps[6] + Rs[6] @ table[0]["c"])[0]) - 0.005)
        host_s.append(M.clearance_field_config(models, [table], desc, d2, q)[0])
    assert min(ref_s) > 0.0 and min(host_s) > 0.0 and np.abs(np.array(ref_s) - np.array(host_s)).max() <= 1e-12, (ref_s, host_s)
    ref = FC.certified_field_np(arrays, [table], origin, h, n, d2, 4, x, T, 0.0, 4, 10)
    clr, cert = one(M, 1, 4, desc, d2, x, T, 0.0, 4, 10, tables=[table])
    for c in (ref["clr"], clr):
        assert c["status"] & 1 and c["n_hit"] >= 1 and c["d_min"] < 0.0
        assert 7 / 20 * T < c["t_min"] < 8 / 20 * T and 7 / 20 * T < c["t_first"] < 8 / 20 * T
        assert c["sphere"] == 0 and d2.reshape(-1)[c["other"]] <= 1          # (the occupied voxel or one that shares a face with it)
    assert ref["gap"] > GAP and ref["face"] > FACE
    check_records(clr, cert, ref, "one voxel")
    print("smallest sampled field clearance %.4f, certified d_min %.4f at t = %.4f T" % (min(ref_s), clr["d_min"], clr["t_min"] / T))


def test_a_plan_that_leaves_the_grid(M):
    """the world cropped to x >= 0: centres on the low side in x are clamped onto the box, and the host statement still matches the reference"""
    origin, h, n, occ = cropped_world()
    d2 = F.edt(occ)
    desc = M.field_desc(origin, h, n)
    _, arrays, tables = robot(1)
    x, T = plans(1, 4, 15)
    outside = 0
    for b in range(x.shape[0]):
        ref = FC.certified_field_np(arrays, tables, origin, h, n, d2, 4, x[b], T[b], -0.05, 4, 3)
        assert ref["gap"] > GAP and ref["face"] > FACE
        clr, cert = one(M, 1, 4, desc, d2, x[b], T[b], -0.05, 4, 3)
        check_records(clr, cert, ref, ("cropped", b))
        q = R.position(4, x[b][:, :7], 0.5)
        outside += bool(R.frames(arrays[0], q)[1][6][0] < origin[0])
    assert outside >= 2


def test_a_small_grid(M):
    """a 7 x 5 x 3 grid of 30 cm voxels with a seeded occupancy"""
    origin, h, n = (-1.013, -0.787, -0.131), 0.3, (7, 5, 3)
    occ = (np.random.default_rng(6).random(n[::-1]) < 0.2).astype(np.uint8)
    assert 3 <= occ.sum() <= 40
    d2 = F.edt(occ)
    desc = M.field_desc(origin, h, n)
    _, arrays, tables = robot(1)
    x, T = plans(1, 4, 14)
    st = set()
    for b in range(x.shape[0]):
        ref = FC.certified_field_np(arrays, tables, origin, h, n, d2, 4, x[b], T[b], -0.3, 1, 6)
        assert ref["gap"] > GAP and ref["face"] > FACE
        clr, cert = one(M, 1, 4, desc, d2, x[b], T[b], -0.3, 1, 6)
        check_records(clr, cert, ref, ("small", b))
        st.add(int(clr["status"]))
    assert len(st) >= 2, st


def test_edge_records(M):
    x, T = plans(1, 4, 15)
    _, arrays, tables = robot(1)
    n = GRIDS[0.04][0]
    desc, d2 = M.field_desc(ORIGIN, 0.04, n), voxel_world(1, 0.04)[1]
    empty = np.full(d2.shape, F.EMPTY, dtype=np.uint32)
    # an empty field, and no spheres: every level-0 interval is a CLEAR leaf
    for d2_, tabs in ((empty, tables), (d2, [tables[0][:0]])):
        clr, cert = one(M, 1, 4, desc, d2_, x[0], T[0], 0.0, 4, 10, tables=tabs)
        assert clr["status"] == 0 and clr["d_min"] == np.inf and clr["t_min"] == -1.0 and clr["sphere"] == -1 and clr["other"] == 0 and clr["n_hit"] == 0
        assert clr["t_first"] == -1.0
        assert cert["d_lower"] == np.inf and cert["n_eval"] == 16 and cert["n_clear"] == 16 and cert["n_undecided"] == 0 and cert["depth"] == 0
        assert cert["t_lower"] == T[0] / 32
        check_records(clr, cert, FC.certified_field_np(arrays, tabs, ORIGIN, 0.04, n, d2_, 4, x[0], T[0], 0.0, 4, 10), "no pair")
    # a NaN node
    bad = x[0].copy(); bad[5, 3] = np.nan
    clr, cert = one(M, 1, 4, desc, d2, bad, T[0], 0.0, 4, 10)
    assert clr["status"] == M.CLR_NAN and np.isnan(clr["d_min"]) and clr["t_min"] == -1.0 and clr["t_first"] == -1.0 and clr["sphere"] == -1
    assert clr["other"] == 0 and clr["n_hit"] == 0
    assert np.isnan(cert["d_lower"]) and cert["t_lower"] == -1.0 and cert["n_eval"] == 0 and cert["n_clear"] == 0 and cert["n_undecided"] == 0
    check_records(clr, cert, FC.certified_field_np(arrays, tables, ORIGIN, 0.04, n, d2, 4, bad, T[0], 0.0, 4, 10), "nan")
    # a NaN in a velocity column is not read
    vel = x[0].copy(); vel[5, 9] = np.nan
    assert one(M, 1, 4, desc, d2, vel, T[0], 0.0, 4, 10)[0]["status"] != M.CLR_NAN


def test_capacity_rule_on_a_grazing_wall(M):
    x, T, table, origin, h, n, occ, margin = capacity_case(M)
    _, arrays, _ = robot(1)
    d2 = F.edt(occ)
    ref = FC.certified_field_np(arrays, [table], origin, h, n, d2, 4, x, T, margin, 1024, 1)
    assert ref["gap"] > GAP and ref["face"] > FACE
    assert ref["cert"]["n_eval"] == 8192 and ref["cert"]["n_undecided"] == 2048 + 4096 and ref["cert"]["n_clear"] == 0 and ref["clr"]["n_hit"] == 0
    clr, cert = one(M, 1, 4, M.field_desc(origin, h, n), d2, x, T, margin, 1024, 1, tables=[table])
    check_records(clr, cert, ref, "capacity")
    assert clr["status"] == M.CLR_UNDECIDED


def test_certificate_merge_in_python():
    """the reference's merge on ties, +inf and NaN (the library's fcert_merge is held to the same rows by tests/host/field_cert_lds_check.cpp, and
    the kernel to this function by tests/test_gpu_field_cert.py)"""
    rows = np.array([(0.25, 1.5, 20, 17, 1, 3), (0.125, 0.5, 16, 16, 0, 0), (0.25, 0.75, 4, 4, 0, 7), (np.inf, 0.0625, 16, 16, 0, 0),
                     (np.inf, 0.125, 8, 8, 0, 0), (np.nan, -1.0, 0, 0, 0, 0)], dtype=FC.CERT_DTYPE)
    a, b = rows[[0, 1, 0, 2, 0, 3, 3, 4, 0, 5]], rows[[1, 0, 2, 0, 3, 0, 4, 3, 5, 0]]
    out = FC.merge_cert(a, b)
    assert list(out["d_lower"][:8]) == [0.125, 0.125, 0.25, 0.25, 0.25, 0.25, np.inf, np.inf] and np.isnan(out["d_lower"][8:]).all()
    assert list(out["t_lower"]) == [0.5, 0.5, 1.5, 0.75, 1.5, 1.5, 0.0625, 0.125, -1.0, -1.0]
    assert list(out["n_eval"]) == [36, 36, 24, 24, 36, 36, 24, 24, 0, 0] and list(out["depth"]) == [3, 3, 7, 7, 3, 3, 0, 0, 0, 0]
    assert list(out["n_undecided"]) == [1, 1, 1, 1, 1, 1, 0, 0, 0, 0] and list(out["n_clear"]) == [33, 33, 21, 21, 33, 33, 24, 24, 0, 0]


def test_argument_validation(M):
    from mpc_motion_planner_amd.capi import host
    models, _, tables = robot(1)
    arr = (M.Model * 1)(*[M.Model.from_buffer_copy(m) for m in models])
    x, T = plans(1, 4, 15)
    n = GRIDS[0.04][0]
    desc, d2 = M.field_desc(ORIGIN, 0.04, n), np.ascontiguousarray(voxel_world(1, 0.04)[1])
    xb = np.ascontiguousarray(x[0]); tab = np.ascontiguousarray(tables[0]); cnt = np.array([tab.shape[0]], dtype=np.int32)
    f = M.lib().mpcmp_clearance_certified_field_one

    def call(**kw):
        rec, cert = np.zeros(1, dtype=M.CLEARANCE_DTYPE), np.zeros(1, dtype=M.CLEARANCE_CERT_DTYPE)
        rec["n_hit"] = 77; cert["n_eval"] = 77
        a = dict(models=arr, narm=1, nseg=4, cnt=host(cnt), tab=host(tab), desc=desc.ctypes.data, d2=host(d2), x=host(xb), T=float(T[0]), margin=0.0,
                 n_start=4, max_depth=10, out=host(rec), cert=host(cert))
        a.update(kw)
        rc = f(a["models"], a["narm"], a["nseg"], a["cnt"], a["tab"], a["desc"], a["d2"], a["x"], a["T"], a["margin"], a["n_start"], a["max_depth"],
               a["out"], a["cert"])
        return rc, bool(rec["n_hit"][0] == 77 and cert["n_eval"][0] == 77)
    assert call() == (0, False)
    assert call(cert=None)[0] == 0
    bad_cnt = np.array([65], dtype=np.int32)
    bad_tab = tab.copy(); bad_tab["joint"][2] = 7
    bad_n, bad_h, bad_o, big = (M.field_desc(ORIGIN, 0.04, (50, 1025, 36)), M.field_desc(ORIGIN, 0.0, n), M.field_desc((np.nan, 0, 0), 0.04, n),
                                M.field_desc(ORIGIN, 0.04, (1024, 1024, 17)))
    for what, kw in (("no models", dict(models=None)), ("narm 0", dict(narm=0)), ("narm 3", dict(narm=3)), ("num_seg 0", dict(nseg=0)),
                     ("no counts", dict(cnt=None)), ("no spheres", dict(tab=None)), ("65 spheres", dict(cnt=host(bad_cnt))),
                     ("joint 7", dict(tab=host(bad_tab))), ("no grid", dict(desc=None)), ("no field", dict(d2=None)),
                     ("n 1025", dict(desc=bad_n.ctypes.data)), ("h 0", dict(desc=bad_h.ctypes.data)), ("origin NaN", dict(desc=bad_o.ctypes.data)),
                     ("2^24 + voxels", dict(desc=big.ctypes.data)), ("no plan", dict(x=None)), ("margin NaN", dict(margin=float("nan"))),
                     ("margin inf", dict(margin=float("inf"))), ("n_start 0", dict(n_start=0)), ("n0 4100", dict(n_start=1025)),
                     ("n_start overflow", dict(n_start=2 ** 30)), ("max_depth -1", dict(max_depth=-1)), ("max_depth 17", dict(max_depth=17)),
                     ("no record", dict(out=None))):
        assert call(**kw) == (-1, True), what
    assert call(n_start=1024, max_depth=0)[0] == 0 and call(max_depth=16, margin=-10.0)[0] == 0
    # the calls on a context refuse a missing context without touching a GPU
    L = M.lib()
    assert L.mpcmp_clearance_certified_field_batch(None, 1, host(xb), host(T), 0.0, 4, 10, host(np.zeros(1, dtype=M.CLEARANCE_DTYPE)), None) == -1
    assert L.mpcmp_clearance_certified_field_batch_device(None, 1, host(xb), host(T), 0.0, 4, 10, host(xb), None, None) == -1
    c = np.zeros(1, dtype=M.CLEARANCE_CERT_DTYPE)
    assert L.mpcmp_clearance_cert_merge_batch(None, 1, host(c), host(c), host(c)) == -1
    assert L.mpcmp_clearance_cert_merge_batch_device(None, 1, host(c), host(c), host(c), None) == -1


def test_selftest_under_the_sanitizers(M, tmp_path):
    """examples/field_cert_selftest.cpp, host part alone (its own main, the host-only unit model_host.cpp, nothing of the GPU) under ASan and UBSan;
    the program checks the properties of the rule itself, what it prints is a consistent set of records"""
    import json
    exe = str(tmp_path / "field_cert_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMPCMP_SELFTEST_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "field_cert_selftest.cpp"), os.path.join(ROOT, "mpc_motion_planner_amd", "csrc", "model_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rows = json.loads(r.stdout)["host"]
    assert [row[0] for row in rows] == [0, 4, 10]
    for depth, status, n_hit, d_min, t_min, voxel, d_lower, n_eval, n_clear, n_und, deepest in rows:
        assert d_lower <= d_min and deepest <= depth and n_eval >= 16 and (status & 4) == (4 if n_und else 0) and (status & 1) == (1 if n_hit else 0)
        assert 0.0 < t_min < 2.0 and 0 <= voxel < 24 * 20 * 16
    assert rows[0][2] == 0 and rows[0][1] == 4 and rows[2][1] & 1 and rows[2][3] <= rows[0][3]


def test_lds_layout_and_merge_rule_under_the_sanitizers(tmp_path):
    """tests/host/field_cert_lds_check.cpp: the layout of k_clearance_cert_field over every table size, its chunk and pitch, and fcert_merge"""
    exe = str(tmp_path / "field_cert_lds_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "host", "field_cert_lds_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok ") and int(out.stdout.split()[1]) == 8 * (65 + 129), out.stdout
