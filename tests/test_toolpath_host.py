"""Tool-line moves (include/mpcmp_toolpath.h), the part that needs no GPU: the ABI table and record sizes, and the host statements of the rule
(mpcmp_tool_line_one, mpcmp_tool_deviation_one) against the NumPy restatement of tests/toolpath_reference.py, with the properties the feature
exists for.  The builders below (robots, draw, special_lines, case, assert_fair, check_line, check_deviation, clean_properties) are what
tests/test_gpu_toolpath.py checks the kernels with as well.

Inputs.  32 seeded lines per robot: start posture mid-range +- a quarter of the joint range, length 0.1 - 0.3 m in a random direction, rotation up to
0.5 rad about a random axis; four special lines (pure translation, pure rotation, zero length, straight out of the workspace).  Robots: the
project's Panda and general robot 11 of tests/robots.py (a random 7R chain with oblique axes; the same draw with a seed of its own).

Fair-test conditions, asserted on the reference alone before anything is compared: of the 32 lines at least 16 track cleanly, at least 4 stop, and at
most 4 are `near` (least manipulability within 10 % of manip_min, or worst error within a factor 10 of eps) and may be left out of parity.

Parity bound.  Measured, not fixed in advance: every case repeats the reference with q_start perturbed by 1e-12 (a random sign per joint) and takes
the largest change of a node value over the clean lines as the amplification of the rule, for q, v and u apart (case() has the rule and
check_line() what is compared).  Measured figures, bounds and the largest differences seen are in DESIGN.md, "Tool-line moves"; run with -s, every
case prints its own.  Statuses and k_fail are equal on every line that is not near.
"""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import toolpath_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NL = 32
DQ = 1e-12           # the perturbation of q_start in the amplification run
SEEDS = {"panda": 5, "general": 3, "dual1": 5}
LENGTH = (0.1, 0.3)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


@functools.lru_cache(maxsize=None)
def robots(name):
    """(ctypes Model, its arrays for the reference)"""
    import pathlib
    import tempfile
    import mpc_motion_planner_amd as M
    import robots as RB
    if name == "panda":
        mdl = M.default_model()
    elif name == "dual1":                      # the second arm of the two-arm robot of the GPU tests
        mdl = M.Model.from_buffer_copy(M.arm_models(M.DUAL_BASES)[1])
    else:
        with tempfile.TemporaryDirectory() as d:
            models, _ = RB.general_models(M, pathlib.Path(d), 11)
        mdl = M.Model.from_buffer_copy(models[0])
    return mdl, R.model_arrays(mdl)


def rot(axis, angle):
    return R.exp3(np.asarray(axis, float) / np.linalg.norm(axis) * angle)


@functools.lru_cache(maxsize=None)
def draw(name):
    """the 32 seeded lines of a robot: (q_start [32][7], R1 [32][3][3], p1 [32][3])"""
    import mpc_motion_planner_amd as M
    lim = M.default_limits()
    mid, rng_q = 0.5 * (lim["qmin"] + lim["qmax"]), lim["qmax"] - lim["qmin"]
    rng = np.random.default_rng(SEEDS[name])
    m = robots(name)[1]
    q = mid + 0.25 * rng_q * rng.uniform(-1.0, 1.0, (NL, 7))
    R1, p1 = np.zeros((NL, 3, 3)), np.zeros((NL, 3))
    for b in range(NL):
        R0, p0, _, _ = R.fk(m, q[b])
        d = rng.normal(size=3); ax = rng.normal(size=3)
        p1[b] = p0 + d / np.linalg.norm(d) * rng.uniform(*LENGTH)
        R1[b] = R0 @ rot(ax, rng.uniform(0.0, 0.5))
    return q, R1, p1


@functools.lru_cache(maxsize=None)
def special_lines(name):
    """pure translation, pure rotation, zero length, straight out of the workspace: (q_start [4][7], R1, p1), from the posture of the clean line
    that stays farthest from a singularity"""
    ref = case(name, 4, 4)[0]
    q0 = draw(name)[0][max((b for b in range(NL) if not ref[b]["status"]), key=lambda b: ref[b]["manip_min"])]
    m = robots(name)[1]
    R0, p0, _, _ = R.fk(m, q0)
    L = LENGTH[0]
    q = np.repeat(q0[None], 4, axis=0)
    R1 = np.stack([R0, R0 @ rot((0.3, -0.5, 0.8), 0.3), R0, R0])
    p1 = np.stack([p0 + np.array([0.0, 0.6, -0.8]) * L, p0, p0, p0 + p0 / np.linalg.norm(p0) * 30.0 * L])
    return q, R1, p1


def row_of(M):
    return M.bounds_from_margins(1, 1, 1, 1, -1)


def reference(name, nseg, n_sub, q, R1, p1, T_in=None, spec=None, rows=None):
    import mpc_motion_planner_amd as M
    m = robots(name)[1]
    sp = dict(spec or {}, n_sub=n_sub)
    out = []
    for b in range(q.shape[0]):
        row = row_of(M) if rows is None else rows[b]
        out.append(R.tool_line_np(m, nseg, row["lbx"][:7], row["ubx"][:7], q[b], R1[b], p1[b], 0.0 if T_in is None else T_in[b], sp))
    return out


@functools.lru_cache(maxsize=None)
def case(name, nseg, n_sub):
    """(reference [32], amplification {q, v, u}, bounds {q, v, u}) of the 32 drawn lines.  A line is clean if it does not stop (a clean line
    may carry the bounds bit).  amplification(X) = the largest change of a node value of X over the clean lines, per unit of the perturbation of
    q_start: rad / rad for q, 1 / s for v, 1 / s^2 for u.  bound(q) = max(100 x amplification(q) x 2^-52 x max |q|, 1e-12), as the issue states it.
    v and u are functions of q, so their bound is the bound of q carried through the measured sensitivity: bound(X) = amplification(X) x
    max(100 x 2^-52 x max |q|, 1e-12) + 100 x e(X): what 100 roundings of q, or the floor of 1e-12 rad in q, change in X, and 100 times the reference's
    own error e(X) in evaluating X at a given q, which is the largest difference over the clean lines between its two routes to v and u (solves
    and the dJ/dq_i form; singular values and the link-velocity recursion): u applies (J J^T + damp I)^-1 twice, and that rounding does not come
    from q."""
    q, R1, p1 = draw(name)
    ref = reference(name, nseg, n_sub, q, R1, p1)
    sgn = np.where(np.random.default_rng(99).random(q.shape) < 0.5, -1.0, 1.0)
    ref2 = reference(name, nseg, n_sub, q + DQ * sgn, R1, p1)
    clean = [b for b in range(NL) if not ref[b]["status"] & (R.STOPPED | R.NAN) and not ref2[b]["status"] & (R.STOPPED | R.NAN) and not ref[b]["near"]]
    qmax = max(np.abs(ref[b]["x"][:, :7]).max() for b in clean)
    amp = {"q": max(np.abs(ref2[b]["x"][:, :7] - ref[b]["x"][:, :7]).max() for b in clean) / DQ,
           "v": max(np.abs(ref2[b]["x"][:, 7:] - ref[b]["x"][:, 7:]).max() for b in clean) / DQ,
           "u": max(np.abs(ref2[b]["u"] - ref[b]["u"]).max() for b in clean) / DQ}
    own = {"v": max(ref[b]["v_err"].max() for b in clean), "u": max(ref[b]["u_err"].max() for b in clean)}
    amp["e_v"], amp["e_u"] = own["v"], own["u"]
    bound = {"q": max(100.0 * amp["q"] * 2.0 ** -52 * qmax, 1e-12), "v": amp["v"] * max(100.0 * 2.0 ** -52 * qmax, 1e-12) + 100.0 * own["v"],
             "u": amp["u"] * max(100.0 * 2.0 ** -52 * qmax, 1e-12) + 100.0 * own["u"]}
    return ref, amp, bound


def assert_fair(ref):
    clean = sum(1 for r in ref if not r["status"] & R.STOPPED)
    stopped = sum(1 for r in ref if r["status"] & R.STOPPED)
    near = sum(1 for r in ref if r["near"])
    assert clean >= 16 and stopped >= 4 and near <= 4, "reference: %d clean, %d stopped, %d near of %d" % (clean, stopped, near, len(ref))
    return clean, stopped, near


def check_line(r, bound, x, u, T, rec, what="", worst=None):
    """one plan x [N][14], u [N][7], T and its TOOL_LINE_DTYPE record against the reference dict r.  Compared: status and k_fail (unless the line is
    near), the NaN pattern, and q, v and u at EVERY node before k_fail, of clean and stopped lines alike.  A stopped line runs into a singularity,
    where u grows without limit (8.7e3 rad/s^2 at the last node of one line here) and the reference's two routes to it differ by 4.8e-9 themselves:
    so at every node the bound of v and u is the case's plus 100 times the reference's own evaluation error AT THAT NODE (v_err, u_err of
    toolpath_reference.tool_line_np).  err_max and manip_min are compared on every line that does not stop; those of a stopped line include the
    diverged step."""
    stopped = bool(r["status"] & R.STOPPED)
    assert (rec["status"] & ~(R.STOPPED | R.Q_OUT_OF_BOUNDS | R.NAN)) == 0, what
    assert abs(T - r["T"]) <= 1e-12 * r["T"], (what, T, r["T"])
    if r["near"]:
        if rec["status"] != r["status"] or rec["k_fail"] != r["k_fail"]:
            return
    assert rec["status"] == r["status"] and rec["k_fail"] == r["k_fail"], (what, rec, r["status"], r["k_fail"])
    n = r["k_fail"] if r["k_fail"] >= 0 else x.shape[0]
    assert np.isnan(x[n:]).all() and np.isnan(u[n:]).all() and np.isfinite(x[:n]).all() and np.isfinite(u[:n]).all(), what
    dq = np.abs(x[:n, :7] - r["x"][:n, :7]).max(initial=0.0)
    assert dq <= bound["q"], (what, "q", dq, bound["q"])
    dv, du = np.abs(x[:n, 7:] - r["x"][:n, 7:]).max(axis=1, initial=0.0), np.abs(u[:n] - r["u"][:n]).max(axis=1, initial=0.0)
    assert (dv <= bound["v"] + 100.0 * r["v_err"][:n]).all(), (what, "v", dv, bound["v"], r["v_err"][:n])
    assert (du <= bound["u"] + 100.0 * r["u_err"][:n]).all(), (what, "u", du, bound["u"], r["u_err"][:n])
    if worst is not None:
        worst["q"] = max(worst.get("q", 0.0), dq)
        if not stopped:
            worst["v"], worst["u"] = max(worst.get("v", 0.0), dv.max(initial=0.0)), max(worst.get("u", 0.0), du.max(initial=0.0))
    if not stopped:
        assert rec["err_max"] <= 1e-9 and r["err_max"] <= 1e-9, (what, rec["err_max"], r["err_max"])
        assert abs(rec["manip_min"] - r["manip_min"]) <= 1e-9 * r["manip_min"], (what, rec["manip_min"], r["manip_min"])
    if n > 0 and np.isfinite(r["q_excess"]):
        assert abs(rec["q_excess"] - r["q_excess"]) <= bound["q"], (what, rec["q_excess"], r["q_excess"])


def check_deviation(name, nseg, x, R1, p1, n_pts, rec, tol_lin=np.inf, tol_ang=np.inf, what=""):
    """a TOOL_DEV_DTYPE record against the reference's samples of the same plan.  1e-12: the forward kinematics sums some twenty products of
    magnitudes below 1 (m, or 1 for a rotation entry), each rounded to 1.1e-16 of it, and the Lagrange weights sum to less than 2 in magnitude, so
    a sampled position or rotation entry carries less than 1e-14; the floor of the parity bound covers it a hundred times"""
    m = robots(name)[1]
    r = R.tool_deviation_np(m, nseg, x[:, :7], R1, p1, n_pts, tol_lin, tol_ang)
    if r["status"] & R.NAN:
        assert rec["status"] == R.NAN and np.isnan(rec["lin_max"]) and np.isnan(rec["perp_max"]) and np.isnan(rec["ang_max"]) and rec["n_over"] == 0
        assert rec["s_lin"] == -1.0 and rec["s_ang"] == -1.0
        return r
    d = r["samples"]
    assert abs(rec["lin_max"] - r["lin_max"]) <= 1e-12 and abs(rec["perp_max"] - r["perp_max"]) <= 1e-12 and abs(rec["ang_max"] - r["ang_max"]) <= 1e-12, (what, rec, r)
    il, ia = int(round(rec["s_lin"] * n_pts)), int(round(rec["s_ang"] * n_pts))
    assert rec["s_lin"] == il / n_pts and rec["s_ang"] == ia / n_pts and d[il, 0] >= r["lin_max"] - 1e-12 and d[ia, 2] >= r["ang_max"] - 1e-12, (what, rec)
    sure = int(((d[:, 0] > tol_lin + 1e-12) | (d[:, 2] > tol_ang + 1e-12)).sum()), int(((d[:, 0] > tol_lin - 1e-12) | (d[:, 2] > tol_ang - 1e-12)).sum())
    assert sure[0] <= rec["n_over"] <= sure[1] and rec["status"] == (R.TD_OVER if rec["n_over"] else 0), (what, rec["n_over"], sure)
    return r


def clean_properties(name, nseg, r, x, u, T, spec=None):
    """what every clean plan must satisfy, checked with the reference's kinematics on the plan under test"""
    m = robots(name)[1]
    sp = dict(R.DEFAULT_SPEC, **(spec or {}))
    tn = R.time_nodes(nseg)
    N = x.shape[0]
    assert (x[0, 7:] == 0.0).all() and (x[-1, 7:] == 0.0).all() and (u[0] == 0.0).all() and (u[-1] == 0.0).all()
    V = r["V"]
    for k in range(N):
        sg = R.sigma(tn[k]) if k < N - 1 else 1.0
        J, Rk, pk, _, _ = R.jacobian(m, x[k, :7])
        e = R.pose_error(Rk, pk, r["R0"] @ R.exp3(sg * r["w"]), r["p0"] + sg * V[:3])
        assert np.linalg.norm(e) <= sp["eps"], (k, np.linalg.norm(e))
        # J v_k = V sd up to the bias of the damping: J J^T (J J^T + damp)^-1 V = V - damp (J J^T + damp)^-1 V, at most damp / s_min^2 of |V|; and up to
        # the rounding of a solve with that matrix, 100 x 2^-52 x its condition number s_max^2 / s_min^2
        sv = np.linalg.svd(J, compute_uv=False)
        sd = R.sigma1(tn[k]) / T if 0 < k < N - 1 else 0.0
        tol = (sp["damp"] / sv[-1] ** 2 + 100.0 * 2.0 ** -52 * (sv[0] / sv[-1]) ** 2) * np.linalg.norm(V) * sd
        assert np.linalg.norm(J @ x[k, 7:] - V * sd) <= tol, (k, np.linalg.norm(J @ x[k, 7:] - V * sd), tol)


def test_abi_table_and_record_sizes(M):
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_toolpath.h")).read(), flags=re.S)
    decl = re.findall(r"\bint\s+(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr)
    assert [d[0] for d in decl] == list(capi.ABI_TOOLPATH) and len(decl) == 6
    for name, args in decl:
        kinds = ""
        for a in [" ".join(a.split()) for a in args.split(",")]:
            kinds += "p" if "*" in a else {"int": "i", "double": "d"}[a.split(" ")[0]]
        assert kinds == capi.ABI_TOOLPATH[name], (name, kinds)
        assert getattr(M.lib(), name).argtypes == [{"p": C.c_void_p, "i": C.c_int, "d": C.c_double}[k] for k in kinds]
    assert not set(capi.ABI_TOOLPATH) & set(capi.SYMBOLS) and '#include "mpcmp_toolpath.h"' in open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    assert capi.TOOL_LINE_SPEC_DTYPE.itemsize == 56 and capi.TOOL_LINE_DTYPE.itemsize == 40 and capi.TOOL_DEV_DTYPE.itemsize == 48


def test_reference_formulas():
    """the reference's closed forms against differences: g' along the flow, and the quintic's derivatives"""
    m = robots("panda")[1]
    q, R1, p1 = draw("panda")
    for b in range(4):
        _, _, _, V = R.line(m, q[b], R1[b], p1[b])
        dg, g = R.field_derivative(m, q[b], V, 1e-8)
        h = 1e-5
        fd = (R.field(m, q[b] + h * g, V, 1e-8) - R.field(m, q[b] - h * g, V, 1e-8)) / (2.0 * h)
        assert np.abs(fd - dg).max() <= 1e-8 * max(1.0, np.abs(dg).max()), (b, np.abs(fd - dg).max(), np.abs(dg).max())
    s = np.linspace(0.0, 1.0, 41); h = 1e-5
    assert np.abs((R.sigma(s + h) - R.sigma(s - h)) / (2 * h) - R.sigma1(s)).max() <= 1e-8
    assert np.abs((R.sigma1(s + h) - R.sigma1(s - h)) / (2 * h) - R.sigma2(s)).max() <= 1e-8
    assert R.sigma(0.0) == 0.0 and R.sigma(1.0) == 1.0 and R.sigma1(0.5) == 1.875 and R.sigma1(0.0) == 0.0 and R.sigma2(0.0) == 0.0
    assert abs(R.sigma1(1.0)) <= 1e-14 and abs(R.sigma2(1.0)) <= 1e-13


CASES = [("panda", 1, 4), ("panda", 4, 4), ("panda", 8, 4), ("panda", 4, 1), ("general", 4, 4), ("general", 8, 1)]


@pytest.mark.parametrize("name,nseg,n_sub", CASES)
def test_host_statement_matches_reference(M, name, nseg, n_sub):
    ref, amp, bound = case(name, nseg, n_sub)
    counts = assert_fair(ref)
    mdl = robots(name)[0]
    q, R1, p1 = draw(name)
    spec = M.tool_line_spec(n_sub=n_sub)
    worst = {}
    for b in range(NL):
        x, u, T, rec = M.tool_line_one(mdl, nseg, row_of(M), q[b], R1[b], p1[b], spec=spec)
        check_line(ref[b], bound, x, u, T, rec, (name, nseg, n_sub, b), worst)
        if not ref[b]["status"] & R.STOPPED and not ref[b]["near"]:
            clean_properties(name, nseg, ref[b], x, u, T)
            # T from the rule: the nominal plan meets the tool-speed maxima exactly at mid-move (or stays below both at T_min)
            peak = max(1.875 * np.linalg.norm(ref[b]["V"][:3]) / T / 1.7, 1.875 * np.linalg.norm(ref[b]["w"]) / T / 2.5)
            assert abs(peak - 1.0) <= 1e-12 if T > 0.2 else peak <= 1.0 + 1e-12, (b, peak, T)
            dev = M.tool_deviation_one(mdl, nseg, x, R1[b], p1[b], 200, 1e-4, 1e-4)
            check_deviation(name, nseg, x, R1[b], p1[b], 200, dev, 1e-4, 1e-4, (name, nseg, b))
    print("tool line %s num_seg %d n_sub %d: %d clean, %d stopped, %d near; amplification q %.2f v %.1f u %.0f, own error v %.1e u %.1e; bounds %.2e %.2e %.2e; worst %.2e %.2e %.2e"
          % ((name, nseg, n_sub) + counts + (amp["q"], amp["v"], amp["u"], amp["e_v"], amp["e_u"], bound["q"], bound["v"], bound["u"], worst["q"], worst["v"], worst["u"])))


@pytest.mark.parametrize("name", ["panda", "general"])
def test_special_lines(M, name):
    mdl = robots(name)[0]
    q, R1, p1 = special_lines(name)
    for nseg, n_sub in ((4, 4), (1, 1)):
        ref = reference(name, nseg, n_sub, q, R1, p1)
        _, _, bound = case(name, 4, 4)
        out = [M.tool_line_one(mdl, nseg, row_of(M), q[b], R1[b], p1[b], spec=M.tool_line_spec(n_sub=n_sub)) for b in range(4)]
        for b in range(4):
            check_line(ref[b], bound, *out[b], what=(name, nseg, b))
        # translation and rotation track cleanly and keep the other half of the pose
        for b in (0, 1):
            assert out[b][3]["status"] == 0, (name, b, out[b][3])
            clean_properties(name, nseg, ref[b], *out[b][:3])
        # zero length: T = T_min, q constant, nothing NaN, everything at rest
        x, u, T, rec = out[2]
        # (the goal is the reference's pose of q_start, the last bit of the library's away: a line of 1e-16 m.  |sigma''| / T^2 <= 5.8 / 0.04)
        assert T == 0.2 and rec["status"] == 0 and rec["k_fail"] == -1 and np.isfinite(x).all() and np.isfinite(u).all()
        assert np.abs(x[:, 7:]).max() <= 1e-13 and np.abs(u).max() <= 1e-11 and (x[0, 7:] == 0.0).all() and (u[-1] == 0.0).all()
        assert np.abs(x[:, :7] - q[2]).max() <= 1e-14
        dev = M.tool_deviation_one(mdl, nseg, x, R1[2], p1[2], 50)
        assert dev["perp_max"] <= 1e-14 and dev["lin_max"] <= 1e-14 and dev["status"] == 0
        # ... and exactly on the start pose of the plan itself: p1 == p0 bit for bit, the perpendicular distance is 0 by definition
        xc = np.repeat(x[:1], x.shape[0], axis=0)
        far = M.tool_deviation_one(mdl, nseg, xc, R1[2], p1[2] + np.array([0.0, 0.0, 1.0]), 8)
        assert abs(far["lin_max"] - 1.0) <= 1e-12 and far["perp_max"] <= 1e-14 and far["s_lin"] == 1.0
        # out of the workspace: stops, and what follows is NaN
        x, u, T, rec = out[3]
        assert rec["status"] & M.TL_STOPPED and 0 < rec["k_fail"] < x.shape[0] and np.isnan(x[rec["k_fail"]:]).all() and np.isfinite(x[:rec["k_fail"]]).all()
        dev = M.tool_deviation_one(mdl, nseg, x, R1[3], p1[3], 50)
        assert dev["status"] == M.TL_NAN and np.isnan(dev["lin_max"]) and dev["s_lin"] == -1.0


def test_finer_nodes_leave_the_line_less(M):
    mdl = robots("panda")[0]
    q, R1, p1 = draw("panda")
    ref = case("panda", 4, 4)[0]
    n = 0
    for b in range(NL):
        if ref[b]["status"] or ref[b]["near"] or case("panda", 8, 4)[0][b]["status"]:
            continue
        d = [M.tool_deviation_one(mdl, ns, M.tool_line_one(mdl, ns, row_of(M), q[b], R1[b], p1[b])[0], R1[b], p1[b], 200) for ns in (4, 8)]
        assert d[1]["lin_max"] < d[0]["lin_max"] and d[1]["perp_max"] < d[0]["perp_max"], (b, d)
        n += 1
    assert n >= 16


def test_explicit_duration_and_bounds_row(M):
    mdl = robots("panda")[0]
    q, R1, p1 = draw("panda")
    ref = case("panda", 4, 4)[0]
    b = next(b for b in range(NL) if not ref[b]["status"] and not ref[b]["near"])
    x0, u0, T0, _ = M.tool_line_one(mdl, 4, row_of(M), q[b], R1[b], p1[b])
    x, u, T, rec = M.tool_line_one(mdl, 4, row_of(M), q[b], R1[b], p1[b], T=2.0 * T0)
    assert T == 2.0 * T0 and np.array_equal(x[:, :7], x0[:, :7]) and np.abs(x[:, 7:] * 2.0 - x0[:, 7:]).max() <= 1e-14 and np.abs(u * 4.0 - u0).max() <= 1e-12
    # a row that ends inside the path: the excess is the largest overshoot of a node, and the bit is set
    row = row_of(M).copy()
    j = int(np.argmax(np.abs(x0[-1, :7] - x0[0, :7])))
    hi = x0[:, j].max(); row["ubx"][j] = hi - 0.01
    rec = M.tool_line_one(mdl, 4, row, q[b], R1[b], p1[b])[3]
    assert abs(rec["q_excess"] - 0.01) <= 1e-12 and rec["status"] == M.TL_Q_OUT_OF_BOUNDS
    assert M.tool_line_one(mdl, 4, row_of(M), q[b], R1[b], p1[b])[3]["q_excess"] < 0.0


def _call_one(M, mdl, nseg, q, R1, p1, T=0.0, spec=None, null=None):
    """the raw call with sentinel-filled outputs: (rc, outputs untouched)"""
    from mpc_motion_planner_amd.capi import host
    N = 3 * max(nseg, 1) + 1
    row = row_of(M)
    x, u, To, rec = np.full((N, 14), 7.5), np.full((N, 7), 7.5), np.full(1, 7.5), np.zeros(1, dtype=M.TOOL_LINE_DTYPE)
    rec["k_fail"] = 77
    args = {"model": C.addressof(mdl), "row": host(row), "q": host(q), "R1": host(R1), "p1": host(p1), "x": host(x), "u": host(u), "T": host(To)}
    if null:
        args[null] = None
    rc = M.lib().mpcmp_tool_line_one(args["model"], nseg, args["row"], None if spec is None else spec.ctypes.data, args["q"], args["R1"], args["p1"], T,
                                     args["x"], args["u"], args["T"], host(rec))
    return rc, bool((x == 7.5).all() and (u == 7.5).all() and To[0] == 7.5 and rec["k_fail"][0] == 77)


def test_argument_validation(M):
    mdl = robots("panda")[0]
    qs, R1s, p1s = draw("panda")
    q, R1, p1 = np.ascontiguousarray(qs[0]), np.ascontiguousarray(R1s[0]), np.ascontiguousarray(p1s[0])
    assert _call_one(M, mdl, 4, q, R1, p1)[0] == 0
    bad = []
    for null in ("model", "row", "q", "R1", "p1", "x", "u", "T"):
        bad.append(("NULL " + null, _call_one(M, mdl, 4, q, R1, p1, null=null)))
    bad.append(("num_seg 0", _call_one(M, mdl, 0, q, R1, p1)))
    bad.append(("num_seg 9", _call_one(M, mdl, 9, q, R1, p1)))
    for what, v in (("q NaN", (q * np.array([1, 1, np.nan, 1, 1, 1, 1]), R1, p1)), ("p1 inf", (q, R1, p1 * np.array([1, np.inf, 1]))),
                    ("R1 NaN", (q, R1 * np.nan, p1)), ("R1 scaled", (q, R1 * 1.001, p1)), ("R1 reflection", (q, R1 @ np.diag([1.0, 1.0, -1.0]), p1)),
                    ("half turn", (q, R.fk(robots("panda")[1], q)[0] @ rot((1.0, 2.0, -1.0), np.pi - 5e-4), p1))):
        bad.append((what, _call_one(M, mdl, 4, *[np.ascontiguousarray(a) for a in v])))
    bad.append(("T NaN", _call_one(M, mdl, 4, q, R1, p1, T=float("nan"))))
    for field, v in (("n_sub", 0), ("n_sub", 65), ("damp", 0.0), ("eps", -1e-9), ("manip_min", np.nan), ("T_min", np.inf), ("T_min", 0.0),
                     ("tool_lin_max", 0.0), ("tool_ang_max", np.nan), ("tool_lin_max", -np.inf)):
        spec = M.tool_line_spec(); spec[field] = v
        bad.append(("%s = %r" % (field, v), _call_one(M, mdl, 4, q, R1, p1, spec=spec)))
    for what, (rc, untouched) in bad:
        assert rc == -1 and untouched, (what, rc, untouched)
    # the tool maxima may be +inf (that term of the rule is 0), and a rotation just short of the half-turn margin passes
    spec = M.tool_line_spec(tool_lin_max=np.inf, tool_ang_max=np.inf)
    assert _call_one(M, mdl, 4, q, R1, p1, spec=spec)[0] == 0 and M.tool_line_one(mdl, 4, row_of(M), q, R1, p1, spec=spec)[2] == 0.2
    assert _call_one(M, mdl, 4, q, np.ascontiguousarray(R.fk(robots("panda")[1], q)[0] @ rot((1.0, 2.0, -1.0), np.pi - 2e-3)), p1)[0] == 0
    # the deviation statement
    from mpc_motion_planner_amd.capi import host
    x = M.tool_line_one(mdl, 4, row_of(M), q, R1, p1)[0]
    rec = np.zeros(1, dtype=M.TOOL_DEV_DTYPE); rec["n_over"] = 77
    f = M.lib().mpcmp_tool_deviation_one
    for a in ((None, 4, host(x), host(R1), host(p1), 10, 1.0, 1.0, host(rec)), (C.addressof(mdl), 0, host(x), host(R1), host(p1), 10, 1.0, 1.0, host(rec)),
              (C.addressof(mdl), 4, None, host(R1), host(p1), 10, 1.0, 1.0, host(rec)), (C.addressof(mdl), 4, host(x), host(R1), host(p1), 0, 1.0, 1.0, host(rec)),
              (C.addressof(mdl), 4, host(x), host(R1), host(p1), 10, -1.0, 1.0, host(rec)), (C.addressof(mdl), 4, host(x), host(R1), host(p1), 10, 1.0, float("nan"), host(rec)),
              (C.addressof(mdl), 4, host(x), host(R1), host(p1), 10, 1.0, 1.0, None)):
        assert f(*a) == -1 and rec["n_over"][0] == 77, a
    assert f(C.addressof(mdl), 4, host(x), host(R1), host(p1), 10, float("inf"), float("inf"), host(rec)) == 0 and rec["n_over"][0] == 0


SAN_MAIN = r'''
#include <cstdio>
#include <cmath>
#include "mpcmp.h"
int main() {
    mpcmp_model m; mpcmp_default_model(&m);
    mpcmp_bounds row; mpcmp_bounds_from_margins(1, 1, 1, 1, -1, &row);
    static const double Q[%(n)d][7] = {%(q)s};
    static const double R1[%(n)d][9] = {%(R)s};
    static const double P1[%(n)d][3] = {%(p)s};
    for (int nseg = 1; nseg <= 8; nseg += 7)
        for (int b = 0; b < %(n)d; b++) {
            double x[25 * 14], u[25 * 7], T;
            mpcmp_tool_line rec; mpcmp_tool_dev dev;
            if (mpcmp_tool_line_one(&m, nseg, &row, nullptr, Q[b], R1[b], P1[b], 0.0, x, u, &T, &rec)) return 2;
            if (mpcmp_tool_deviation_one(&m, nseg, x, R1[b], P1[b], 65, 1e-4, 1e-4, &dev)) return 3;
            std::printf("line %%d %%d status %%d k_fail %%d T %%.17g q %%.17g dev %%d %%.17g\n", nseg, b, rec.status, rec.k_fail, T, x[14 * (rec.k_fail > 0 ? rec.k_fail - 1 : 0) + 3],
                        dev.status, dev.lin_max);
        }
    return 0;
}
'''


def test_host_statements_under_the_sanitizers(M, tmp_path):
    """a stand-alone program (its own main, the host-only unit model_host.cpp, nothing of the GPU) under ASan and UBSan runs three lines, a stopped
    one among them, at num_seg 1 and 8, and prints what the library gives through ctypes"""
    ref = case("panda", 4, 4)[0]
    q, R1, p1 = draw("panda")
    clean = [b for b in range(NL) if not ref[b]["status"] and not ref[b]["near"]][:2]
    stopped = [b for b in range(NL) if ref[b]["status"] & R.STOPPED and not ref[b]["near"] and ref[b]["k_fail"] > 0][:1]
    pick = clean + stopped
    assert len(pick) == 3
    lit = lambda a: ", ".join("{" + ", ".join(repr(float(v)) for v in row.ravel()) + "}" for row in a)
    src = tmp_path / "tool_line_san.cpp"
    src.write_text(SAN_MAIN % {"n": 3, "q": lit(q[pick]), "R": lit(R1[pick]), "p": lit(p1[pick])})
    exe = str(tmp_path / "tool_line_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
                           "-I" + os.path.join(ROOT, "include"), "-o", exe, str(src), os.path.join(ROOT, "mpc_motion_planner_amd", "csrc", "model_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 6
    mdl = robots("panda")[0]
    i = 0
    for nseg in (1, 8):
        for b in pick:
            x, u, T, rec = M.tool_line_one(mdl, nseg, row_of(M), q[b], R1[b], p1[b])
            dev = M.tool_deviation_one(mdl, nseg, x, R1[b], p1[b], 65, 1e-4, 1e-4)
            f = lines[i].split(); i += 1
            assert int(f[4]) == rec["status"] and int(f[6]) == rec["k_fail"] and int(f[12]) == dev["status"], (lines[i - 1], rec, dev)
            qv = x[rec["k_fail"] - 1 if rec["k_fail"] > 0 else 0, 3]
            assert abs(float(f[8]) - T) <= 1e-12 * T and abs(float(f[10]) - qv) <= 1e-12, (lines[i - 1], T, qv)
            assert (np.isnan(float(f[13])) and np.isnan(dev["lin_max"])) or abs(float(f[13]) - dev["lin_max"]) <= 1e-12
    assert any(int(l.split()[4]) & 1 for l in lines)
