"""Certified clearance in a moving world (include/mpcmp_moving_cert.h), the part that needs no GPU: the host statement of the rule
(mpcmp_clearance_certified_timed_one) against the NumPy restatement of tests/moving_cert_reference.py, and the properties the feature exists for.
The builders below (CASES, case_data, case_reference, one, the three constructed cases) are what tests/test_gpu_moving_cert.py checks the kernel
with as well.

Plans are the synthetic swings of tests/test_clearance_cert_host.py, each scaled by a seeded amplitude between 1 and 0 (a plan of amplitude 0 rests):
a certificate at max_depth 0 exists only for short moves, so every case holds long and short ones.  The world is the static world of that file (one
of each primitive) plus one of each primitive PARKED far outside the reach and carried through the cell by a track.

Bounds.  Doubles within 1e-12 (1 + |x|), the bound of the static certificate's tests and for the same reason: every quantity is a sum of a few
dozen products of magnitudes of order 1 (m, rad, s), each rounded to 1.1e-16.  Integer fields and leaf counts are compared exactly, which is fair only
while no decision of the reference lies within rounding of the margin: every case asserts ON THE REFERENCE that its smallest decision gap is above
1e-9 for every plan, and that at least two of its twelve plans are hits and at least two are certified clear.
"""
import collections
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import clearance_cert_reference as R
import moving_cert_reference as MC
import test_clearance_cert_host as H
from test_clearance_cert_host import GAP, NP, TOL, check_records, close, robot, swing

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARK = np.array([0.0, 0.0, 5.0])


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


# name; arms, num_seg; self_gap, n_start, n_rest, max_depth; n_key, n_tracks; one set per problem; wait and hold positive; the sign of t_start; the
# keys' window relative to the mean start time (inside the shortest motion: the track starts after and ends before every plan's window, so both
# clamps are exercised; or wider than every plan's window); margin; seed.
Case = collections.namedtuple("Case", "name narm nseg self_gap n_start n_rest max_depth n_key n_tracks per_problem wait hold ts_sign window margin seed")
CASES = [
    Case("1arm-seg1-depth0", 1, 1, 0, 1, 1, 0, 1, 1, False, False, False, 0, (0.3, 0.9), 0.02, 101),
    Case("1arm-seg1-wait", 1, 1, 4, 4, 3, 3, 2, 4, True, True, False, -1, (-1.5, 4.5), 0.02, 102),
    Case("1arm-seg4-hold-64tracks", 1, 4, 0, 4, 1, 10, 40, 64, False, False, True, 1, (-1.5, 4.5), 0.02, 103),
    Case("1arm-seg4-both", 1, 4, 4, 1, 3, 10, 40, 4, True, True, True, 0, (0.3, 0.9), 0.02, 104),
    Case("2arm-seg6-both", 2, 6, 0, 1, 3, 3, 2, 4, False, True, True, 1, (-1.5, 4.5), 0.02, 105),
    Case("2arm-seg6-depth10", 2, 6, 4, 4, 1, 10, 40, 4, True, False, False, -1, (0.3, 0.9), 0.02, 106),
    Case("2arm-seg6-depth0", 2, 6, 0, 4, 3, 0, 1, 1, False, True, True, 0, (0.3, 0.9), 0.02, 107),
]
IDS = [c.name for c in CASES]
AMPLITUDES = np.array([1.0, 0.6, 0.3, 0.15, 0.08, 0.04, 0.02, 0.01, 0.005, 0.002, 0.001, 0.0])


def moving_rows(M, narm, rng=None):
    """the four tracked obstacles at PARK and the ends of their paths [4][2][3]: a ball crossing along x, a pole (capsule) driving past along y, a
    box coming back along x, a ceiling (half-space, solid above) that comes down; rng: a seeded shift of the paths (one set per problem)"""
    cx = 0.0 if narm == 1 else 0.5
    side = 0.35 if narm == 1 else 0.5
    sh = np.zeros((4, 3)) if rng is None else rng.uniform(-0.08, 0.08, (4, 3))
    rows = [(M.OBS_SPHERE, tuple(PARK), (0, 0, 0), 0.08), (M.OBS_CAPSULE, tuple(PARK), tuple(PARK + [0, 0, 0.8]), 0.05),
            (M.OBS_BOX, tuple(PARK), (0.10, 0.20, 0.10), 0.0), (M.OBS_HALFSPACE, (0.0, 0.0, -1.0), (-PARK[2], 0, 0), 0.0)]
    pole = [[0.45, -0.9, 0.0], [0.45, 0.9, 0.0]] if narm == 1 else [[0.5, -1.2, 0.0], [0.5, -0.45, 0.0]]      # (two arms: it stops short of their line)
    box = [[cx + 0.9, -side, 0.55], [cx - 0.3, -side, 0.55]] if narm == 1 else [[1.4, -0.7, 0.8], [0.2, -0.7, 0.8]]
    ends = np.array([[[cx - 0.9, side, 0.45], [cx + 0.9, side, 0.45]], pole, box, [[0.0, 0.0, 1.9], [0.0, 0.0, 1.25]]])
    return rows, ends + sh[:, None, :]


@functools.lru_cache(maxsize=None)
def case_data(case, still=None, shift=(0.0, 0.0, 0.0)):
    """dict: x [NP][N][14 narm], T, ts, w, h [NP]; obs [NP] record arrays and tracks [NP] = (track_of, offsets [n_tracks][n_key][3], t0, dt): the
    same objects for every plan unless the case has one set per problem.
    For robots that stand elsewhere: still: the (type, a, b, r) rows of the four standing obstacles (default: H.world(narm)); shift: a translation of
    the tracked obstacles' paths (the defaults are the cases as they always were)"""
    import mpc_motion_planner_amd as M
    lim = M.default_limits()
    narm, nseg = case.narm, case.nseg
    lo, span = np.tile(lim["qmin"], narm), np.tile(lim["qmax"] - lim["qmin"], narm)
    rng = np.random.default_rng(case.seed)
    q0 = lo + (0.1 + 0.8 * rng.random((NP, 7 * narm))) * span
    q1 = lo + (0.1 + 0.8 * rng.random((NP, 7 * narm))) * span
    rip, phase = 0.05 * rng.uniform(-1.0, 1.0, (NP, 7 * narm)), rng.uniform(0.0, 6.28, (NP, 7 * narm))
    amp = AMPLITUDES[rng.permutation(NP)]
    x = np.stack([swing(nseg, q0[b], q0[b] + amp[b] * (q1[b] - q0[b]), (amp[b] * rip[b], phase[b])) for b in range(NP)])
    T = 1.0 + 2.0 * rng.random(NP)
    ts = case.ts_sign * 0.7 + (0.1 * rng.uniform(-1.0, 1.0, NP) if case.ts_sign else np.zeros(NP))
    w = 0.2 + 0.6 * rng.random(NP) if case.wait else np.zeros(NP)
    h = 0.2 + 0.6 * rng.random(NP) if case.hold else np.zeros(NP)
    t0 = case.ts_sign * 0.7 + case.window[0]
    dt = (case.window[1] - case.window[0]) / (case.n_key - 1) if case.n_key > 1 else 1.0
    fr = np.array([0.5]) if case.n_key == 1 else np.arange(case.n_key) / (case.n_key - 1)
    slots = [0] if case.n_tracks == 1 else ([5, 17, 40, 63] if case.n_tracks == 64 else [0, 1, 2, 3])
    obs, tracks = [], []
    for b in range(NP if case.per_problem else 1):
        rows, ends = moving_rows(M, narm, np.random.default_rng(case.seed + 1000 + b) if case.per_problem else None)
        n_mv = len(slots)
        path = ends[:n_mv, 0, None, :] + fr[None, :, None] * (ends[:n_mv, 1] - ends[:n_mv, 0])[:, None, :]          # [n_mv][n_key][3]
        if case.n_key > 2 and n_mv > 2:
            path[2, :, 1] += 0.1 * np.sin(2 * np.pi * fr)          # (a wobble that only more than two keys can show)
        off = np.random.default_rng(case.seed + 2000 + b).uniform(-1.0, 1.0, (case.n_tracks, case.n_key, 3))      # (tracks nobody follows)
        off[slots] = path - PARK + np.asarray(shift, dtype=np.float64)
        standing = H.world(narm, still)
        moving = np.array([M.obstacle(*r) for r in rows[:n_mv]], dtype=M.OBSTACLE_DTYPE)
        # tracked and standing obstacles interleaved, so that the obstacle loop changes branch
        order = [standing[0], moving[0]] + ([standing[1], moving[1], moving[2], standing[2], standing[3], moving[3]] if n_mv == 4 else list(standing[1:]))
        tof = [-1, slots[0]] + ([-1, slots[1], slots[2], -1, -1, slots[3]] if n_mv == 4 else [-1] * 3)
        obs.append(np.array(order, dtype=M.OBSTACLE_DTYPE))
        tracks.append((np.array(tof, dtype=np.int32), np.ascontiguousarray(off), t0, dt))
    if not case.per_problem:
        obs, tracks = obs * NP, tracks * NP
    return dict(x=x, T=T, ts=ts, w=w, h=h, obs=obs, tracks=tracks, amp=amp)


@functools.lru_cache(maxsize=None)
def case_reference(case):
    """the reference's answer for the plans of a case, computed once and shared: [dict(clr, cert, gap)]"""
    _, arrays, tables = robot(case.narm)
    d = case_data(case)
    return [MC.certified_timed_np(arrays, tables, d["obs"][b], d["tracks"][b], case.nseg, d["x"][b], d["T"][b], d["ts"][b], d["w"][b], d["h"][b],
                                  case.margin, case.self_gap, case.n_start, case.n_rest, case.max_depth) for b in range(NP)]


def assert_fair(case, ref):
    gaps = [r["gap"] for r in ref]
    n_hit = sum(bool(r["clr"]["status"] & 1) for r in ref)
    n_clear = sum(r["clr"]["status"] == 0 for r in ref)
    print("%s: %d hit, %d certified clear, %d undecided only; n_eval %d .. %d; depth <= %d; smallest decision gap %.2e"
          % (case.name, n_hit, n_clear, NP - n_hit - n_clear, min(r["cert"]["n_eval"] for r in ref), max(r["cert"]["n_eval"] for r in ref),
             max(r["cert"]["depth"] for r in ref), min(gaps)))
    assert min(gaps) > GAP, ("reference: a decision within 1e-9 of the margin", case.name, gaps)
    assert n_hit >= 2 and n_clear >= 2, ("reference: too few hits or certified plans", case.name, n_hit, n_clear)


def one(M, narm, nseg, obstacles, tracks, x, T, ts, w, h, margin, self_gap, n_start, n_rest, max_depth, tables=None, models=None):
    models, _, tabs = robot(narm, models, tables)
    return M.clearance_certified_timed_one(models, nseg, tabs if tables is None else tables, obstacles, tracks, x, T, ts, w, h, margin, self_gap,
                                           n_start, n_rest, max_depth)


def one_of_case(M, case, b):
    d = case_data(case)
    return one(M, case.narm, case.nseg, d["obs"][b], d["tracks"][b], d["x"][b], d["T"][b], d["ts"][b], d["w"][b], d["h"][b], case.margin,
               case.self_gap, case.n_start, case.n_rest, case.max_depth)


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_abi_table(M):
    import re
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_moving_cert.h")).read(), flags=re.S)
    decl = re.findall(r"\bint\s+(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr)
    assert [d[0] for d in decl] == list(capi.ABI_MOVING_CERT) and len(decl) == 3
    for name, args in decl:
        kinds = "".join("p" if "*" in a else ("d" if "double" in a else "i") for a in args.split(","))
        assert kinds == capi.ABI_MOVING_CERT[name], (name, kinds)
        assert getattr(M.lib(), name).argtypes == [{"p": C.c_void_p, "i": C.c_int, "d": C.c_double}[k] for k in kinds]
    mp = open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    assert mp.index('#include "mpcmp_moving.h"') < mp.index('#include "mpcmp_moving_cert.h"')


def test_reference_track_bound_is_the_largest_displacement():
    """the reference's E_k against brute force: 4,001 points of the polyline on the interval never lie farther from p_m, and one comes as close
    to it as the spacing of the points allows (dyadic and other clocks, intervals inside one piece, over many keys, and outside the keys on either side)"""
    rng = np.random.default_rng(9)
    P = rng.normal(size=(12, 3))
    for t0, dt in ((0.25, 0.5), (0.3, 0.07)):
        for ta, tb in ((t0 + 1.1 * dt, t0 + 1.6 * dt), (t0 + 0.5 * dt, t0 + 7.25 * dt), (t0 - 3.0, t0 + 2.0 * dt), (t0 + 9.5 * dt, t0 + 40 * dt),
                       (t0 - 2.0, t0 - 1.0), (t0 + 3 * dt, t0 + 5 * dt)):
            tm = 0.5 * (ta + tb)
            pm, E, _ = MC.track_bound(P, t0, dt, ta, tm, tb)
            d = [np.linalg.norm(MC.track_point(P, t0, dt, t) - pm) for t in np.linspace(ta, tb, 4001)]
            step = (tb - ta) / 4000 * np.linalg.norm(np.diff(P, axis=0), axis=1).max() / dt          # (how far the polyline moves between two points)
            assert max(d) <= E + 1e-13 and max(d) >= E - step, (t0, dt, ta, tb, E, max(d))
    assert MC.track_bound(P[:1], 0.0, 1.0, -5.0, 0.0, 5.0)[1] == 0.0


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_host_statement_matches_reference(M, case):
    ref = case_reference(case)
    assert_fair(case, ref)
    for b in range(NP):
        clr, cert = one_of_case(M, case, b)
        check_records(clr, cert, ref[b], (case.name, b))
        assert clr["d_min"] >= cert["d_lower"]


def test_the_cases_see_every_kind_of_leaf_and_phase():
    """over the cases the reference has hit, certified and undecided plans, and names t_min in a wait, in a motion and in a hold"""
    st, where = [], set()
    for case in CASES:
        d = case_data(case)
        for b, r in enumerate(case_reference(case)):
            st.append(r["clr"]["status"])
            t = r["clr"]["t_min"]
            where.add("wait" if t < d["w"][b] else "motion" if t < d["w"][b] + d["T"][b] else "hold")
    assert any(s & 1 for s in st) and any(s == 0 for s in st) and any(s & 4 for s in st)
    assert where == {"wait", "motion", "hold"}, where


@pytest.mark.parametrize("narm,nseg,self_gap,n_start,max_depth,seed", [H.CASES[1], H.CASES[4], H.CASES[6]])
def test_no_tracks_and_no_rests_is_the_static_certificate(M, narm, nseg, self_gap, n_start, max_depth, seed):
    x, T = H.plans(narm, nseg, seed)
    for b in range(NP):
        clr0, cert0 = H.one(M, narm, nseg, H.world(narm), x[b], T[b], H.MARGIN, self_gap, n_start, max_depth)
        for ts in (0.0, -3.25, 17.0):
            clr, cert = one(M, narm, nseg, H.world(narm), None, x[b], T[b], ts, 0.0, 0.0, H.MARGIN, self_gap, n_start, 2, max_depth)
            check_records(clr, cert, dict(clr=clr0, cert=cert0), ("static", narm, nseg, b, ts))


def shifted(obs, tof, p):
    """the obstacle records moved by their tracks' offsets p [n_tracks][3]"""
    out = obs.copy()
    for o in range(obs.shape[0]):
        if tof[o] < 0:
            continue
        if obs["type"][o] == 3:
            out["b"][o][0] = obs["b"][o][0] + obs["a"][o] @ p[tof[o]]
        else:
            out["a"][o] = obs["a"][o] + p[tof[o]]
            if obs["type"][o] == 1:
                out["b"][o] = obs["b"][o] + p[tof[o]]
    return out


def dense_minimum(M, narm, nseg, obs, tracks, x, T, ts, w, h, self_gap, tables=None, n_motion=20000, n_rest=5000, models=None):
    """the smallest clearance over n_motion + 1 samples of the motion and n_rest + 1 of each rest, by mpcmp_clearance_config on the posture (the
    reference's interpolant) against the obstacles moved by mpcmp_track_offset; the motion also by mpcmp_clearance_timed_one at the 4,097 samples it
    takes at most"""
    models, _, tabs = robot(narm, models, tables)
    tabs = tabs if tables is None else tables
    tof, off, t0, dt = tracks if tracks is not None else (np.full(obs.shape[0], -1), np.zeros((0, 1, 3)), 0.0, 1.0)
    best = M.clearance_timed_one(models, nseg, tabs, obs, tracks, x, T, None, ts, 4096, 0.0, self_gap)["d_min"]
    spans = [(np.linspace(0.0, 1.0, n_motion + 1), lambda s: ts + s * T, lambda s: R.position(nseg, x[:, :7 * narm], s))]
    if w > 0.0:
        spans.append((np.linspace(0.0, 1.0, n_rest + 1), lambda s: ts - w + s * w, lambda s: x[0, :7 * narm]))
    if h > 0.0:
        spans.append((np.linspace(0.0, 1.0, n_rest + 1), lambda s: ts + T + s * h, lambda s: x[-1, :7 * narm]))
    for ss, tau_of, q_of in spans:
        for s in ss:
            p = np.array([M.track_offset(off[k], t0, dt, tau_of(s)) for k in sorted(set(int(k) for k in tof if k >= 0))] or [[0.0, 0.0, 0.0]])
            full = np.zeros((max(off.shape[0], 1), 3))
            for i, k in enumerate(sorted(set(int(k) for k in tof if k >= 0))):
                full[k] = p[i]
            best = min(best, M.clearance_config(models, tabs, shifted(obs, tof, full), q_of(s), self_gap)[0])
    return best


@pytest.mark.parametrize("case", [CASES[1], CASES[4]], ids=[IDS[1], IDS[4]])
def test_lower_bound_is_sound(M, case):
    """against dense sampling of the motion (20,001 samples) and of both rests (5,001 each): nothing lies below d_lower, and nothing below the margin
    where status == 0.  mpcmp_clearance_timed_one takes n_pts <= 4096, so it contributes its 4,097 samples and the 20,001 come from
    mpcmp_clearance_config on the posture against the obstacles moved by mpcmp_track_offset, as the rests do"""
    d = case_data(case)
    ref = case_reference(case)
    picks = [b for b in range(NP) if ref[b]["clr"]["status"] == 0][:2] + [b for b in range(NP) if ref[b]["clr"]["status"] != 0][:1]
    n_cert = 0
    for b in picks:
        clr, cert = one_of_case(M, case, b)
        dmin = dense_minimum(M, case.narm, case.nseg, d["obs"][b], d["tracks"][b], d["x"][b], d["T"][b], d["ts"][b], d["w"][b], d["h"][b],
                             case.self_gap, n_motion=20000, n_rest=5000)
        assert dmin >= cert["d_lower"] - 1e-12 and clr["d_min"] >= cert["d_lower"], (case.name, b, dmin, clr, cert)
        if clr["status"] == 0:
            n_cert += 1
            assert dmin >= case.margin, (case.name, b, dmin)
    assert n_cert >= 2


# ---------------------------------------------------------------------------------------------------------------------------------------------
# What samples cannot see.  The robot of the three cases is the one of thin_capsule_case (tests/test_clearance_cert_host.py): one arm whose only
# sphere is a wrist sphere of 5 mm, a quintic swing of the first and fourth joint over T = 2 s at num_seg 4.  The obstacle is a sphere of 3 mm on a
# track of two keys 1 s apart that lie 2 m apart: a straight line at 2 m/s through a chosen point c of the wrist sphere's path, at right angles to
# the robot's direction of travel there, passing c at the world time tau_c.  Robot and obstacle touch while their centres are within 8 mm.
CrossCase = collections.namedtuple("CrossCase", "x T table obs tracks tau_c")


def crossing_case(s_c, tau_c, lateral=0.0, t0=None, n_key=2):
    """the obstacle passes the point of the path at normalised time s_c at world time tau_c; lateral: a shift of its line along the third direction;
    t0, n_key: the keys' clock, 1 s apart (default: two keys, half a second before and after the crossing)"""
    import mpc_motion_planner_amd as M
    _, arrays, _ = robot(1)
    x, T, table, _, _ = H.thin_capsule_case()

    def centre(s):
        Rs, ps = R.frames(arrays[0], R.position(4, x, s))
        return ps[6] + Rs[6] @ np.array([0.0, 0.0, 0.05])
    sa, sb = (max(s_c - 0.01, 0.0), min(s_c + 0.01, 1.0))
    v = centre(sb) - centre(sa); v /= np.linalg.norm(v)
    u = np.cross(v, [0.0, 0.0, 1.0]); u /= np.linalg.norm(u)
    c = centre(s_c) + lateral * np.cross(u, v)
    obs = np.array([M.obstacle(M.OBS_SPHERE, (0.0, 0.0, 0.0), (0, 0, 0), 0.003)], dtype=M.OBSTACLE_DTYPE)
    t0 = tau_c - 0.5 if t0 is None else t0
    tracks = (np.array([0], dtype=np.int32), np.array([[c + 2.0 * (t0 + j - tau_c) * u for j in range(n_key)]]), t0, 1.0)
    return CrossCase(x, T, table, obs, tracks, tau_c)


def case_a():
    """During the motion.  The plan starts at t_start = 0.3; n_pts = 20 samples it every 0.1 s of its clock, samples 7 and 8 at t = 0.70 and 0.80.
    The obstacle passes the point of the path at s = 0.37, t = 0.74, at the world time 0.3 + 0.74 = 1.04.  At sample 7 it is 2 m/s x 0.04 s = 8 cm from
    that point and at sample 8 12 cm, sideways to a path that the wrist leaves by less than that: every sample is clear.  At t = 0.74 the centres
    coincide: the clearance is -8 mm"""
    return crossing_case(0.37, 0.3 + 0.74), 0.3


def case_b():
    """During the hold.  The plan starts at t_start = 0.3 and ends at the world time 2.3; the obstacle passes the target posture's wrist sphere at
    2.35, 0.05 s after the end.  At the end it is still 2 m/s x 0.05 s = 10 cm away, earlier farther: every sample of the plan is clear, and the plan
    alone (hold_after = 0) is certified clear.  The robot resting at its target is hit at the record time T + 0.05 = 2.05"""
    return crossing_case(1.0, 0.3 + 2.0 + 0.05), 0.3


C_DELAYS = np.array([0.0, 0.5, 1.0])


def case_c():
    """During the wait.  Candidate delays 0, 0.5 and 1 s; the robot waits at its start posture from the world time 0.  The obstacle passes the
    start posture's wrist sphere at 0.25, between the first two candidates; at 0 and at 0.5 it is 2 m/s x 0.25 s = 0.5 m away, so the wait samples of
    mpcmp_start_delay_one see nothing, and the run that starts at 0.5 is clear of an obstacle that is already leaving.  With wait_before = 0.5 the
    certified check sees the crossing at the record time 0.25"""
    return crossing_case(0.0, 0.25)


def test_a_crossing_between_samples_of_the_motion_is_found(M):
    (cc, ts), models = case_a(), robot(1)[0]
    timed = M.clearance_timed_one(models, 4, [cc.table], cc.obs, cc.tracks, cc.x, cc.T, None, ts, 20, 0.0)
    assert timed["status"] == 0 and timed["d_min"] > 0.05, timed
    clr, cert = one(M, 1, 4, cc.obs, cc.tracks, cc.x, cc.T, ts, 0.0, 0.0, 0.0, 0, 4, 2, 10, tables=[cc.table])
    assert clr["status"] & M.CLR_HIT and clr["n_hit"] >= 1 and -0.008 - 1e-12 <= clr["d_min"] < 0.0, (clr, cert)
    assert 0.7 < clr["t_min"] < 0.8 and 0.7 < clr["t_first"] < 0.8 and abs(clr["t_min"] - 0.74) < 0.005
    assert cert["d_lower"] <= clr["d_min"] and clr["sphere"] == 0 and clr["other"] == 0


def test_an_arrival_after_the_plan_is_found_in_the_hold(M):
    (cc, ts), models = case_b(), robot(1)[0]
    for n_pts in (20, 4096):
        timed = M.clearance_timed_one(models, 4, [cc.table], cc.obs, cc.tracks, cc.x, cc.T, None, ts, n_pts, 0.0)
        assert timed["status"] == 0 and timed["d_min"] > 0.09, timed
    clr, cert = one(M, 1, 4, cc.obs, cc.tracks, cc.x, cc.T, ts, 0.0, 0.2, 0.0, 0, 4, 2, 10, tables=[cc.table])
    assert clr["status"] & M.CLR_HIT and clr["d_min"] < 0.0 and clr["t_min"] > cc.T and abs(clr["t_min"] - (cc.T + 0.05)) < 0.005, (clr, cert)
    clr, cert = one(M, 1, 4, cc.obs, cc.tracks, cc.x, cc.T, ts, 0.0, 0.0, 0.0, 0, 4, 2, 10, tables=[cc.table])
    assert clr["status"] == 0 and cert["d_lower"] >= 0.0 and cert["n_undecided"] == 0, (clr, cert)


def test_a_crossing_of_the_waiting_robot_is_found(M):
    cc, models = case_c(), robot(1)[0]
    rec, d_all = M.start_delay_one(models, 4, [cc.table], cc.obs, cc.tracks, cc.x, cc.T, C_DELAYS, None, True, 20, 0.0)
    assert d_all[1] >= 0.0 and rec["index"] in (0, 1), (rec, d_all)           # (the sampled search calls the delay 0.5 clear)
    clr, cert = one(M, 1, 4, cc.obs, cc.tracks, cc.x, cc.T, C_DELAYS[1], C_DELAYS[1] - C_DELAYS[0], 0.0, 0.0, 0, 4, 2, 10, tables=[cc.table])
    assert clr["status"] & M.CLR_HIT and clr["d_min"] < 0.0 and abs(clr["t_min"] - 0.25) < 0.005 and clr["t_min"] < 0.5, (clr, cert)


def test_capacity_with_rest_intervals_and_a_deep_hit(M):
    """n0 = 4096 with the rests: 4 x 1020 motion intervals and 2 x 8 rest intervals.  The graze of the static capacity test (a sphere sliding 1e-5
    above the margin over a floor) makes every motion interval want to be split; the first 2048 of the LEVEL are, wait intervals included in the
    count.  And max_depth 16 on a hit deep in the tree: the obstacle of case (a) passes 5 um inside the touching distance, so that only midpoints
    of level 10 and deeper fall into the crossing"""
    _, arrays, _ = robot(1)
    nseg, n_start, n_rest = 4, 1020, 8
    q0 = np.array([-1.0, -0.5, 0.0, -2.0, 0.0, 1.6, 0.0]); q1 = q0.copy(); q1[0] = 1.0; q1[1] = -0.5 + 1e-5
    tau = M.time_nodes(nseg)
    x = np.zeros((tau.shape[0], 14)); x[:, :7] = q0[None] + (q1 - q0)[None] * tau[:, None]
    table = M.spheres([3], [[0.0, 0.0, 0.0]], 0.05)
    z = [R.frames(arrays[0], R.position(nseg, x, t))[1][3][2] for t in np.linspace(0.0, 1.0, 2001)]
    floor = min(z) - 0.05 - H.MARGIN - 1e-5
    ob = np.array([M.obstacle(M.OBS_HALFSPACE, (0.0, 0.0, 1.0), (floor, 0, 0), 0.0)], dtype=M.OBSTACLE_DTYPE)
    ref = MC.certified_timed_np(arrays, [table], ob, None, nseg, x, 2.0, 0.5, 0.25, 0.75, H.MARGIN, 0, n_start, n_rest, 1)
    assert ref["gap"] > GAP and ref["cert"]["n_eval"] == 4096 + 4096, ref["cert"]
    assert ref["cert"]["n_undecided"] >= 2048 + 4096 - 16 and ref["clr"]["status"] == MC.UNDECIDED, ref["cert"]
    clr, cert = one(M, 1, nseg, ob, None, x, 2.0, 0.5, 0.25, 0.75, H.MARGIN, 0, n_start, n_rest, 1, tables=[table])
    check_records(clr, cert, ref, "capacity")
    cc = crossing_case(0.37, 0.3 + 0.74, lateral=0.008 - 5e-6)
    ref = MC.certified_timed_np(arrays, [cc.table], cc.obs, cc.tracks, 4, cc.x, cc.T, 0.3, 0.1, 0.1, 0.0, 0, 1, 1, 16)
    assert ref["gap"] > GAP and ref["clr"]["status"] & 1 and 10 <= ref["cert"]["depth"] <= 16, (ref["clr"], ref["cert"], ref["gap"])
    clr, cert = one(M, 1, 4, cc.obs, cc.tracks, cc.x, cc.T, 0.3, 0.1, 0.1, 0.0, 0, 1, 1, 16, tables=[cc.table])
    check_records(clr, cert, ref, "deep hit")


def test_nan_records(M):
    case = CASES[3]
    d = case_data(case)
    bad = d["x"][0].copy(); bad[5, 3] = np.nan
    for kw in (dict(x=bad), dict(T=np.inf), dict(ts=np.nan), dict(w=np.inf), dict(h=np.nan)):
        a = dict(x=d["x"][0], T=d["T"][0], ts=d["ts"][0], w=d["w"][0], h=d["h"][0]); a.update(kw)
        clr, cert = one(M, case.narm, case.nseg, d["obs"][0], d["tracks"][0], a["x"], a["T"], a["ts"], a["w"], a["h"], case.margin, 0, 4, 3, 10)
        assert clr["status"] == M.CLR_NAN and np.isnan(clr["d_min"]) and clr["t_min"] == -1.0 and clr["t_first"] == -1.0 and clr["sphere"] == -1
        assert clr["other"] == 0 and clr["n_hit"] == 0 and np.isnan(cert["d_lower"]) and cert["t_lower"] == -1.0
        assert cert["n_eval"] == 0 and cert["n_clear"] == 0 and cert["n_undecided"] == 0 and cert["depth"] == 0
        _, arrays, tables = robot(case.narm)
        check_records(clr, cert, MC.certified_timed_np(arrays, tables, d["obs"][0], d["tracks"][0], case.nseg, a["x"], a["T"], a["ts"], a["w"], a["h"],
                                                       case.margin, 0, 4, 3, 10), "nan")


def test_argument_validation_writes_nothing(M):
    from mpc_motion_planner_amd import capi
    case = CASES[3]
    d = case_data(case)
    models, _, tables = robot(1)
    args, keep = capi._moving_one_args(models, case.nseg, tables, d["obs"][0], d["tracks"][0], d["x"][0])
    f = M.lib().mpcmp_clearance_certified_timed_one

    def call(**kw):
        rec, cert = np.zeros(1, dtype=M.CLEARANCE_DTYPE), np.zeros(1, dtype=M.CLEARANCE_CERT_DTYPE)
        rec["n_hit"] = 77; cert["n_eval"] = 77
        a = dict(T=2.0, ts=0.1, w=0.2, h=0.3, margin=0.02, self_gap=0, n_start=4, n_rest=3, max_depth=10, out=capi.host(rec), cert=capi.host(cert), dt=None)
        a.update(kw)
        lead = list(args)
        if a["dt"] is not None:
            lead[11] = a["dt"]
        rc = f(*lead, a["T"], a["ts"], a["w"], a["h"], a["margin"], a["self_gap"], a["n_start"], a["n_rest"], a["max_depth"], a["out"], a["cert"])
        return rc, bool(rec["n_hit"][0] == 77 and cert["n_eval"][0] == 77)
    assert call() == (0, False) and call(cert=None)[0] == 0
    for what, kw in (("n_rest 0", dict(n_rest=0)), ("n_rest -1", dict(n_rest=-1)), ("n0 4097", dict(n_start=1022, n_rest=5)), ("n_start 0", dict(n_start=0)),
                     ("n_start overflow", dict(n_start=2 ** 30)), ("n_rest overflow", dict(n_rest=2 ** 30)), ("max_depth -1", dict(max_depth=-1)),
                     ("max_depth 17", dict(max_depth=17)), ("wait < 0", dict(w=-1e-9)), ("hold < 0", dict(h=-0.5)), ("margin NaN", dict(margin=float("nan"))),
                     ("self_gap -1", dict(self_gap=-1)), ("dt 0", dict(dt=0.0)), ("no record", dict(out=None))):
        assert call(**kw) == (-1, True), what
    assert call(n_start=1022, n_rest=4, max_depth=0)[0] == 0 and call(max_depth=16, margin=-10.0)[0] == 0


def test_kernel_uses_no_scratch():
    """the compiler's resource remarks of clearance_cert.hip, by the mechanism of tests/test_kernel_resources.py (hipcc cross-compiles: no GPU needed):
    the kernel of this check is k_clearance_cert_timed, the text of k_clearance_cert with a timeline; the static certificate is held to the same"""
    import tempfile
    import test_kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        proc, _ = kr._compile("clearance_cert.hip", [], tmp, "mvc")
        _, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-3000:]
        hit = [(k, v) for k, v in kr._resources(err).items() if "k_clearance_cert" in k]
        assert len(hit) == 2, hit
        for k, v in hit:
            print("%s: %s" % (k, v))
            assert v["scratch"] == 0 and v["vgpr"] <= 160, hit


def test_selftest_under_the_sanitizers(M, tmp_path):
    """examples/moving_cert_selftest.cpp, host part alone (its own main, the host-only unit model_host.cpp, nothing of the GPU) under ASan and UBSan;
    what it prints is a consistent set of records: the world at rest is certified, the swing that meets the pole is a hit between the bounds, and the
    swing that waits for the pole to pass and holds afterwards is certified clear with its closest approach during the wait"""
    import json
    exe = str(tmp_path / "moving_cert_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMPCMP_SELFTEST_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "moving_cert_selftest.cpp"), os.path.join(ROOT, "mpc_motion_planner_amd", "csrc", "model_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rows = json.loads(r.stdout)["host"]
    assert [row[0] for row in rows] == [1, 8]
    for (nseg, still_status, still_d, still_low, still_n, meet_status, meet_d, meet_t, meet_low, meet_n, meet_depth, late_status, late_d, late_t, late_low,
         late_n, late_und) in rows:
        assert still_status == 0 and 0.02 <= still_low <= still_d and still_n >= 4 * nseg
        assert meet_status & 1 and meet_low <= meet_d < 0.02 and 0.0 < meet_t < 2.0 and meet_n > still_n and meet_depth >= 1
        assert late_status == 0 and late_und == 0 and 0.02 <= late_low <= late_d and late_t < 4.0


# ---------------------------------------------------------------------------------------------------------------------------------------------
# Candidates for the selection and problems for the certified start search, shared with the GPU tests
def clean_plan(dq=0.4):
    """the swing of the constructed cases with the second joint dq further back: its wrist stays away from their obstacles"""
    a, b = np.array([-0.9, -0.4 - dq, 0.2, -2.0, 0.1, 1.8, 0.5]), np.array([1.1, -0.4 - dq, 0.2, -1.4, 0.1, 1.8, 0.5])
    return swing(4, a, b)


def search_batch():
    """four problems with one obstacle set each and the candidate delays C_DELAYS, for the certified start search:
    0  case (c): the obstacle crosses the start posture at 0.25.  Every delay but the first has that crossing in its wait (a wait only grows with
       the delay, so no later delay can be certified either); the run that starts at 0 has left the start posture by 2 cm when the obstacle comes;
    1  the obstacle crosses the path point of s = 0.37 at the world time 0.74: the run that starts at 0 meets it between samples 7 and 8, the run that
       starts at 0.5 comes by 0.5 s after it has passed;
    2  the clean plan in the world of problem 1; 3  the plan of problem 1 with the obstacle parked: nothing to meet.
    -> (x [4][13][14], T [4], the sphere table, obs [4][1], tracks = (track_of [4][1], offsets [4][1][3][3], t0, dt))"""
    c0, c1 = crossing_case(0.0, 0.25, t0=-0.5, n_key=3), crossing_case(0.37, 0.74, t0=-0.5, n_key=3)      # (one clock per table: keys at -0.5, 0.5, 1.5)
    off0 = c0.tracks[1]
    far = c1.tracks[1] + np.array([0.0, 0.0, 50.0])
    x = np.stack([c0.x, c1.x, clean_plan(), c1.x])
    T = np.array([c0.T, c1.T, 2.5, c1.T])
    obs = np.stack([c0.obs, c1.obs, c1.obs, c1.obs])
    off = np.stack([off0, c1.tracks[1], c1.tracks[1], far])
    return x, T, c1.table, obs, (np.zeros((4, 1), dtype=np.int32), off, c1.tracks[2], 1.0)


def certified_start_on_the_host(M, x, T, table, obs, tracks, delays, margin=0.0, n_pts=20, max_rounds=4):
    """BatchMotionPlanner.first_certified_start restated with the host statements, one problem at a time: (index [B], status of the last record [B],
    the sampled search's lowest clear delay [B])"""
    models = robot(1)[0]
    index, status, sampled = [], [], []
    for b in range(x.shape[0]):
        trk = (tracks[0][b], tracks[1][b], tracks[2], tracks[3])
        rec, d_all = M.start_delay_one(models, 4, [table], obs[b], trk, x[b], T[b], delays, None, True, n_pts, margin)
        cand = [k for k in range(len(delays)) if not d_all[k] < margin]
        sampled.append(int(rec["index"]))
        got, st = -1, -1
        for k in cand[:max_rounds]:
            clr, _ = M.clearance_certified_timed_one(models, 4, [table], obs[b], trk, x[b], T[b], delays[k], delays[k] - delays[0], 0.0, margin)
            st = int(clr["status"])
            if st == 0:
                got = k
                break
        index.append(got); status.append(st)
    return index, status, sampled


def test_search_batch_on_the_host(M):
    """the expectations the GPU test of first_certified_start relies on, from the host statements alone"""
    x, T, table, obs, tracks = search_batch()
    index, status, sampled = certified_start_on_the_host(M, x, T, table, obs, tracks, C_DELAYS)
    print("certified start on the host: index %s, last status %s, sampled index %s" % (index, status, sampled))
    assert sampled[1] == 0 and index[1] == 1 and status[1] == 0          # the sampled search's delay is skipped, the next one is certified
    assert index[2] == 0 and index[3] == 0 and sampled[2] == 0 and sampled[3] == 0
    assert index[0] == 0 and sampled[0] == 0                              # case (c): the robot that starts at once is gone when the obstacle comes ...
    cc = case_c()
    for tau in (0.0, 0.1, 0.25, 0.7):                                     # problem 0's track on the table's clock is the track of case (c)
        assert np.abs(MC.track_point(tracks[1][0, 0], tracks[2], tracks[3], tau) - MC.track_point(cc.tracks[1][0], cc.tracks[2], cc.tracks[3], tau)).max() < 1e-14
    for k in (1, 2):                                                    # ... and every wait holds the crossing
        assert one(M, 1, 4, cc.obs, cc.tracks, cc.x, cc.T, C_DELAYS[k], C_DELAYS[k], 0.0, 0.0, 0, 4, 4, 10, tables=[cc.table])[0]["status"] & M.CLR_HIT


def selection_case(which):
    """two candidates of one group in the world of a constructed case: the plan that meets the obstacle (the faster one) and the clean plan;
    -> (x [2][13][14], T [2], table, obs, tracks, t_start, wait_before, hold_after)"""
    if which == "a":
        cc, ts = case_a()
        w, h = 0.0, 0.0
    elif which == "b":
        cc, ts = case_b()
        w, h = 0.0, 0.2
    else:
        cc, ts, w, h = case_c(), C_DELAYS[1], C_DELAYS[1] - C_DELAYS[0], 0.0
    return np.stack([cc.x, clean_plan()]), np.array([cc.T, 2.5]), cc.table, cc.obs, cc.tracks, ts, w, h


@pytest.mark.parametrize("which", ["a", "b", "c"])
def test_selection_candidates_on_the_host(M, which):
    """what the GPU test of the selection relies on: sampled, both candidates are clear; certified, the faster one is a hit and the other clear"""
    x, T, table, obs, tracks, ts, w, h = selection_case(which)
    models = robot(1)[0]
    for b, want in ((0, M.CLR_HIT), (1, 0)):
        assert M.clearance_timed_one(models, 4, [table], obs, tracks, x[b], T[b], None, ts, 20, 0.0)["status"] == 0
        clr, cert = one(M, 1, 4, obs, tracks, x[b], T[b], ts, w, h, 0.0, 0, 4, 3, 10, tables=[table])
        assert clr["status"] == want, (which, b, clr, cert)
