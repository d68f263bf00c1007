"""Clearance in a moving world (include/mpcmp_moving.h), the part that needs no GPU: the host statements mpcmp_track_offset,
mpcmp_clearance_timed_one and mpcmp_start_delay_one against the NumPy reference of tests/moving_reference.py, their rejections, the compiler's
resource remarks of the three kernels and the host part of examples/moving_world_selftest.cpp under the host sanitizers.

The scene, the plans and the comparison helpers below are what tests/test_gpu_moving_world.py checks the kernels with as well.

Bounds, as in tests/test_gpu_clearance.py: d_min within 1e-10 of the reference (the host statement runs the kernels' source; the reference moves the
obstacle where they move the point, so the two differ by rounding); the pair and the sample a record names are checked tie-robustly; n_hit, t_first,
status, index and n_clear are exact for every problem whose reference per-sample minima (the wait samples of the delay search included) keep 1e-9
away from the margin.  The fairness conditions on the reference are asserted by assert_fair / assert_fair_delays in every parity case.
"""
import os
import subprocess

import numpy as np
import pytest

import moving_reference as mr
import oracle_py as o
from test_clearance_host import named_pair_value, scene
from test_gpu_clearance import MARGINS, MARGIN, SEED, moves, world

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 32
# The margin of these cases.  Of the B = 32 moves of test_gpu_clearance.moves about two thirds dip under the floor of world() or graze its other
# obstacles, so at the margin 0.02 of the static tests no scene could leave a quarter clear AND let the tracks change a quarter.  At -0.12 (a hit
# is a penetration of 12 cm: legitimate, the margin is any finite number and the comparison is the same code) 1 to 4 of them hit the world at rest.
MV_MARGIN = -0.12


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


# ---------------------------------------------------------------------------------------------------------------------------------------------
# plans, scene, profiles: shared with the GPU tests
_MOVES = {}


def plans(narm, nseg):
    """the B moves of test_gpu_clearance.moves (sx, sT) with their node controls su, which retiming reads: the same draws in the same order"""
    if (narm, nseg) not in _MOVES:
        sx, sT = moves(narm, nseg, B)
        lim = o.default_limits()
        vmax, amax, jmax = MARGINS[1] * lim["vmax"], MARGINS[2] * lim["amax"], MARGINS[4] * lim["jmax"]
        su = np.zeros((B, 3 * nseg + 1, 7 * narm))
        for b in range(B):
            gen = o.warm_start_jerk if narm == 1 else o.warm_start_jerk_multi
            x, su[b], T = gen(nseg, vmax, amax, jmax, sx[b][0], sx[b][-1])
            assert np.array_equal(x, sx[b]) and T == sT[b]
        _MOVES[(narm, nseg)] = (sx, su, sT)
    return _MOVES[(narm, nseg)]


def robot(M, narm):
    models = list(M.arm_models(M.DUAL_BASES)) if narm == 2 else [M.default_model()]
    return models, [M.link_spheres(m, 0.06, 0.08) for m in models]


# The four tracked obstacles are PARKED far outside the reach (where the tracks-ignored world leaves them) and their tracks carry them through the
# cell: a ball crossing at table height along x at about 0.5 m/s, a pole (capsule) driving past along y, a box on a conveyor along x with a sideways
# wobble that only more than two keys can show, and a ceiling (half-space) that comes down.  Keys span `window` seconds; key j of n_key stands at
# the fraction j / (n_key - 1) of the way (one key: the middle).
PARK = np.array([0.0, 0.0, 5.0])
CEILING = {1: (1.10, 0.70), 2: (1.14, 1.00)}          # height of the ceiling at the first and the last key, per arm count
PRESS = {1: (1.40, 0.70), 2: (1.40, 1.00)}            # ... and of the press of the delay search: its height at the ends and at its flat bottom


def moving_world(M, narm, n_key, window, press=False):
    """-> (obstacle records: world(M, narm) + 4 tracked, tracks = (track_of, offsets [4][n_key][3], t0, dt)).  press: the ceiling is a press that starts
    at once, comes down to a flat bottom and lifts again (the world of the delay search: waiting can help)"""
    cx = 0.0 if narm == 1 else 0.5                       # the middle of the cell
    fr = np.array([0.5]) if n_key == 1 else np.arange(n_key) / (n_key - 1)
    side = 0.35 if narm == 1 else 0.5                    # how far beside the line through the bases the ball and the box pass
    ball = np.stack([cx - 0.9 + 1.8 * fr, np.full_like(fr, side), np.full_like(fr, 0.30)], axis=1)
    pole = np.stack([np.full_like(fr, 0.45 if narm == 1 else 0.5), -0.9 + 1.8 * fr, np.zeros_like(fr)], axis=1)
    box = np.stack([cx + 0.9 - 1.2 * fr, -side + 0.1 * np.sin(2 * np.pi * fr), np.full_like(fr, 0.45)], axis=1)
    h0, h1 = PRESS[narm] if press else CEILING[narm]
    ceil = np.stack([np.zeros_like(fr), np.zeros_like(fr), h0 + (h1 - h0) * (np.minimum(1.0, 2.5 * np.sin(np.pi * fr)) if press else fr)], axis=1)
    rows = [(M.OBS_SPHERE, tuple(PARK), (0, 0, 0), 0.10),
            (M.OBS_CAPSULE, tuple(PARK), tuple(PARK + [0, 0, 0.8]), 0.05),
            (M.OBS_BOX, tuple(PARK), (0.10, 0.20, 0.10), 0.0),
            (M.OBS_HALFSPACE, (0.0, 0.0, -1.0), (-PARK[2], 0, 0), 0.0)]                   # (solid: z >= 5)
    obs = np.concatenate([world(M, narm), scene(M, rows)])
    offsets = np.stack([ball - PARK, pole - PARK, box - PARK, ceil - PARK])
    track_of = np.array([-1, -1, -1, -1, 0, 1, 2, 3], dtype=np.int32)
    dt = window / max(n_key - 1, 1)
    return obs, (track_of, np.ascontiguousarray(offsets), 0.0 if press else 0.25 * window, dt)


def window_of(sT):
    return 0.8 * float(np.mean(sT))


def start_times(sT, seed=SEED + 1):
    return np.random.default_rng(seed).random(sT.shape[0]) * 0.6 * float(np.mean(sT))


def slow_rows(M, n=B):
    """bound rows at 45 % of the velocity limits: the plans run at up to 90 % of them, so every retimed plan is slower than its sol_T"""
    return np.full(n, M.bounds_from_margins(MARGINS[0], 0.45, MARGINS[2], MARGINS[3]), dtype=M.BOUNDS_DTYPE)


def host_profiles(M, models, nseg, sx, su, sT, n_grid=64):
    row = slow_rows(M, 1)[0]
    prof = np.zeros((sx.shape[0], n_grid + 1, 2))
    for b in range(sx.shape[0]):
        prof[b], rec = M.retime_one(models, nseg, row, sx[b], su[b], sT[b], n_grid)
        assert rec["status"] == 0 and rec["T_new"] > sT[b] * 1.05, (b, rec)
    return prof


_SAMPLES = {}


def timed_references(models, tables, wld, nseg, sx, su, sT, prof, t_start, n_pts, margin, self_gap=0, key=None):
    """key: a name under which the plans' samples are kept for the cases that share plans, profiles and n_pts (they do not depend on the world)"""
    out = []
    for b in range(sx.shape[0]):
        pf = None if prof is None else prof[b]
        if key is None or (key, b) not in _SAMPLES:
            _SAMPLES[(key, b)] = mr.plan_samples(models, nseg, sx[b], su[b], sT[b], pf, n_pts)
        t, q = _SAMPLES[(key, b)]
        r = mr.timed_reference(models, tables, wld, q, t, mr.run_time(sT[b], pf), 0.0 if t_start is None else t_start[b], n_pts, margin, self_gap)
        r["t"], r["q"] = t, q
        out.append(r)
    return out


def assert_fair(ref, what=""):
    n = len(ref)
    n_near, n_hit = sum(r["near"] for r in ref), sum(r["status"] for r in ref)
    changed = sum(r["status"] != r["status_rest"] for r in ref)
    assert n_near <= 0.02 * n, "reference %s: %d of %d problems within 1e-9 of the margin" % (what, n_near, n)
    assert n_hit >= n / 4 and n - n_hit >= n / 4, "reference %s: %d of %d problems hit" % (what, n_hit, n)
    assert changed >= n / 4, "reference %s: the tracks change the status of %d of %d problems only" % (what, changed, n)


def check_timed_records(got, ref, T_run, n_pts, what=""):
    """check_records of tests/test_gpu_clearance.py on the running clock"""
    for b, (g, r) in enumerate(zip(got, ref)):
        tag = (what, b)
        assert abs(g["d_min"] - r["d_min"]) <= 1e-10, (tag, g["d_min"], r["d_min"])
        ip = int(round(g["t_min"] / T_run[b] * n_pts))
        assert 0 <= ip <= n_pts and g["t_min"] == (ip / n_pts) * T_run[b], (tag, g["t_min"])
        assert 0 <= g["sphere"] < r["dob"].shape[1], tag
        assert abs(named_pair_value(r["dob"], r["drb"], ip, int(g["sphere"]), int(g["other"])) - r["d_min"]) <= 1e-10, (tag, ip, g["sphere"], g["other"])
        if not r["near"]:
            assert g["n_hit"] == r["n_hit"] and g["t_first"] == r["t_first"] and g["status"] == r["status"], (tag, g, r["n_hit"], r["t_first"])


def delay_grid(K, window):
    """K candidate delays: 0, then equally spaced up to 1.5 windows (the tracks' keys end at 1.25 windows)"""
    return np.zeros(1) if K == 1 else np.linspace(0.0, 1.5 * window, K)


def delay_references(models, tables, wld, nseg, sx, su, sT, prof, n_pts, delays, check_wait, margin, self_gap=0):
    out = []
    for b in range(sx.shape[0]):
        t, q = mr.plan_samples(models, nseg, sx[b], su[b], sT[b], None if prof is None else prof[b], n_pts)
        out.append(mr.delay_reference(models, tables, wld, q, t, delays, check_wait, margin, self_gap))
    return out


def assert_fair_delays(ref, ref_other_wait, K, what=""):
    """ref: the case's own references; ref_other_wait: the same case with the other check_wait value"""
    n = len(ref)
    assert sum(r["near"] for r in ref) <= 0.02 * n, "reference %s: too many problems within 1e-9 of the margin" % what
    if K < 33:
        return
    later, none = sum(r["index"] > 0 for r in ref), sum(r["index"] < 0 for r in ref)
    assert later >= n / 4, "reference %s: waiting helps %d of %d problems only" % (what, later, n)
    assert none >= 1, "reference %s: every problem has a clear delay" % what
    assert sum(a["index"] != c["index"] for a, c in zip(ref, ref_other_wait)) >= 1, "reference %s: check_wait changes no index" % what


def check_delay_records(got, d_all, ref, delays, what=""):
    for b, (g, r) in enumerate(zip(got, ref)):
        tag = (what, b)
        if d_all is not None:
            assert np.abs(d_all[b] - r["d_all"]).max() <= 1e-10, (tag, d_all[b], r["d_all"])
        assert abs(g["d_min"] - r["d_min"]) <= 1e-10 or r["near"], (tag, g["d_min"], r["d_min"])
        if not r["near"]:
            assert g["index"] == r["index"] and g["n_clear"] == r["n_clear"] and g["status"] == r["status"], (tag, g, r["index"], r["n_clear"])
            assert g["delay"] == (delays[r["index"]] if r["index"] >= 0 else -1.0), (tag, g["delay"])


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_track_offset_follows_the_rule(M):
    rng = np.random.default_rng(5)
    P = rng.normal(size=(9, 3))
    t0, dt = 0.25, 0.5                                   # (dyadic: the key times are exact)
    for k in range(9):
        assert np.array_equal(M.track_offset(P, t0, dt, t0 + k * dt), P[k]), k
    for tau in (-7.0, t0 - 1e-9, t0):
        assert np.array_equal(M.track_offset(P, t0, dt, tau), P[0])
    for tau in (t0 + 8 * dt, t0 + 8 * dt + 1e-9, 1e6):
        assert np.array_equal(M.track_offset(P, t0, dt, tau), P[8])
    assert np.array_equal(M.track_offset(P, t0, dt, t0 + 2.5 * dt), 0.5 * P[2] + 0.5 * P[3])
    for tau in (-3.0, 0.0, 1e9):
        assert np.array_equal(M.track_offset(P[4:5], 0.3, 0.7, tau), P[4])       # one key: a constant
    for tau in rng.uniform(-1.0, 6.0, 200):              # a clock that is not dyadic, against the reference
        assert np.abs(M.track_offset(P, 0.3, 0.7, tau) - mr.track_np(P, 0.3, 0.7, tau)).max() <= 1e-13
    out = np.full(3, -7.0)
    f = M.lib().mpcmp_track_offset
    for n_key, a, d, pp, tau, oo in ((0, t0, dt, P, 1.0, out), (1025, t0, dt, P, 1.0, out), (9, np.nan, dt, P, 1.0, out), (9, t0, 0.0, P, 1.0, out),
                                     (9, t0, -1.0, P, 1.0, out), (9, t0, np.inf, P, 1.0, out), (9, t0, dt, P, np.nan, out), (9, t0, dt, None, 1.0, out),
                                     (9, t0, dt, P, 1.0, None)):
        rc = f(n_key, float(a), float(d), None if pp is None else pp.ctypes.data, float(tau), None if oo is None else oo.ctypes.data)
        assert rc == -1 and np.all(out == -7.0), (n_key, a, d, tau)


def test_reference_moves_the_obstacle_as_the_rule_moves_the_point(M):
    """a check of the reference alone: the clearance against the moved obstacle is the formula of include/mpcmp.h at the point moved the other way"""
    from test_clearance_host import host_scene, sd_np
    rng = np.random.default_rng(6)
    cen, rad, p = rng.uniform(-1, 1, (40, 5, 3)), rng.uniform(0.02, 0.1, 5), rng.uniform(-0.5, 0.5, (40, 3))
    for ob in host_scene(M):
        got = mr.moved_clearance(ob, cen, rad, p)
        for i in range(40):
            assert np.abs(got[i] - (sd_np(ob, cen[i] - p[i]) - rad)).max() <= 1e-12, (ob["type"], i)


def test_reference_clock_agrees_with_the_retimed_sampler(M):
    models, tables = robot(M, 1)
    sx, su, sT = plans(1, 4)
    prof = host_profiles(M, models, 4, sx[:4], su[:4], sT[:4])
    for b in range(4):
        t, q = mr.plan_samples(models, 4, sx[b], su[b], sT[b], prof[b], 37)
        for i in range(38):
            assert np.abs(mr.posture_at(4, sx[b], mr.retimed_s(prof[b], sT[b], t[i])) - q[i]).max() <= 1e-12, (b, i)


@pytest.mark.parametrize("narm", [1, 2])
def test_timed_one_matches_the_reference(M, narm):
    nseg, n_pts = 4, 50
    models, tables = robot(M, narm)
    sx, su, sT = plans(narm, nseg)
    prof_all = host_profiles(M, models, nseg, sx, su, sT)
    ts = start_times(sT)
    for n_key in (1, 17):
        obs, tracks = moving_world(M, narm, n_key, window_of(sT))
        wld = mr.World(obs, tracks)
        for prof, t_start in ((None, None), (prof_all, ts)):
            ref = timed_references(models, tables, wld, nseg, sx, su, sT, prof, t_start, n_pts, MV_MARGIN)
            assert_fair(ref, (narm, n_key, prof is not None))
            T_run = sT if prof is None else prof[:, -1, 0]
            got = [M.clearance_timed_one(models, nseg, tables, obs, tracks, sx[b], sT[b], None if prof is None else prof[b],
                                         0.0 if t_start is None else t_start[b], n_pts, MV_MARGIN) for b in range(B)]
            check_timed_records(got, ref, T_run, n_pts, (narm, n_key, prof is not None))
    # no tracks: the world at rest, and a NaN plan
    ref = timed_references(models, tables, mr.World(obs), nseg, sx[:4], su[:4], sT[:4], None, None, n_pts, MV_MARGIN)
    got = [M.clearance_timed_one(models, nseg, tables, obs, None, sx[b], sT[b], None, 0.0, n_pts, MV_MARGIN) for b in range(4)]
    check_timed_records(got, ref, sT, n_pts, "rest")
    bad = sx[0].copy(); bad[3, 2] = np.nan
    for r in (M.clearance_timed_one(models, nseg, tables, obs, tracks, bad, sT[0]), M.clearance_timed_one(models, nseg, tables, obs, tracks, sx[0], np.inf),
              M.clearance_timed_one(models, nseg, tables, obs, tracks, sx[0], sT[0], t_start=np.nan),
              M.clearance_timed_one(models, nseg, tables, obs, tracks, sx[0], sT[0], prof=np.full((9, 2), np.nan))):
        assert r["status"] == M.CLR_NAN and np.isnan(r["d_min"]) and r["t_min"] == -1.0 and r["sphere"] == -1 and r["n_hit"] == 0


@pytest.mark.parametrize("narm", [1, 2])
def test_start_delay_one_matches_the_reference(M, narm):
    nseg, n_pts = 4, 50
    models, tables = robot(M, narm)
    sx, su, sT = plans(narm, nseg)
    w = window_of(sT)
    obs, tracks = moving_world(M, narm, 17, w, press=True)
    wld = mr.World(obs, tracks)
    prof_all = host_profiles(M, models, nseg, sx, su, sT)
    for K, prof in ((33, None), (33, prof_all), (2, None), (1, None)):
        delays = delay_grid(K, w)
        refs = {cw: delay_references(models, tables, wld, nseg, sx, su, sT, prof, n_pts, delays, cw, MV_MARGIN) for cw in (False, True)}
        for cw in (False, True):
            assert_fair_delays(refs[cw], refs[not cw], K, (narm, K, cw))
            got = [M.start_delay_one(models, nseg, tables, obs, tracks, sx[b], sT[b], delays, None if prof is None else prof[b], cw, n_pts, MV_MARGIN)
                   for b in range(B)]
            check_delay_records([g[0] for g in got], np.array([g[1] for g in got]), refs[cw], delays, (narm, K, cw))
    rec, d_all = M.start_delay_one(models, nseg, tables, obs, tracks, sx[0], np.nan, delay_grid(2, w))
    assert rec["status"] == M.CLR_NAN and rec["index"] == -1 and rec["delay"] == -1.0 and rec["n_clear"] == 0 and np.isnan(d_all).all()


def test_host_statements_reject_bad_arguments(M):
    models, tables = robot(M, 1)
    sx, su, sT = plans(1, 4)
    obs, tracks = moving_world(M, 1, 3, 1.0)
    ok = M.clearance_timed_one(models, 4, tables, obs, tracks, sx[0], sT[0], n_pts=10)
    assert ok["status"] in (0, 1)
    tof, off, t0, dt = tracks
    bad_tof = tof.copy(); bad_tof[5] = 4
    low_tof = tof.copy(); low_tof[0] = -2
    bad_off = off.copy(); bad_off[1, 2, 0] = np.inf
    for what, kw in (("track_of past the tracks", dict(tracks=(bad_tof, off, t0, dt))), ("track_of -2", dict(tracks=(low_tof, off, t0, dt))),
                     ("offset inf", dict(tracks=(tof, bad_off, t0, dt))), ("dt 0", dict(tracks=(tof, off, t0, 0.0))),
                     ("dt < 0", dict(tracks=(tof, off, t0, -1.0))), ("t0 NaN", dict(tracks=(tof, off, np.nan, dt))),
                     ("65 tracks", dict(tracks=(tof, np.zeros((65, 3, 3)), t0, dt))), ("1025 keys", dict(tracks=(tof, np.zeros((4, 1025, 3)), t0, dt))),
                     ("n_pts 0", dict(n_pts=0)), ("n_pts 4097", dict(n_pts=4097)), ("margin NaN", dict(margin=np.nan)), ("self_gap -1", dict(self_gap=-1)),
                     ("n_grid 4097", dict(prof=np.ones((4098, 2))))):
        a = dict(tracks=tracks, n_pts=10, margin=0.0, self_gap=0, prof=None)
        a.update(kw)
        with pytest.raises(M.MpcmpError):
            M.clearance_timed_one(models, 4, tables, obs, a["tracks"], sx[0], sT[0], a["prof"], 0.0, a["n_pts"], a["margin"], a["self_gap"])
    for what, delays in (("no delays", []), ("257 delays", np.arange(257.0)), ("descending", [0.0, 1.0, 0.5]), ("negative", [-0.1, 0.0]),
                         ("NaN", [0.0, np.nan]), ("inf", [0.0, np.inf])):
        with pytest.raises(M.MpcmpError):
            M.start_delay_one(models, 4, tables, obs, tracks, sx[0], sT[0], delays, n_pts=10)
    rec, _ = M.start_delay_one(models, 4, tables, obs, tracks, sx[0], sT[0], [0.0, 0.0, 0.5], n_pts=10)       # (equal delays are ascending)
    assert rec["status"] in (0, 1)


def test_record_layout_matches_the_header(M, tmp_path):
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu %d %d %d\\n", '
                   'sizeof(mpcmp_start_delay), offsetof(mpcmp_start_delay, index), offsetof(mpcmp_start_delay, n_clear), '
                   'offsetof(mpcmp_start_delay, status), MPCMP_MAX_TRACKS, MPCMP_MAX_TRACK_KEYS, MPCMP_MAX_DELAYS); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sz = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    D = M.START_DELAY_DTYPE
    assert sz == [D.itemsize, D.fields["index"][1], D.fields["n_clear"][1], D.fields["status"][1], M.MAX_TRACKS, M.MAX_TRACK_KEYS, M.MAX_DELAYS], sz


def test_every_declared_function_is_in_the_abi_table(M):
    import re
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_moving.h")).read(), flags=re.S)
    names = re.findall(r"\bint\s+(mpcmp_\w+)\s*\(", hdr)
    assert names == list(capi.ABI_MOVING) and len(names) == 11
    for name in names:
        args = re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, hdr).group(1).split(",")
        kinds = "".join("p" if "*" in a else ("d" if "double" in a else "i") for a in args)
        assert kinds == capi.ABI_MOVING[name], (name, kinds, capi.ABI_MOVING[name])
        assert hasattr(M.lib(), name)


def test_moving_kernels_use_no_scratch():
    """the compiler's resource remarks of moving.hip, by the mechanism of tests/test_kernel_resources.py (hipcc cross-compiles: no GPU needed)"""
    import tempfile
    import test_kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        proc, _ = kr._compile("moving.hip", [], tmp, "mv")
        _, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-3000:]
        res = kr._resources(err)
        for kernel in ("k_clearance_timed", "k_start_delay", "k_sphere_tracks"):
            hit = [(k, v) for k, v in res.items() if kernel in k]
            assert len(hit) == 1, (kernel, list(res))
            v = hit[0][1]
            print("%s: %d VGPRs, %d B of scratch per lane" % (kernel, v["vgpr"], v["scratch"]))
            assert v["scratch"] == 0 and v["vgpr"] <= 160, (kernel, v)


def test_selftest_under_the_sanitizers(M, tmp_path):
    """examples/moving_world_selftest.cpp, host part alone (its own main, the host-only unit model_host.cpp, nothing of the GPU) under ASan and
    UBSan; what it prints is a consistent set of records: the pole hits the swing that starts at 0.25 s, the retimed swing is past it, and the first
    clear delay is the second candidate"""
    import json
    exe = str(tmp_path / "moving_world_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMPCMP_SELFTEST_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "moving_world_selftest.cpp"), os.path.join(ROOT, "mpc_motion_planner_amd", "csrc", "model_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    rows = json.loads(r.stdout)["host"]
    assert [row[0] for row in rows] == [1, 8]
    for (nseg, still_status, still_d, mv_status, mv_d, mv_t, slow_status, slow_d, slow_t, index, n_clear, delay, d_min, index_w, status_w, d_at) in rows:
        assert still_status == 0 and still_d > 0.3 and mv_status == 1 and mv_d < 0.02 and 0.0 < mv_t < 2.0
        assert slow_status == 0 and 0.0 < slow_t < 4.0 and mv_d < slow_d < still_d
        assert index == 1 and delay == 0.5 and n_clear == 5 and d_min == d_at >= 0.02 and index_w == 1 and status_w == 0
