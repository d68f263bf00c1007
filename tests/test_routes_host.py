"""CPU-side checks of the via-point routes (include/mpcmp.h, "via-point routes"): the chord rule and the leg / normalised-time rule against NumPy
restatements written here, the argument checks that need no device and the record layouts (the prototypes: tests/test_capi_host.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


# ---- the rules, restated ----
def limits_np(row, narm):
    vlim = np.tile(np.minimum(row["ubx"][7:], -row["lbx"][7:]), narm)
    alim = np.tile(np.minimum(row["ubu"], -row["lbu"]), narm)
    return vlim, alim


def chord_np(pa, pi, pb, row, narm, speed):
    """the chord rule of include/mpcmp.h, as written there"""
    vlim, alim = limits_np(row, narm)
    a, b = pi - pa, pb - pi
    d = np.where((a * b > 0) & (vlim > 0) & (alim > 0), 0.5 * (a + b), 0.0)
    mv = d != 0
    if not mv.any():
        return np.zeros_like(d)
    cap = np.minimum(vlim[mv], np.sqrt(2.0 * alim[mv] * np.minimum(np.abs(a[mv]), np.abs(b[mv]))))
    s = np.min(cap / np.abs(d[mv]))
    return speed * s * d


def locate_np(T, t):
    """smallest m with t < E_m (sequential prefix sums), the last leg if there is none; tau = clamp((t - E_{m-1}) / T_m, 0, 1), 0 for 0 / 0"""
    Ep, m = 0.0, 0
    while True:
        E = Ep + T[m]
        if t < E or m == len(T) - 1:
            break
        Ep, m = E, m + 1
    with np.errstate(all="ignore"):
        x = np.float64(t - Ep) / np.float64(T[m])
    return m, (0.0 if not x > 0 else (1.0 if x > 1 else float(x)))


def _rows(M):
    d = M.bounds_from_config(M.default_config(4, 2))
    g = M.bounds_from_margins(0.9, 0.8, 0.5, 0.9, 0.05)
    lock = g.copy()
    lock["lbx"][2] = lock["ubx"][2] = 0.3          # joint 2 locked: position pinned, zero velocity box
    lock["lbx"][9] = lock["ubx"][9] = 0.0
    return {"default": d, "margins": g, "locked": lock}


def _points(narm, seed):
    r = np.random.default_rng(seed)
    pa = r.uniform(-1.0, 1.0, 7 * narm)
    a = r.uniform(0.05, 0.6, 7 * narm) * r.choice([-1.0, 1.0], 7 * narm)
    b = a * r.uniform(0.3, 2.5, 7 * narm)            # generic: every joint keeps its direction
    return pa, pa + a, pa + a + b


@pytest.mark.parametrize("narm", [1, 2])
@pytest.mark.parametrize("rowname", ["default", "margins", "locked"])
def test_chord_rule_matches_its_restatement(M, narm, rowname):
    row = _rows(M)[rowname]
    vlim, alim = limits_np(row, narm)
    cases = []
    pa, pi, pb = _points(narm, 7)
    cases.append(("generic", pa, pi, pb))
    pr = pb.copy(); pr[1] = pi[1] - (pb[1] - pi[1]); pr[-1] = pi[-1] - (pb[-1] - pi[-1])        # joints that reverse: a_j b_j < 0
    cases.append(("reverse", pa, pi, pr))
    ps = pa.copy(); ps[3] = pi[3]                                                                # a joint at rest before the via: a_j = 0
    cases.append(("rest", ps, pi, pb))
    cases.append(("via equals its neighbour", pa, pa.copy(), pb))
    cases.append(("via equals the next", pa, pb.copy(), pb))
    for name, a, i, b in cases:
        for speed in (0.0, 0.37, 1.0):
            v = M.route_via_velocity(a, i, b, row, narm, speed)
            ref = chord_np(a, i, b, row, narm, speed)
            assert np.all(np.abs(v - ref) <= 1e-13 * np.abs(ref)), (name, speed, v, ref)
            assert np.all(v[ref == 0] == 0), (name, speed)                     # the hard zeros are exact
            da, db = np.abs(i - a), np.abs(b - i)
            assert np.all(np.abs(v) <= vlim), (name, speed)
            assert np.all(v * v <= 2.0 * alim * np.minimum(da, db) * (1.0 + 1e-12)), (name, speed)
            if speed == 0.0 or name.startswith("via equals"):
                assert np.all(v == 0)
        if name == "reverse":
            v = M.route_via_velocity(a, i, b, row, narm, 1.0)
            assert v[1] == 0 and v[-1] == 0 and np.any(v != 0)
        if name == "rest":
            assert M.route_via_velocity(a, i, b, row, narm, 1.0)[3] == 0
    if rowname == "locked":
        v = M.route_via_velocity(pa, pi, pb, row, narm, 1.0)
        assert v[2] == 0 and (narm == 1 or v[9] == 0) and np.any(v != 0)      # the locked joint of every arm stays out of the tangent
    # speed 1 reaches a limit: some joint sits on its velocity limit or on the speed of its shorter chord
    v = M.route_via_velocity(pa, pi, pb, row, narm, 1.0)
    cap = np.minimum(vlim, np.sqrt(2.0 * alim * np.minimum(np.abs(pi - pa), np.abs(pb - pi))))
    assert np.any(np.abs(np.abs(v) - cap) <= 1e-12 * cap)


def test_chord_rule_rejects_bad_arguments(M):
    L, row = M.lib(), _rows(M)["default"]
    p = np.zeros(14); q = np.zeros(14); rp = row.ctypes.data
    ok = lambda *a: L.mpcmp_route_via_velocity(*a)
    assert ok(p.ctypes.data, p.ctypes.data, p.ctypes.data, rp, 1, 1.0, q.ctypes.data) == 0
    assert ok(None, p.ctypes.data, p.ctypes.data, rp, 1, 1.0, q.ctypes.data) == -1
    assert ok(p.ctypes.data, p.ctypes.data, p.ctypes.data, None, 1, 1.0, q.ctypes.data) == -1
    assert ok(p.ctypes.data, p.ctypes.data, p.ctypes.data, rp, 1, 1.0, None) == -1
    for narm in (0, 3):
        assert ok(p.ctypes.data, p.ctypes.data, p.ctypes.data, rp, narm, 1.0, q.ctypes.data) == -1
    for speed in (-0.1, 1.5, float("nan")):
        assert ok(p.ctypes.data, p.ctypes.data, p.ctypes.data, rp, 1, speed, q.ctypes.data) == -1
    bad = p.copy(); bad[3] = np.inf
    assert ok(p.ctypes.data, bad.ctypes.data, p.ctypes.data, rp, 1, 1.0, q.ctypes.data) == -1


def test_locate_matches_its_restatement(M):
    legs = [[1.0, 1.0, 2.0], [0.7], [0.3, 0.0, 1.1], [0.9, 1.3, 0.0], [0.1, 0.2, 0.3, 0.4]]
    for T in legs:
        R = 0.0
        for x in T:
            R += x
        ts = [0.0, R, 0.5 * R, -0.25, R + 1.0] + [i / 17 * R for i in range(18)]
        E = 0.0
        for x in T:
            E += x
            ts += [E, np.nextafter(E, 0.0), np.nextafter(E, 10.0)]
        for t in ts:
            assert M.route_locate(T, t) == locate_np(T, t), (T, t)
    # a junction belongs to the later leg at normalised time 0
    assert M.route_locate([1.0, 1.0, 2.0], 1.0) == (1, 0.0)
    assert M.route_locate([1.0, 1.0, 2.0], 2.0) == (2, 0.0)
    assert M.route_locate([1.0, 1.0, 2.0], 0.0) == (0, 0.0)
    assert M.route_locate([1.0, 1.0, 2.0], 4.0) == (2, 1.0)
    assert M.route_locate([1.0, 1.0, 2.0], 3.0) == (2, 0.5)
    assert M.route_locate([0.7], 0.35) == (0, 0.5)                      # M = 0
    assert M.route_locate([0.3, 0.0, 1.1], 0.3) == (2, 0.0)            # a leg of length 0 holds no time
    L = M.lib()
    T = np.ones(2); leg, tau = C.c_int(0), C.c_double(0)
    assert L.mpcmp_route_locate(0, T.ctypes.data, 0.5, C.addressof(leg), C.addressof(tau)) == -1
    assert L.mpcmp_route_locate(2, None, 0.5, C.addressof(leg), C.addressof(tau)) == -1
    assert L.mpcmp_route_locate(2, T.ctypes.data, 0.5, None, C.addressof(tau)) == -1
    assert L.mpcmp_route_locate(2, T.ctypes.data, 0.5, C.addressof(leg), None) == -1
    assert L.mpcmp_route_locate(2, T.ctypes.data, float("nan"), C.addressof(leg), C.addressof(tau)) == -1


def test_null_context_is_rejected(M):
    """every host-pointer and device-pointer entry point checks its context before anything else: MPCMP_EINVAL without a device"""
    L = M.lib()
    p = np.zeros(64).ctypes.data
    assert L.mpcmp_route_legs(None, 1, 0, p, None, None, None, p, p, p, None) == -1
    assert L.mpcmp_route_legs_device(None, 1, 0, p, None, None, None, p, p, p, None, None) == -1
    assert L.mpcmp_route_join(None, 1, 0, p, p, p, p, None, p, p, p, None) == -1
    assert L.mpcmp_route_join_device(None, 1, 0, p, p, p, p, None, p, p, p, None, None) == -1
    assert L.mpcmp_solve_route_batch(None, 1, 0, p, None, None, None, p, None, p, p, p, None, p, p, p, None) == -1
    assert L.mpcmp_solve_route_batch_device(None, 1, 0, p, None, None, None, p, None, p, p, p, None, p, p, p, None, None) == -1
    assert L.mpcmp_sample_route_batch(None, 1, 0, p, p, p, 10, p) == -1
    assert L.mpcmp_sample_route_batch_device(None, 1, 0, p, p, p, 10, p, None) == -1


def test_struct_layouts_match_the_header(M, tmp_path):
    from mpc_motion_planner_amd import capi
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu %zu\\n", '
                   'sizeof(mpcmp_route_seam), offsetof(mpcmp_route_seam, state_jump_inf), offsetof(mpcmp_route_seam, acc_jump_inf), '
                   'offsetof(mpcmp_route_seam, leg_longest), offsetof(mpcmp_route_seam, leg_first_bad), sizeof(mpcmp_info), sizeof(mpcmp_clearance)); '
                   'return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sz = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    d = capi.ROUTE_SEAM_DTYPE
    assert sz == [d.itemsize] + [d.fields[n][1] for n in ("state_jump_inf", "acc_jump_inf", "leg_longest", "leg_first_bad")] + \
        [capi.INFO_DTYPE.itemsize, capi.CLEARANCE_DTYPE.itemsize], sz


def test_repeat_gives_one_row_per_leg_slot(M):
    rows = np.arange(6.0).reshape(3, 2)
    r = M.Solver.repeat(rows, 2)
    assert r.shape == (9, 2) and np.array_equal(r[::3], rows) and np.array_equal(r[1::3], rows) and np.array_equal(r[2::3], rows)
    b = np.zeros(2, dtype=M.BOUNDS_DTYPE); b["ubu"][1] = 3.0
    rb = M.Solver.repeat(b, 1)
    assert rb.dtype == M.BOUNDS_DTYPE and rb.shape == (4,) and np.all(rb["ubu"][2:] == 3.0) and np.all(rb["ubu"][:2] == 0.0)
    assert np.array_equal(M.Solver.repeat(rows, 0), rows)
