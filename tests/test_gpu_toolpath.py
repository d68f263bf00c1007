"""Tool-line moves on the GPU (include/mpcmp_toolpath.h): k_tool_line and k_tool_deviation against the NumPy restatement of
tests/toolpath_reference.py, with the builders, fair-test conditions and measured parity bounds of tests/test_toolpath_host.py; then what the
feature is for: line move -> limits -> retime to the limits -> sample on a physical clock, all on the GPU.

Measured bounds and the largest GPU-to-reference differences seen: DESIGN.md, "Tool-line moves"; run with -s, every case prints its own."""
import json
import os
import subprocess

import numpy as np
import pytest

import retime_reference as RR
import toolpath_reference as R
from test_retime_host import check_limits_hold
from test_toolpath_host import NL, assert_fair, case, check_deviation, check_line, clean_properties, draw, robots, row_of, special_lines

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1
MARGINS = (0.9, 0.9, 0.5, 0.9)
CHUNK = 64           # samples per pass of k_tool_deviation (TD_NT, csrc/toolpath.hpp)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


def solver(M, nseg, max_batch=130, narm=1):
    """(margins 1: the position rows of test_toolpath_host.row_of)"""
    return M.Solver(M.default_config(nseg, 1), max_batch, models=M.arm_models(M.DUAL_BASES) if narm == 2 else None)


def batch(name, B):
    """B lines: the 32 drawn ones over and over, the four special lines in the last four places"""
    q, R1, p1 = draw(name)
    idx = np.arange(B) % NL
    q, R1, p1 = q[idx].copy(), R1[idx].copy(), p1[idx].copy()
    sq, sR, sp = special_lines(name)
    q[-4:], R1[-4:], p1[-4:] = sq, sR, sp
    return idx, q, R1, p1


@pytest.mark.parametrize("nseg,n_sub", [(1, 4), (4, 4), (8, 4), (4, 1)])
def test_parity_with_the_numpy_reference(M, nseg, n_sub):
    ref, amp, bound = case("panda", nseg, n_sub)
    assert_fair(ref)
    s = solver(M, nseg)
    spec = M.tool_line_spec(n_sub=n_sub)
    worst = {}
    first = None
    for B in (33, 130):
        idx, q, R1, p1 = batch("panda", B)
        sx, su, sT, rec = s.tool_line(q, R1, p1, spec=spec)
        for b in range(B - 4):
            check_line(ref[idx[b]], bound, sx[b], su[b], sT[b], rec[b], (nseg, n_sub, B, b), worst)
        if first is None:
            first = (sx, su, sT, rec)
            clean = [b for b in range(B - 4) if not ref[idx[b]]["status"] and not ref[idx[b]]["near"]]
            for b in clean[:6]:
                clean_properties("panda", nseg, ref[idx[b]], sx[b], su[b], sT[b])
            for n_pts in (1, 200, CHUNK - 1, CHUNK, CHUNK + 1):
                dev = s.tool_deviation(sx, R1, p1, n_pts, 1e-4, 1e-4)
                for b in range(B):
                    check_deviation("panda", nseg, sx[b], R1[b], p1[b], n_pts, dev[b], 1e-4, 1e-4, (nseg, n_pts, b))
        else:
            # a line is the same plan wherever it stands: the second batch repeats the first bit for bit, block after block
            for b in range(B - 4):
                f = idx[b]
                w = first if f < 33 - 4 else (sx, su, sT, rec)         # (the last four places of the first batch hold the special lines)
                assert sx[b].tobytes() == w[0][f].tobytes() and su[b].tobytes() == w[1][f].tobytes() and sT[b] == w[2][f], (B, b)
                assert rec[b].tobytes() == w[3][f].tobytes(), (B, b)
            for a, b in zip(range(B - 4, B), range(33 - 4, 33)):
                assert sx[a].tobytes() == first[0][b].tobytes() and rec[a].tobytes() == first[3][b].tobytes()
    print("GPU tool line num_seg %d n_sub %d: largest differences from the reference q %.2e v %.2e u %.2e (bounds %.2e %.2e %.2e)"
          % (nseg, n_sub, worst["q"], worst["v"], worst["u"], bound["q"], bound["v"], bound["u"]))


def test_special_lines(M):
    s = solver(M, 4)
    q, R1, p1 = special_lines("panda")
    sx, su, sT, rec = s.tool_line(q, R1, p1)
    assert rec["status"][0] == 0 and rec["status"][1] == 0 and rec["status"][2] == 0 and rec["status"][3] & M.TL_STOPPED
    assert sT[2] == 0.2 and np.abs(sx[2, :, :7] - q[2]).max() <= 1e-14 and np.isfinite(sx[2]).all()
    k = rec["k_fail"][3]
    assert 0 < k < 13 and np.isnan(sx[3, k:]).all() and np.isnan(su[3, k:]).all() and np.isfinite(sx[3, :k]).all()
    # the downstream checkers answer the NaN nodes with their own NaN bits
    assert s.limits(sx, su, sT, 50)["status"][3] == M.LIM_NAN and s.retime(sx, su, sT, 50)[1]["status"][3] == M.RT_NAN
    assert s.tool_deviation(sx, R1, p1, 50)["status"][3] == M.TL_NAN


def test_two_arms_write_one_arm_and_share_T(M):
    nseg = 6
    ref, amp, bound = case("dual1", nseg, 4)
    assert_fair(ref)
    s = solver(M, nseg, 64, narm=2)
    q, R1, p1 = draw("dual1")
    N = 3 * nseg + 1
    rng = np.random.default_rng(3)
    sx, su = rng.normal(size=(NL, N, 28)), rng.normal(size=(NL, N, 14))
    sT = np.array([r["T"] for r in ref]) * rng.uniform(1.0, 2.0, NL)
    keep = (sx.copy(), su.copy(), sT.copy())
    ref_T = [R.tool_line_np(robots("dual1")[1], nseg, row_of(M)["lbx"][:7], row_of(M)["ubx"][:7], q[b], R1[b], p1[b], sT[b]) for b in range(NL)
             if not ref[b]["status"]][:4]
    with pytest.raises(M.MpcmpError) as e:
        s.tool_line(q, R1, p1, None, arm=1, out=(sx, su, sT))
    assert e.value.code == EINVAL and sx.tobytes() == keep[0].tobytes() and sT.tobytes() == keep[2].tobytes()
    _, _, _, rec = s.tool_line(q, R1, p1, sT, arm=1, out=(sx, su, sT))
    assert sT.tobytes() == keep[2].tobytes()                                  # the shared T is honoured ...
    assert np.array_equal(sx[:, :, :7], keep[0][:, :, :7]) and np.array_equal(sx[:, :, 14:21], keep[0][:, :, 14:21])      # ... and arm 0 untouched
    assert np.array_equal(su[:, :, :7], keep[1][:, :, :7])
    i = 0
    for b in range(NL):
        x = np.concatenate([sx[b, :, 7:14], sx[b, :, 21:28]], axis=1)
        r = ref[b]
        if not r["near"]:
            assert rec[b]["status"] == r["status"] and rec[b]["k_fail"] == r["k_fail"], (b, rec[b])
        if not r["status"]:
            assert np.abs(x[:, :7] - r["x"][:, :7]).max() <= bound["q"], b       # (the path does not depend on T)
            if i < len(ref_T):
                check_line(ref_T[i], bound, x, su[b, :, 7:], sT[b], rec[b], ("two arms", b)); i += 1
    dev = s.tool_deviation(sx, R1, p1, 100, arm=1)
    for b in range(NL):
        check_deviation("dual1", nseg, np.concatenate([sx[b, :, 7:14], sx[b, :, 21:28]], axis=1), R1[b], p1[b], 100, dev[b], what=("two arms", b))


def test_a_plan_does_not_depend_on_its_place_in_the_batch(M):
    s = solver(M, 4)
    idx, q, R1, p1 = batch("panda", 70)
    sx, su, sT, rec = s.tool_line(q, R1, p1)
    dev = s.tool_deviation(sx, R1, p1, 150, 1e-4, 1e-4)
    perm = np.random.default_rng(5).permutation(70)
    px, pu, pT, prec = s.tool_line(q[perm], R1[perm], p1[perm])
    pdev = s.tool_deviation(px, R1[perm], p1[perm], 150, 1e-4, 1e-4)
    for i, b in enumerate(perm):
        assert px[i].tobytes() == sx[b].tobytes() and pu[i].tobytes() == su[b].tobytes() and pT[i] == sT[b] and prec[i].tobytes() == rec[b].tobytes()
        assert pdev[i].tobytes() == dev[b].tobytes()
    for b in (7, 40, 66):          # alone, first and last
        for sel in ([b], [b] + list(range(20)), list(range(33)) + [b]):
            ax, au, aT, arec = s.tool_line(q[sel], R1[sel], p1[sel])
            adev = s.tool_deviation(ax, R1[sel], p1[sel], 150, 1e-4, 1e-4)
            j = sel.index(b) if sel[0] == b else len(sel) - 1
            assert ax[j].tobytes() == sx[b].tobytes() and au[j].tobytes() == su[b].tobytes() and aT[j] == sT[b] and arec[j].tobytes() == rec[b].tobytes()
            assert adev[j].tobytes() == dev[b].tobytes()


def test_bound_rows_and_argument_validation(M):
    s = solver(M, 4, 40)
    idx, q, R1, p1 = batch("panda", 36)
    sx, su, sT, rec = s.tool_line(q, R1, p1)
    rows = s.bounds_table(36)
    tight = [b for b in range(32) if rec["status"][b] == 0][::2]
    for b in tight:                          # these problems' rows end 0.01 rad inside the path of joint 3
        rows["ubx"][b][3] = sx[b, :, 3].max() - 0.01
    s.set_bounds(rows)
    _, _, _, rrec = s.tool_line(q, R1, p1)
    for b in range(32):
        if rec["status"][b] == 0:
            assert (abs(rrec["q_excess"][b] - 0.01) <= 1e-12 and rrec["status"][b] == M.TL_Q_OUT_OF_BOUNDS) if b in tight else \
                (rrec["q_excess"][b] == rec["q_excess"][b] and rrec["status"][b] == 0), (b, rrec[b])
    s.set_bounds(rows[:20])
    out = (np.full_like(sx, 7.5), np.full_like(su, 7.5), np.full_like(sT, 7.5))

    def refused(**kw):
        a = dict(q_start=q, R=R1, p=p1, T=None, spec=None, arm=0, out=out); a.update(kw)
        with pytest.raises(M.MpcmpError) as e:
            s.tool_line(**a)
        assert e.value.code == EINVAL and all((o == 7.5).all() for o in out), kw
    refused()                                                       # more problems than rows
    s.clear_bounds()
    refused(arm=1); refused(arm=-1)
    refused(q_start=q * np.where(np.arange(7) == 2, np.nan, 1.0))
    refused(R=R1 * 1.01); refused(p=p1 + np.inf)
    refused(R=np.array([R.fk(robots("panda")[1], q[b])[0] @ R.exp3(np.array([0.0, np.pi - 5e-4, 0.0])) for b in range(36)]))
    refused(T=np.full(36, np.nan))
    for field, v in (("n_sub", 0), ("n_sub", 65), ("damp", 0.0), ("eps", np.nan), ("manip_min", -1.0), ("T_min", np.inf), ("tool_lin_max", 0.0)):
        spec = M.tool_line_spec(); spec[field] = v
        refused(spec=spec)
    from mpc_motion_planner_amd.capi import host
    f = M.lib().mpcmp_tool_line_batch
    for B in (0, 41):
        assert f(s._ctx, B, 0, host(q), host(R1.reshape(36, 9)), host(p1), None, None, host(out[0]), host(out[1]), host(out[2]), None) == EINVAL
    assert f(s._ctx, 36, 0, None, host(R1.reshape(36, 9)), host(p1), None, None, host(out[0]), host(out[1]), host(out[2]), None) == EINVAL
    assert f(s._ctx, 36, 0, host(q), host(R1.reshape(36, 9)), host(p1), None, None, host(out[0]), host(out[1]), None, None) == EINVAL
    assert all((o == 7.5).all() for o in out)
    dev = np.zeros(36, dtype=M.TOOL_DEV_DTYPE); dev["n_over"] = 77
    g = M.lib().mpcmp_tool_deviation_batch
    for a in ((0, 0, host(sx), 10, 1.0), (41, 0, host(sx), 10, 1.0), (36, 1, host(sx), 10, 1.0), (36, 0, None, 10, 1.0), (36, 0, host(sx), 0, 1.0),
              (36, 0, host(sx), 10, -1.0), (36, 0, host(sx), 10, float("nan"))):
        assert g(s._ctx, a[0], a[1], a[2], host(R1.reshape(36, 9)), host(p1), a[3], a[4], 1.0, host(dev)) == EINVAL and (dev["n_over"] == 77).all(), a
    # after all that the context plans as before
    again = s.tool_line(q, R1, p1)
    assert again[0].tobytes() == sx.tobytes() and again[3].tobytes() == rec.tobytes()


def test_a_solve_is_untouched_by_tool_lines(M):
    from mpc_motion_planner_amd import scenarios
    cfg = M.default_config(4, 2, margins=MARGINS)
    x0, xf = scenarios.make_batch(6, MARGINS + (0.1,))
    plain = M.Solver(cfg, 36).solve(x0, xf)
    s = M.Solver(cfg, 36)
    got = s.solve(x0, xf)
    idx, q, R1, p1 = batch("panda", 36)
    sx, su, sT, rec = s.tool_line(q, R1, p1)
    s.tool_deviation(sx, R1, p1, 100)
    again = s.solve(x0, xf)
    for a, b, c in zip(plain, got, again):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    # ... and a clean line is a legal start guess
    b = int(np.argmax(rec["status"] == 0))
    x0b = sx[b:b + 1, 0].copy(); xfb = sx[b:b + 1, -1].copy()
    info = s.solve(x0b, xfb, (sx[b:b + 1], su[b:b + 1], sT[b:b + 1]))[3]
    assert not info["status"][0] & M.STATUS_HARD


@pytest.mark.parametrize("nseg", [4, 8])
def test_line_to_limits_to_retime_to_samples(M, nseg):
    """the chain the feature is for, on the clean lines.  Tool maxima 0.5 m/s and 0.8 rad/s: the duration rule then makes these short lines slower
    than the joints need, which is what retiming with rate_max 4 wins back"""
    lin_max, ang_max, n_grid = 0.5, 0.8, 100
    ref = case("panda", nseg, 4)[0]
    pick = [b for b in range(NL) if not ref[b]["status"] and not ref[b]["near"]]
    q, R1, p1 = [a[pick] for a in draw("panda")]
    B = len(pick)
    s = M.Solver(M.default_config(nseg, 1), 64)
    table = np.repeat(M.bounds_from_config(s.cfg).reshape(1), B)
    sx, su, sT, rec = s.tool_line(q, R1, p1, spec=M.tool_line_spec(lin_max, ang_max))
    assert (rec["status"] == 0).all()
    dev = s.tool_deviation(sx, R1, p1, 200)
    lim = s.limits(sx, su, sT, 200, None, lin_max, ang_max)
    # (the nominal plan meets the tool maxima at mid-move; what the interpolant adds to that is for retiming to take away)
    assert not (lim["status"] & M.LIM_NAN).any()
    print("num_seg %d: tool-speed excess of the interpolant over the maxima: linear %.2e m/s, angular %.2e rad/s"
          % (nseg, lim["excess"][:, M.LIM_TOOL_LIN].max(), lim["excess"][:, M.LIM_TOOL_ANG].max()))
    prof, rt = s.retime(sx, su, sT, n_grid, M.retime_spec(lin_max, ang_max, 4.0))
    assert (rt["status"] == 0).all(), rt["status"]             # every clean line can be retimed: it is at rest at both ends and inside its limits when slowed
    feasible = list(range(B))
    out = s.sample_retimed(sx, su, sT, prof, 60)
    m = robots("panda")[1]
    mdl = [robots("panda")[0]]
    faster = 0
    for b in feasible:
        P = RR.path_values(mdl, nseg, sx[b], su[b], sT[b], n_grid)
        check_limits_hold(dict(P=P, T=sT[b]), table[b], prof[b, :, 1], lin_max, ang_max, what=b)
        d = p1[b] - ref[pick[b]]["p0"]
        for i in range(61):
            p = R.fk(m, out[b, i, 1:8])[1] - ref[pick[b]]["p0"]
            off = np.linalg.norm(p - (p @ d) / (d @ d) * d)
            assert off <= dev["lin_max"][b] + 1e-9, (b, i, off, dev["lin_max"][b])
        assert abs(out[b, -1, 0] - rt["T_new"][b]) <= 1e-12 * rt["T_new"][b]
        faster += rt["T_new"][b] < sT[b] - 1e-3 * sT[b]
    print("num_seg %d: %d of %d lines retimed, %d faster than the tool-speed rule; median T_new / T %.3f" % (nseg, len(feasible), B, faster, np.median(rt["T_new"][feasible] / sT[feasible])))
    assert faster >= 4, faster


def test_planner_members(M):
    p = M.BatchMotionPlanner(max_batch=8, num_seg=4, sqp_iters=2)
    q, R1, p1 = [a[:4] for a in draw("panda")]
    p.set_current_state(q, np.zeros((4, 7)))
    rec = p.plan_tool_line(R1, p1)
    s = M.Solver(M.default_config(4, 2), 8)
    sx, su, sT, want = s.tool_line(q, R1, p1)
    assert rec.tobytes() == want.tobytes() and p.solution()[0].tobytes() == sx.tobytes()
    assert p.check_tool_line(100, 1e-4, 1e-4).tobytes() == s.tool_deviation(sx, R1, p1, 100, 1e-4, 1e-4).tobytes()
    assert p.check_limits(50).tobytes() == s.limits(sx, su, sT, 50).tobytes()
    prof, rt = p.retime(50)
    assert prof.tobytes() == s.retime(sx, su, sT, 50)[0].tobytes()
    assert p.get_retimed_trajectory(20).tobytes() == s.sample_retimed(sx, su, sT, prof, 20).tobytes()
    assert p.get_MPC_trajectory(20)[1].tobytes() == s.sample(sx, su, sT, 20)[..., 1:8].tobytes()


def test_cpp_shim_members(M, tmp_path):
    """examples/tool_line_selftest.cpp builds with plain g++ -Wall -Werror and prints consistent records"""
    exe = str(tmp_path / "tool_line_selftest")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "tool_line_selftest.cpp"), "-L" + os.path.join(ROOT, "mpc_motion_planner_amd"), "-lmpcmp",
                           "-Wl,-rpath," + os.path.join(ROOT, "mpc_motion_planner_amd"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    o = json.loads(r.stdout)
    assert o["tl_status"] == 0 and o["k_fail"] == -1 and o["err_max"] <= 1e-9 and o["manip_min"] >= 1e-3 and o["q_excess"] < 0.0
    assert abs(o["T"] - max(1.875 * 0.15 / 1.7, 0.2)) <= 1e-12                          # a pure translation: the linear term of the rule, or T_min
    assert 0.0 < o["dev_perp"] <= o["dev_lin"] < 1e-4 and o["dev_ang"] < 1e-4 and o["dev_n_over"] == 0 and o["dev_status"] == 0
    assert o["lim_status"] & 128 == 0 and o["rt_status"] == 0 and 0.0 < o["rt_T_new"] < 10.0 * o["T"]
    assert o["rt_off_line"] <= o["dev_lin"] + 1e-9 and abs(o["rt_rise"] - 0.15) <= 1e-9 and abs(o["t_last"] - o["T"]) <= 1e-12
