"""Batched tool-pose targets on the GPU (mpcmp_pose_targets_batch[_device], include/mpcmp.h): multi-start DLS inverse kinematics, the choice
of one start per problem under the joint bounds, the joint velocity of a tool twist, and the target written into xf.  The reference is the
host path: mpcmp_inverse_kinematics per start (the same DLS step: kinematics_host.hpp), the wrap and choice rules restated in numpy, and
mpcmp_inverse_velocities.  Poses come from forward kinematics of random in-bounds configurations."""
import ctypes as C

import numpy as np
import pytest

MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)
TWO_PI = 2.0 * np.pi
EPS = 1e-4
# fraction of the end-to-end batch (B = 512, S = 16, margins above) whose IK target has status 0; measured on an MI355X: 468 / 512 = 0.914
MIN_IK_OK = 0.90


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def _cfg(M, nseg=4, sqp=3):
    return M.default_config(nseg, sqp, margins=MARGINS)


def _poses(M, model, q):
    R = np.zeros((len(q), 3, 3)); p = np.zeros((len(q), 3))
    for b in range(len(q)):
        _, p[b], R[b] = M.tool_jacobian(model, q[b])
    return R, p


def _true_q(M, B, off):
    from mpc_motion_planner_amd import scenarios
    return scenarios.sample_states(B, MARGINS, stream_offset=off)[:, :7]


def _wrap(q, lo, hi):
    """rule 2 of include/mpcmp.h in numpy"""
    klo, khi = np.ceil((lo - q) / TWO_PI), np.floor((hi - q) / TWO_PI)
    k = np.where(klo > 0, klo, np.where(khi < 0, khi, 0.0))
    k = np.where(klo > khi, 0.0, k)
    return q + TWO_PI * k


def _host_runs(M, model, R, p, seeds, lo, hi):
    """mpcmp_inverse_kinematics for every (problem, start): wrapped q [B][S][7], converged [B][S], iterations [B][S]"""
    B, S = seeds.shape[:2]
    q = np.zeros((B, S, 7)); conv = np.zeros((B, S), dtype=bool); its = np.zeros((B, S), dtype=int)
    for b in range(B):
        for s in range(S):
            q[b, s], conv[b, s], its[b, s] = M.inverse_kinematic(model, R[b], p[b], seeds[b, s])
    return _wrap(q, lo, hi), conv, its


def _bounds(cfg):
    return np.array(cfg.lbx[:7]), np.array(cfg.ubx[:7]), np.array(cfg.lbx[7:14]), np.array(cfg.ubx[7:14])


def _choose(q, conv, err, lo, hi, q_ref=None):
    """rule 4 of include/mpcmp.h in numpy for one problem: q [S][7] wrapped, conv [S], err [S] -> chosen start"""
    qual = conv & np.all((q >= lo) & (q <= hi), axis=1)
    if qual.any():
        if q_ref is None:
            return int(np.argmax(qual))
        d = np.where(qual, ((q - q_ref) ** 2).sum(axis=1), np.inf)
        return int(np.argmin(d))                   # argmin: ties to the lowest index
    e = np.where(np.isnan(err), np.inf, err)
    return int(np.argmin(e))


@pytest.mark.gpu
def test_per_start_parity_with_host(M):
    """S = 1: the device start is the host start (same DLS step; FMA contraction is the only difference), wrapped by rule 2"""
    B = 256
    cfg = _cfg(M); model = M.default_model(); lo, hi, _, _ = _bounds(cfg)
    qt = _true_q(M, B, 300)
    R, p = _poses(M, model, qt)
    rng = np.random.default_rng(7)
    seeds = (qt + rng.uniform(-0.3, 0.3, qt.shape))[:, None, :]
    s = M.Solver(cfg, B)
    xf, info = s.pose_targets(R, p, seeds)
    qh, conv, its = _host_runs(M, model, R, p, seeds, lo, hi)
    same = info["iters"] == its[:, 0]
    assert same.mean() >= 0.99, (same.mean(), np.nonzero(~same))
    dq = np.abs(xf[:, :7] - qh[:, 0]).max(axis=1)
    print("per-start parity: iterations equal for %d / %d, worst |dq|_inf %.3g where equal" % (same.sum(), B, dq[same].max()))
    assert dq[same].max() <= 1e-8
    assert (info["seed"] == 0).all()
    st_conv = (info["status"] & M.IK_NOT_CONVERGED) == 0
    assert (st_conv[same] == conv[same, 0]).all()
    assert (info["err"][st_conv] < EPS).all() and (info["err"][~st_conv] >= EPS).all()
    assert np.array_equal(xf[:, 7:], np.zeros((B, 7)))           # no twist: qd = 0


@pytest.mark.gpu
@pytest.mark.parametrize("with_ref", [False, True], ids=["lowest", "q_ref"])
def test_choice_rule(M, with_ref):
    """S = 16: the chosen start is rule 4 applied to the 16 host runs (errors of non-qualifying starts from S = 1 device runs of each start)"""
    from mpc_motion_planner_amd import scenarios
    B, S = 128, 16
    cfg = _cfg(M); model = M.default_model(); lo, hi, _, _ = _bounds(cfg)
    qt = _true_q(M, B, 400)
    R, p = _poses(M, model, qt)
    seeds = scenarios.ik_seeds(B, S, cfg)
    q_ref = _true_q(M, B, 500) if with_ref else None
    s = M.Solver(cfg, B)
    xf, info = s.pose_targets(R, p, seeds, q_ref=q_ref)
    qh, conv, its = _host_runs(M, model, R, p, seeds, lo, hi)
    err1 = np.zeros((B, S)); its1 = np.zeros((B, S), dtype=int)
    for k in range(S):
        _, i1 = s.pose_targets(R, p, seeds[:, k:k + 1])
        err1[:, k], its1[:, k] = i1["err"], i1["iters"]
    want = np.array([_choose(qh[b], conv[b], err1[b], lo, hi, None if q_ref is None else q_ref[b]) for b in range(B)])
    diff = info["seed"] != want
    explained = (its1 != its).any(axis=1)         # a start whose host and device iteration counts differ (FMA contraction)
    print("choice rule: %d / %d differ from the host recomputation, %d of them explained" % (diff.sum(), B, (diff & explained).sum()))
    assert not (diff & ~explained).any(), np.nonzero(diff & ~explained)
    assert diff.mean() <= 0.02
    # the record is the chosen start's: its wrapped q, iterations and error
    b = np.arange(B)
    ok = ~diff
    assert np.abs(xf[ok, :7] - qh[b[ok], info["seed"][ok]]).max() <= 1e-8
    assert (info["iters"] == its1[b, info["seed"]]).all() and np.array_equal(info["err"], err1[b, info["seed"]])
    qual = conv & np.all((qh >= lo) & (qh <= hi), axis=2)
    some = qual.any(axis=1) & ~diff
    assert (info["status"][some] & (M.IK_NOT_CONVERGED | M.IK_Q_OUT_OF_BOUNDS) == 0).all()
    assert (info["status"][~qual.any(axis=1) & ~diff] & (M.IK_NOT_CONVERGED | M.IK_Q_OUT_OF_BOUNDS) != 0).all()
    assert some.mean() > 0.8


@pytest.mark.gpu
def test_unreachable_pose(M):
    from mpc_motion_planner_amd import scenarios
    B, S = 4, 16
    cfg = _cfg(M)
    R = np.tile(np.eye(3), (B, 1, 1)); p = np.tile([3.0, 0.0, 0.0], (B, 1))
    seeds = scenarios.ik_seeds(B, S, cfg, seed=11)
    s = M.Solver(cfg, B)
    xf, info = s.pose_targets(R, p, seeds)
    assert (info["status"] & M.IK_NOT_CONVERGED).all() and (info["iters"] == 1000).all()
    err1 = np.stack([s.pose_targets(R, p, seeds[:, k:k + 1])[1]["err"] for k in range(S)], axis=1)
    assert np.array_equal(info["seed"], np.argmin(err1, axis=1))
    assert np.array_equal(info["err"], err1.min(axis=1))


@pytest.mark.gpu
def test_twist(M):
    from mpc_motion_planner_amd import scenarios
    B, S = 64, 8
    cfg = _cfg(M); model = M.default_model(); _, _, lv, uv = _bounds(cfg)
    qt = _true_q(M, B, 600)
    R, p = _poses(M, model, qt)
    seeds = scenarios.ik_seeds(B, S, cfg)
    rng = np.random.default_rng(3)
    tw = np.concatenate([rng.uniform(-0.1, 0.1, (B, 3)), rng.uniform(-0.2, 0.2, (B, 3))], axis=1)
    s = M.Solver(cfg, B)
    xf, info = s.pose_targets(R, p, seeds, twist=tw)
    for b in range(B):
        qd = M.inverse_velocities(model, xf[b, :7], tw[b, :3], tw[b, 3:])
        assert np.abs(xf[b, 7:] - qd).max() <= 1e-9 * np.abs(qd).max(), b
    xf0, _ = s.pose_targets(R, p, seeds)
    assert np.array_equal(xf0[:, :7], xf[:, :7])
    # the bit is rule 5's test of qd against the velocity rows; a small twist leaves most targets inside them (not all: near-singular poses)
    out = ((xf[:, 7:] < lv) | (xf[:, 7:] > uv)).any(axis=1)
    assert np.array_equal((info["status"] & M.IK_QD_OUT_OF_BOUNDS) != 0, out)
    assert out.mean() < 0.25
    xb, big = s.pose_targets(R, p, seeds, twist=100.0 * tw)
    assert np.array_equal(xb[:, :7], xf[:, :7]) and np.allclose(xb[:, 7:], 100.0 * xf[:, 7:], rtol=0, atol=1e-12 * np.abs(xb[:, 7:]).max())
    out = ((xb[:, 7:] < lv) | (xb[:, 7:] > uv)).any(axis=1)
    assert np.array_equal((big["status"] & M.IK_QD_OUT_OF_BOUNDS) != 0, out)
    assert out.all()


@pytest.mark.gpu
def test_two_arms_fill_one_target(M):
    B, nseg = 96, 6
    cfg = _cfg(M, nseg, 2); lo, hi, _, _ = _bounds(cfg)
    models = M.arm_models(M.DUAL_BASES)
    s = M.Solver(cfg, B, models=models)
    rng = np.random.default_rng(5)
    xf = np.full((B, 28), 7.25)
    runs = []
    for arm in range(2):
        qt = _true_q(M, B, 700 + 1000 * arm)
        R, p = _poses(M, models[arm], qt)
        seeds = (qt + rng.uniform(-0.3, 0.3, qt.shape))[:, None, :]
        out, info = s.pose_targets(R, p, seeds, arm=arm, xf=xf)
        assert out is xf
        if arm == 0:
            assert (xf[:, 7:14] == 7.25).all() and (xf[:, 21:28] == 7.25).all()
            assert not (xf[:, 0:7] == 7.25).any() and (xf[:, 14:21] == 0).all()
        runs.append((R, p, seeds, info))
    assert not (xf == 7.25).any()
    for arm, (R, p, seeds, info) in enumerate(runs):
        qh, _, its = _host_runs(M, models[arm], R, p, seeds, lo, hi)
        same = info["iters"] == its[:, 0]
        assert same.mean() >= 0.97, arm
        assert np.abs(xf[same, 7 * arm:7 * arm + 7] - qh[same, 0]).max() <= 1e-8, arm
        # the other arm's model gives other answers: each arm used its own
        qo, _, _ = _host_runs(M, models[1 - arm], R[:8], p[:8], seeds[:8], lo, hi)
        assert np.abs(xf[:8, 7 * arm:7 * arm + 7] - qo[:, 0]).max() > 1e-3


def _inputs(M, B, S, cfg, off):
    from mpc_motion_planner_amd import scenarios
    model = M.default_model()
    qt = _true_q(M, B, off)
    R, p = _poses(M, model, qt)
    seeds = scenarios.ik_seeds(B, S, cfg, seed=off)
    q_ref = _true_q(M, B, off + 50)
    rng = np.random.default_rng(off)
    tw = np.concatenate([rng.uniform(-0.1, 0.1, (B, 3)), rng.uniform(-0.2, 0.2, (B, 3))], axis=1)
    return R, p, seeds, q_ref, tw


@pytest.mark.gpu
def test_device_variant_equals_host_variant(M):
    """inputs written by torch on its current stream behind a sleep, pose_targets_device on that stream: bitwise the host variant"""
    import torch
    B, S = 256, 16
    cfg = _cfg(M)
    R, p, seeds, q_ref, tw = _inputs(M, B, S, cfg, 800)
    s = M.Solver(cfg, B)
    xh, ih = s.pose_targets(R, p, seeds, q_ref=q_ref, twist=tw)
    stream = torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(20_000_000)                                  # the inputs land late on this stream
        t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda", non_blocking=True) * 1.0
             for a in (R.reshape(B, 9), p, tw, seeds, q_ref)]
        txf = torch.zeros((B, 14), dtype=torch.float64, device="cuda")
        tinfo = torch.zeros((B, M.IK_INFO_DTYPE.itemsize), dtype=torch.uint8, device="cuda")
        s.pose_targets_device(B, 0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), S, t[3].data_ptr(), t[4].data_ptr(),
                              txf.data_ptr(), tinfo.data_ptr(), stream=stream.cuda_stream)
        xd = txf.cpu()                                                 # ordered after the kernel on the same stream
        idv = tinfo.cpu()
    stream.synchronize()
    assert np.array_equal(xd.numpy(), xh)
    assert idv.numpy().tobytes() == ih.tobytes()


@pytest.mark.gpu
def test_errors_leave_target_untouched(M):
    B, S = 8, 4
    cfg = _cfg(M)
    R, p, seeds, q_ref, tw = _inputs(M, B, S, cfg, 900)
    s = M.Solver(cfg, B)
    L = M.lib()
    vp = C.c_void_p
    EINVAL = -1

    def call(B_=B, arm=0, R_=R, p_=p, tw_=tw, S_=S, seeds_=seeds, q_ref_=q_ref, xf_=True):
        xf = np.full((B, 14), -3.5)
        arrs = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (R_, p_, tw_, seeds_, q_ref_)]
        ptr = [vp(a.ctypes.data) if a is not None else None for a in arrs]
        rc = L.mpcmp_pose_targets_batch(s._ctx, B_, arm, ptr[0], ptr[1], ptr[2], S_, ptr[3], ptr[4], vp(xf.ctypes.data) if xf_ else None, None)
        return rc, xf

    rc, xf = call()
    assert rc == 0 and not (xf == -3.5).any()
    bad = []
    for kw in (dict(B_=0), dict(S_=0), dict(S_=65), dict(arm=1), dict(arm=-1), dict(R_=None), dict(p_=None), dict(seeds_=None), dict(xf_=False)):
        bad.append((kw, call(**kw)))
    for name, a in (("R_", R), ("p_", p), ("tw_", tw), ("seeds_", seeds), ("q_ref_", q_ref)):
        for v in (np.nan, np.inf):
            a2 = a.copy(); a2.reshape(-1)[a2.size // 2] = v
            bad.append(({name: v}, call(**{name: a2})))
    Rs = R.copy(); Rs[3] *= 1.0 + 1e-5                                       # not orthogonal
    Rr = R.copy(); Rr[5] = -Rr[5]                                            # det = -1
    bad += [("scaled", call(R_=Rs)), ("reflection", call(R_=Rr))]
    for kw, (rc, xf) in bad:
        assert rc == EINVAL, kw
        assert (xf == -3.5).all(), kw
    # a rotation inside the tolerance is accepted
    Rt = R.copy(); Rt[2] *= 1.0 + 1e-8
    assert call(R_=Rt)[0] == 0
    # the device variant checks the scalars and NULL pointers
    import torch
    d = torch.zeros(4096, dtype=torch.float64, device="cuda")
    P = d.data_ptr()
    for args in ((0, 0, P, P, 0, S, P, 0, P), (B, 0, P, P, 0, 0, P, 0, P), (B, 0, P, P, 0, 65, P, 0, P), (B, 1, P, P, 0, S, P, 0, P),
                 (B, 0, 0, P, 0, S, P, 0, P), (B, 0, P, 0, 0, S, P, 0, P), (B, 0, P, P, 0, S, 0, 0, P), (B, 0, P, P, 0, S, P, 0, 0)):
        with pytest.raises(M.MpcmpError) as e:
            s.pose_targets_device(*args, 0)
        assert e.value.code == EINVAL, args
    torch.cuda.synchronize()
    assert (d == 0).all()


def _rot_angle(Ra, Rb):
    c = (np.trace(Ra.T @ Rb) - 1.0) / 2.0
    return np.arccos(np.clip(c, -1.0, 1.0))


@pytest.mark.gpu
def test_end_to_end_pose_to_solve(M):
    """B = 512 poses, S = 16, q_ref = the start state's q -> xf -> mpcmp_solve_batch at N = 19 (20 SQP iterations, jerk-limited warm start)"""
    from mpc_motion_planner_amd import scenarios
    B, S = 512, 16
    cfg = _cfg(M, 6, 20)
    model = M.default_model()
    x0, _ = scenarios.make_batch(B, MARGINS, stream_offset=2000)
    qt = _true_q(M, B, 3000)
    R, p = _poses(M, model, qt)
    seeds = scenarios.ik_seeds(B, S, cfg)
    s = M.Solver(cfg, B)
    xf, info = s.pose_targets(R, p, seeds, q_ref=x0[:, :7])
    ok = info["status"] == 0
    print("end to end: IK status 0 for %d / %d (%.3f)" % (ok.sum(), B, ok.mean()))
    assert ok.mean() >= MIN_IK_OK
    for b in np.nonzero(ok)[0]:
        _, pb, Rb = M.tool_jacobian(model, xf[b, :7])
        assert np.linalg.norm(pb - p[b]) < 1e-4 and _rot_angle(R[b], Rb) < 1e-4, b
    warm = s.warm_start_jerk(x0, xf, MARGINS[4] * M.default_limits()["jmax"])
    sx, su, sT, si = s.solve(x0, xf, warm)
    assert (si["status"][ok] & M.STATUS_HARD == 0).all()
    done = ok & (si["status"] == 0)
    st, cnt = np.unique(si["status"][ok], return_counts=True)
    print("end to end: solve status 0 for %d of them; statuses %s" % (done.sum(), dict(zip(st.tolist(), cnt.tolist()))))
    assert done.any()
    assert (si["term_err_inf"][done] <= cfg.eps_target + cfg.eps_abs).all()


@pytest.mark.gpu
def test_closed_loop_device_targets(M):
    """pose_targets_batch_device -> rh_update_device(idx = NULL, xf) on a running N = 13 loop: bitwise the same xf through host rh_update"""
    import torch
    from mpc_motion_planner_amd import scenarios
    B, S, dt = 64, 8, 0.05
    cfg = _cfg(M, 4, 3)
    x0, xf0 = scenarios.make_batch(B, MARGINS, stream_offset=4000)
    R, p, seeds, q_ref, tw = _inputs(M, B, S, cfg, 4100)
    host, dev = M.Solver(cfg, B), M.Solver(cfg, B)
    for s in (host, dev):
        s.rh_init(x0, xf0)
        s.rh_run(2, dt, use_graph=True)
    xh, _ = host.pose_targets(R, p, seeds, q_ref=q_ref, twist=tw)
    host.rh_update(xf=xh)
    stream = torch.cuda.current_stream()
    with torch.cuda.stream(stream):
        t = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda", non_blocking=True) * 1.0 for a in (R.reshape(B, 9), p, tw, seeds, q_ref)]
        txf = torch.zeros((B, 14), dtype=torch.float64, device="cuda")
        dev.pose_targets_device(B, 0, t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), S, t[3].data_ptr(), t[4].data_ptr(), txf.data_ptr(), 0,
                                stream=stream.cuda_stream)
        dev.rh_update_device(B, 0, 0, txf.data_ptr(), stream=stream.cuda_stream)
    for s in (host, dev):
        s.rh_run(3, dt, use_graph=True)
    stream.synchronize()
    a, b = host.rh_get(), dev.rh_get()
    for u, v in zip(a[:4], b[:4]):
        assert np.array_equal(u, v)
    assert a[4].tobytes() == b[4].tobytes()
    assert np.array_equal(txf.cpu().numpy(), xh)
