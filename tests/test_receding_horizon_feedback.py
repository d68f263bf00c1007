"""Feedback into the receding-horizon driver (mpcmp_rh_update / mpcmp_rh_update_device, include/mpcmp.h): measured states and moving targets
between two steps of a running loop, the reference's set_current_state / set_target_state + solve_trajectory(false) (motionPlanner.cpp:27-53,
177-208).  The reference is `rh_chain_events`: oracle_py.rh_chain with events applied before chosen steps.  CPU tests anchor it to rh_chain and check
the error path without a GPU; the GPU tests (-m gpu) compare the driver with it, eager and with graph replay, with the tolerances of
test_gpu_receding_horizon.py, and check that an update which changes nothing changes nothing, bit for bit."""
import ctypes as C

import numpy as np
import pytest

import oracle_py as o
from test_gpu_receding_horizon import MARGINS, _arrival_setup, _check_step, _omodels, _solver, dual_states


def rh_chain_events(cfg, x0, xf, steps, dt, events=None, models=None):
    """oracle_py.rh_chain with feedback: events {step: [(b, x or None, xf or None, restart)]} are applied before that step (counted from 1): the
    current state and / or the target of instance b are set; a retired instance is revived (no longer retired, one fewer arrived) and restarts; a
    new target or `restart` restarts (the driver's start guess, zero multipliers).  Returns rh_chain's record."""
    events = events or {}
    B = len(x0); xc = o.f64(x0).copy(); xf = o.f64(xf).copy(); prev = [None] * B; lam = [None] * B
    retired = np.zeros(B, dtype=bool); its = np.zeros(B, dtype=int); status = np.zeros(B, dtype=int); T_last = np.zeros(B); n_solves = 0
    retired_at = np.zeros(B, dtype=int); restarts = np.zeros(B, dtype=int)
    h = {k: [] for k in ("hist_x", "hist_T", "hist_its", "hist_status", "hist_retired", "hist_n_solves")}
    for step in range(1, steps + 1):
        for b, x_new, xf_new, restart in events.get(step, ()):
            if x_new is not None:
                xc[b] = x_new
            if xf_new is not None:
                xf[b] = xf_new
            if retired[b]:
                retired[b] = False
                restart = True
            if xf_new is not None or restart:
                prev[b] = None; lam[b] = None
        for b in range(B):
            if retired[b]:
                continue
            n_solves += 1
            if prev[b] is None or (prev[b][3] & (1 | 2 | 4 | 32)):
                wx, wu, wT = o.rh_start_guess(cfg, xc[b], xf[b])
                restarts[b] += prev[b] is not None
            else:
                wx, wu, wT = prev[b][0].copy(), prev[b][1], prev[b][2]
                wx[0] = xc[b]; wx[-1] = xf[b]
            if models is None:
                xs, us, T, oi, lam[b] = o.solve_carry(cfg, xc[b], xf[b], wx, wu, wT, lam=lam[b])
            else:
                xs, us, T, oi, lam[b] = o.solve_carry_multi(models, cfg, xc[b], xf[b], wx, wu, wT, lam=lam[b])
            prev[b] = (xs, us, T, oi.status); its[b] = oi.qp_iters_total; status[b] = oi.status; T_last[b] = T
            xc[b], retired[b] = o.rh_advance(cfg, xs, us, T, oi.status, dt, xf[b], xc[b])
            if retired[b]:
                retired_at[b] = step
        for k, v in (("hist_x", xc), ("hist_T", T_last), ("hist_its", its), ("hist_status", status), ("hist_retired", retired)):
            h[k].append(v.copy())
        h["hist_n_solves"].append(n_solves)
    return dict(x=xc, T=T_last, its=its, status=status, retired=retired, n_solves=n_solves, retired_at=retired_at, restarts=restarts, **h)


def _same_record(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k.startswith("hist_"):
            assert len(a[k]) == len(b[k]), k
            for u, v in zip(a[k], b[k]):
                assert np.array_equal(u, v), k
        else:
            assert np.array_equal(a[k], b[k]), k


# ---- CPU: the reference loop and the error path without a GPU ---------------------------------------------------------------------------
@pytest.mark.parametrize("narm", [1, 2], ids=["one_arm", "two_arms"])
def test_event_chain_without_events_is_rh_chain(narm):
    """no events: rh_chain_events returns oracle_py.rh_chain's record element for element (N = 13 one arm, N = 19 two arms)"""
    from mpc_motion_planner_amd import scenarios
    nseg = 4 if narm == 1 else 6
    ocfg = o.default_config(nseg, 2, margins=MARGINS, carry_multipliers=1, qp_warm_start=1)
    x0, xf = scenarios.make_batch(3, MARGINS, stream_offset=40) if narm == 1 else dual_states(2, off=50)
    ref = o.rh_chain(ocfg, x0, xf, 3, 0.05, models=_omodels(narm))
    _same_record(rh_chain_events(ocfg, x0, xf, 3, 0.05, models=_omodels(narm)), ref)
    _same_record(rh_chain_events(ocfg, x0, xf, 3, 0.05, events={}, models=_omodels(narm)), ref)


def test_event_chain_applies_events():
    """an event on one instance changes that instance only: a new target restarts it, the other rows are rh_chain's"""
    from mpc_motion_planner_amd import scenarios
    ocfg = o.default_config(4, 2, margins=MARGINS, carry_multipliers=1, qp_warm_start=1)
    x0, xf = scenarios.make_batch(3, MARGINS, stream_offset=40)
    ref = o.rh_chain(ocfg, x0, xf, 3, 0.05)
    ev = rh_chain_events(ocfg, x0, xf, 3, 0.05, events={2: [(1, None, x0[1], False)]})
    for k in range(3):
        assert np.array_equal(ev["hist_x"][k][[0, 2]], ref["hist_x"][k][[0, 2]])
    assert np.array_equal(ev["hist_x"][0], ref["hist_x"][0])
    assert not np.array_equal(ev["hist_x"][1][1], ref["hist_x"][1][1])


def test_rh_update_without_context_is_einval():
    """both entry points refuse a NULL context with MPCMP_EINVAL (no GPU needed)"""
    import mpc_motion_planner_amd as M
    M.build_library()
    L = M.lib()
    x = np.zeros((1, 14))
    idx = np.zeros(1, dtype=np.int32)
    assert L.mpcmp_rh_update(None, 1, idx.ctypes.data_as(C.POINTER(C.c_int)), M.capi.host(x), None, 0) == -1
    assert L.mpcmp_rh_update(None, 1, None, None, None, M.RH_RESTART) == -1
    assert L.mpcmp_rh_update_device(None, 1, None, x.ctypes.data, None, 0, None) == -1
    assert M.RH_RESTART == 1


# ---- GPU --------------------------------------------------------------------------------------------------------------------------------
CASES = [(4, 1), (6, 1), (8, 1), (6, 2), (8, 2)]          # (num_seg, arms): N = 13, 19, 25 one arm; N = 19, 25 two arms
IDS = ["n13", "n19", "n25", "dual_n19", "dual_n25"]


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def _plan(M, nseg, narm):
    """The arrival set-up of test_gpu_receding_horizon (control periods of 0.4 s) and an event schedule on distinct instances, chosen from the
    loop without events (instances are independent, so an instance's state before its own event is the one of that loop):
      step 2: a perturbed measured state of a live instance (re-guess, carried multipliers);
      step 2: a new target (the start state of another instance) of a second live instance;
      step 3: MPCMP_RH_RESTART with its own state, third live instance;
      the step after the first arrival: the arrived instance gets a new target (its own start state) and is revived."""
    cfg, ocfg, x0, xf, dt = _arrival_setup(M, nseg, narm)
    B, steps = len(x0), 10
    base = o.rh_chain(ocfg, x0, xf, steps, dt, models=_omodels(narm))
    ra = base["retired_at"]
    assert (ra > 0).any(), ra
    rev = int(np.argmin(np.where(ra > 0, ra, steps + 1)))
    k_rev = int(ra[rev]) + 1
    assert k_rev <= steps - 2, ra
    live = [b for b in range(B) if b != rev and not base["hist_retired"][2][b]]
    assert len(live) >= 3, (ra, base["hist_retired"][2])
    b1, b2, b3 = live[:3]
    nx = 14 * narm
    pert = base["hist_x"][0][b1].copy()
    pert[:nx // 2] += 2e-3 * np.cos(np.arange(nx // 2))                  # a measured position off the plan
    pert[nx // 2:] *= 0.98                                              # and a slower velocity (stays inside its bounds)
    events = {2: [(b1, pert, None, False), (b2, None, x0[b3].copy(), False)],
              3: [(b3, base["hist_x"][1][b3].copy(), None, True)]}
    events.setdefault(k_rev, []).append((rev, None, x0[rev].copy(), False))
    ch = rh_chain_events(ocfg, x0, xf, steps, dt, events=events, models=_omodels(narm))
    assert ch["hist_retired"][k_rev - 2][rev] and not ch["hist_retired"][k_rev - 1][rev]       # arrived, then revived: it is solved again
    assert ch["hist_n_solves"][-1] != base["hist_n_solves"][-1] or not np.array_equal(ch["x"], base["x"])
    return cfg, x0, xf, dt, steps, events, ch


def _apply(s, evs):
    for b, x, xf, restart in evs:
        s.rh_update([b], x=None if x is None else x[None], xf=None if xf is None else xf[None], restart=restart)


def _snapshot(s):
    return s.rh_get() + (s.rh_stats(),)


def _assert_bitwise(a, b, ctx):
    for u, v in zip(a, b):
        if isinstance(u, np.ndarray):
            assert u.tobytes() == v.tobytes(), ctx
        else:
            assert u == v, ctx


@pytest.mark.gpu
@pytest.mark.parametrize("nseg,narm", CASES, ids=IDS)
def test_feedback_vs_oracle(M, nseg, narm):
    """a perturbed state, a new target, a flagged restart and the revival of an arrived instance, applied between rh_run(1) calls: after every
    step the driver equals rh_chain_events (states <= 1e-6, |dT| <= 1e-6 T, equal ADMM iterations, status words, ARRIVED bits and rh_stats),
    eager and with graph replay; and graph replay equals eager bit for bit after every step"""
    cfg, x0, xf, dt, steps, events, ch = _plan(M, nseg, narm)
    snaps = {}
    for use_graph in (False, True):
        s = _solver(M, cfg, narm, len(x0))
        s.rh_init(x0, xf)
        snaps[use_graph] = []
        for k in range(steps):
            _apply(s, events.get(k + 1, ()))
            s.rh_run(1, dt, use_graph=use_graph)
            _check_step(M, s, ch, k, (nseg, narm, use_graph, k))
            snaps[use_graph].append(_snapshot(s))
    for k in range(steps):
        _assert_bitwise(snaps[False][k], snaps[True][k], (nseg, narm, k))


@pytest.mark.gpu
@pytest.mark.parametrize("nseg,narm", [(6, 1), (8, 2)], ids=["n19", "dual_n25"])
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_update_with_the_current_state_changes_nothing(M, nseg, narm, use_graph):
    """rh_update of every live instance with its own current state, no flag, before every step: the loop is bitwise the loop without updates
    (states, solutions, records, rh_stats) - the re-guess path and the captured step are untouched"""
    cfg, ocfg, x0, xf, dt = _arrival_setup(M, nseg, narm)
    B, steps = len(x0), 10
    ref = _solver(M, cfg, narm, B)
    ref.rh_init(x0, xf)
    s = _solver(M, cfg, narm, B)
    s.rh_init(x0, xf)
    arrived = 0
    for k in range(steps):
        if k:
            xg, _, _, _, info = s.rh_get()
            live = np.nonzero((info["status"] & M.STATUS_ARRIVED) == 0)[0]
            if len(live):
                s.rh_update(live, x=xg[live])
        ref.rh_run(1, dt, use_graph=use_graph)
        s.rh_run(1, dt, use_graph=use_graph)
        a, b = _snapshot(ref), _snapshot(s)
        _assert_bitwise(a, b, (nseg, narm, use_graph, k))
        arrived = a[-1][1]
    assert arrived >= 1, arrived           # (the live set shrank on the way)


@pytest.mark.gpu
@pytest.mark.parametrize("nseg,narm,B", [(6, 1, 512), (8, 2, 256)], ids=["n19_B512", "dual_n25_B256"])
def test_graph_equals_eager_with_updates_two_streams(M, nseg, narm, B):
    """batches solved as two halves on two streams: the same updates (all states perturbed, a third of the targets moved, a flagged restart of
    every seventh) before steps 3 and 5, graph replay and eager bitwise equal after every step"""
    from mpc_motion_planner_amd import scenarios
    from test_gpu_receding_horizon import _configs
    cfg, _ = _configs(M, nseg, True)
    x0, xf = scenarios.make_batch(B, MARGINS, stream_offset=300) if narm == 1 else dual_states(B, off=300)
    steps, dt, nx = 6, 0.02, 14 * narm
    moved = np.arange(0, B, 3)
    flagged = np.arange(1, B, 7)
    snaps = {}
    for use_graph in (False, True):
        s = _solver(M, cfg, narm, B)
        s.rh_init(x0, xf)
        snaps[use_graph] = []
        for k in range(steps):
            if k in (2, 4):
                xg = s.rh_get()[0]
                xm = xg.copy(); xm[:, nx // 2:] *= 0.99
                s.rh_update(x=xm)
                s.rh_update(moved, xf=x0[moved[::-1]])
                s.rh_update(flagged, x=xm[flagged], restart=True)
            s.rh_run(1, dt, use_graph=use_graph)
            snaps[use_graph].append(_snapshot(s))
    for k in range(steps):
        _assert_bitwise(snaps[False][k], snaps[True][k], (nseg, narm, k))
    xg, sx, su, sT, info = snaps[True][-1][:5]
    assert np.all(np.isfinite(xg)) and np.all(np.isfinite(sT))


@pytest.mark.gpu
@pytest.mark.parametrize("nseg,narm", [(6, 1), (8, 2)], ids=["n19", "dual_n25"])
def test_device_variant_equals_host_variant(M, nseg, narm):
    """the schedule of test_feedback_vs_oracle, each step's updates written by torch on a non-default stream and passed to rh_update_device on
    that stream, rh_run at once (graph replay): bitwise the host variant after every step"""
    import torch
    cfg, x0, xf, dt, steps, events, ch = _plan(M, nseg, narm)
    B, nx = len(x0), 14 * narm
    host = _solver(M, cfg, narm, B)
    host.rh_init(x0, xf)
    dev = _solver(M, cfg, narm, B)
    dev.rh_init(x0, xf)
    stream = torch.cuda.Stream()
    keep = []
    for k in range(steps):
        evs = events.get(k + 1, ())
        _apply(host, evs)
        for b, x, xt, restart in evs:
            with torch.cuda.stream(stream):
                ti = torch.full((1,), b, dtype=torch.int32, device="cuda")
                tx = torch.from_numpy(x[None]).to("cuda", non_blocking=True) * 1.0 if x is not None else None
                tf = torch.from_numpy(xt[None]).to("cuda", non_blocking=True) + 0.0 if xt is not None else None
            keep.append((ti, tx, tf))                  # (alive until the stream has run the update)
            dev.rh_update_device(1, ti.data_ptr(), tx.data_ptr() if tx is not None else 0, tf.data_ptr() if tf is not None else 0,
                                 restart=restart, stream=stream.cuda_stream)
        host.rh_run(1, dt, use_graph=True)
        dev.rh_run(1, dt, use_graph=True)
        _assert_bitwise(_snapshot(host), _snapshot(dev), (nseg, narm, k))
        _check_step(M, dev, ch, k, (nseg, narm, "device", k))
    torch.cuda.synchronize()
    assert nx == x0.shape[1]


@pytest.mark.gpu
def test_bad_updates_raise_and_change_nothing(M):
    """every error rule of mpcmp_rh_update raises MpcmpError and writes nothing: the loop after the bad calls equals a loop that never saw them,
    bit for bit; the device variant refuses what it can check (n, NULL pointers, flags, no loop) the same way"""
    import torch
    cfg, ocfg, x0, xf, dt = _arrival_setup(M, 6, 1)
    B, nx = len(x0), 14
    fresh = _solver(M, cfg, 1, B)
    with pytest.raises(M.MpcmpError):                  # before rh_init
        fresh.rh_update([0], x=x0[:1])
    with pytest.raises(M.MpcmpError):
        fresh.rh_update_device(1, 0, torch.zeros((1, nx), dtype=torch.float64, device="cuda").data_ptr(), 0)
    ref = _solver(M, cfg, 1, B)
    ref.rh_init(x0, xf)
    s = _solver(M, cfg, 1, B)
    s.rh_init(x0, xf)
    for k in range(4):
        ref.rh_run(1, dt, use_graph=True)
        s.rh_run(1, dt, use_graph=True)
        xg = s.rh_get()[0]
        bad = xg[:2].copy(); bad[1, 3] = np.nan
        inf = xf[:1].copy(); inf[0, 9] = np.inf
        calls = [lambda: s.rh_update(x=xg[:0]),                                   # n < 1
                 lambda: s.rh_update(x=np.concatenate([xg, xg[:1]])),              # n > B
                 lambda: s.rh_update([0, B], x=xg[:2]),                            # index out of range
                 lambda: s.rh_update([-1], x=xg[:1]),
                 lambda: s.rh_update([1, 1], x=xg[:2]),                            # repeated
                 lambda: s.rh_update([0, 1]),                                      # x and xf both NULL
                 lambda: s.rh_update([0, 1], x=bad),                               # not finite
                 lambda: s.rh_update([2], xf=inf),
                 lambda: M.capi.check(M.lib().mpcmp_rh_update(s._ctx, 1, np.zeros(1, np.int32).ctypes.data_as(C.POINTER(C.c_int)),
                                                              M.capi.host(xg[:1].copy()), None, 2), s._ctx)]          # unknown flag bit
        for i, call in enumerate(calls):
            with pytest.raises(M.MpcmpError) as e:
                call()
            assert e.value.code == -1 and "mpcmp_rh_update" in str(e.value), (k, i, str(e.value))
        tx = torch.from_numpy(xg).to("cuda")
        for n, x, flags in ((0, tx.data_ptr(), 0), (B + 1, tx.data_ptr(), 0), (B, 0, 0), (B, tx.data_ptr(), 4)):
            with pytest.raises(M.MpcmpError):
                M.capi.check(M.lib().mpcmp_rh_update_device(s._ctx, n, None, x, None, flags, None), s._ctx)
        torch.cuda.synchronize()
        _assert_bitwise(_snapshot(ref), _snapshot(s), k)
    ref.rh_run(2, dt, use_graph=True)
    s.rh_run(2, dt, use_graph=True)
    _assert_bitwise(_snapshot(ref), _snapshot(s), "after")
