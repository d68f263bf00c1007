"""The energy-based inverse-dynamics reference (tests/rbd_reference.py) and, through it, a pin on the oracle's rigid-body layer for robots that are
not the Panda.  CPU only.

Order of trust: the reference first shows its own accuracy (complex128 against long double, Richardson estimate); it is pinned to the stored Pinocchio
outputs on the Panda; then the oracle is compared with it on the Panda, on three general robots (rotated joint frames, oblique axes, a fixed
intermediate link, full inertia tensors: robots.general_models) and on a general robot under a tilted gravity vector."""
import json
import os

import numpy as np
import pytest

import oracle_py as o
import rbd_reference as rr
from robots import general_models, tilted_gravity_models

GENERAL_SEEDS = (11, 12, 13)
TILTED_SEED = 14
DUAL_SEED = 21          # the two-chain robot of tests/test_gpu_general_robot.py: chain 0 on the oblique axes, chain 1 on random ones


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as m
    if not os.path.exists(m.library_path()):
        pytest.skip("libmpcmp.so not built")
    return m


@pytest.fixture(scope="module")
def robots(M, tmp_path_factory):
    """name -> ctypes Model: the Panda, the general robots, the tilted-gravity robot and both chains of the two-chain robot"""
    d = tmp_path_factory.mktemp("robots")
    out = {"panda": M.default_model()}
    for s in GENERAL_SEEDS:
        out["general_%d" % s] = general_models(M, d, s)[0][0]
    out["tilted_%d" % TILTED_SEED] = tilted_gravity_models(M, d, TILTED_SEED)[0][0]
    dual = general_models(M, d, DUAL_SEED, 2)[0]
    out["dual_%d_chain0" % DUAL_SEED], out["dual_%d_chain1" % DUAL_SEED] = dual[0], dual[1]
    return out


def samples(n, seed):
    """q inside the Panda joint ranges, velocities and accelerations up to the limits the configurations apply"""
    rng = np.random.default_rng(seed)
    lim = o.default_limits()
    return (rng.uniform(lim["qmin"], lim["qmax"], (n, 7)), rng.uniform(-1, 1, (n, 7)) * lim["vmax"], rng.uniform(-1, 1, (n, 7)) * lim["amax"])


def test_reference_states_its_own_accuracy(robots):
    """tau, M and dtau/dqd once in complex128 and once in clongdouble on the same samples; the Richardson estimate of dtau/dq.  The figures are
    printed and stand in the docstring of rbd_reference.py.  The bounds: a tenth of the 1e-11 the comparisons with this reference allow, so that the
    reference's own rounding takes at most a tenth of any bar; and an estimate that leaves the dq comparison (bar or ten times the estimate) a hundred
    times below the 1e-6 of the oracle's own central-difference check"""
    worst = dict(tau=0.0, M=0.0, dqd=0.0, est=0.0, tau_abs=0.0, dq_abs=0.0); ests = []
    for name, m in robots.items():
        q, v, a = samples(20, 3)
        r64, r80 = rr.Reference.from_model(m), rr.Reference.from_model(m, real=np.longdouble)
        worst["tau"] = max(worst["tau"], float(np.abs(r64.tau(q, v, a) - r80.tau(q, v, a)).max()))
        worst["M"] = max(worst["M"], float(np.abs(r64.mass_matrix(q) - r80.mass_matrix(q.astype(np.longdouble))).max()))
        worst["dqd"] = max(worst["dqd"], float(np.abs(r64.dtau_dqd(q, v) - r80.dtau_dqd(q, v)).max()))
        dq, est = r64.dtau_dq(q, v, a)
        ests.append(est.max(axis=(1, 2)))
        worst["est"] = max(worst["est"], float(est.max())); worst["dq_abs"] = max(worst["dq_abs"], float(np.abs(dq).max()))
        worst["tau_abs"] = max(worst["tau_abs"], float(np.abs(r64.tau(q, v, a)).max()))
    print("complex128 vs clongdouble: tau %.2e (|tau| <= %.1f), M %.2e, dtau/dqd %.2e; Richardson estimate of dtau/dq: max %.2e, median %.2e (|dq| <= %.1f)"
          % (worst["tau"], worst["tau_abs"], worst["M"], worst["dqd"], worst["est"], float(np.median(np.concatenate(ests))), worst["dq_abs"]))
    assert np.finfo(np.longdouble).eps < 1e-18         # (an extended type is there to compare with)
    assert worst["tau"] < 1e-12 and worst["M"] < 1e-12 and worst["dqd"] < 1e-12
    assert 10.0 * worst["est"] < 1e-8


def test_reference_vs_stored_pinocchio_outputs(robots, golden_dir):
    """the bars tests/test_oracle_rigid_body.py holds the oracle to (the stored numbers carry 6 significant figures)"""
    r = rr.Reference.from_model(robots["panda"])
    k = np.loadtxt(os.path.join(golden_dir, "kat_rnea.csv"), delimiter=",")
    assert np.abs(r.tau(k[:, 1:8], k[:, 8:15], k[:, 15:22]) - k[:, 22:29]).max() < 2.5e-4
    f = np.loadtxt(os.path.join(golden_dir, "kat_fk_link8.csv"), delimiter=",")
    assert np.abs(r.fk(f[:, :7])["link8"] - f[:, 7:]).max() < 1e-12
    j = json.load(open(os.path.join(golden_dir, "kat_jac.json")))
    J1 = r.frame_jacobian(np.array(j["J1"]["q"]), [0, 0, 0]) @ np.array(j["J1"]["qd"])
    assert np.abs(J1 - j["J1"]["world_aligned_joint7_velocity"]).max() < 1e-8
    J2 = r.frame_jacobian(np.array(j["J2"]["q"]), [0, 0, 0]) @ np.array(j["J2"]["qd"])
    assert np.abs(J2 - j["J2"]["world_aligned_joint7_velocity"]).max() < 6e-4
    fk = r.fk(np.array(j["FK1"]["q"]))
    assert np.abs(fk["p"][6] - j["FK1"]["oMi7_p"]).max() < 1e-6 and np.abs(fk["R"][6] - np.array(j["FK1"]["oMi7_R"])).max() < 1e-6


def oracle_vs_reference(model, n, seed, what):
    om = o.Model.from_buffer_copy(model)
    r = rr.Reference.from_model(model)
    q, v, a = samples(n, seed)
    x = np.concatenate([q, v], axis=1)
    tau = r.tau(q, v, a)
    g1, G1, est = r.constraints(x, a, quirk=1)
    G0 = G1.copy(); G0[:, :, 21] = 0.0          # (quirk off: only the T column differs; the reference computes it so, asserted below)
    g0_4, G0_4, _ = r.constraints(x[:4], a[:4], quirk=0)
    assert np.array_equal(g0_4, g1[:4]) and np.array_equal(G0_4, G0[:4])
    f = r.fk(q)
    M_ref, dv_ref = r.mass_matrix(q), r.dtau_dqd(q, v)
    for i in range(n):
        tag = (what, i)
        assert np.abs(o.rnea(q[i], v[i], a[i], model=om) - tau[i]).max() < rr.TAU_TOL, tag
        t, dq, dv, Mm = o.rnea_derivatives(q[i], v[i], a[i], model=om)
        bar = rr.jac_tol(G1[i])
        assert np.abs(t - tau[i]).max() < rr.TAU_TOL and np.abs(dv - dv_ref[i]).max() < bar and np.abs(Mm - M_ref[i]).max() < bar, tag
        assert np.all(np.abs(dq - G1[i, :7, :7]) < np.maximum(bar, 10.0 * est[i])), (tag, np.abs(dq - G1[i, :7, :7]).max(), est[i].max())
        g, G = o.eval_constraints(x[i], a[i], quirk=1, model=om)
        rr.assert_constraints_close(g, G, g1[i], G1[i], est[i], tag)
        g, G = o.eval_constraints(x[i], a[i], quirk=0, model=om)
        rr.assert_constraints_close(g, G, g1[i], G0[i], est[i], tag)
        assert np.all(G[:, 21] == 0.0) and np.abs(G1[i, :7, 21]).max() > 1e-3
        p7, R7, p8, pt = o.fk(q[i], model=om)
        for got, want in ((p7, f["p"][i, 6]), (R7, f["R"][i, 6]), (p8, f["link8"][i]), (pt, f["tool"][i])):
            assert np.abs(got - want).max() < rr.TAU_TOL, tag
        J = o.frame_jacobian(q[i], np.array(model.tool[:]), model=om)
        assert np.abs(J - f["J"][i]).max() < rr.jac_tol(f["J"][i]), tag


def test_oracle_vs_reference_on_the_panda(robots):
    oracle_vs_reference(robots["panda"], 50, 21, "panda")


@pytest.mark.parametrize("name", ["general_%d" % s for s in GENERAL_SEEDS] + ["tilted_%d" % TILTED_SEED]
                         + ["dual_%d_chain%d" % (DUAL_SEED, c) for c in (0, 1)])
def test_oracle_vs_reference_on_general_robots(robots, name):
    """THE pin on the oracle off the Panda: 50 random (q, qd, qdd) per robot, velocities and accelerations up to the limits.  Both chains of the
    two-chain robot are robots of their own here (chain 1 turns about random axes): the references of the finished-plan readers take rnea, fk and
    frame_jacobian from the oracle on them (tests/test_general_robot_readers_host.py)"""
    m = robots[name]
    if name.startswith("tilted"):
        assert min(abs(m.gravity[0]), abs(m.gravity[1])) > 1.0
    oracle_vs_reference(m, 50, 22, name)


def test_general_robots_are_general_and_inside_the_torque_limits(M, robots):
    """what the GPU tests rely on: no structural zeros in the model constants, and gravity torques well inside the Panda torque limits"""
    lim = o.default_limits()
    for name, m in robots.items():
        if name == "panda":
            continue
        f = rr.model_fields(m)
        # (floors far above the comparison bars: a dropped R0 entry of 1e-4 moves torques of order 10 N m by 1e-3, eight orders above 1e-11.
        # The smallest R0 entry of the random-axes chain of the two-chain robot is 7.2e-4)
        assert np.abs(f["R0"]).min() > 1e-4 and np.abs(f["p"]).min() > 1e-4 and np.abs(f["com"]).min() > 1e-5, name
        assert min(abs(f["I"][i][r, c]) for i in range(7) for r in range(3) for c in range(3) if r != c) > 1e-6, name
        assert np.abs(f["tool"][:2]).min() > 1e-3, name
        q = samples(200, 5)[0]
        tg = rr.Reference.from_model(m).gravity_term(q)
        assert np.all(np.abs(tg).max(axis=0) < 0.5 * lim["taumax"]), (name, np.abs(tg).max(axis=0))
        # the reference's tool pose is the product's (host FK of libmpcmp.so)
        fk = rr.Reference.from_model(m).fk(q[:5])
        for i in range(5):
            J, p, R = M.tool_jacobian(m, q[i])
            assert np.abs(p - fk["tool"][i]).max() < 1e-12 and np.abs(R - fk["R"][i, 6]).max() < 1e-12 and np.abs(J - fk["J"][i]).max() < 1e-12
