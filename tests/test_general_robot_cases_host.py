"""The choices behind tests/test_gpu_general_robot.py, re-derived on the CPU.  That module states that its solve cases were qualified with the oracle
alone, that its clearance scenes give both outcomes, that its tool-velocity trajectories keep clear of the thresholds and that the inverse-kinematics
starts converge.  Each statement is an assertion here, on the very case tables and helper functions the GPU tests use, so that it is checked again
whenever a seed, the oracle or robots.make_spec changes."""
import os

import numpy as np
import pytest

import oracle_py as o
import rbd_reference as rr
import test_gpu_general_robot as g

HARD_FAILURE = 1 | 2 | 4
N_PERTURBATIONS, REL = 3, 1e-12


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as m
    if not os.path.exists(m.library_path()):
        pytest.skip("libmpcmp.so not built")
    return m


def perturbed(models, rng):
    """oracle Models with every constant (R0, p, mass, com, I, tool, link8, gravity) times 1 +- 1e-12, random signs"""
    out = (o.Model * len(models))()
    for a in range(len(models)):
        m = o.Model.from_buffer_copy(models[a])
        v = np.frombuffer(m, dtype=np.float64)
        v *= 1.0 + REL * rng.choice([-1.0, 1.0], v.shape)
        out[a] = m
    return out


def qualifies(solve_one, models, B, tag):
    """every problem: finite outputs, no hard-failure bit, and qp_iters_total unchanged under the perturbations of the model"""
    base = [solve_one(g.omodels(models), b) for b in range(B)]
    for b, (xs, us, T, info) in enumerate(base):
        assert np.isfinite(xs).all() and np.isfinite(us).all() and np.isfinite(T), (tag, b)
        assert (info.status & HARD_FAILURE) == 0, (tag, b, info.status)
    rng = np.random.default_rng(7)
    for k in range(N_PERTURBATIONS):
        pm = perturbed(models, rng)
        for b in range(B):
            it = solve_one(pm, b)[3].qp_iters_total
            assert it == base[b][3].qp_iters_total, (tag, b, k, it, base[b][3].qp_iters_total)
    print(tag, "qp_iters_total", [x[3].qp_iters_total for x in base], "status", [x[3].status for x in base])


def oracle_cases():
    seen = []
    for name, nseg, sqp, B, _, _ in g.SOLVE_CASES:          # (the environment selects a GPU kernel: the oracle's problem is the same)
        if (name, nseg, sqp, B) not in seen:
            seen.append((name, nseg, sqp, B))
    return seen


@pytest.mark.parametrize("name,nseg,sqp,B", oracle_cases())
def test_one_arm_solve_cases_qualify(M, tmp_path_factory, name, nseg, sqp, B):
    ocfg = g._cfgs(M, nseg, sqp)[1]
    x0, xf, wx, wu, wT = g.single_problems(ocfg, B)
    qualifies(lambda om, b: o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b], model=om[0]), g.robot(M, tmp_path_factory, name), B, (name, nseg, sqp))


@pytest.mark.parametrize("nseg,sqp,B", g.DUAL_CASES)
def test_two_arm_solve_cases_qualify(M, tmp_path_factory, nseg, sqp, B):
    ocfg = g._cfgs(M, nseg, sqp)[1]
    x0, xf = g.dual_states(B, g.DUAL_OFFSET)
    wx, wu, wT = g.dual_warm(nseg, x0, xf)
    qualifies(lambda om, b: o.solve_multi(om, ocfg, x0[b], xf[b], wx[b], wu[b], wT[b]), g.robot(M, tmp_path_factory, "dual_%d" % g.DUAL_SEED), B, ("dual", nseg, sqp))


def test_payload_solve_case_qualifies(M, tmp_path_factory):
    from test_gpu_payload import PAYLOADS
    name, nseg, sqp, B, kinds = g.PAYLOAD_CASE
    ocfg = g._cfgs(M, nseg, sqp)[1]
    model = g.robot(M, tmp_path_factory, name)[0]
    x0, xf, wx, wu, wT = g.single_problems(ocfg, B)
    for b in range(B):                                     # (problem b carries row b of the table)
        lumped = (M.Model * 1)(); lumped[0] = M.model_add_payload(model, M.payload(*PAYLOADS[kinds[b]]))
        qualifies(lambda om, _, b=b: o.solve(ocfg, x0[b], xf[b], wx[b], wu[b], wT[b], model=om[0]), lumped, 1, ("payload", b))


@pytest.mark.parametrize("name", list(g.CLEARANCE_CASES))
def test_clearance_cases_give_both_outcomes(M, tmp_path_factory, name):
    """clearance_reference asserts it: some moves hit, some stay clear, no per-sample minimum within 1e-9 of the margin"""
    g.clearance_reference(M, g.robot(M, tmp_path_factory, name), *g.CLEARANCE_CASES[name])


@pytest.mark.parametrize("name", g.SINGLE)
def test_tool_velocity_cases_keep_clear_of_the_thresholds(M, tmp_path_factory, name):
    """tool_velocity_case asserts it: every speed ratio at least 1e-3 from 1, both flags take both values; and the aimed ratios are the aims"""
    c = g.tool_velocity_case(rr.Reference.from_model(g.robot(M, tmp_path_factory, name)[0]), 4, 6, 20)
    ratio = np.where(np.arange(6) % 2 == 0, c["lin"] / 1.7, c["ang"] / 2.5)
    print(name, "linear / 1.7:", np.round(c["lin"] / 1.7, 4), "angular / 2.5:", np.round(c["ang"] / 2.5, 4))
    assert np.abs(ratio - np.array(g.TOOL_AIMS)).max() < 1e-12


def test_pose_target_starts_converge_on_the_host(M, tmp_path_factory):
    """the host inverse kinematics (the same DLS step as the kernel's) from the starts of the GPU test: at least two starts of every target
    converge, so that one start whose iteration count differs on the GPU (FMA contraction) does not leave a target without a solution"""
    models = g.robot(M, tmp_path_factory, "dual_%d" % g.DUAL_SEED)
    for arm in range(2):
        _, f, seeds = g.pose_target_case(models, arm)
        conv = np.zeros(seeds.shape[:2], dtype=bool); its = np.zeros(seeds.shape[:2], dtype=int)
        for b in range(seeds.shape[0]):
            for k in range(seeds.shape[1]):
                _, conv[b, k], its[b, k] = M.inverse_kinematic(models[arm], f["R"][b, 6], f["tool"][b], seeds[b, k])
        print("arm %d: %d of %d starts converge, at least %d per target, %d .. %d DLS iterations (median %d)"
              % (arm, conv.sum(), conv.size, conv.sum(axis=1).min(), its[conv].min(), its[conv].max(), np.median(its[conv])))
        assert conv.sum(axis=1).min() >= 2, (arm, conv.sum(axis=1))
