"""Clearance checks, the part that needs no GPU: the skeleton sphere model, the host statement of the rules (mpcmp_clearance_config) against a NumPy
restatement written out here, and the compiler's resource remarks of the kernel.

The NumPy reference below is what tests/test_gpu_clearance.py checks the kernel against as well.  Its forward kinematics are formed from the Model
fields by the chain of include/mpcmp.h (p_w[i] = p_w[i-1] + R_w[i-1] p[i], R_w[i] = R_w[i-1] R0[i] Rz(q_i)) and pinned to the oracle's orc_fk.
"""
import ctypes as C
import os

import numpy as np
import pytest

import oracle_py as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


# ---------------------------------------------------------------------------------------------------------------------------------------------
# NumPy reference
def model_arrays(m):
    return (np.array(m.R0).reshape(7, 3, 3), np.array(m.p).reshape(7, 3), np.array(m.tool[:]))


def fk_np(m, q):
    """world rotation [..., 7, 3, 3] and origin [..., 7, 3] of the joint frames for q [..., 7]"""
    R0, p, _ = model_arrays(m)
    q = np.asarray(q, dtype=np.float64)
    lead = q.shape[:-1]
    Rp = np.broadcast_to(np.eye(3), lead + (3, 3)); pp = np.zeros(lead + (3,))
    Rw, pw = [], []
    for i in range(7):
        c, s = np.cos(q[..., i]), np.sin(q[..., i])
        Rz = np.zeros(lead + (3, 3))
        Rz[..., 0, 0] = c; Rz[..., 0, 1] = -s; Rz[..., 1, 0] = s; Rz[..., 1, 1] = c; Rz[..., 2, 2] = 1.0
        pi = pp + np.einsum("...ij,j->...i", Rp, p[i])
        Ri = np.einsum("...ij,jk,...kl->...il", Rp, R0[i], Rz)
        Rw.append(Ri); pw.append(pi)
        Rp, pp = Ri, pi
    return np.stack(Rw, axis=-3), np.stack(pw, axis=-2)


def sphere_centres(models, tables, q):
    """world centres [..., nsph, 3], radii, arm and joint of every sphere (arm-major) for q [..., 7 narm]"""
    cen, rad, arm, jnt = [], [], [], []
    for a, (m, t) in enumerate(zip(models, tables)):
        Rw, pw = fk_np(m, np.asarray(q)[..., 7 * a:7 * a + 7])
        for s in range(t.shape[0]):
            j = int(t["joint"][s])
            cen.append(pw[..., j, :] + np.einsum("...ij,j->...i", Rw[..., j, :, :], t["c"][s]))
            rad.append(float(t["r"][s])); arm.append(a); jnt.append(j)
    lead = np.asarray(q).shape[:-1]
    cen = np.stack(cen, axis=-2) if cen else np.zeros(lead + (0, 3))
    return cen, np.array(rad), np.array(arm, dtype=int), np.array(jnt, dtype=int)


def sd_np(ob, x):
    """signed distance of the points x [..., 3] to one obstacle record: the four formulas of include/mpcmp.h"""
    a, b, r, kind = np.array(ob["a"], dtype=np.float64), np.array(ob["b"], dtype=np.float64), float(ob["r"]), int(ob["type"])
    if kind == 0:
        return np.linalg.norm(x - a, axis=-1) - r
    if kind == 1:
        ab = b - a; l2 = ab @ ab
        t = np.clip((x - a) @ ab / l2, 0.0, 1.0) if l2 > 0 else np.zeros(x.shape[:-1])
        return np.linalg.norm(x - a - t[..., None] * ab, axis=-1) - r
    if kind == 2:
        d = np.abs(x - a) - b
        return np.linalg.norm(np.maximum(d, 0.0), axis=-1) + np.minimum(d.max(axis=-1), 0.0) - r
    return x @ a - b[0]


def clearances_np(models, tables, obstacles, q, self_gap):
    """every clearance of the configurations q [S, 7 narm]: obstacle pairs [S, nsph, n_obs] and robot pairs [S, nsph, nsph] (inf where the pair
    is not in the set: t <= s, or one arm and joints closer than self_gap / self_gap == 0)"""
    cen, rad, arm, jnt = sphere_centres(models, tables, q)
    S, ns = cen.shape[0], cen.shape[1]
    n_obs = 0 if obstacles is None else obstacles.shape[0]
    dob = np.full((S, ns, n_obs), np.inf)
    for k in range(n_obs):
        dob[:, :, k] = sd_np(obstacles[k], cen) - rad[None, :]
    drb = np.full((S, ns, ns), np.inf)
    for s in range(ns):
        for t in range(s + 1, ns):
            if arm[s] != arm[t] or (self_gap > 0 and abs(jnt[s] - jnt[t]) >= self_gap):
                drb[:, s, t] = np.linalg.norm(cen[:, s] - cen[:, t], axis=-1) - rad[s] - rad[t]
    return dob, drb


def named_pair_value(dob, drb, sample, sphere, other):
    """the reference clearance of the pair a record names"""
    return dob[sample, sphere, other] if other >= 0 else drb[sample, sphere, -1 - other]


def scene(M, rows):
    return np.array([M.obstacle(*r) for r in rows], dtype=M.OBSTACLE_DTYPE)


# a world with all four primitives; the box and the half-space are placed so that robot spheres lie INSIDE them for part of the configurations
def host_scene(M):
    return scene(M, [(M.OBS_SPHERE, (0.55, 0.0, 0.75), (0, 0, 0), 0.10),
                     (M.OBS_BOX, (0.45, 0.1, 0.55), (0.15, 0.2, 0.15), 0.02),
                     (M.OBS_CAPSULE, (-0.5, 0.5, 0.2), (-0.5, 0.5, 1.0), 0.04),
                     (M.OBS_HALFSPACE, (0.0, 1.0, 0.0), (-0.35, 0, 0), 0.0),                    # (solid: y <= -0.35)
                     (M.OBS_CAPSULE, (0.2, -0.4, 0.6), (0.2, -0.4, 0.6), 0.05)])          # (a == b: t = 0)


# ---------------------------------------------------------------------------------------------------------------------------------------------
def test_reference_kinematics_agree_with_the_oracle(M):
    rng = np.random.default_rng(7)
    lim = o.default_limits()
    for model, omodel in ((M.default_model(), o.default_model()), (M.arm_models(M.DUAL_BASES)[1], o.arm_models(o.DUAL_BASES)[1])):
        for _ in range(20):
            q = lim["qmin"] + rng.random(7) * (lim["qmax"] - lim["qmin"])
            Rw, pw = fk_np(model, q)
            p7, R7, _, pt = o.fk(q, model=omodel)
            tool = pw[6] + Rw[6] @ np.array(model.tool[:])
            assert np.abs(pw[6] - p7).max() <= 1e-12 and np.abs(Rw[6] - R7).max() <= 1e-12 and np.abs(tool - pt).max() <= 1e-12


def expected_link_spheres(m, radius, spacing):
    _, p, tool = model_arrays(m)
    rows = []
    for i in range(7):
        e = p[i + 1] if i < 6 else tool
        L = float(np.linalg.norm(e))
        k = int(np.ceil(L / spacing)) + 1 if L > 0 else 1
        for c in range(k):
            rows.append((i, (c / (k - 1) if k > 1 else 0.0) * e, radius))
    return rows


def test_link_spheres_follow_the_rule(M):
    for model in (M.default_model(), M.arm_models(((0.7, (0.2, -0.1, 0.05)),))[0]):
        for radius, spacing in ((0.06, 0.08), (0.03, 0.05), (0.1, 1.0)):
            got = M.link_spheres(model, radius, spacing)
            exp = expected_link_spheres(model, radius, spacing)
            assert got.shape[0] == len(exp)
            for g, (j, c, r) in zip(got, exp):
                assert g["joint"] == j and g["r"] == r and np.abs(g["c"] - c).max() <= 1e-15
    assert M.link_spheres(M.default_model(), 0.06, 0.08).shape[0] == 24
    # a yawed base moves the chain, not the skeleton (it is given in the joint frames); joint 0 starts at its own origin
    a = M.link_spheres(M.default_model(), 0.06, 0.08); b = M.link_spheres(M.arm_models(((0.7, (0.2, -0.1, 0.05)),))[0], 0.06, 0.08)
    assert np.array_equal(a["c"], b["c"])


def test_link_spheres_rejections(M):
    m = M.default_model()
    for radius, spacing, mx in ((0.0, 0.08, 64), (-0.1, 0.08, 64), (0.06, 0.0, 64), (0.06, -1.0, 64), (0.06, 0.08, 23), (float("nan"), 0.08, 64)):
        out = np.zeros(64, dtype=M.SPHERE_DTYPE); out["r"] = -7.0; n = C.c_int(-3)
        rc = M.lib().mpcmp_link_spheres(C.addressof(m), radius, spacing, mx, out.ctypes.data, C.addressof(n))
        assert rc == -1 and n.value == -3 and np.all(out["r"] == -7.0), (radius, spacing, mx)
    with pytest.raises(M.MpcmpError):
        M.link_spheres(m, 0.06, 0.08, max_spheres=10)


@pytest.mark.parametrize("narm", [1, 2])
@pytest.mark.parametrize("self_gap", [0, 3])
def test_clearance_config_matches_the_numpy_reference(M, narm, self_gap):
    models = [M.default_model()] if narm == 1 else list(M.arm_models(M.DUAL_BASES))
    tables = [M.link_spheres(m, 0.06, 0.08) for m in models]
    obs = host_scene(M)
    lim = o.default_limits()
    rng = np.random.default_rng(1000 + 10 * narm + self_gap)
    n = 240
    q = np.tile(lim["qmin"], narm) + rng.random((n, 7 * narm)) * np.tile(lim["qmax"] - lim["qmin"], narm)
    dob, drb = clearances_np(models, tables, obs, q, self_gap)
    # the reference itself exercises negative distances of the box and of the half-space (points inside / behind them), and robot pairs
    radii = np.concatenate([t["r"] for t in tables])
    assert (dob[:, :, 1] + radii).min() < -0.01 and (dob[:, :, 3] + radii).min() < -0.01
    assert np.isfinite(drb).any() == (narm == 2 or self_gap > 0)
    # the whole scene, and (where the pair set has robot pairs) the robot pairs alone, so that both kinds of winner are checked
    for with_obs in (True, False):
        if not with_obs and not np.isfinite(drb).any():
            continue
        ref = drb.reshape(n, -1).min(axis=1)
        if with_obs:
            ref = np.minimum(ref, dob.reshape(n, -1).min(axis=1))
        if with_obs:          # (a check of the reference alone: the minimum moves with the configuration.  Within one arm the skeleton's fixed
            assert np.unique(np.round(ref, 9)).shape[0] > n // 4          # pairs, coincident joint origins, decide the robot-only minimum)
        for i in range(n):
            d, sp, ot = M.clearance_config(models if narm == 2 else models[0], tables if narm == 2 else tables[0], obs if with_obs else None, q[i],
                                           self_gap)
            assert abs(d - ref[i]) <= 1e-12, (i, d, ref[i])
            assert 0 <= sp < dob.shape[1] and (with_obs or ot < 0)
            assert abs(named_pair_value(dob, drb, i, sp, ot) - ref[i]) <= 1e-12, (i, sp, ot)


def test_clearance_config_without_pairs_and_rejections(M):
    m = M.default_model(); sp = M.link_spheres(m, 0.06, 0.08); q = np.zeros(7)
    d, s, ot = M.clearance_config(m, sp, None, q)
    assert d == np.inf and s == -1 and ot == 0
    d, s, ot = M.clearance_config(m, sp[:0], host_scene(M), q)
    assert d == np.inf and s == -1
    bad = sp.copy(); bad["joint"][3] = 7
    with pytest.raises(M.MpcmpError):
        M.clearance_config(m, bad, host_scene(M), q)
    with pytest.raises(M.MpcmpError):
        M.clearance_config(m, sp, host_scene(M), q, self_gap=-1)
    with pytest.raises(M.MpcmpError):
        M.clearance_config(m, np.concatenate([sp, sp, sp]), None, q)       # 72 spheres on one arm


def test_record_layouts_match_the_header(M, tmp_path):
    import subprocess
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu %zu %zu\\n", sizeof(mpcmp_sphere), '
                   'sizeof(mpcmp_obstacle), sizeof(mpcmp_clearance), offsetof(mpcmp_sphere, r), offsetof(mpcmp_obstacle, r), '
                   'offsetof(mpcmp_clearance, sphere)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sz = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert sz == [M.SPHERE_DTYPE.itemsize, M.OBSTACLE_DTYPE.itemsize, M.CLEARANCE_DTYPE.itemsize, M.SPHERE_DTYPE.fields["r"][1],
                  M.OBSTACLE_DTYPE.fields["r"][1], M.CLEARANCE_DTYPE.fields["sphere"][1]], sz


def test_clearance_kernel_uses_no_scratch():
    """the compiler's resource remarks of clearance.hip, by the mechanism of tests/test_kernel_resources.py (hipcc cross-compiles: no GPU needed)"""
    import tempfile
    import test_kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        proc, _ = kr._compile("clearance.hip", [], tmp, "clr")
        _, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-3000:]
        res = kr._resources(err)
        hit = [(k, v) for k, v in res.items() if k.startswith("_ZN5mpcmp11k_clearance")]
        assert len(hit) == 1, list(res)
        name, v = hit[0]
        print("k_clearance: %d VGPRs, %d B of scratch per lane" % (v["vgpr"], v["scratch"]))
        assert v["scratch"] == 0 and v["vgpr"] <= 128, (name, v)
        for k, v in res.items():
            if "k_select" in k:
                assert v["scratch"] == 0, (k, v)
