"""General URDF reader (mpcmp_models_from_urdf; reference: robot_utils/pandaWrapper.cpp:3-12 hands any URDF to Pinocchio).
CPU only: the reader is host code of libmpcmp.so.  The expectations are computed independently in numpy from the same numbers
the URDF text holds (transform composition, inertia rotation, parallel-axis lumping, chain forward kinematics)."""
import os

import numpy as np
import pytest

import oracle_py as o
from robots import chain_fk_tool, expected, fl, make_spec, rot_axis, rpy_R, write_urdf, xf


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as m
    if not os.path.exists(m.library_path()):
        pytest.skip("libmpcmp.so not built")
    return m


def check_models(M, models, chains, tol=1e-12):
    assert len(models) == len(chains)
    for m, ch in zip(models, chains):
        e = expected(ch)
        for i in range(7):
            assert np.abs(np.array(m.R0[i][:]).reshape(3, 3) - e["R0"][i]).max() < tol
            assert np.abs(np.array(m.p[i][:]) - e["p"][i]).max() < tol
            assert abs(m.mass[i] - e["mass"][i]) < tol
            assert np.abs(np.array(m.com[i][:]) - e["com"][i]).max() < tol
            assert np.abs(np.array(m.I[i][:]).reshape(3, 3) - e["I"][i]).max() < tol
        assert np.abs(np.array(m.tool[:]) - e["tool"]).max() < tol and np.abs(np.array(m.link8[:]) - e["link8"]).max() < tol
        assert m.gravity[2] == -9.81


def test_two_arm_urdf_rotated_everything(M, tmp_path):
    """two chains on one base; rotated base placements, fixed joints (one between revolute joints), inertial frames and tool frame"""
    rng = np.random.default_rng(5)
    chains = make_spec(rng, 2, rotated=True)
    p = str(tmp_path / "two_arm.urdf"); write_urdf(p, chains)
    models = M.models_from_urdf(p)
    check_models(M, models, chains)
    # kinematics of the reader's model == kinematics of the URDF (host FK of the product library)
    for m, ch in zip(models, chains):
        for _ in range(5):
            q = rng.uniform(-2, 2, 7)
            _, ptool, _ = M.tool_jacobian(m, q)
            assert np.abs(ptool - chain_fk_tool(ch, q)).max() < 1e-12
    with pytest.raises(M.MpcmpError):          # the single-chain entry point refuses a two-chain robot
        M.model_from_urdf(p)


def test_general_joint_axes(M, tmp_path):
    """axes other than +z (-z, x, y, oblique) are absorbed by a constant rotation of the child frame"""
    rng = np.random.default_rng(6)
    axes = [(0, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.3, -0.5, 0.8), (0, -1, 0), (-1, 0, 0)]
    chains = make_spec(rng, 1, rotated=True, axes=axes)
    p = str(tmp_path / "axes.urdf"); write_urdf(p, chains)
    models = M.models_from_urdf(p)
    check_models(M, models, chains)
    for _ in range(8):
        q = rng.uniform(-2, 2, 7)
        _, ptool, _ = M.tool_jacobian(models[0], q)
        assert np.abs(ptool - chain_fk_tool(chains[0], q)).max() < 1e-12
    # gravity torques: the product's model through the oracle's RNEA == finite differences of the potential energy of the URDF's bodies
    ch = chains[0]
    def potential(q):
        T = xf(*ch["base"]); U = 0.0
        for i in range(7):
            if i == 3:
                T = T @ xf(*ch["mid_T"]); U += 9.81 * ch["mid"]["m"] * (T[:3, :3] @ ch["mid"]["com"] + T[:3, 3])[2]
            j = ch["joints"][i]
            R = np.eye(4); R[:3, :3] = rot_axis(j["axis"], q[i])
            T = T @ xf(j["xyz"], j["rpy"]) @ R
            U += 9.81 * ch["links"][i]["m"] * (T[:3, :3] @ ch["links"][i]["com"] + T[:3, 3])[2]
        T1 = T @ xf(*ch["f1_T"]); U += 9.81 * ch["f1"]["m"] * (T1[:3, :3] @ ch["f1"]["com"] + T1[:3, 3])[2]
        T2 = T1 @ xf(*ch["f2_T"]); U += 9.81 * ch["f2"]["m"] * (T2[:3, :3] @ ch["f2"]["com"] + T2[:3, 3])[2]
        return U
    om = o.Model.from_buffer_copy(models[0])
    q = rng.uniform(-1.5, 1.5, 7)
    tau = o.rnea(q, np.zeros(7), np.zeros(7), model=om)
    g = np.array([(potential(q + 1e-6 * np.eye(7)[i]) - potential(q - 1e-6 * np.eye(7)[i])) / 2e-6 for i in range(7)])
    assert np.abs(tau - g).max() < 1e-6 * max(1.0, np.abs(g).max())


def test_unrotated_urdf_is_bit_exact(M, tmp_path):
    """without rotated fixed joints / inertial frames the reader hands the numbers of the file through unchanged (identity factors
    are skipped), as the round-1 reader did for panda_arm.urdf"""
    rng = np.random.default_rng(7)
    chains = make_spec(rng, 1, rotated=False)
    chains[0]["base"] = (np.zeros(3), (0.0, 0.0, 0.0))
    chains[0]["mid_T"] = (np.zeros(3), (0.0, 0.0, 0.0)); chains[0]["mid"]["m"] = 0.0; chains[0]["mid"]["I"] = np.zeros((3, 3))
    p = str(tmp_path / "plain.urdf"); write_urdf(p, chains)
    m = M.model_from_urdf(p)
    ch = chains[0]
    for i in (0, 1, 3, 4, 5):       # (the third joint frame carries the massless intermediate link: lumped; the seventh the tool bodies)
        assert np.array_equal(np.array(m.p[i][:]), ch["joints"][i]["xyz"])
        assert np.array_equal(np.array(m.R0[i][:]).reshape(3, 3), rpy_R(ch["joints"][i]["rpy"]))
        assert m.mass[i] == ch["links"][i]["m"] and np.array_equal(np.array(m.com[i][:]), ch["links"][i]["com"])
        I = ch["links"][i]["I"]
        assert np.array_equal(np.array(m.I[i][:]).reshape(3, 3), np.array([[I[0, 0], I[0, 1], I[0, 2]], [I[0, 1], I[1, 1], I[1, 2]], [I[0, 2], I[1, 2], I[2, 2]]]))


def test_reader_rejections(M, tmp_path):
    rng = np.random.default_rng(8)
    chains = make_spec(rng, 1)
    p = str(tmp_path / "ok.urdf"); write_urdf(p, chains)
    txt = open(p).read()
    bad = str(tmp_path / "prismatic.urdf"); open(bad, "w").write(txt.replace('name="c0_j3" type="revolute"', 'name="c0_j3" type="prismatic"'))
    with pytest.raises(M.MpcmpError):
        M.models_from_urdf(bad)
    six = str(tmp_path / "six.urdf"); open(six, "w").write(txt.replace('name="c0_j7" type="revolute"', 'name="c0_j7" type="fixed"'))
    with pytest.raises(M.MpcmpError):
        M.models_from_urdf(six)
    # a second revolute joint hanging on link 2: a tree, not a serial chain
    branch = txt.replace("</robot>", '<link name="extra"/><joint name="jx" type="revolute"><parent link="c0_l2"/><child link="extra"/><axis xyz="0 0 1"/></joint></robot>')
    br = str(tmp_path / "branch.urdf"); open(br, "w").write(branch)
    with pytest.raises(M.MpcmpError):
        M.models_from_urdf(br)
    three = make_spec(rng, 3)
    p3 = str(tmp_path / "three.urdf"); write_urdf(p3, three)
    with pytest.raises(M.MpcmpError):
        M.models_from_urdf(p3, max_chains=2)
    assert len(M.models_from_urdf(p3)) == 3


def test_dual_panda_urdf_matches_arm_models(M, tmp_path):
    """the dual-arm robot of BASELINE.json configs[3] (two compiled-in Pandas on one base, capi.DUAL_BASES) written as ONE URDF
    gives the models the benches and GPU tests build with arm_models()"""
    d = M.default_model()
    x = ['<robot name="dual">', '<link name="world"/>']
    for a, (yaw, xyz) in enumerate(M.DUAL_BASES):
        n = "a%d_" % a
        x.append('<link name="%slink0"/><joint name="%smount" type="fixed"><origin xyz="%r %r %r" rpy="0 0 %r"/><parent link="world"/><child link="%slink0"/></joint>'
                 % (n, n, *fl(xyz), float(yaw), n))
        parent = n + "link0"
        for i in range(7):
            R = np.array(d.R0[i][:]).reshape(3, 3)
            rpy = (float(np.arctan2(R[2, 1], R[2, 2])), float(-np.arcsin(R[2, 0])), float(np.arctan2(R[1, 0], R[0, 0])))
            I = np.array(d.I[i][:]).reshape(3, 3)
            x.append('<link name="%slink%d"><inertial><origin xyz="%r %r %r"/><mass value="%r"/><inertia ixx="%r" ixy="%r" ixz="%r" iyy="%r" iyz="%r" izz="%r"/></inertial></link>'
                     % (n, i + 1, *fl(d.com[i][:]), float(d.mass[i]), *fl((I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]))))
            x.append('<joint name="%sjoint%d" type="revolute"><origin xyz="%r %r %r" rpy="%r %r %r"/><parent link="%s"/><child link="%slink%d"/><axis xyz="0 0 1"/></joint>'
                     % (n, i + 1, *fl(d.p[i][:]), *rpy, parent, n, i + 1))
            parent = "%slink%d" % (n, i + 1)
        x.append('<link name="%slink8"/><joint name="%sj8" type="fixed"><origin xyz="%r %r %r"/><parent link="%s"/><child link="%slink8"/></joint>'
                 % (n, n, *fl(d.link8[:]), parent, n))
        off = np.array(d.tool[:]) - np.array(d.link8[:])
        x.append('<link name="%stool"/><joint name="%sjt" type="fixed"><origin xyz="%r %r %r"/><parent link="%slink8"/><child link="%stool"/></joint>'
                 % (n, n, *fl(off), n, n))
    x.append("</robot>")
    p = str(tmp_path / "dual_panda.urdf"); open(p, "w").write("\n".join(x))
    got, want = M.models_from_urdf(p), M.arm_models(M.DUAL_BASES)
    assert len(got) == 2
    for g, w in zip(got, want):
        for f in ["R0", "p", "mass", "com", "I", "tool", "link8", "gravity"]:
            assert np.abs(np.array(getattr(g, f)) - np.array(getattr(w, f))).max() < 1e-15, f
