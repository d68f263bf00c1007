"""Per-problem payloads, host side (include/mpcmp.h: mpcmp_model_add_payload, mpcmp_set_payloads): the lumping of a payload into body 7
against a NumPy restatement of the parallel-axis theorem, against the URDF reader (the payload as one more fixed link), and against the
physics of the static case; the rejections of bad payloads and the Python shape checks.  No GPU needed."""
import os

import numpy as np
import pytest

import oracle_py as o

# 0.5 - 3 kg with an off-axis COM and a full symmetric inertia (the Panda's rated payload is 3 kg)
I_FULL = np.array([[2.1e-3, 3.0e-4, -1.5e-4], [3.0e-4, 1.7e-3, 2.5e-4], [-1.5e-4, 2.5e-4, 2.6e-3]])
COM_OFF = np.array([0.012, -0.021, 0.287])


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    return M


def _arr(m, f):
    return np.array(getattr(m, f))


def _lumped_numpy(m, mass, com, I):
    """body 7 of m plus the payload, restated: total mass, mass-weighted COM, both inertias moved to the new COM"""
    M7, c7, I7 = m.mass[6], np.array(m.com[6][:]), np.array(m.I[6][:]).reshape(3, 3)
    Mt = M7 + mass
    c = (M7 * c7 + mass * np.asarray(com)) / Mt
    def shift(mk, ck):
        d = ck - c
        return mk * (d @ d * np.eye(3) - np.outer(d, d))
    It = I7 + shift(M7, c7) + np.asarray(I) + shift(mass, np.asarray(com))
    return Mt, c, It


@pytest.mark.parametrize("mass", [0.5, 2.0, 3.0])
def test_add_payload_matches_parallel_axis(M, mass):
    base = M.default_model()
    out = M.model_add_payload(base, M.payload(mass, COM_OFF, I_FULL))
    Mt, c, It = _lumped_numpy(base, mass, COM_OFF, I_FULL)
    assert abs(out.mass[6] - Mt) <= 1e-14 * Mt
    assert np.abs(np.array(out.com[6][:]) - c).max() <= 1e-14 * np.abs(c).max()
    assert np.abs(np.array(out.I[6][:]).reshape(3, 3) - It).max() <= 1e-14 * np.abs(It).max()
    # the other bodies and the frames are untouched, bit for bit
    for f in ["R0", "p", "tool", "link8", "gravity"]:
        assert _arr(out, f).tobytes() == _arr(base, f).tobytes(), f
    for f in ["mass", "com", "I"]:
        assert _arr(out, f)[:6].tobytes() == _arr(base, f)[:6].tobytes(), f


def test_zero_payload_returns_the_model_bitwise(M):
    base = M.default_model()
    for com in ((0.0, 0.0, 0.0), COM_OFF):
        out = M.model_add_payload(base, M.payload(0.0, com, np.zeros((3, 3))))
        assert bytes(out) == bytes(base)
    # a payload with a mass changes body 7, and m == out (in place) gives the same result as a separate output
    p = M.payload(1.5, COM_OFF, I_FULL)
    a = M.model_add_payload(base, p)
    assert bytes(a) != bytes(base)
    import ctypes as C
    inplace = M.Model.from_buffer_copy(base)
    assert M.lib().mpcmp_model_add_payload(C.byref(inplace), C.byref(p), C.byref(inplace)) == 0
    assert bytes(inplace) == bytes(a)


def test_payload_as_urdf_link_matches_add_payload(M, tmp_path, golden_dir):
    """the Panda URDF with one more fixed link under panda_tool that holds the payload, read by mpcmp_model_from_urdf, equals
    add_payload(model_from_urdf(plain URDF), payload) (within 1e-12: the reader lumps four bodies in one sum, add_payload one onto the
    lumped three)"""
    plain = os.path.join(golden_dir, "panda_arm.urdf")
    txt = open(plain).read()
    mass = 2.0
    tool_z = 0.107 + 0.15                                  # panda_tool in the joint-7 frame (panda_joint8 + panda_joint9, unrotated)
    org = COM_OFF - np.array([0.0, 0.0, tool_z])
    I = I_FULL
    link = ('  <link name="payload">\n    <inertial>\n      <origin rpy="0 0 0" xyz="%r %r %r"/>\n      <mass value="%r"/>\n'
            '      <inertia ixx="%r" ixy="%r" ixz="%r" iyy="%r" iyz="%r" izz="%r"/>\n    </inertial>\n  </link>\n'
            '  <joint name="payload_joint" type="fixed">\n    <origin rpy="0 0 0" xyz="0 0 0"/>\n    <parent link="panda_tool"/>\n'
            '    <child link="payload"/>\n    <axis xyz="0 0 0"/>\n  </joint>\n'
            % tuple(float(v) for v in (org[0], org[1], org[2], mass, I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2])))
    p = str(tmp_path / "panda_payload.urdf")
    open(p, "w").write(txt.replace("</robot>", link + "</robot>"))
    loaded = M.model_from_urdf(p)
    ref = M.model_add_payload(M.model_from_urdf(plain), M.payload(mass, COM_OFF, I_FULL))
    for f in ["R0", "p", "mass", "com", "I", "tool", "link8", "gravity"]:
        a, b = _arr(loaded, f), _arr(ref, f)
        assert np.abs(a - b).max() <= 1e-12 * max(1.0, np.abs(b).max()), (f, np.abs(a - b).max())


def test_static_torque_is_the_payload_weight_through_the_jacobian(M):
    """tau(lumped, q, 0, 0) - tau(base, q, 0, 0) = J_v(q, c)^T (0, 0, m g): a payload at rest only adds its weight at its COM"""
    base = M.default_model()
    mass = 3.0
    lumped = M.model_add_payload(base, M.payload(mass, COM_OFF, I_FULL))
    ob, ol = o.Model.from_buffer_copy(base), o.Model.from_buffer_copy(lumped)
    lim = o.default_limits()
    rng = np.random.default_rng(2024)
    z = np.zeros(7)
    for _ in range(100):
        q = rng.uniform(lim["qmin"], lim["qmax"])
        dtau = o.rnea(q, z, z, model=ol) - o.rnea(q, z, z, model=ob)
        Jv = o.frame_jacobian(q, COM_OFF, model=ob)[:3]
        expect = Jv.T @ np.array([0.0, 0.0, mass * 9.81])
        assert np.abs(dtau - expect).max() <= 1e-10, (q, dtau, expect)


def test_bad_payloads_are_rejected(M):
    base = M.default_model()
    bad = [M.payload(-0.1, COM_OFF, I_FULL), M.payload(float("nan"), COM_OFF, I_FULL), M.payload(float("inf"), COM_OFF, I_FULL),
           M.payload(1.0, (0.0, float("nan"), 0.2), I_FULL)]
    asym = I_FULL.copy(); asym[0, 1] += 1e-6
    bad.append(M.payload(1.0, COM_OFF, asym))
    negd = I_FULL.copy(); negd[2, 2] = -1e-4
    bad.append(M.payload(1.0, COM_OFF, negd))
    nan_i = I_FULL.copy(); nan_i[1, 1] = float("nan")
    bad.append(M.payload(1.0, COM_OFF, nan_i))
    for p in bad:
        with pytest.raises(M.MpcmpError) as e:
            M.model_add_payload(base, p)
        assert e.value.code == -1                 # MPCMP_EINVAL


def test_payload_table_shapes(M):
    """Solver.payload_table: [n] / [n,3] / [n,3,3] for one arm, [n,narm] / [n,narm,3] / [n,narm,3,3] for more; com defaults to the tool
    point and inertia to 0; a wrong shape raises ValueError before anything reaches the library (no GPU needed: the table is built on the
    host, on an object that never created a context)"""
    s = M.Solver.__new__(M.Solver)
    s.narm = 1
    s._models = [M.default_model()]
    t = s.payload_table([0.0, 2.0], [[0, 0, 0.2], [0.01, 0, 0.25]], np.stack([np.zeros((3, 3)), I_FULL]))
    assert t.shape == (2, 1) and t.dtype.itemsize == 104
    assert np.array_equal(t["I"][1, 0], I_FULL.ravel()) and t["mass"][1, 0] == 2.0
    t = s.payload_table(np.array([1.0, 2.0, 3.0]))
    assert np.array_equal(t["com"][:, 0], np.tile([0.0, 0.0, 0.257], (3, 1))) and not t["I"].any()
    for args in (([[1.0, 2.0]], None, None), ([1.0], [0, 0, 0.2], None), ([1.0], None, np.eye(3)), ([1.0, 2.0], np.zeros((3, 3)), None),
                 (np.zeros((0,)), None, None)):
        with pytest.raises(ValueError):
            s.payload_table(*args)
    s.narm = 2
    s._models = [M.default_model(), M.default_model()]
    t = s.payload_table(np.ones((4, 2)), np.zeros((4, 2, 3)), np.zeros((4, 2, 3, 3)))
    assert t.shape == (4, 2)
    for args in ((np.ones(4), None, None), (np.ones((4, 2)), np.zeros((4, 3)), None), (np.ones((4, 2)), None, np.zeros((4, 3, 3)))):
        with pytest.raises(ValueError):
            s.payload_table(*args)


def test_payload_symbols_exported(M):
    import ctypes as C
    assert C.sizeof(M.capi.Payload) == 104 and M.Solver.PAYLOAD_DTYPE.itemsize == 104
