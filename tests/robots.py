"""Robots for the tests: random serial 7-revolute chains written as URDF text (rotated joint frames, oblique axes, a fixed intermediate link, full
inertia tensors, several chains on one base), the model fields the reader must make of them computed independently in numpy, and general_models():
such robots read back through models_from_urdf, scaled so that their torques stay inside the Panda limits the configurations apply."""
import numpy as np


def rpy_R(rpy):
    r, p, y = rpy
    cr, sr, cp, sp, cy, sy = np.cos(r), np.sin(r), np.cos(p), np.sin(p), np.cos(y), np.sin(y)
    return np.array([[cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr],
                     [sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr],
                     [-sp, cp * sr, cp * cr]])


def xf(xyz=(0, 0, 0), rpy=(0, 0, 0)):
    T = np.eye(4); T[:3, :3] = rpy_R(rpy); T[:3, 3] = xyz
    return T


def axis_R(a):
    a = np.asarray(a, float) / np.linalg.norm(a)
    z = np.array([0.0, 0.0, 1.0])
    if np.allclose(a, z):
        return np.eye(3)
    if np.allclose(a, -z):
        return np.diag([1.0, -1.0, -1.0])
    v = np.cross(z, a); c = a[2]
    V = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + V + V @ V / (1.0 + c)


def rot_axis(a, q):
    a = np.asarray(a, float) / np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(q) * K + (1 - np.cos(q)) * K @ K


def fl(seq):
    """plain Python floats (numpy 2 prints np.float64(...) under %r)"""
    return tuple(float(v) for v in seq)


def inertial_xml(b):
    I = b["I"]
    return ('<inertial><origin xyz="%r %r %r" rpy="%r %r %r"/><mass value="%r"/>'
            '<inertia ixx="%r" ixy="%r" ixz="%r" iyy="%r" iyz="%r" izz="%r"/></inertial>'
            % (*fl(b["com"]), *fl(b["irpy"]), float(b["m"]), *fl((I[0, 0], I[0, 1], I[0, 2], I[1, 1], I[1, 2], I[2, 2]))))


def make_spec(rng, n_chains, rotated=True, axes=None):
    """random robot: a base link, per chain a fixed base joint, seven revolute joints (a fixed, possibly rotated, intermediate
    link between joints 3 and 4), and two fixed frames behind joint 7 (the second one rotated)"""
    chains = []
    for c in range(n_chains):
        def body():
            A = rng.normal(size=(3, 3)); I = A @ A.T * 0.01 + np.eye(3) * 0.02
            return {"m": float(rng.uniform(0.5, 4)), "com": rng.normal(size=3) * 0.05,
                    "irpy": rng.normal(size=3) * (0.5 if rotated else 0.0), "I": I}
        ch = {"base": (rng.normal(size=3), (0.0, 0.0, float(rng.uniform(-3, 3))) if rotated else (0.0, 0.0, 0.0)),
              "joints": [], "links": [body() for _ in range(7)], "mid": body(), "mid_T": (rng.normal(size=3) * 0.1, rng.normal(size=3) * (0.4 if rotated else 0.0)),
              "f1": body(), "f1_T": (np.array([0.0, 0.0, 0.1]), (0.0, 0.0, 0.0)), "f2": body(), "f2_T": (rng.normal(size=3) * 0.1, rng.normal(size=3) * (0.6 if rotated else 0.0))}
        for i in range(7):
            ax = (0.0, 0.0, 1.0) if axes is None else axes[i]
            ch["joints"].append({"xyz": rng.normal(size=3) * 0.2, "rpy": rng.choice([-np.pi / 2, 0.0, np.pi / 2], size=3) if not rotated else rng.normal(size=3), "axis": ax})
        chains.append(ch)
    return chains


def write_urdf(path, chains):
    x = ['<?xml version="1.0"?>', '<robot name="t">', '<link name="base"/>']
    for c, ch in enumerate(chains):
        n = "c%d_" % c
        x.append('<link name="%sl0"/>' % n)
        x.append('<joint name="%sbase" type="fixed"><origin xyz="%r %r %r" rpy="%r %r %r"/><parent link="base"/><child link="%sl0"/></joint>'
                 % (n, *fl(ch["base"][0]), *fl(ch["base"][1]), n))
        parent = n + "l0"
        for i in range(7):
            j = ch["joints"][i]
            if i == 3:      # a fixed intermediate link between joints 3 and 4 (hangs on joint frame 3)
                x.append('<link name="%smid">%s</link>' % (n, inertial_xml(ch["mid"])))
                x.append('<joint name="%smidj" type="fixed"><origin xyz="%r %r %r" rpy="%r %r %r"/><parent link="%s"/><child link="%smid"/></joint>'
                         % (n, *fl(ch["mid_T"][0]), *fl(ch["mid_T"][1]), parent, n))
                parent = n + "mid"
            x.append('<link name="%sl%d">%s</link>' % (n, i + 1, inertial_xml(ch["links"][i])))
            x.append('<joint name="%sj%d" type="revolute"><origin xyz="%r %r %r" rpy="%r %r %r"/><parent link="%s"/><child link="%sl%d"/>'
                     '<axis xyz="%r %r %r"/><limit lower="-2" upper="2" effort="10" velocity="2"/></joint>'
                     % (n, i + 1, *fl(j["xyz"]), *fl(j["rpy"]), parent, n, i + 1, *fl(j["axis"])))
            parent = "%sl%d" % (n, i + 1)
        for k, nm in ((1, "f1"), (2, "f2")):
            x.append('<link name="%s%s">%s</link>' % (n, nm, inertial_xml(ch[nm])))
            x.append('<joint name="%s%sj" type="fixed"><origin xyz="%r %r %r" rpy="%r %r %r"/><parent link="%s"/><child link="%s%s"/></joint>'
                     % (n, nm, *fl(ch[nm + "_T"][0]), *fl(ch[nm + "_T"][1]), parent, n, nm))
            parent = n + nm
    x.append("</robot>")
    open(path, "w").write("\n".join(x))


def expected(ch):
    """model fields of one chain, numpy"""
    out = {"R0": [], "p": [], "mass": [], "com": [], "I": []}
    C = xf(*ch["base"])                        # link frame in the current model frame
    bodies = None
    def add(body, C):
        R = C[:3, :3] @ rpy_R(body["irpy"])
        bodies.append((body["m"], C[:3, :3] @ body["com"] + C[:3, 3], R @ body["I"] @ R.T))
    def flush():
        M_ = sum(b[0] for b in bodies); c = sum(b[0] * b[1] for b in bodies) / M_
        I = sum(b[2] + b[0] * (np.dot(b[1] - c, b[1] - c) * np.eye(3) - np.outer(b[1] - c, b[1] - c)) for b in bodies)
        out["mass"].append(M_); out["com"].append(c); out["I"].append(I)
    for i in range(7):
        if i == 3:
            C = C @ xf(*ch["mid_T"]); add(ch["mid"], C)
        j = ch["joints"][i]
        Ra = np.eye(4); Ra[:3, :3] = axis_R(j["axis"])
        P = C @ xf(j["xyz"], j["rpy"]) @ Ra
        out["R0"].append(P[:3, :3]); out["p"].append(P[:3, 3])
        if bodies is not None:
            flush()
        bodies = []
        C = np.linalg.inv(Ra)
        add(ch["links"][i], C)
    C1 = C @ xf(*ch["f1_T"]); add(ch["f1"], C1)
    C2 = C1 @ xf(*ch["f2_T"]); add(ch["f2"], C2)
    flush()
    out["link8"] = C1[:3, 3]; out["tool"] = C2[:3, 3]
    return out


def chain_fk_tool(ch, q):
    T = xf(*ch["base"])
    for i in range(7):
        if i == 3:
            T = T @ xf(*ch["mid_T"])
        j = ch["joints"][i]
        R = np.eye(4); R[:3, :3] = rot_axis(j["axis"], q[i])
        T = T @ xf(j["xyz"], j["rpy"]) @ R
    return (T @ xf(*ch["f1_T"]) @ xf(*ch["f2_T"]))[:3, 3]


# the axes of test_general_joint_axes: -z, x, y, +z, one oblique, -y, -x
OBLIQUE_AXES = [(0, 0, -1), (1, 0, 0), (0, 1, 0), (0, 0, 1), (0.3, -0.5, 0.8), (0, -1, 0), (-1, 0, 0)]
TILTED_GRAVITY = (1.2, -2.3, -9.0)
MASS_SCALE, LENGTH_SCALE = 0.2, 0.5


def scale_spec(chains, mass=MASS_SCALE, length=LENGTH_SCALE):
    """make_spec draws ten bodies of 0.5 .. 4 kg per chain on lever arms of a few 0.1 m: about 100 N m of static torque at the first joints and
    30 N m at the last three, above the Panda limits (87 and 12 N m) every configuration applies.  Masses x 0.2 and lengths x 0.5 (inertias
    x 0.2 x 0.25) leave about a tenth of that: roughly 2.2 kg behind joint 5 on 0.15 m, 3 N m static against 12."""
    for ch in chains:
        for b in ch["links"] + [ch["mid"], ch["f1"], ch["f2"]]:
            b["m"] *= mass; b["com"] = b["com"] * length; b["I"] = b["I"] * (mass * length * length)
        for j in ch["joints"]:
            j["xyz"] = j["xyz"] * length
        for k in ("mid_T", "f1_T", "f2_T"):
            ch[k] = (np.asarray(ch[k][0]) * length, ch[k][1])
    return chains


def general_spec(seed, n_chains):
    """the chains general_models writes: everything rotated; chain 0 turns about OBLIQUE_AXES, every further chain about random unit axes;
    bodies, placements and base yaws differ per chain (one random stream); the bases stand 0.7 m apart, 1 m above the floor of the height row"""
    rng = np.random.default_rng(seed)
    chains = scale_spec(make_spec(rng, n_chains, rotated=True, axes=OBLIQUE_AXES))
    for c, ch in enumerate(chains):
        ch["base"] = (np.array([0.7 * c, 0.1 * c, 1.0]), ch["base"][1])
        if c > 0:
            for j in ch["joints"]:
                a = rng.normal(size=3); j["axis"] = fl(a / np.linalg.norm(a))
    return chains


def general_models(M, tmp_path, seed, n_chains=1, gravity=None):
    """ctypes array of n_chains Models: general_spec(seed, n_chains) written as one URDF and read back through M.models_from_urdf;
    gravity (3 numbers, e.g. TILTED_GRAVITY) is set on every struct after reading.  Returns (models, chains)"""
    chains = general_spec(seed, n_chains)
    path = str(tmp_path / ("general_%d_%d.urdf" % (seed, n_chains)))
    write_urdf(path, chains)
    models = M.models_from_urdf(path)
    assert len(models) == n_chains
    if gravity is not None:
        for m in models:
            for d in range(3):
                m.gravity[d] = float(gravity[d])
    return models, chains


def tilted_gravity_models(M, tmp_path, seed, n_chains=1):
    """general_models under a gravity vector with all three components"""
    return general_models(M, tmp_path, seed, n_chains, gravity=TILTED_GRAVITY)
