"""Voxel worlds (include/mpcmp_field.h), the part that needs no GPU: the exact transform mpcmp_field_edt against brute force and SciPy, the distance
mpcmp_field_sd against its properties and its NumPy restatement, mpcmp_clearance_field_config against NumPy, the ABI table, the self-test under the
host sanitizers and the compiler's resource remarks of the kernels.

Bounds.  The transform is integer: bit-exact.  The distance: 1e-12 against the restatement (a handful of double operations on values below 10^2);
soundness sd <= true + 1e-12 and tightness true - sd <= (3 sqrt(3)/2) h + 1e-12 are the header's statements with the same rounding allowance."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import field_reference as F
from test_clearance_host import sphere_centres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


def occupancy(shape, kind, rng):
    """shape = (n0, n1, n2); the array is [n2][n1][n0]"""
    dims = shape[::-1]
    if kind == "none":
        return np.zeros(dims, dtype=np.uint8)
    if kind == "all":
        return np.ones(dims, dtype=np.uint8)
    if kind == "one":
        occ = np.zeros(dims, dtype=np.uint8)
        occ.reshape(-1)[rng.integers(occ.size)] = 1
        return occ
    return (rng.random(dims) < {"1%": 0.01, "50%": 0.5}[kind]).astype(np.uint8)


def test_reference_transform_is_the_brute_force_minimum():
    """the reference checks itself: SciPy's transform squared and rounded = min |v - w|^2 on tiny grids"""
    rng = np.random.default_rng(3)
    for shape in ((1, 1, 1), (7, 1, 1), (1, 9, 1), (1, 1, 11), (5, 6, 7), (9, 8, 3)):
        for kind in ("none", "one", "1%", "50%", "all"):
            occ = occupancy(shape, kind, rng)
            assert np.array_equal(F.edt(occ), F.edt_brute(occ)), (shape, kind)


@pytest.mark.parametrize("shape", [(1, 1, 1), (7, 1, 1), (1, 9, 1), (1, 1, 11), (5, 6, 7)])
@pytest.mark.parametrize("kind", ["none", "one", "1%", "50%", "all"])
def test_edt_is_bit_exact_against_brute_force(M, shape, kind):
    rng = np.random.default_rng(11 + sum(shape))
    occ = occupancy(shape, kind, rng)
    got = M.field_edt(M.field_desc((0.1, -0.2, 0.3), 0.05, shape), occ)
    assert got.dtype == np.uint32 and got.shape == occ.shape
    assert np.array_equal(got, F.edt_brute(occ))
    if not occ.any():
        assert np.all(got == M.FIELD_EMPTY) and M.FIELD_EMPTY == 0xFFFFFFFF


def test_edt_is_bit_exact_against_scipy(M):
    rng = np.random.default_rng(5)
    shape = (40, 33, 21)
    for p in (0.002, 0.05, 0.5):
        occ = (rng.random(shape[::-1]) < p).astype(np.uint8)
        assert occ.any()
        assert np.array_equal(M.field_edt(M.field_desc((0, 0, 0), 0.02, shape), occ), F.edt(occ)), p


def test_edt_and_sd_rejections(M):
    from mpc_motion_planner_amd.capi import host
    occ = np.ones(8, dtype=np.uint8)
    for what, (origin, h, n) in (("n 0", ((0, 0, 0), 0.1, (0, 2, 2))), ("n 1025", ((0, 0, 0), 0.1, (1025, 1, 1))), ("h 0", ((0, 0, 0), 0.0, (2, 2, 2))),
                                 ("h < 0", ((0, 0, 0), -0.1, (2, 2, 2))), ("h inf", ((0, 0, 0), np.inf, (2, 2, 2))),
                                 ("h nan", ((0, 0, 0), np.nan, (2, 2, 2))), ("origin nan", ((0, np.nan, 0), 0.1, (2, 2, 2))),
                                 ("2^24 + 1024 voxels", ((0, 0, 0), 0.1, (1024, 1024, 17)))):
        d = M.field_desc(origin, h, n)
        d2 = np.full(8, 7, dtype=np.uint32)
        assert M.lib().mpcmp_field_edt(d.ctypes.data, host(occ), host(d2)) == EINVAL and np.all(d2 == 7), what
        sd, x = C.c_double(77.0), np.zeros(3)
        assert M.lib().mpcmp_field_sd(d.ctypes.data, host(d2), host(x), C.byref(sd), None) == EINVAL and sd.value == 77.0, what
    good = M.field_desc((0, 0, 0), 0.1, (2, 2, 2))
    d2 = np.full(8, 7, dtype=np.uint32)
    assert M.lib().mpcmp_field_edt(None, host(occ), host(d2)) == EINVAL and M.lib().mpcmp_field_edt(good.ctypes.data, None, host(d2)) == EINVAL
    assert M.lib().mpcmp_field_edt(good.ctypes.data, host(occ), None) == EINVAL and np.all(d2 == 7)
    sd = C.c_double(77.0)
    for x in ((np.nan, 0, 0), (0, np.inf, 0)):
        xx = np.array(x, dtype=np.float64)
        assert M.lib().mpcmp_field_sd(good.ctypes.data, host(d2), host(xx), C.byref(sd), None) == EINVAL and sd.value == 77.0
    assert M.lib().mpcmp_field_edt(good.ctypes.data, host(occ), host(d2)) == 0 and np.all(d2 == 0)
    with pytest.raises(ValueError):
        M.field_edt(good, np.ones(9))


# ---- the distance of a point ------------------------------------------------------------------------------------------------------------------
GRID = ((-0.213, 0.107, 0.019), 0.05, (12, 10, 8))


@pytest.fixture(scope="module")
def sd_case(M):
    origin, h, n = GRID
    rng = np.random.default_rng(20261020)
    occ = np.zeros(n[::-1], dtype=np.uint8)
    occ.reshape(-1)[rng.choice(occ.size, 20, replace=False)] = 1
    d2 = M.field_edt(M.field_desc(origin, h, n), occ)
    lo, hi = np.asarray(origin) - 5 * h, np.asarray(origin) + h * (np.asarray(n) + 5)
    x = lo + rng.random((2000, 3)) * (hi - lo)
    x[:40] = np.asarray(origin) + h * (np.argwhere(occ)[rng.integers(20, size=40)][:, ::-1] + rng.random((40, 3)))      # (inside occupied voxels)
    got = np.array([M.field_sd(M.field_desc(origin, h, n), d2, p) for p in x])
    return dict(occ=occ, d2=d2, x=x, sd=got[:, 0], vox=got[:, 1].astype(np.int64), true=F.true_distance(origin, h, occ, x))


def test_sd_is_a_lower_bound_everywhere(M, sd_case):
    """soundness for all points, in and up to 5 h outside the grid; negative inside an occupied voxel; sd <= max(true, 0)"""
    c = sd_case
    assert np.array_equal(c["d2"], F.edt(c["occ"]))
    assert np.all(c["sd"] <= c["true"] + 1e-12), float((c["sd"] - c["true"]).max())
    assert np.all(c["sd"] <= np.maximum(c["true"], 0.0) + 1e-12)
    inside_solid = c["true"] == 0.0
    assert inside_solid.sum() >= 40 and np.all(c["sd"][inside_solid] < 0.0)
    print("true - sd: %.4f .. %.4f (h = %.2f)" % ((c["true"] - c["sd"]).min(), (c["true"] - c["sd"]).max(), GRID[1]))


def test_sd_is_within_the_stated_gap_inside_the_grid(M, sd_case):
    origin, h, n = GRID
    c = sd_case
    u = (c["x"] - np.asarray(origin)) / h
    inside = np.all((u >= 0) & (u <= np.asarray(n)), axis=1)
    assert 200 <= inside.sum() <= 1800
    assert np.all((c["true"] - c["sd"])[inside] <= 1.5 * np.sqrt(3.0) * h + 1e-12), float((c["true"] - c["sd"])[inside].max())


def test_sd_matches_the_numpy_restatement(M, sd_case):
    origin, h, n = GRID
    c = sd_case
    sd, vox = F.sd_field(origin, h, n, c["d2"], c["x"])
    robust = F.face_distance(origin, h, n, c["x"]) > 1e-9
    assert robust.sum() >= 1990
    assert np.array_equal(c["vox"][robust], vox[robust])
    assert np.abs(c["sd"] - sd)[robust].max() <= 1e-12
    # an empty field is +inf everywhere, and the voxel is still the one the point falls in
    e2 = np.full(c["d2"].shape, M.FIELD_EMPTY, dtype=np.uint32)
    s, v = M.field_sd(M.field_desc(origin, h, n), e2, c["x"][100])
    assert s == np.inf and v == vox[100]
    # the corners of the clamp: far outside on every axis reads the corner voxel
    assert M.field_sd(M.field_desc(origin, h, n), c["d2"], (9.0, 9.0, 9.0))[1] == n[0] * n[1] * n[2] - 1
    assert M.field_sd(M.field_desc(origin, h, n), c["d2"], (-9.0, -9.0, -9.0))[1] == 0


# ---- one configuration ------------------------------------------------------------------------------------------------------------------------
def robot(M, narm):
    models = [M.default_model()] if narm == 1 else list(M.arm_models(M.DUAL_BASES))
    return models, [M.link_spheres(m, 0.06, 0.08) for m in models]


def config_world(M):
    """a 0.04 m grid around both arms with a wall between the bases and a block in a far corner"""
    origin, h, n = (-1.013, -0.987, -0.131), 0.04, (64, 50, 36)
    occ = np.zeros(n[::-1], dtype=np.uint8)
    occ[:, :, 38:40] = 1
    occ[30:, :8, :10] = 1
    return origin, h, n, occ


@pytest.mark.parametrize("narm", [1, 2])
def test_clearance_field_config_matches_the_numpy_reference(M, narm):
    import oracle_py as o
    models, tables = robot(M, narm)
    origin, h, n, occ = config_world(M)
    desc = M.field_desc(origin, h, n)
    d2 = M.field_edt(desc, occ)
    assert np.array_equal(d2, F.edt(occ))
    lim = o.default_limits()
    rng = np.random.default_rng(17 + narm)
    q = np.tile(lim["qmin"], narm) + rng.random((60, 7 * narm)) * np.tile(lim["qmax"] - lim["qmin"], narm)
    cen, rad, _, _ = sphere_centres(models, tables, q)
    sd, vox = F.sd_field(origin, h, n, d2, cen)
    d = sd - rad[None, :]
    robust = (F.face_distance(origin, h, n, cen) > 1e-9).all(axis=1)
    assert robust.sum() >= 55
    n_neg = int((d[robust].min(axis=1) < 0).sum())
    assert n_neg >= 10 and robust.sum() - n_neg >= 10, n_neg              # (the reference: configurations in the wall, and clear of it)
    for i in np.nonzero(robust)[0]:
        got_d, got_s, got_v = M.clearance_field_config(models if narm == 2 else models[0], tables if narm == 2 else tables[0], desc, d2, q[i])
        assert abs(got_d - d[i].min()) <= 1e-12, (i, got_d, d[i].min())
        assert 0 <= got_s < d.shape[1] and abs(d[i, got_s] - d[i].min()) <= 1e-12 and got_v == vox[i, got_s], (i, got_s, got_v)


def test_clearance_field_config_without_pairs_and_rejections(M):
    from mpc_motion_planner_amd.capi import host
    models, tables = robot(M, 1)
    origin, h, n, occ = config_world(M)
    desc = M.field_desc(origin, h, n)
    d2 = M.field_edt(desc, occ)
    q = np.zeros(7)
    assert M.clearance_field_config(models[0], tables[0][:0], desc, d2, q) == (np.inf, -1, 0)                      # no spheres
    assert M.clearance_field_config(models[0], tables[0], desc, np.full(d2.shape, M.FIELD_EMPTY, dtype=np.uint32), q) == (np.inf, -1, 0)
    arr = (M.Model * 1)(models[0]); tab = np.ascontiguousarray(tables[0]); cnt = np.array([tab.shape[0]], dtype=np.int32)
    f = M.lib().mpcmp_clearance_field_config

    def call(**kw):
        d, s, v = C.c_double(77.0), C.c_int(77), C.c_int(77)
        a = dict(models=arr, narm=1, cnt=host(cnt), tab=host(tab), desc=desc.ctypes.data, d2=host(d2), q=host(q), d=C.byref(d))
        a.update(kw)
        rc = f(a["models"], a["narm"], a["cnt"], a["tab"], a["desc"], a["d2"], a["q"], a["d"], C.byref(s), C.byref(v))
        return rc, (d.value, s.value, v.value) == (77.0, 77, 77)
    assert call() == (0, False)
    bad_tab = tab.copy(); bad_tab["joint"][3] = 7
    bad_cnt = np.array([65], dtype=np.int32)
    bad_desc = M.field_desc(origin, -h, n)
    bad_q = q.copy(); bad_q[2] = np.nan
    for what, kw in (("no models", dict(models=None)), ("narm 0", dict(narm=0)), ("narm 3", dict(narm=3)), ("no counts", dict(cnt=None)),
                     ("no spheres", dict(tab=None)), ("65 spheres", dict(cnt=host(bad_cnt))), ("joint 7", dict(tab=host(bad_tab))),
                     ("no grid", dict(desc=None)), ("bad grid", dict(desc=bad_desc.ctypes.data)), ("no field", dict(d2=None)), ("no q", dict(q=None)),
                     ("q nan", dict(q=host(bad_q))), ("no d_min", dict(d=None))):
        assert call(**kw) == (EINVAL, True), what


# ---- the ABI ----------------------------------------------------------------------------------------------------------------------------------
def test_field_desc_is_48_bytes(M, tmp_path):
    assert M.FIELD_DESC_DTYPE.itemsize == 48
    src = tmp_path / "abi.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mpcmp.h"\nint main(void) { printf("%zu %zu %zu %zu\\n", sizeof(mpcmp_field_desc), '
                   'offsetof(mpcmp_field_desc, h), offsetof(mpcmp_field_desc, n), offsetof(mpcmp_field_desc, pad)); return 0; }\n')
    exe = tmp_path / "abi"
    subprocess.run(["gcc", "-std=c99", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    sz = [int(v) for v in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    f = M.FIELD_DESC_DTYPE.fields
    assert sz == [48, f["h"][1], f["n"][1], f["pad"][1]] == [48, 24, 32, 44], sz


def test_abi_table_matches_the_header_and_the_library(M):
    """capi.ABI_FIELD against include/mpcmp_field.h: the same functions in the same order, for each the exact argument kinds, and on the loaded
    library the exact argtypes and restype (the check of tests/test_capi_host.py, for this header)"""
    from mpc_motion_planner_amd import capi
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "mpcmp_field.h")).read(), flags=re.S)
    decl = []
    for ret, name, args in re.findall(r"\b(int|const\s+char\s*\*)\s*(mpcmp_\w+)\s*\(([^)]*)\)\s*;", hdr):
        kinds = ""
        for a in [" ".join(a.split()) for a in args.split(",")]:
            kinds += "p" if "*" in a else {"int": "i", "double": "d", "long": "l"}.get(a.split(" ")[0] if re.fullmatch(r"\w+ \w+", a) else "", "?")
        assert ret == "int"
        decl.append((name, kinds))
    assert len(decl) == 12 and [d[0] for d in decl] == list(capi.ABI_FIELD)
    ctype = {"p": C.c_void_p, "i": C.c_int, "d": C.c_double, "l": C.c_long}
    for name, kinds in decl:
        assert "?" not in kinds and set(kinds) <= set("pidl") and kinds == capi.ABI_FIELD[name], (name, kinds, capi.ABI_FIELD[name])
        f = getattr(M.lib(), name)
        assert f.argtypes == [ctype[k] for k in kinds] and f.restype is C.c_int, name
    # mpcmp.h gains the #include and nothing else that declares a function
    main = open(os.path.join(ROOT, "include", "mpcmp.h")).read()
    assert '#include "mpcmp_field.h"' in main and not set(capi.ABI_FIELD) & set(capi.ABI)


def test_context_entry_points_reject_a_missing_context(M):
    d = M.field_desc((0, 0, 0), 0.1, (2, 2, 2))
    occ = np.ones(8, dtype=np.uint8); rec = np.zeros(1, dtype=M.CLEARANCE_DTYPE)
    L = M.lib()
    assert L.mpcmp_set_field(None, d.ctypes.data, occ.ctypes.data) == EINVAL and L.mpcmp_set_field_points(None, d.ctypes.data, 0, None) == EINVAL
    assert L.mpcmp_get_field(None, d.ctypes.data, None) == EINVAL
    assert L.mpcmp_clearance_field_batch(None, 1, rec.ctypes.data, rec.ctypes.data, 10, 0.0, rec.ctypes.data) == EINVAL
    assert L.mpcmp_clearance_merge_batch(None, 1, rec.ctypes.data, rec.ctypes.data, rec.ctypes.data, None) == EINVAL
    assert b"no context" in L.mpcmp_last_error(None)


# ---- the self-test and the kernels' resources -------------------------------------------------------------------------------------------------
def test_selftest_under_the_sanitizers(M, tmp_path):
    """examples/field_selftest.cpp, host part alone (its own main, the host-only unit model_host.cpp, nothing of the GPU) under ASan and UBSan"""
    exe = str(tmp_path / "field_san")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DMPCMP_SELFTEST_HOST_ONLY", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-fno-omit-frame-pointer", "-I" + os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "examples", "field_selftest.cpp"), os.path.join(ROOT, "mpc_motion_planner_amd", "csrc", "model_host.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, env={**os.environ, "ASAN_OPTIONS": "detect_leaks=1"})
    assert r.returncode == 0, r.stderr[-2000:]
    assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
    h = json.loads(r.stdout)["host"]
    assert h["voxels"] == 24 * 20 * 16 and h["occupied"] == 13 and h["wrong"] == 0 and h["not_empty"] == 0
    assert h["sd_in"] < 0 and h["v_in_occupied"] == 1 and 0.1 < h["sd_beside"] < 0.25 and h["sd_out"] > 0 and h["sd_none_is_inf"] == 1
    assert h["v_out"] // (24 * 20) == 15                                   # (clamped onto the top layer)
    assert 0 <= h["sphere"] < 3 and 0 <= h["voxel"] < h["voxels"] and h["none_is_inf"] == 1 and h["none_sphere"] == -1


def test_field_kernels_use_no_scratch():
    """the compiler's resource remarks of field.hip, by the mechanism of tests/test_kernel_resources.py (hipcc cross-compiles: no GPU needed)"""
    import tempfile
    import test_kernel_resources as kr
    with tempfile.TemporaryDirectory() as tmp:
        proc, _ = kr._compile("field.hip", [], tmp, "fld")
        _, err = proc.communicate(timeout=600)
        assert proc.returncode == 0, err[-3000:]
        res = {k: v for k, v in kr._resources(err).items() if k.startswith("_ZN5mpcmp")}
        names = ("k_field_mark", "k_field_pass_x", "k_field_passE", "k_clearance_field", "k_clearance_merge")
        assert len(res) == 5 and all(sum(nm in k for k in res) == 1 for nm in names), list(res)
        for k, v in res.items():
            print("%s: %d VGPRs, %d B of scratch per lane" % (k, v["vgpr"], v["scratch"]))
            assert v["scratch"] == 0 and v["vgpr"] <= 128, (k, v)
