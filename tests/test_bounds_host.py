"""Per-problem bounds, the part that needs no GPU (mpcmp_bounds, mpcmp_bounds_from_config, mpcmp_bounds_from_margins and the declarations of
mpcmp_set_bounds[_device]; include/mpcmp.h): exported symbols and header declarations (prototypes: tests/test_capi_host.py), the size of a row, and the two host helpers
bit for bit against the configuration helpers they restate.  (The setters' error paths need a context: tests/test_gpu_bounds.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mpcmp_bounds_from_config", "mpcmp_bounds_from_margins", "mpcmp_set_bounds", "mpcmp_set_bounds_device")
TABLES = (("lbx", 14), ("ubx", 14), ("lbu", 7), ("ubu", 7), ("lbg", 8), ("ubg", 8))
MARGIN_SETS = ((1.0, 1.0, 1.0, 1.0, 0.05), (0.9, 0.9, 0.5, 0.9, 0.05), (0.9, 0.45, 0.25, 0.9, 0.05), (0.9, 0.9, 0.5, 0.5, 0.05),
               (0.8, 0.9, 0.5, 0.9, 0.05), (0.9, 0.9, 0.5, 0.9, 0.25), (0.37, 0.61, 0.13, 0.77, -0.2), (1.0 / 3.0, 2.0 / 3.0, 1e-3, 0.1, 1.0))


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


def _header():
    return open(os.path.join(ROOT, "include", "mpcmp.h")).read()


def test_library_exports_and_header_declares_the_four_symbols(M):
    from mpc_motion_planner_amd import capi
    L = M.lib()
    text = re.sub(r"/\*.*?\*/", " ", _header(), flags=re.S)
    for name in NEW:
        assert name in capi.SYMBOLS
        assert hasattr(L, name), name
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name


def test_row_is_464_bytes_in_c_and_in_numpy(M, tmp_path):
    from mpc_motion_planner_amd import capi
    assert capi.BOUNDS_DTYPE.itemsize == 464
    off = 0
    for name, n in TABLES:
        assert capi.BOUNDS_DTYPE.fields[name][1] == off and capi.BOUNDS_DTYPE[name].shape == (n,), name
        off += 8 * n
    src = tmp_path / "b.c"
    src.write_text('#include <stddef.h>\n#include "mpcmp.h"\n'
                   "_Static_assert(sizeof(mpcmp_bounds) == 464, \"size\");\n"
                   + "".join("_Static_assert(offsetof(mpcmp_bounds, %s) == %d, \"%s\");\n" % (name, capi.BOUNDS_DTYPE.fields[name][1], name)
                             for name, _ in TABLES)
                   + "int use(mpcmp_ctx *c, const mpcmp_config *g, mpcmp_bounds *r, void *s) {\n"
                     "  return mpcmp_bounds_from_config(g, r) + mpcmp_bounds_from_margins(0.9, 0.9, 0.5, 0.9, 0.05, r) + mpcmp_set_bounds(c, 1, r)\n"
                     "         + mpcmp_set_bounds(c, 0, NULL) + mpcmp_set_bounds_device(c, 1, r, s);\n}\n")
    subprocess.check_call(["cc", "-std=c11", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", "-o", str(tmp_path / "b.o"), str(src)])


def _tables(cfg):
    return b"".join(bytes(getattr(cfg, name)) for name, _ in TABLES)


def test_bounds_from_config_is_the_six_tables_bit_for_bit(M):
    rng = np.random.default_rng(5)
    for nseg in (1, 4, 6, 8):
        cfg = M.default_config(nseg, 2, margins=(0.9, 0.45, 0.5, 0.7))
        for name, n in TABLES:
            for i in range(n):
                getattr(cfg, name)[i] = rng.normal()
        cfg.lbg[3], cfg.ubg[7], cfg.lbx[2] = -np.inf, np.inf, -0.0
        row = M.bounds_from_config(cfg)
        assert row.tobytes() == _tables(cfg)
        for name, n in TABLES:
            assert np.array_equal(row[name], np.array(getattr(cfg, name)[:]))
    assert M.lib().mpcmp_bounds_from_config(None, row.ctypes.data) == -1 and M.lib().mpcmp_bounds_from_config(C.addressof(cfg), None) == -1


@pytest.mark.parametrize("mg", MARGIN_SETS)
def test_bounds_from_margins_is_default_config_plus_margins_plus_height(M, mg):
    cfg = M.default_config(6, 2)
    M.capi.check(M.lib().mpcmp_set_margins(C.byref(cfg), *[C.c_double(x) for x in mg[:4]]))
    M.capi.check(M.lib().mpcmp_set_min_height(C.addressof(cfg), mg[4]))
    row = M.bounds_from_margins(*mg)
    assert row.tobytes() == _tables(cfg)
    assert row["lbg"][7] == mg[4] and row["ubg"][7] == np.inf
    assert M.lib().mpcmp_bounds_from_margins(*mg, None) == -1


def test_default_row_of_the_parity_check_is_the_margins_config(M):
    """mpcmp_set_margins sets the height 0.05: the `default` row of the GPU parity check is the configuration of its context"""
    cfg = M.default_config(4, 3, margins=(0.9, 0.9, 0.5, 0.9, 0.1))
    assert M.bounds_from_margins(0.9, 0.9, 0.5, 0.9, 0.05).tobytes() == M.bounds_from_config(cfg).tobytes()


def test_bounds_table_broadcasts(M):
    """Solver.bounds_table needs no context: exercised through an object that only carries a configuration"""
    from mpc_motion_planner_amd.planner import Solver
    s = Solver.__new__(Solver)
    s.cfg = M.default_config(4, 3, margins=(0.9, 0.9, 0.5, 0.9))
    s._ctx = None
    t = s.bounds_table(n=3)
    assert t.shape == (3,) and all(t[i].tobytes() == M.bounds_from_config(s.cfg).tobytes() for i in range(3))
    t = s.bounds_table(margins=[(0.9, 0.45, 0.25, 0.9), (0.9, 0.9, 0.5, 0.5)], min_height=[0.05, 0.25])
    assert t[0].tobytes() == M.bounds_from_margins(0.9, 0.45, 0.25, 0.9, 0.05).tobytes()
    assert t[1].tobytes() == M.bounds_from_margins(0.9, 0.9, 0.5, 0.5, 0.25).tobytes()
    t = s.bounds_table(n=4, min_height=0.3, ubu=np.arange(7.0))
    assert np.array_equal(t["lbg"][:, 7], np.full(4, 0.3)) and np.array_equal(t["ubu"], np.tile(np.arange(7.0), (4, 1)))
    assert np.array_equal(t["lbx"], np.tile(np.array(s.cfg.lbx[:]), (4, 1)))
    with pytest.raises(ValueError):
        s.bounds_table(n=3, margins=np.ones((2, 4)))
    with pytest.raises(ValueError):
        s.bounds_table(lbz=np.zeros(3))
