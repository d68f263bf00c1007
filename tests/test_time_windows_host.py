"""CPU-side checks of the final-time entry points (per-problem windows, time scaling, time-synchronised solve; include/mpcmp.h): the library
exports them, they reject a missing context without touching a GPU (their ctypes prototypes: tests/test_capi_host.py), and the header's stated
arithmetic of the time scaling, restated in NumPy, scales the collocation defects of oracle solutions as a change of time unit must."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle_py as o

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["mpcmp_set_time_windows", "mpcmp_set_time_windows_device", "mpcmp_time_scale_batch", "mpcmp_time_scale_batch_device",
       "mpcmp_solve_batch_synced", "mpcmp_solve_batch_synced_device"]
MARGINS = (0.9, 0.9, 0.5, 0.9, 0.1)


@pytest.fixture(scope="module")
def M():
    import mpc_motion_planner_amd as M
    M.build_library()
    return M


def time_scale_np(narm, x0, xf, sx, su, sT, T_new):
    """include/mpcmp.h, mpcmp_time_scale_batch, operation for operation"""
    s = sT / T_new
    ox = sx.copy()
    ox[:, 1:-1, 7 * narm:] = sx[:, 1:-1, 7 * narm:] * s[:, None, None]
    ox[:, 0] = x0
    ox[:, -1] = xf
    ou = su * (s * s)[:, None, None]
    return ox, ou, np.array(T_new, dtype=np.float64)


def test_library_exports_the_final_time_entry_points(M):
    L = M.lib()
    for s in NEW:
        assert hasattr(L, s), s


def test_null_context_is_rejected(M):
    L = M.lib()
    d = np.zeros(64)
    p = d.ctypes.data_as(C.c_void_p)
    g = np.zeros(4, dtype=np.int32).ctypes.data_as(C.c_void_p)
    assert L.mpcmp_set_time_windows(None, 1, p, p) == -1
    assert L.mpcmp_set_time_windows(None, 0, None, None) == -1
    assert L.mpcmp_set_time_windows_device(None, 1, p, p, None) == -1
    assert L.mpcmp_time_scale_batch(None, 1, p, p, p, p, p, p, p, p, p) == -1
    assert L.mpcmp_time_scale_batch_device(None, 1, p, p, p, p, p, p, p, p, p, None) == -1
    assert L.mpcmp_solve_batch_synced(None, 1, p, p, None, None, None, g, 1, p, p, p, None, p) == -1
    assert L.mpcmp_solve_batch_synced_device(None, 1, p, p, None, None, None, g, 1, p, p, p, None, p, None) == -1


def test_header_compiles_against_the_new_declarations(tmp_path):
    """a C caller of every new entry point, through a C compiler (declarations and argument types as a user sees them)"""
    src = tmp_path / "tw.c"
    src.write_text('#include <stddef.h>\n#include "mpcmp.h"\n'
                   'int use(mpcmp_ctx *c, const double *x, double *y, const int *g, mpcmp_info *inf, void *s) {\n'
                   '  int r = mpcmp_set_time_windows(c, 1, x, x) + mpcmp_set_time_windows_device(c, 1, x, x, s);\n'
                   '  r += mpcmp_time_scale_batch(c, 1, x, x, x, x, x, x, y, y, y) + mpcmp_time_scale_batch_device(c, 1, x, x, x, x, x, x, y, y, y, s);\n'
                   '  r += mpcmp_solve_batch_synced(c, 1, x, x, NULL, NULL, NULL, g, 1, y, y, y, inf, y);\n'
                   '  r += mpcmp_solve_batch_synced_device(c, 1, x, x, x, x, x, g, 1, y, y, y, inf, NULL, s);\n'
                   '  return r;\n}\n')
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-c", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "tw.o"), str(src)],
                   check=True)


@pytest.mark.parametrize("nseg", [2, 4, 6])
def test_time_scale_restatement_scales_collocation_defects(nseg):
    """between states at rest a stretch by 1 / s is a change of time unit: it leaves the position rows of every collocation defect as they are and
    multiplies the velocity rows by s (d/dtau of qd against T u), to round-off.  Oracle solutions from rest to rest, end velocities set to 0"""
    from mpc_motion_planner_amd import scenarios
    cfg = o.default_config(nseg, 6, margins=MARGINS)
    x0, xf = scenarios.make_batch(3, MARGINS, stream_offset=20 + nseg)
    x0[:, 7:] = 0.0
    xf[:, 7:] = 0.0
    for b in range(3):
        wx, wu, wT = o.warm_start(cfg, x0[b], xf[b])
        xs, us, T, info = o.solve(cfg, x0[b], xf[b], wx, wu, wT)
        assert info.status & 1 == 0
        xs[0, 7:] = 0.0
        xs[-1, 7:] = 0.0
        d0 = o.collocation_defects(nseg, xs, us, T)
        for f in (0.8, 1.0, 1.37, 2.5):
            Tn = np.array([T * f])
            ox, ou, oT = time_scale_np(1, xs[0][None], xs[-1][None], xs[None], us[None], np.array([T]), Tn)
            assert oT[0] == Tn[0]
            s = T / Tn[0]
            d1 = o.collocation_defects(nseg, ox[0], ou[0], oT[0])
            scale = 1e-12 * (1 + np.abs(xs).max() + np.abs(us).max() * T)
            assert np.abs(d1[..., :7] - d0[..., :7]).max() <= scale, (nseg, b, f)
            assert np.abs(d1[..., 7:] - s * d0[..., 7:]).max() <= scale, (nseg, b, f)
        # the end nodes are the given states, whatever the stretch
        ox, _, _ = time_scale_np(1, x0[b][None], xf[b][None], xs[None], us[None], np.array([T]), np.array([2 * T]))
        assert np.array_equal(ox[0, 0], x0[b]) and np.array_equal(ox[0, -1], xf[b])
