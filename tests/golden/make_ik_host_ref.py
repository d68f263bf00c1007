#!/usr/bin/env python3
"""Host inverse-kinematics fixture: ik_host_ref.npz.

64 poses of the Panda tool frame (FK of seeded uniform configurations inside the joint limits; the last pose, p = [3, 0, 0], is
out of reach) with one seeded uniform start each, and what mpcmp_inverse_kinematics returns for them: q, iterations and the return
code.  Generated with the library of the commit before the DLS loop became a step shared with the device kernel, so that the test
pins the host results across that refactor (tests/test_pose_targets_host.py).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import mpc_motion_planner_amd as M  # noqa: E402


def main():
    rng = np.random.default_rng(20261015)
    L = M.default_limits()
    model = M.default_model()
    n = 64
    q_true = rng.uniform(L["qmin"], L["qmax"], size=(n, 7))
    q_init = rng.uniform(L["qmin"], L["qmax"], size=(n, 7))
    R = np.zeros((n, 3, 3)); p = np.zeros((n, 3))
    for i in range(n):
        _, p[i], R[i] = M.tool_jacobian(model, q_true[i])
    p[-1] = [3.0, 0.0, 0.0]
    q = np.zeros((n, 7)); iters = np.zeros(n, dtype=np.int32); rc = np.zeros(n, dtype=np.int32)
    for i in range(n):
        q[i], ok, iters[i] = M.inverse_kinematic(model, R[i], p[i], q_init[i])
        rc[i] = 0 if ok else 1
    np.savez(os.path.join(HERE, "ik_host_ref.npz"), R=R, p=p, q_init=q_init, q=q, iters=iters, rc=rc)
    print("converged %d / %d, iterations %s" % ((rc == 0).sum(), n, np.percentile(iters, [0, 50, 100])))


if __name__ == "__main__":
    main()
