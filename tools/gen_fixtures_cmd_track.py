#!/usr/bin/env python3
"""Golden fixture of the command tracker's law: tests/golden/cmd_track.npz

TEST INFRASTRUCTURE -- needs the reference tree (REF of oracle/gen_fixtures.py); the .npz it writes is committed and holds data
only.  Drives the reference's own SingleInt2D.des_pose_vel (trajopt/rom_dynamics.py, numpy backend) and quat2yaw, yaw2rot,
wrap_angles (deep_tube_learning/utils.py), imported by file path with the stand-in modules of
oracle/gen_fixtures_trajectory.py::load_trajectory_modules, through the error-and-command lines of
deep_tube_learning/data_collection_velocity.py:123-141, in float64 as the reference runs them.

64 poses with arbitrary orientations (roll and pitch up to 0.6 rad, any yaw), a non-diagonal Kp, track_yaw both ways, bounds
tight enough that every axis clips on some rows at both ends, and yaw errors that wrap from each side.

    python tools/gen_fixtures_cmd_track.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import gen_fixtures as gf  # noqa: E402
import gen_fixtures_trajectory as gft  # noqa: E402

N, SEED = 64, 11
KP = [[1.5, 0.2, -0.1], [-0.3, 1.2, 0.05], [0.1, -0.2, 0.8]]
U_MIN, U_MAX = [-0.6, -0.4, -0.05], [0.7, 0.5, 0.06]


def main():
    gf._build_isaacgym_stub(gf._STATE)
    gf._load_reference_modules()
    gft.load_trajectory_modules()
    rd, du = sys.modules["trajopt.rom_dynamics"], sys.modules["deep_tube_learning.utils"]
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(SEED)
    rom = rd.SingleInt2D(0.02, [-1e9, -1e9], [1e9, 1e9], [-1.0, -1.0], [1.0, 1.0], n_robots=N, backend="numpy")
    eul = np.stack([rng.uniform(-0.6, 0.6, N), rng.uniform(-0.6, 0.6, N), rng.uniform(-np.pi, np.pi, N)], 1)
    quat = Rotation.from_euler("xyz", eul).as_quat().astype(np.float32)            # xyzw, unit up to float32 rounding
    quat[::4] *= np.float32(1.0) + rng.uniform(-0.3, 0.3, (N + 3) // 4).astype(np.float32)[:, None]   # ... and some of other norms
    base = np.zeros((N, 13), np.float32)
    base[:, :2] = rng.uniform(-2, 2, (N, 2))
    base[:, 2] = 0.6
    base[:, 3:7] = quat
    z = (base[:, :2] + rng.uniform(-0.5, 0.5, (N, 2))).astype(np.float32)
    v = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
    v[:4] = 0.0                                                                     # atan2(0, 0) = 0
    base, z, v = base.astype(np.float64), z.astype(np.float64), v.astype(np.float64)
    Kp, u_min, u_max = np.array(KP), np.array(U_MIN), np.array(U_MAX)
    out = {"base": base.astype(np.float32), "z": z.astype(np.float32), "v": v.astype(np.float32), "Kp": Kp.astype(np.float32).reshape(9),
           "u_min": u_min.astype(np.float32), "u_max": u_max.astype(np.float32)}
    # the constants as the device holds them
    Kp, u_min, u_max = (a.astype(np.float32).astype(np.float64) for a in (Kp, u_min, u_max))
    for track_yaw in (False, True):
        des_pose, des_vel = rom.des_pose_vel(z, v)
        robot_pose = np.hstack((base[:, :2], du.quat2yaw(base[:, 3:7])[:, None]))
        y2r = du.yaw2rot(robot_pose[:, 2])
        err_global = des_pose - robot_pose
        raw_yaw_err = err_global[:, 2].copy()
        err_global[:, 2] = np.where(track_yaw, du.wrap_angles(err_global[:, 2]), 0)
        err_local = err_global.copy()
        err_local[:, :2] = np.squeeze(y2r @ err_global[:, :2][:, :, None])
        des_vel_local = des_vel.copy()
        des_vel_local[:, :2] = np.squeeze(y2r @ des_vel[:, :2, None])
        raw = des_vel_local + (Kp @ err_local.T).T
        ut = np.clip(raw, u_min, u_max)
        k = f"yaw{int(track_yaw)}_"
        out.update({k + "u": ut, k + "raw": raw, k + "err_local": err_local, k + "des_vel_local": des_vel_local})
        if track_yaw:
            out["yaw"], out["yaw_err"] = robot_pose[:, 2], raw_yaw_err
            assert (raw_yaw_err > np.pi).any() and (raw_yaw_err < -np.pi).any(), "a yaw error wrapped from each side"
        for j in range(3):
            assert (raw[:, j] < u_min[j]).any() and (raw[:, j] > u_max[j]).any(), ("both clips active on axis", j, track_yaw)
    dst = os.path.join(ROOT, "tests", "golden", "cmd_track.npz")
    np.savez_compressed(dst, **out)
    print(f"{dst}: {N} poses, {os.path.getsize(dst) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
