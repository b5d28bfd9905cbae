#!/usr/bin/env python3
"""Golden fixtures for the evaluation trajectory generators (trajopt/rom_dynamics.py:618-699: ZeroTrajectoryGenerator,
SquareTrajectoryGenerator, CircleTrajectoryGenerator) in the trajectory-tracking env:
    tests/golden/anymal_c_flat_traj_{zero,square,circle}.npz

TEST INFRASTRUCTURE -- needs the reference tree (REF of oracle/gen_fixtures.py); the .npz files it writes are committed.  The
recording itself is oracle/gen_fixtures_trajectory.py::make_traj_case, unchanged: the reference's own LeggedRobotTrajectory /
AnymalTrajectory on scripted physics, with every torch.rand* draw recorded.  This script only swaps trajectory_generator.cls (and
rom.v_min / v_max) on the cfg, adds the Circle generator's per-env ``center`` to every snapshot (init_tg_center,
s<t>_post_tg_center), which the generic recorder does not know about, and keeps only the arrays the replay
(tests/test_eval_generators.py) installs or compares.  The rest -- the actuator network's state after every step, the
per-substep torques, the post-step copies of the prescribed physics -- the evaluation generators do not touch, and the
anymal_c_flat_trajectory fixture already pins it; dropping it keeps each file small.

Files (64 envs, 4 recorded steps: resets on 3 of them with the rest of the envs carrying on, none on the third):
    anymal_c_flat_traj_zero.npz     ZeroTrajectoryGenerator
    anymal_c_flat_traj_square.npz   SquareTrajectoryGenerator, ROM bounds +-2 m/s: envs turn corners inside the recorded steps
    anymal_c_flat_traj_circle.npz   CircleTrajectoryGenerator: every env re-centred on the steps with resets

    python tools/gen_fixtures_eval_traj.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, ROOT)
import gen_fixtures as gf  # noqa: E402
import gen_fixtures_trajectory as gft  # noqa: E402

# name -> (generator class, rom.v_min, rom.v_max, seed).  Square: +-2 m/s puts the corners at 1.0 / 1.5 / 2.5 / 3.0 s, inside the
# 0..3 s the recorder's scattered clocks reach (make_traj_case advances every env by 0..150 env steps), so envs turn corners
# during the recorded steps; the reset envs restart at t ~ 0, on the edge of the first interval.
CASES = {
    "anymal_c_flat_traj_zero": ("ZeroTrajectoryGenerator", [-0.35, -0.35], [0.35, 0.35], 41),
    "anymal_c_flat_traj_square": ("SquareTrajectoryGenerator", [-2.0, -2.0], [2.0, 2.0], 42),
    "anymal_c_flat_traj_circle": ("CircleTrajectoryGenerator", [-0.35, -0.35], [0.35, 0.35], 43),
}
N_STEPS = 4
# what the replay reads: the initial snapshot it installs, the per-step inputs it forces, the outputs it compares
KEEP_INIT = ("root_states", "dof_state", "last_actions", "last_dof_vel", "last_root_vel", "feet_air_time", "env_origins", "prev_error",
             "trajectory", "lstm_h", "lstm_c", "last_contacts", "episode_length_buf", "time_until_next_push", "episode_sums",
             "common_step_counter", "tg_")
KEEP_STEP = ("pre_episode_length_buf", "actions", "sub_dof", "new_root", "contact_forces", "uniforms", "reset", "time_out",
             "post_episode_length_buf", "n_reset", "post_tg_", "post_trajectory", "post_prev_error", "obs", "rew",
             "post_time_until_next_push", "post_episode_sums", "extras_episode")


def kept(key):
    if key.startswith(("const_", "meta_")):
        return True
    if key.startswith("init_"):
        k = key[len("init_"):]
        return any(k == w or (w.endswith("_") and k.startswith(w)) for w in KEEP_INIT)
    step, k = key.split("_", 1)
    assert step[0] == "s" and step[1:].isdigit(), key
    return any(k == w or (w.endswith("_") and k.startswith(w)) for w in KEEP_STEP)


def install_push_spies(cls):
    """The push mask of a step, as gen_fixtures_trajectory.main() observes it (make_traj_case reads it as a module global)."""
    orig_push, orig_pps = cls._push_robots, cls.post_physics_step

    def push_spy(self, push_idx):
        gft.env_push_mask = push_idx.numpy().copy()
        return orig_push(self, push_idx)

    def pps_spy(self):
        gft.env_push_mask = np.zeros(self.num_envs, bool)
        return orig_pps(self)
    cls._push_robots = push_spy
    cls.post_physics_step = pps_spy


def main():
    gf._build_isaacgym_stub(gf._STATE)
    gf._load_reference_modules()
    mods = gft.load_trajectory_modules()
    install_push_spies(mods["LeggedRobotTrajectory"])
    env_cls = mods["AnymalTrajectory"]
    orig_step = env_cls.step
    for name, (gen, v_min, v_max, seed) in CASES.items():
        def make_cfg(gen=gen, v_min=v_min, v_max=v_max):
            cfg = mods["AnymalCFlatTrajectoryCfg"]()
            cfg.trajectory_generator.cls = gen
            cfg.rom.v_min, cfg.rom.v_max = list(v_min), list(v_max)
            return cfg
        mods["EvalCfg"] = make_cfg
        centers = []                                  # Circle: center before the first recorded step, then after every step

        def step_spy(self, actions):
            tg = self.traj_gen
            if not centers and hasattr(tg, "center"):
                centers.append(tg.center.numpy().copy())
            out = orig_step(self, actions)
            if hasattr(tg, "center"):
                centers.append(tg.center.numpy().copy())
            return out
        env_cls.step = step_spy
        try:
            gft.make_traj_case(mods, name, N_STEPS, seed, cfg_name="EvalCfg")
        finally:
            env_cls.step = orig_step
        dst = os.path.join(ROOT, "tests", "golden", f"{name}.npz")
        with np.load(dst) as z:
            out = {k: z[k] for k in z.files if kept(k)}
        if centers:
            out["init_tg_center"] = centers[0]
            for t in range(N_STEPS):
                out[f"s{t}_post_tg_center"] = centers[t + 1]
        np.savez_compressed(dst, **out)
        print(f"{name}: kept {len(out)} arrays, {os.path.getsize(dst) / 1024:.0f} KiB" + (" (+ Circle centres)" if centers else ""))


if __name__ == "__main__":
    main()
