"""Roll a VELOCITY-COMMAND policy (anymal_c_flat, anymal_c_rough, a1, anymal_b, cassie) behind a reduced-order model and record
what the tube-learning stage consumes -- the reference's deep_tube_learning/data_collection_velocity.py:84-156 with the ROM, the
command law and the recorder on the device (legged_gym_dev_amd/tube/cmd_track.py, lg_cmdtrack_*): a SingleInt2D ROM at
rom.dt = env.dt follows a random input; a proportional law turns its pose and velocity into the body-frame velocity command the
policy observes.  One ``epoch_<k>.pickle`` per epoch with numpy arrays z (N, T+1, 2), v (N, T, 2), pz_x (N, T+1, 2), done (N, T)
[, x (N, T+1, 7 + A + 6 + A), u (N, T, 3)] -- ENV-MAJOR, the layout of scripts/collect_trajectory_data.py (the reference's velocity
script is time-major) -- and a ``config.json``, so ``train_tube.py --data DIR`` runs on the result:

    python legged_gym_dev_amd/scripts/collect_velocity_data.py --task anymal_c_flat --num_envs 4096 --epochs 2 \\
        --out rom_tracking_data/vel0 [--steps T] [--Kp 1 0 0 0 1 0 0 0 1] [--track_yaw] [--u_min a b c] [--u_max a b c] \\
        [--raw_commands] [--rom_v_max vx vy] [--untrained] [--save_debugging_data] [--load_run -1 --checkpoint -1]

--raw_commands writes the command into the observation unscaled, as the reference does; the default multiplies it by the env's
commands_scale, which is what the observation holds.  No host synchronisation inside an epoch.
"""
import argparse
import json
import os
import pickle
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402


def parse(argv=None):
    ap = argparse.ArgumentParser(add_help=False)
    ap.add_argument("--epochs", type=int, default=1)
    ap.add_argument("--out", type=str, default="rom_tracking_data/vel")
    ap.add_argument("--steps", type=int, default=None, help="env steps (= ROM steps) per epoch; default: the episode length")
    ap.add_argument("--episode_length_s", type=float, default=None, help="override env.episode_length_s")
    ap.add_argument("--Kp", type=float, nargs="+", default=[1.0], help="1 value (Kp I), 3 (a diagonal) or 9 (row-major 3 x 3)")
    ap.add_argument("--track_yaw", action="store_true")
    ap.add_argument("--u_min", type=float, nargs=3, default=[-1.0, -1.0, -1.0])
    ap.add_argument("--u_max", type=float, nargs=3, default=[1.0, 1.0, 1.0])
    ap.add_argument("--raw_commands", action="store_true", help="cmd_scale = (1, 1, 1): the reference's literal observation write")
    ap.add_argument("--rom_v_max", type=float, nargs=2, default=[1.0, 1.0], help="ROM input bounds +-(vx, vy)")
    ap.add_argument("--save_debugging_data", action="store_true")
    ap.add_argument("--untrained", action="store_true", help="do not resume a checkpoint (random policy)")
    return ap.parse_known_args(argv)


def kp_matrix(vals):
    """--Kp as the row-major 3 x 3."""
    vals = [float(x) for x in vals]
    if len(vals) == 1:
        vals = vals * 3
    if len(vals) == 3:
        return [vals[0], 0.0, 0.0, 0.0, vals[1], 0.0, 0.0, 0.0, vals[2]]
    if len(vals) == 9:
        return vals
    raise SystemExit(f"--Kp takes 1, 3 or 9 values; got {len(vals)}")


def refuse_trajectory_task(task):
    """A trajectory task has no command columns: collect_trajectory_data.py serves it."""
    from legged_gym_dev_amd.envs import task_registry            # importing the package registers the tasks
    if task not in task_registry.env_cfgs:
        raise SystemExit(f"{task} is not a registered task")
    env_cfg, train_cfg = task_registry.get_cfgs(task)
    if hasattr(env_cfg, "trajectory_generator"):
        raise SystemExit(f"{task} is a trajectory-tracking task: its observation has no command columns "
                         "(collect_trajectory_data.py serves it)")
    return env_cfg, train_cfg


def main(argv=None, keep=None):
    """keep: a dict that receives the env, the tracker and the last epoch's device records (tests)."""
    own, rest = parse(argv)
    from legged_gym_dev_amd.utils import get_args
    args = get_args(rest)
    env_cfg, train_cfg = refuse_trajectory_task(args.task)
    Kp = kp_matrix(own.Kp)
    if own.epochs < 1:
        raise SystemExit(f"--epochs {own.epochs} must be at least 1")
    if own.steps is not None and own.steps < 1:
        raise SystemExit(f"--steps {own.steps} must be at least 1")
    import copy
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.tube import cmd_track as ct
    env_cfg, train_cfg = copy.deepcopy(env_cfg), copy.deepcopy(train_cfg)
    if own.episode_length_s is not None:
        env_cfg.env.episode_length_s = own.episode_length_s
    env, env_cfg = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = not own.untrained
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg,
                                                      log_root=None if own.untrained else "default")
    policy = runner.get_inference_policy(device=env.device)
    T = int(own.steps if own.steps is not None else env.max_episode_length)
    cfg = ct.CmdTrackCfg.from_env(env, raw_commands=own.raw_commands, want_x=own.save_debugging_data, kind=ct.RANDOM, Kp=tuple(Kp),
                                  track_yaw=own.track_yaw, u_min=tuple(own.u_min), u_max=tuple(own.u_max),
                                  rom_v_min=tuple(-float(x) for x in own.rom_v_max), rom_v_max=tuple(float(x) for x in own.rom_v_max))
    tracker = ct.HipCommandTracker(env, cfg)
    os.makedirs(own.out, exist_ok=True)
    with open(os.path.join(own.out, "config.json"), "w") as f:
        json.dump({"task": args.task, "num_envs": env.num_envs, "epochs": own.epochs, "rom_dt": float(env.dt),
                   "episode_length_s": float(env.max_episode_length_s), "steps": T, "Kp": Kp, "track_yaw": bool(own.track_yaw),
                   "u_min": list(own.u_min), "u_max": list(own.u_max), "cmd_scale": [float(x) for x in cfg.cmd_scale],
                   "rom_v_max": list(own.rom_v_max), "layout": "env-major"}, f)
    recs = []
    for e in range(own.epochs):
        dev = ct.collect(env, policy, tracker, 1, T, first_epoch=e, want_u=own.save_debugging_data, to_host=False)[0]
        rec = {k: v.cpu().numpy() for k, v in dev.items()}
        with open(os.path.join(own.out, f"epoch_{e}.pickle"), "wb") as f:
            pickle.dump(rec, f)
        recs.append(rec)
    err = np.linalg.norm(recs[-1]["z"] - recs[-1]["pz_x"], axis=-1)
    print(f"wrote {own.epochs} epoch(s) to {own.out}: mean tracking error {err.mean():.3f} m, done rate {recs[-1]['done'].mean():.4f}")
    if keep is not None:
        keep.update(env=env, tracker=tracker, device_records=dev, policy=policy)
    else:
        tracker.close()
    return recs


if __name__ == "__main__":
    main()
