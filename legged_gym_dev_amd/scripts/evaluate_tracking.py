"""python legged_gym_dev_amd/scripts/evaluate_tracking.py --traj_cls {zero,square,circle} [--task anymal_c_flat_trajectory]
    [--load_run R --checkpoint K] [--num_envs 1] [--steps 1000] [--push_robots] [--out eval_tracking.npz] [--plot]
Evaluate a tracking policy on a fixed reference path (the RL branch of the reference's deep_tube_learning/evaluation/
evaluate_rl_policy.py:14-124, without wandb / hydra / the hopper and its Raibert heuristic): the trajectory env with
ZeroTrajectoryGenerator, SquareTrajectoryGenerator or CircleTrajectoryGenerator (trajopt/rom_dynamics.py:618-699) and the
reference's overrides (20 s episodes, hold time 21 s, no randomisation, no ROM start offset, no curriculum).  The policy is the
latest checkpoint of the task's experiment as play.py finds it (or --load_run / --checkpoint); without one, a fresh policy.

Records, as the reference does, x = (base pose, joint positions, base twist, joint velocities), z = the oldest point of the ROM
window and pz_x = the projected base position, each (steps + 1, N, .), with z of an env that terminated on a step set to its pz_x;
the loop runs steps - 1 times, so the last row stays zero as there.  Writes them to --out and prints the RMS / max of
|z - pz_x| over the recorded rows."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from legged_gym_dev_amd import LEGGED_GYM_ROOT_DIR  # noqa: E402
from legged_gym_dev_amd.envs import *  # noqa: E402,F401,F403
from legged_gym_dev_amd.utils import get_args, task_registry  # noqa: E402
from legged_gym_dev_amd.utils.helpers import get_load_path  # noqa: E402

TRAJ_CLS = {"zero": "ZeroTrajectoryGenerator", "square": "SquareTrajectoryGenerator", "circle": "CircleTrajectoryGenerator"}


def parse(argv=None):
    argv = sys.argv[1:] if argv is None else list(argv)
    p = argparse.ArgumentParser(description="tracking evaluation on a fixed reference path")
    p.add_argument("--traj_cls", choices=sorted(TRAJ_CLS), required=True)
    p.add_argument("--steps", type=int, default=1000)
    p.add_argument("--push_robots", action="store_true", default=False)
    p.add_argument("--out", type=str, default="eval_tracking.npz")
    p.add_argument("--plot", action="store_true", default=False)
    own, rest = p.parse_known_args(argv)
    args = get_args(rest)
    if not any(a == "--task" or a.startswith("--task=") for a in rest):
        args.task = "anymal_c_flat_trajectory"
    if args.num_envs is None:
        args.num_envs = 1                                          # evaluate_rl_policy.py:22
    for k, v in vars(own).items():
        setattr(args, k, v)
    return args


def _checkpoint(train_cfg, args):
    """play.py's choice of checkpoint (the latest run / model unless --load_run / --checkpoint), or None when there is none."""
    root = os.path.join(LEGGED_GYM_ROOT_DIR, "logs", train_cfg.runner.experiment_name)
    try:
        path = get_load_path(root, load_run=args.load_run if args.load_run else -1,
                             checkpoint=args.checkpoint if args.checkpoint is not None else -1)
    except (ValueError, OSError, IndexError):
        return None
    return path if os.path.isfile(path) else None


def evaluate(args):
    if args.steps < 2:
        raise ValueError("--steps must be at least 2")
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    if not hasattr(env_cfg, "trajectory_generator"):
        raise ValueError(f"task {args.task!r} is not a trajectory-tracking task")
    # the overrides of evaluate_rl_policy.py:21-49 that exist in this configuration
    env_cfg.env.num_envs = args.num_envs
    env_cfg.env.episode_length_s = 20
    tg = env_cfg.trajectory_generator
    tg.cls, tg.t_low, tg.t_high = TRAJ_CLS[args.traj_cls], 21, 21
    dr = env_cfg.domain_rand
    dr.randomize_friction = dr.randomize_base_mass = dr.randomize_inv_base_mass = False
    dr.push_robots = bool(args.push_robots)
    rsp = dr.rigid_shape_properties
    rsp.randomize_restitution = rsp.randomize_compliance = rsp.randomize_thickness = False
    dr.randomize_rom_distance = False
    env_cfg.curriculum.use_curriculum = False
    env, env_cfg = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = False
    ppo_runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg, log_root=None)
    path = _checkpoint(train_cfg, args)
    if path is not None:
        print(f"Loading model from: {path}")
        ppo_runner.load(path)
    else:
        print("No checkpoint found: evaluating a freshly initialised policy")
    policy = ppo_runner.get_inference_policy(device=env.device)

    obs = env.get_actor_observations()                              # obs_buf, or the history row under --obs_history
    steps, n = args.steps, env.num_envs
    x_n = env.dof_pos.shape[1] + env.dof_vel.shape[1] + env.root_states.shape[1]
    x = torch.zeros((steps + 1, n, x_n), device=env.device)
    z = torch.zeros((steps + 1, n, env.rom.n), device=env.device)
    pz_x = torch.zeros((steps + 1, n, env.rom.n), device=env.device)
    base = env.root_states
    x[0] = env.get_state()
    z[0] = env.rom.proj_z(base)
    pz_x[0] = env.rom.proj_z(base)
    env.traj_gen.reset(env.rom.proj_z(env.root_states))
    with torch.no_grad():
        for t in range(steps - 1):                                 # evaluate_rl_policy.py:96-124
            actions = policy(obs.detach())
            _, _, _, done, _ = env.step(actions.detach())
            obs = env.get_actor_observations()
            done = done.bool()
            proj = env.rom.proj_z(env.root_states)
            x[t + 1] = env.get_state()
            z[t + 1] = env.traj_gen.trajectory[:, 0, :]
            z[t + 1, done] = proj[done]                             # terminated envs restart with zero tracking error
            pz_x[t + 1] = proj
    x, z, pz_x = x.cpu().numpy(), z.cpu().numpy(), pz_x.cpu().numpy()
    err = np.linalg.norm(z[:steps] - pz_x[:steps], axis=-1)
    print(f"{TRAJ_CLS[args.traj_cls]}: {n} envs x {steps} steps, |z - pz_x| rms {np.sqrt(np.mean(err ** 2)):.4f} m, "
          f"max {err.max():.4f} m")
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    np.savez(args.out, x=x, z=z, pz_x=pz_x, traj_cls=TRAJ_CLS[args.traj_cls], dt=np.float64(env.dt))
    print(f"wrote {args.out}")
    if args.plot:
        import matplotlib
        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
        fig, axes = plt.subplots(1, min(n, 2), figsize=(6 * min(n, 2), 6), squeeze=False)
        for i, ax in enumerate(axes[0]):                           # evaluate_rl_policy.py:163-171: robots 0 and 1
            ax.plot(pz_x[2:-2, i, 0], pz_x[2:-2, i, 1], ".-b", label="robot (pz_x)")
            ax.plot(z[2:-2, i, 0], z[2:-2, i, 1], ".-k", label="reference (z)")
            ax.set_title(f"env {i}: {TRAJ_CLS[args.traj_cls]}")
            ax.set_xlabel("x [m]")
            ax.set_ylabel("y [m]")
            ax.axis("equal")
            ax.legend()
        png = os.path.splitext(args.out)[0] + ".png"
        fig.savefig(png, dpi=100)
        print(f"wrote {png}")
    return {"x": x, "z": z, "pz_x": pz_x}


if __name__ == "__main__":
    evaluate(parse())
