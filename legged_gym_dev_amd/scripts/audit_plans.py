"""Score plans against a tube, track them on the ROM-on-ROM model and audit whether the tube held: the question the reference's
deep_tube_learning/evaluation/evaluate_tube_simple_oneshot_on_mpc_traj.py asks of one solved plan, asked of a batch of plans from any
source, on the HIP kernels (legged_gym_dev_amd/tube/plan.py), without CasADi, IPOPT, wandb or hydra.

    python legged_gym_dev_amd/scripts/audit_plans.py (--run tube_runs/run0 | --tube l1|l2|l1_rolling|l2_rolling [--scaling s] [--window_size n]) \\
        (--problem gap|right|right_wide | --problem_json F) \\
        (--plans F.npz | --warm_start start|goal|interpolate [--perturb K --sigma s --seed n]) \\
        [--calibration [PATH] | --age_calibration [PATH] [--trajectory_margin]] [--H_rev h] [--coverage c] [--level l] \\
        [--checkpoint best|latest] [--sim_cfg KEY=VALUE ...] [--out DIR] [--scenes F.npz] \\
        [--robot [--task anymal_c_flat_trajectory] [--load_run R] [--policy_checkpoint K] [--push_robots] [--allow_fast]]

--run: a train_tube.py run of a one-shot tube (dataset scalar_horizon or scalar_horizon_level): the plans have N = the run's H_fwd
nodes, and the tube item's past (H_rev error norms and inputs) is zero, as the reference's solve_tube starts.  Or a run of a flat
scalar tube (dataset scalar or scalar_level, dN = 1), which is rolled node by node along the plan: N is --N
(default 50), the window and --recursive come from its config.json, the history is --H_rev steps (default: the taps - 1), and
--age_calibration [PATH] [--coverage c] [--trajectory_margin] (calibrate_tube.py --by_age) or --calibration pick the offsets.  Vector,
error-dynamics and Alpha runs are refused.
--tube: an analytic baseline tube instead (trajopt/tube_trajopt.py:489-540); N is --N (default 50).
--plans: an .npz with z0 (B, 2) and v (B, N, 2).  --warm_start: the reference's warm start of the problem and, with --perturb K, K
clipped Gaussian perturbations of it beside it (sigma in the input's units, clipped to the problem's input bounds).
--calibration [PATH] (default PATH: the run's calibration.json) adds the conformal offset per step ahead: --coverage picks the set of a
scalar_horizon calibration, --level that of a scalar_horizon_level one (the level also conditions the model).
--sim_cfg: fields of the tracking model's configuration (RomSimCfg: env.model.dt=0.05 controller.Kp=10 ...); rom.dt is the problem's dt.

--robot: the plans are tracked by the legged robot instead -- one simulated robot of --task per plan under the task's trained policy
(the latest checkpoint of its experiment as play.py finds it, or --load_run / --policy_checkpoint; without one, a fresh policy), on
the HIP env with PlanTrajectoryGenerator (legged_gym_dev_amd/tube/plan_env.py): track_env, then the score
with the robot's own history as the tube item's past, then audit_env, which adds completed / terminated / covered_plans_of_all and
a "tracker": "robot" field.  The policy's checkpoint has its own flag because --checkpoint already names the tube's.  The problem's
dt must be the task's rom.dt and the inputs must lie inside its rom.v_min / v_max (--allow_fast lifts the latter).

--scenes F.npz: a Scenes file (plan_tube.py --scenes writes scenes.npz beside plans.npz): plan b is scored
and audited against scene b's own goal and obstacles, so the file holds as many scenes as --plans holds plans.  With --warm_start
every scene gets the warm start to its own goal and, with --perturb K, K perturbations of it (seed + the scene's number): S (K + 1)
plans, scene by scene, each scene repeated K + 1 times on the host.  The audit gains its per-plan lists (by_plan).  A file with
velocities (array obs_v; section 10.18) holds obstacles that move: obs_c is where they are at node 0, the plans are scored against
c + u (k dt) at node k, and actual safety is taken against each obstacle where it is at each node's time.  --robot does not follow
obstacles that move.

Writes audit.json to --out (default: the run folder, or the working directory) and prints the reference script's
"Total Success Rate" line: the share of (plan, node) pairs with tube >= realised error.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402

from legged_gym_dev_amd.tube import plan as pl  # noqa: E402

ONE_SHOT = ("scalar_horizon", "scalar_horizon_level")
STEP = ("scalar", "scalar_level")                   # the flat scalar tubes, rolled node by node along the plan (tube_kind nn_step)
LEVEL_RUNS = ("scalar_horizon_level", "scalar_level")
ANALYTIC = ("l1", "l2", "l1_rolling", "l2_rolling")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    tube = ap.add_mutually_exclusive_group(required=True)
    tube.add_argument("--run", help="folder train_tube.py wrote for a one-shot tube")
    tube.add_argument("--tube", choices=list(ANALYTIC), help="an analytic tube")
    ap.add_argument("--scaling", type=float, default=0.5)
    ap.add_argument("--window_size", type=int, default=10)
    ap.add_argument("--N", type=int, default=None, help="nodes of an analytic-tube problem (default 50); a run fixes it to its H_fwd")
    prob = ap.add_mutually_exclusive_group(required=True)
    prob.add_argument("--problem", choices=sorted(pl.PROBLEMS))
    prob.add_argument("--problem_json", help="a PlanProblem as JSON")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--plans", help=".npz with z0 (B, 2) and v (B, N, 2)")
    src.add_argument("--warm_start", choices=["start", "goal", "interpolate", "nominal"])
    ap.add_argument("--perturb", type=int, default=0)
    ap.add_argument("--sigma", type=float, default=0.05)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--calibration", nargs="?", const="", default=None, metavar="PATH")
    add_step_flags(ap)
    ap.add_argument("--coverage", type=float, default=None)
    ap.add_argument("--level", type=float, default=None)
    ap.add_argument("--checkpoint", choices=["best", "latest"], default="best")
    ap.add_argument("--sim_cfg", nargs="*", default=[], metavar="KEY=VALUE")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--robot", action="store_true", help="track the plans on the legged robot (one env per plan) instead of the ROM-on-ROM model")
    ap.add_argument("--task", default=None, help="with --robot: a trajectory-tracking task (default anymal_c_flat_trajectory)")
    ap.add_argument("--load_run", default=None, help="with --robot: the policy's run folder (default: the latest)")
    ap.add_argument("--policy_checkpoint", type=int, default=None, help="with --robot: the policy's checkpoint number (default: the latest)")
    ap.add_argument("--push_robots", action="store_true", help="with --robot: push the robots on the task's timers")
    ap.add_argument("--allow_fast", action="store_true", help="with --robot: accept inputs beyond the task's rom.v_min / v_max")
    ap.add_argument("--scenes", default=None, metavar="F.npz", help="a Scenes file: plan b against scene b's own goal and obstacles")
    a = ap.parse_args(argv)
    if a.scenes is not None and not a.scenes.endswith(".npz"):
        ap.error(f"--scenes {a.scenes}: a .npz file (plan_tube.py --scenes writes scenes.npz)")
    if not a.robot:
        for flag in ("task", "load_run", "policy_checkpoint", "push_robots", "allow_fast"):
            if getattr(a, flag) not in (None, False):
                ap.error(f"--{flag} belongs to --robot")
    elif a.sim_cfg:
        ap.error("--sim_cfg configures the ROM-on-ROM tracking model; --robot tracks on the legged env")
    if a.perturb and a.plans:
        ap.error("--perturb belongs to --warm_start; --plans are taken as they are")
    if a.perturb < 0 or a.sigma < 0:
        ap.error("--perturb and --sigma must not be negative")
    if a.calibration is not None and not a.run:
        ap.error("--calibration belongs to --run: an analytic tube has none")
    if a.tube and a.level is not None:
        ap.error("--level belongs to a level-conditioned --run")
    check_step_flags(ap, a)
    return a


def add_step_flags(ap):
    """The flags of a step run (dataset scalar / scalar_level), shared with plan_tube.py."""
    ap.add_argument("--age_calibration", nargs="?", const="", default=None, metavar="PATH",
                    help="a step run: the per-age offsets calibrate_tube.py --by_age wrote (default PATH: the run's calibration_age.json)")
    ap.add_argument("--trajectory_margin", action="store_true", help="--age_calibration: add its trajectory margin")
    ap.add_argument("--H_rev", type=int, default=None, help="a step run: past steps of the plan's history (default: the model's taps - 1)")


def check_step_flags(ap, a):
    if a.age_calibration is not None and not a.run:
        ap.error("--age_calibration belongs to --run: an analytic tube has none")
    if a.age_calibration is not None and a.calibration is not None:
        ap.error("--age_calibration and --calibration both name the offsets: give one")
    if a.trajectory_margin and a.age_calibration is None:
        ap.error("--trajectory_margin belongs to --age_calibration")
    if a.H_rev is not None and (not a.run or a.H_rev < 0):
        ap.error("--H_rev belongs to a step --run and is not negative")


def run_config(run):
    """config.json of the run; ValueError unless it trained a one-shot tube or a flat scalar tube with dN = 1."""
    from legged_gym_dev_amd.tube.model import read_config
    cfg = read_config(run)
    kind = cfg.get("dataset")
    if kind in STEP:
        missing = [k for k in ("N", "dN", "recursive") if k not in cfg]
        if missing:
            raise ValueError(f"{run}: config.json of the {kind!r} run holds no {', '.join(missing)}, so its rows cannot be rebuilt along a plan; "
                             f"plans are scored by such a step run or by a one-shot tube (dataset {' or '.join(ONE_SHOT)})")
        if cfg["dN"] != 1:
            raise ValueError(f"{run} trained with dN = {cfg['dN']}; a tube is rolled along a plan node by node: dN must be 1")
        return cfg
    if kind not in ONE_SHOT:
        raise ValueError(f"{run} trained a {kind!r} model; plans are scored by a one-shot tube (dataset {' or '.join(ONE_SHOT)}) or by a "
                         f"flat scalar tube rolled along the plan (dataset {' or '.join(STEP)}); vector, error-dynamics and Alpha tubes are not")
    return cfg


def is_step(cfg):
    return bool(cfg) and cfg.get("dataset") in STEP


def load_calibration(a, cfg):
    """The calibration --calibration / --age_calibration names, or None.  A step run takes either; a one-shot run --calibration."""
    from legged_gym_dev_amd.tube.calibrate import AgeCalibration, Calibration, default_age_path, default_path
    if a.age_calibration is not None:
        if not is_step(cfg):
            raise ValueError(f"--age_calibration belongs to a step run (dataset {' or '.join(STEP)}); {a.run} trained {cfg.get('dataset')!r}")
        path = a.age_calibration or default_age_path(a.run)
        if not os.path.isfile(path):
            raise FileNotFoundError(f"{path} is missing: calibrate_tube.py --run {a.run} --by_age writes it")
        return AgeCalibration.load(path)
    if a.calibration is None:
        return None
    path = a.calibration or default_path(a.run)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} is missing: calibrate_tube.py --run {a.run} writes it")
    return Calibration.load(path)


def build_problem(a, cfg):
    if is_step(cfg):
        kw = {"tube_kind": "nn_step", "recursive": bool(cfg["recursive"]), **({"N": a.N} if a.N else {}),
              "H_rev": max(int(cfg["N"]) - 1, 0) if getattr(a, "H_rev", None) is None else a.H_rev}
    elif cfg:
        kw = {"tube_kind": "nn", "N": cfg["H_fwd"], "H_rev": cfg["H_rev"]}
    else:
        kw = {"tube_kind": a.tube, "scaling": a.scaling, "window_size": a.window_size, **({"N": a.N} if a.N else {})}
    if a.problem:
        return pl.PlanProblem.named(a.problem, **kw)
    with open(a.problem_json) as f:
        given = json.load(f)
    p = pl.PlanProblem.from_json(a.problem_json)
    for k, v in kw.items():
        if k in ("N", "H_rev") and cfg and not is_step(cfg) and k in given and given[k] != v:
            raise ValueError(f"{a.problem_json}: {k}={given[k]} differs from the run's {v}")
        setattr(p, k, v)
    return p


def build_scene_plans(a, p):
    """--scenes: (z0, v, source, Scenes of S = B).  --plans: one scene per plan.  --warm_start: per scene the warm start to its own
    goal and its --perturb K perturbations, the scene repeated K + 1 times."""
    import torch
    scenes = pl.Scenes.load(a.scenes)
    if a.plans:
        z0, v, source = build_plans(a, p)
        if scenes.S != v.shape[0]:
            raise ValueError(f"--scenes {a.scenes} holds {scenes.S} scenes and --plans {a.plans} {v.shape[0]} plans: one scene per plan")
        return z0, v, {**source, "scenes_file": a.scenes}, scenes
    vs = []
    for s, goal in enumerate(scenes.goals(p)):
        v = torch.as_tensor(pl.warm_start(a.warm_start, p.start, goal, p.N, p.dt)[1], dtype=torch.float32)[None]
        if a.perturb:
            v = torch.cat([v, pl.perturb(v[0], a.sigma, a.perturb, a.seed + s, p.rom_v_min, p.rom_v_max)])
        vs.append(v)
    v = torch.cat(vs)
    z0 = torch.tensor(p.start, dtype=torch.float32).repeat(v.shape[0], 1)
    source = {"warm_start": a.warm_start, "perturb": a.perturb, "sigma": a.sigma, "seed": a.seed, "scenes_file": a.scenes}
    return z0, v, source, scenes.take(np.repeat(np.arange(scenes.S), a.perturb + 1))


def build_plans(a, p):
    """(z0 (B, 2), v (B, N, 2)) float32 tensors and a description of where they come from."""
    import torch
    if a.plans:
        d = np.load(a.plans)
        missing = [k for k in ("z0", "v") if k not in d]
        if missing:
            raise ValueError(f"{a.plans}: array(s) {missing} missing; a plan file holds z0 (B, 2) and v (B, N, 2)")
        return torch.as_tensor(d["z0"], dtype=torch.float32), torch.as_tensor(d["v"], dtype=torch.float32), {"plans_file": a.plans}
    _, v = pl.warm_start(a.warm_start, p.start, p.goal, p.N, p.dt)
    v = torch.as_tensor(v, dtype=torch.float32)[None]
    if a.perturb:
        v = torch.cat([v, pl.perturb(v[0], a.sigma, a.perturb, a.seed, p.rom_v_min, p.rom_v_max)])
    z0 = torch.tensor(p.start, dtype=torch.float32).repeat(v.shape[0], 1)
    return z0, v, {"warm_start": a.warm_start, "perturb": a.perturb, "sigma": a.sigma, "seed": a.seed}


def sim_config(a, p):
    from legged_gym_dev_amd.tube.rom_sim import RomSimCfg
    rc = RomSimCfg()
    rc.env.num_envs = 1
    rc.rom.dt = p.dt
    for item in a.sim_cfg:
        key, eq, val = item.partition("=")
        node, parts = rc, key.split(".")
        try:
            for part in parts[:-1]:
                node = getattr(node, part)
            old = getattr(node, parts[-1])
        except AttributeError:
            raise ValueError(f"--sim_cfg {item}: RomSimCfg has no field {key!r}") from None
        if not eq:
            raise ValueError(f"--sim_cfg {item}: KEY=VALUE")
        setattr(node, parts[-1], val if isinstance(old, str) else json.loads(val))
    return rc


def robot_env(a, B):
    """The env of --robot with one robot per plan and its inference policy: plan_env_cfg's configuration, the checkpoint chosen as
    evaluate_tracking.py chooses it."""
    import evaluate_tracking
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.tube.plan_env import plan_env_cfg
    from legged_gym_dev_amd.utils import get_args
    task = a.task or "anymal_c_flat_trajectory"
    env_cfg, train_cfg = plan_env_cfg(task, B, push_robots=a.push_robots)
    args = get_args(["--task", task, "--num_envs", str(B), "--headless"])
    args.sim_device = args.rl_device = a.device
    args.load_run, args.checkpoint = a.load_run, a.policy_checkpoint
    env, env_cfg = task_registry.make_env(name=task, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = False
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=task, args=args, train_cfg=train_cfg, log_root=None)
    path = evaluate_tracking._checkpoint(train_cfg, args)
    if path is not None:
        print(f"Loading model from: {path}")
        runner.load(path)
    else:
        print("No checkpoint found: tracking with a freshly initialised policy")
    return env, runner, runner.get_inference_policy(device=env.device), path


def main_robot(a, p, scorer, z0, v, scenes=None):
    """--robot: track_env, score with the robot's own history, audit_env."""
    import torch
    from legged_gym_dev_amd.tube.plan_env import audit_env, track_env
    env, runner, policy, path = robot_env(a, v.shape[0])
    try:
        if abs(float(env.rom.dt) - float(p.dt)) > 1e-9:
            raise ValueError(f"the problem's dt = {p.dt} differs from the task's rom.dt = {env.rom.dt}")
        t = track_env(env, policy, v, z0, H_rev=p.H_rev, allow_fast=a.allow_fast)
        skw = {} if scenes is None else {"scenes": scenes}
        s = scorer.score(z0, v, e=t["e_past"], v_prev=t["v_prev"], w0=t["w0"], **skw)
        torch.cuda.synchronize()
        res = audit_env(s, t, p, **skw)
    finally:
        runner.ppo.close()
        env.close()
    return s, res, {"tracker": "robot", "task": a.task or "anymal_c_flat_trajectory", "policy": path, "push_robots": bool(a.push_robots)}


def main(argv=None):
    a = parse_args(argv)
    cfg = run_config(a.run) if a.run else None
    p = build_problem(a, cfg)
    if a.warm_start == "nominal":
        pl.warm_start("nominal", p.start, p.goal, p.N, p.dt)          # raises, naming the missing solver
    import torch
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim
    model = calib = sim = None
    level = a.level
    if a.run:
        from legged_gym_dev_amd.tube.model import HipTubeModel
        if cfg["dataset"] in LEVEL_RUNS and level is None:
            raise ValueError(f"--level is required: the run is level-conditioned ({cfg['dataset']})")
        calib = load_calibration(a, cfg)
    else:
        pl.check_envelope(p)
    scenes = None
    if a.scenes is not None:
        z0, v, source, scenes = build_scene_plans(a, p)
        if scenes.obs_v is not None and getattr(a, "robot", False):
            raise ValueError(f"--scenes {a.scenes} carries velocities (obs_v): --robot does not follow obstacles that move")
    else:
        z0, v, source = build_plans(a, p)
    skw = {} if scenes is None else {"scenes": scenes}
    try:
        if a.run:
            model = HipTubeModel.load(a.run, checkpoint=a.checkpoint, device=a.device)
        scorer = pl.HipPlanScorer(model, p, calibration=calib, level=level, coverage=a.coverage, device=a.device,
                                  trajectory=a.trajectory_margin)
        robot = {}
        if a.robot:
            s, res, robot = main_robot(a, p, scorer, z0, v, **skw)
        else:
            sim = HipRomSim(sim_config(a, p), device=a.device)
            s = scorer.score(z0, v, **skw)
            t = pl.track(sim, s["z"], v)
            torch.cuda.synchronize()
            res = pl.audit(s, t, p, **skw)
        cost, clear = s["cost"].cpu().double(), s["min_clear"].cpu().double()
        extra = {"cost_mean": float(cost.mean()), "cost_min": float(cost.min()), "best_plan": int(cost.argmin()),
                 "min_clear_min": float(clear.min()) if p.n_obs or (scenes is not None and bool(np.isfinite(clear.numpy()).any())) else None, "n_viol_plans": [int(x) for x in (s["n_viol"] > 0).sum(dim=0).cpu()],
                 "problem": p.to_json(), "run": a.run, "tube": a.tube or p.tube_kind, "level": level,
                 "calibrated": calib is not None, "sim_cfg": list(a.sim_cfg), "source": source, **robot}
        assert not set(extra) & set(res), "a key of the audit would be overwritten"
        res.update(extra)
    finally:
        if sim is not None:
            sim.close()
        if model is not None:
            model.close()
    out = a.out or a.run or "."
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "audit.json"), "w") as f:
        json.dump(res, f, indent=1, allow_nan=False)
    if a.robot:
        print(f"{res['plans']} plans x {res['nodes']} nodes on the robot: completed {res['completed']}, terminated {res['terminated']}, "
              f"covered at every node (of all) {res['covered_plans_of_all']:.4f}")
        if not res["completed"]:
            print("Total Success Rate: None (no robot completed its plan)")
            return res
    print(f"{res['plans']} plans x {res['nodes']} nodes: predicted safe {res['predicted_safe']:.4f}, actually safe {res['actually_safe']:.4f}, "
          f"covered at every node {res['covered_plans']:.4f}; realised error mean {res['w_true_mean']:.4f} max {res['w_true_max']:.4f}")
    print(f"Total Success Rate: {res['coverage']}")
    return res


if __name__ == "__main__":
    main()
