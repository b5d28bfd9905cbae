"""Plan through a problem with a tube: the reference's trajopt/tube_trajopt.py (one plan) and trajopt/tube_planning_closed_loop.py
(replanning at every step) with a sampling planner -- batched MPPI on the HIP kernels (legged_gym_dev_amd/tube/plan.py; DESIGN.md
section 10.10) --, a first-order one -- projected Adam on the HIP plan gradient (section 10.11) -- or the second after the first, in
place of CasADi / IPOPT, for many starts at once.

    python legged_gym_dev_amd/scripts/plan_tube.py (--run tube_runs/run0 | --tube l1|l2|l1_rolling|l2_rolling [--scaling s] [--window_size n]) \\
        --problem gap|right|right_wide|F.json [--level l] [--calibration [PATH] | --age_calibration [PATH] [--trajectory_margin]] \\
        [--H_rev h] [--coverage c] [--w0 zero|error] \\
        [--K 256] [--iters 20] [--sigma 0.3] [--sigma_decay 1] [--lambda 1] [--rho_g 1e4] [--rho_w 0] [--rho_z 0] [--seed 0] \\
        [--planner mppi|grad|mppi+grad] [--lr 0.05] [--grad_iters 100] \\
        [--starts P --start_noise s] [--closed_loop H] [--sim_cfg KEY=VALUE ...] [--out DIR] \\
        [--robot [--task anymal_c_flat_trajectory] [--load_run R] [--policy_checkpoint K] [--push_robots] [--allow_fast]] \\
        [--scenes random|FILE.npz [--scene_seed n] [--scene_obs LO,HI] [--scene_radius LO,HI] [--scene_margin M] [--scene_speed LO,HI]] \\
        [--fleet SEPARATION [--fleet_sense R] [--fleet_neighbours K]]

--run, --tube, --calibration, --coverage, --level, --checkpoint, --sim_cfg: as audit_plans.py takes them; a run that audit_plans.py
refuses is refused here; a step run (dataset scalar / scalar_level, rolled along the plan: DESIGN.md section 10.13) plans with
--planner mppi only, and --w0 error starts each replanning of --closed_loop at the tracking error, the quantity its first column was
trained on.  --planner: mppi (the default), grad (--grad_iters steps of rate --lr from the warm start; the rho are shared) or mppi+grad (MPPI,
then the gradient planner from MPPI's best plan).  --problem: one of the reference's problems, or a PlanProblem as JSON (a path ending
in .json).  --starts P: P instances; the first starts at the problem's start, the others at start + start_noise * standard normal.
Without --closed_loop every start gets one plan, which is scored, tracked and audited as audit_plans.py does.  With --closed_loop H
every robot replans at each of H control steps (closed_loop) and the audit is audit_closed_loop's.

--scenes: every start plans in a scene of its own -- its own goal and obstacles -- in the same launches.
FILE.npz: a Scenes file (goal (S, 2), obs_c, obs_r, n_obs) of S = --starts scenes.  random: random_scenes(--starts, --scene_seed, the
problem's start) with --scene_obs LO,HI obstacles (default 1,3) of radius in --scene_radius LO,HI (default 0.1,0.4), centres in the box
the problem's start and goal span (padded by 0.25), goals within 0.5 of the problem's goal, the start and the goal at least
--scene_margin (default 0.05) outside every obstacle.  scenes.npz is written beside plans.npz, one scene per row of it (with
--closed_loop the starts' scenes once per step), so audit_plans.py --plans plans.npz --scenes scenes.npz reads both; plan.json gains
"scenes" (the source) and the audit its per-scene lists (by_plan / by_robot).  Without --scenes the output is what it was.
--scene_speed LO,HI (with --scenes random): every obstacle moves in a uniform direction at a uniform speed in
[LO, HI] m/s; a FILE.npz brings its own velocities (obs_v).  With --closed_loop, scenes.npz then holds the scenes where they were at
each step's time.

--closed_loop H --fleet SEPARATION: the robots avoid each other (section 10.18) -- before each plan every robot's scene is rebuilt on
the device from the fleet's positions: its static obstacles (the problem's, or its --scenes scene), then its --fleet_neighbours
(default 8) nearest robots within --fleet_sense (default 1.0) as discs of radius SEPARATION that move with their plans' next input.
The audit gains min_separation and collision_free, plan.json "fleet"; scenes.npz holds the scenes each plan ran against.

--closed_loop H --robot: the legged robot is the tracker -- one simulated robot of --task per start under the
task's trained policy, replanning from the window point it is heading for at each of H ROM steps (plan_env.closed_loop_env), env,
policy, planner and recorder on one device.  --task, --load_run, --policy_checkpoint, --push_robots, --allow_fast: as audit_plans.py
--robot takes them.  plan.json gains "tracker": "robot", the task, the policy and audit_closed_loop_env's audit (completed /
terminated / covered_robots_of_all); plans.npz holds the plans in force in the plan frame.  --robot without --closed_loop is refused:
audit_plans.py --robot tracks open-loop plans.  Without --robot the output is what it was.

Writes plan.json -- the audit, the history of the (first) plan, the settings -- and plans.npz with z0 (B, 2), v (B, N, 2): the final
mean plans, or with --closed_loop every plan in force, step by step; audit_plans.py --plans reads it.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402

import audit_plans  # noqa: E402
from legged_gym_dev_amd.tube import plan as pl  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    tube = ap.add_mutually_exclusive_group(required=True)
    tube.add_argument("--run", help="folder train_tube.py wrote for a one-shot tube")
    tube.add_argument("--tube", choices=list(audit_plans.ANALYTIC), help="an analytic tube")
    ap.add_argument("--scaling", type=float, default=0.5)
    ap.add_argument("--window_size", type=int, default=10)
    ap.add_argument("--N", type=int, default=None, help="nodes of an analytic-tube problem (default 50); a run fixes it to its H_fwd")
    ap.add_argument("--problem", required=True, help="gap, right, right_wide, or a PlanProblem as JSON (F.json)")
    ap.add_argument("--calibration", nargs="?", const="", default=None, metavar="PATH")
    audit_plans.add_step_flags(ap)
    ap.add_argument("--w0", choices=["zero", "error"], default="zero",
                    help="--closed_loop: start every replanning's tube at 0 or at the tracking error |z_k - pz_x_k|")
    ap.add_argument("--coverage", type=float, default=None)
    ap.add_argument("--level", type=float, default=None)
    ap.add_argument("--checkpoint", choices=["best", "latest"], default="best")
    d = pl.MppiCfg()
    ap.add_argument("--K", type=int, default=d.K)
    ap.add_argument("--iters", type=int, default=d.iters)
    ap.add_argument("--sigma", type=float, default=d.sigma)
    ap.add_argument("--sigma_decay", type=float, default=d.sigma_decay)
    ap.add_argument("--lambda", dest="lambda_", type=float, default=d.lambda_)
    ap.add_argument("--rho_g", type=float, default=d.rho_g)
    ap.add_argument("--rho_w", type=float, default=d.rho_w)
    ap.add_argument("--rho_z", type=float, default=d.rho_z)
    ap.add_argument("--seed", type=int, default=0)
    g = pl.GradCfg()
    ap.add_argument("--planner", choices=PLANNERS, default="mppi")
    ap.add_argument("--lr", type=float, default=g.lr)
    ap.add_argument("--grad_iters", type=int, default=g.iters)
    ap.add_argument("--starts", type=int, default=1)
    ap.add_argument("--start_noise", type=float, default=0.0)
    ap.add_argument("--closed_loop", type=int, default=None, metavar="H")
    ap.add_argument("--goal_tol", type=float, default=0.1)
    ap.add_argument("--sim_cfg", nargs="*", default=[], metavar="KEY=VALUE")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    add_scene_flags(ap)
    ap.add_argument("--fleet", type=float, default=None, metavar="SEPARATION", help="with --closed_loop: the robots keep this distance from each other")
    ap.add_argument("--fleet_sense", type=float, default=None, metavar="R", help="with --fleet: robots farther than this are not seen (default 1.0)")
    ap.add_argument("--fleet_neighbours", type=int, default=None, metavar="K", help="with --fleet: the nearest K robots are kept (default 8)")
    ap.add_argument("--robot", action="store_true", help="with --closed_loop: replan on the legged robot (one env per start) instead of the ROM-on-ROM model")
    ap.add_argument("--task", default=None, help="with --robot: a trajectory-tracking task (default anymal_c_flat_trajectory)")
    ap.add_argument("--load_run", default=None, help="with --robot: the policy's run folder (default: the latest)")
    ap.add_argument("--policy_checkpoint", type=int, default=None, help="with --robot: the policy's checkpoint number (default: the latest)")
    ap.add_argument("--push_robots", action="store_true", help="with --robot: push the robots on the task's timers")
    ap.add_argument("--allow_fast", action="store_true", help="with --robot: accept ROM input bounds beyond the task's rom.v_min / v_max")
    a = ap.parse_args(argv)
    check_scene_flags(ap, a)
    check_fleet_flags(ap, a)
    if not a.robot:
        for flag in ("task", "load_run", "policy_checkpoint", "push_robots", "allow_fast"):
            if getattr(a, flag):
                ap.error(f"--{flag} belongs to --robot")
    elif a.closed_loop is None:
        ap.error("--robot belongs to --closed_loop H: it replans on the legged robot at every ROM step; audit_plans.py --robot tracks "
                 "open-loop plans on it")
    elif a.sim_cfg:
        ap.error("--sim_cfg configures the ROM-on-ROM tracking model; --robot tracks on the legged env")
    elif a.scene_speed is not None:
        ap.error("--scene_speed: obstacles that move are not followed by --robot's loop (its robots live in per-env frames)")
    if a.problem not in pl.PROBLEMS and not a.problem.endswith(".json"):
        ap.error(f"--problem {a.problem}: one of {sorted(pl.PROBLEMS)} or a .json file")
    if a.calibration is not None and not a.run:
        ap.error("--calibration belongs to --run: an analytic tube has none")
    if a.tube and a.level is not None:
        ap.error("--level belongs to a level-conditioned --run")
    if a.starts < 1 or a.start_noise < 0:
        ap.error("--starts must be at least 1 and --start_noise not negative")
    if a.closed_loop is not None and a.closed_loop < 1:
        ap.error("--closed_loop H: at least 1 step")
    if a.w0 != "zero" and a.closed_loop is None:
        ap.error("--w0 belongs to --closed_loop")
    audit_plans.check_step_flags(ap, a)
    try:
        if "mppi" in a.planner:
            mppi_cfg(a).check(a.starts)
        if "grad" in a.planner:
            grad_cfg(a).check(a.starts)
    except ValueError as e:
        ap.error(str(e))
    return a


PLANNERS = ("mppi", "grad", "mppi+grad")
SCENE_DEFAULTS = {"scene_seed": 0, "scene_obs": (1, 3), "scene_radius": (0.1, 0.4), "scene_margin": 0.05}


def add_scene_flags(ap):
    ap.add_argument("--scenes", default=None, metavar="random|FILE.npz", help="a scene of its own per start: random, or a Scenes file")
    ap.add_argument("--scene_seed", type=int, default=None)
    ap.add_argument("--scene_obs", default=None, metavar="LO,HI", help="obstacles per random scene (default 1,3)")
    ap.add_argument("--scene_radius", default=None, metavar="LO,HI", help="radius of a random obstacle (default 0.1,0.4)")
    ap.add_argument("--scene_margin", type=float, default=None, help="start and goal stay this far outside every random obstacle")
    ap.add_argument("--scene_speed", default=None, metavar="LO,HI", help="speed in m/s of a random obstacle (default: it stands still)")


FLEET_DEFAULTS = {"fleet_sense": 1.0, "fleet_neighbours": 8}


def check_fleet_flags(ap, a):
    """Refuse what does not fit --fleet and fill its defaults."""
    if a.fleet is None:
        for k in FLEET_DEFAULTS:
            if getattr(a, k) is not None:
                ap.error(f"--{k} belongs to --fleet")
        return
    if a.closed_loop is None:
        ap.error("--fleet belongs to --closed_loop H: the robots avoid each other while they replan")
    if a.robot:
        ap.error("--fleet plans in one common frame; --robot's robots live in per-env frames")
    for k, v in FLEET_DEFAULTS.items():
        if getattr(a, k) is None:
            setattr(a, k, v)
    try:
        fleet_cfg(a).check()
    except ValueError as e:
        ap.error(f"--fleet: {e}")


def fleet_cfg(a):
    return pl.FleetCfg(separation=a.fleet, sense_radius=a.fleet_sense, max_neighbours=a.fleet_neighbours)


def build_fleet(a, p, scenes):
    """The FleetScenes of --fleet: the goals and obstacles of --scenes as its goals and static part, else the problem's obstacles."""
    if scenes is not None:
        static = None if scenes.obs_c is None else pl.Scenes(obs_c=scenes.obs_c, obs_r=scenes.obs_r, n_obs=scenes.n_obs, obs_v=scenes.obs_v)
        return pl.FleetScenes(a.starts, fleet_cfg(a), goal=scenes.goal, static=static)
    rep = pl.Scenes.repeat(p, a.starts) if p.n_obs else None
    return pl.FleetScenes(a.starts, fleet_cfg(a), static=None if rep is None else pl.Scenes(obs_c=rep.obs_c, obs_r=rep.obs_r, n_obs=rep.n_obs))


def check_scene_flags(ap, a):
    """Refuse what does not fit, parse the LO,HI pairs and fill the defaults of --scenes random."""
    given = [k for k in list(SCENE_DEFAULTS) + ["scene_speed"] if getattr(a, k) is not None]
    if a.scenes is None:
        if given:
            ap.error(f"--{given[0]} belongs to --scenes random")
        return
    if a.scenes != "random":
        if not a.scenes.endswith(".npz"):
            ap.error(f"--scenes {a.scenes}: random or a .npz file")
        if given:
            ap.error(f"--{given[0]} belongs to --scenes random; {a.scenes} is taken as it is")
        return
    for k, kind in (("scene_obs", int), ("scene_radius", float), ("scene_speed", float)):
        v = getattr(a, k)
        if v is None:
            continue
        try:
            lo, hi = (kind(x) for x in v.split(","))
        except ValueError:
            ap.error(f"--{k} {v}: LO,HI")
        if not 0 <= lo <= hi or (k == "scene_obs" and hi > 8):
            ap.error(f"--{k} {v}: 0 <= LO <= HI" + (" <= 8" if k == "scene_obs" else ""))
        setattr(a, k, (lo, hi))
    for k, v in SCENE_DEFAULTS.items():
        if getattr(a, k) is None:
            setattr(a, k, v)
    if a.scene_margin < 0:
        ap.error("--scene_margin must not be negative")


def build_scenes(a, p):
    """(Scenes of S = --starts, what plan.json says of them), or (None, None) without --scenes."""
    if a.scenes is None:
        return None, None
    if a.scenes != "random":
        sc = pl.Scenes.load(a.scenes)
        if sc.S != a.starts:
            raise ValueError(f"--scenes {a.scenes} holds {sc.S} scenes; --starts is {a.starts} (one scene per start)")
        return sc, {"file": a.scenes, "S": sc.S}
    s, g = np.asarray(p.start, np.float64), np.asarray(p.goal, np.float64)
    kw = dict(n_obs=a.scene_obs, radius=a.scene_radius, margin=a.scene_margin,
              centre_box=((np.minimum(s, g) - 0.25).tolist(), (np.maximum(s, g) + 0.25).tolist()),
              goal_box=((g - 0.5).tolist(), (g + 0.5).tolist()))
    if a.scene_speed is not None:
        kw["speed"] = a.scene_speed
    return pl.random_scenes(a.starts, a.scene_seed, p.start, **kw), {"random": {"seed": a.scene_seed, **{k: list(v) if isinstance(v, tuple) else v for k, v in kw.items()}}, "S": a.starts}


def mppi_cfg(a):
    return pl.MppiCfg(K=a.K, iters=a.iters, seed=a.seed, sigma=a.sigma, sigma_decay=a.sigma_decay, lambda_=a.lambda_, rho_g=a.rho_g,
                      rho_w=a.rho_w, rho_z=a.rho_z)


def grad_cfg(a):
    return pl.GradCfg(iters=a.grad_iters, lr=a.lr, rho_g=a.rho_g, rho_w=a.rho_w, rho_z=a.rho_z)


def make_planner(a, model, p, calib, scenes=None):
    """The planner --planner names, on one scorer's arguments."""
    kw = dict(calibration=calib, level=a.level, coverage=a.coverage, device=a.device)
    if scenes is not None:
        kw["scenes"] = scenes
    if a.planner == "mppi":
        return pl.HipMppiPlanner(model, p, mppi_cfg(a), trajectory=a.trajectory_margin, **kw)
    if p.tube_kind == "nn_step":
        raise ValueError(pl.NO_GRADIENT)
    if a.planner == "grad":
        return pl.HipGradPlanner(model, p, grad_cfg(a), **kw)
    return pl.ChainedPlanner(pl.HipMppiPlanner(model, p, mppi_cfg(a), **kw), pl.HipGradPlanner(model, p, grad_cfg(a), **kw))


def build_problem(a, cfg):
    named = a.problem in pl.PROBLEMS
    return audit_plans.build_problem(argparse.Namespace(tube=a.tube, scaling=a.scaling, window_size=a.window_size, N=a.N, H_rev=a.H_rev,
                                                        problem=a.problem if named else None, problem_json=None if named else a.problem), cfg)


def starts(a, p):
    """(P, 2) float32: the problem's start, then start + start_noise * standard normal from a torch generator on the host."""
    import torch
    s = torch.tensor(p.start, dtype=torch.float32).repeat(a.starts, 1)
    if a.starts > 1 and a.start_noise > 0:
        g = torch.Generator().manual_seed(int(a.seed))
        s[1:] += float(a.start_noise) * torch.randn(a.starts - 1, 2, generator=g)
    return s


def main_robot(a, planner, z0, scenes=None):
    """--closed_loop H --robot: closed_loop_env on audit_plans.py's --robot env, audit_closed_loop_env."""
    import torch
    from legged_gym_dev_amd.tube.plan_env import audit_closed_loop_env, closed_loop_env
    env, runner, policy, path = audit_plans.robot_env(a, z0.shape[0])
    try:
        res = closed_loop_env(env, policy, planner, a.closed_loop, start=z0, keep_plans=True, w0=a.w0, allow_fast=a.allow_fast)
        torch.cuda.synchronize()
        audit = audit_closed_loop_env(res, planner.problem, goal_tol=a.goal_tol, **({} if scenes is None else {"scenes": scenes}))
    finally:
        runner.ppo.close()
        env.close()
    return res, audit, {"tracker": "robot", "task": a.task or "anymal_c_flat_trajectory", "policy": path, "push_robots": bool(a.push_robots)}


def main(argv=None):
    a = parse_args(argv)
    cfg = audit_plans.run_config(a.run) if a.run else None
    p = build_problem(a, cfg)
    import torch
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim
    model = calib = sim = None
    robot = {}
    if a.run:
        from legged_gym_dev_amd.tube.model import HipTubeModel
        if cfg["dataset"] in audit_plans.LEVEL_RUNS and a.level is None:
            raise ValueError(f"--level is required: the run is level-conditioned ({cfg['dataset']})")
        calib = audit_plans.load_calibration(a, cfg)
    else:
        pl.check_envelope(p)
    z0 = starts(a, p)
    scenes, scenes_src = build_scenes(a, p)
    plan_scenes = scenes
    if a.robot and scenes is not None and scenes.obs_v is not None:
        raise ValueError(f"--scenes {a.scenes} carries velocities (obs_v): obstacles that move are not followed by --robot's loop")
    fleet = build_fleet(a, p, scenes) if a.fleet is not None else None
    try:
        if a.run:
            model = HipTubeModel.load(a.run, checkpoint=a.checkpoint, device=a.device)
        planner = make_planner(a, model, p, calib, scenes if fleet is None else fleet)
        if not a.robot:
            sim = HipRomSim(audit_plans.sim_config(a, p), device=a.device)
        if a.closed_loop is None:
            sol = planner.plan(z0)
            t = pl.track(sim, sol["score"]["z"], sol["v"])
            torch.cuda.synchronize()
            audit = pl.audit(sol["score"], t, p) if scenes is None else pl.audit(sol["score"], t, p, scenes=scenes)
            hist, plans_z0, plans_v = sol["hist"], z0, sol["v"]
            extra = {"best_J": [float(x) for x in sol["best_J"].cpu()], "n_bad": [int(x) for x in sol["n_bad"].cpu()],
                     "cost": [float(x) for x in sol["score"]["cost"].cpu()]}
        else:
            first = planner.plan(z0)                                     # the history of the first plan; closed_loop makes it again
            if a.robot:
                res, audit, robot = main_robot(a, planner, z0, scenes)
            else:
                res = pl.closed_loop(planner, sim, a.closed_loop, z0, keep_plans=True, w0=a.w0)
                torch.cuda.synchronize()
                akw = {} if scenes is None else {"scenes": scenes}
                if fleet is not None:
                    akw = {"scenes": fleet, "fleet": fleet.cfg}
                audit = pl.audit_closed_loop(res, p, goal_tol=a.goal_tol, **akw)
            if fleet is not None:                                       # the scenes each plan ran against, as the loop built them
                fo, fv, fn = (res["fleet_" + k].cpu().numpy() for k in ("obs", "vel", "n"))
                plan_scenes = pl.Scenes(goal=None if fleet.goal is None else np.tile(fleet.goal, (a.closed_loop, 1)),
                                        obs_c=fo[..., :2].reshape(-1, 8, 2), obs_r=fo[..., 2].reshape(-1, 8), n_obs=fn.reshape(-1),
                                        obs_v=fv.reshape(-1, 8, 2))
            elif scenes is not None and scenes.obs_v is not None:       # the starts' scenes where they were at each step's time
                at = [scenes.at(k * p.dt) for k in range(a.closed_loop)]
                cat = lambda key: None if getattr(scenes, key) is None else np.concatenate([getattr(s, key) for s in at])
                plan_scenes = pl.Scenes(cat("goal"), cat("obs_c"), cat("obs_r"), cat("n_obs"), cat("obs_v"))
            elif scenes is not None:                                    # plans.npz holds (H, P) plans: the starts' scenes once per step
                plan_scenes = scenes.take(np.tile(np.arange(scenes.S), a.closed_loop))
            hist = first["hist"]
            plans_z0, plans_v = res["plans_z"][:, :, 0].reshape(-1, 2), res["plans_v"].reshape(-1, p.N, 2)
            extra = {"n_bad": [int(x) for x in res["n_bad"].sum(dim=1).cpu()], "cost": res["cost"].cpu().double().tolist(),
                     "min_clear": res["min_clear"].cpu().double().tolist() if p.n_obs else None}
            if scenes is not None or fleet is not None:                 # a scene without obstacles has min_clear = +inf: null in JSON
                clear = res["min_clear"].cpu().double()
                extra["min_clear"] = [[float(x) if np.isfinite(x) else None for x in row] for row in clear.tolist()]
    finally:
        if sim is not None:
            sim.close()
        if model is not None:
            model.close()
    out = {"audit": audit, "hist": hist.cpu().double().tolist(), "closed_loop": a.closed_loop, "starts": z0.double().tolist(),
           "mppi": {**{k: v for k, v in vars(mppi_cfg(a)).items() if k != "lambda_"}, "lambda": a.lambda_}, "problem": p.to_json(),
           "run": a.run, "tube": a.tube or p.tube_kind, "level": a.level, "calibrated": calib is not None, "sim_cfg": list(a.sim_cfg), **extra, **robot}
    if a.w0 != "zero":
        out["w0"] = a.w0
    if a.planner != "mppi":
        out.update({"planner": a.planner, "grad": vars(grad_cfg(a))})
    if scenes is not None:
        out["scenes"] = scenes_src
    if fleet is not None:
        out["fleet"] = vars(fleet.cfg)
    folder = a.out or a.run or "."
    os.makedirs(folder, exist_ok=True)
    with open(os.path.join(folder, "plan.json"), "w") as f:
        json.dump(out, f, indent=1, allow_nan=False)
    np.savez(os.path.join(folder, "plans.npz"), z0=plans_z0.cpu().numpy(), v=plans_v.cpu().numpy())
    if plan_scenes is not None:
        plan_scenes.save(os.path.join(folder, "scenes.npz"))
    if a.closed_loop is None:
        print(f"{audit['plans']} plans x {audit['nodes']} nodes: predicted safe {audit['predicted_safe']:.4f}, actually safe "
              f"{audit['actually_safe']:.4f}, covered at every node {audit['covered_plans']:.4f}")
    elif a.robot and not audit["completed"]:
        print(f"{audit['robots']} robots x {audit['steps']} steps on the robot: completed 0, terminated {audit['terminated']}")
    else:
        if a.robot:
            print(f"on the robot: completed {audit['completed']} of {audit['robots']}, terminated {audit['terminated']}, covered at every "
                  f"step, of all: {audit['covered_robots_of_all']:.4f}; of the completed:")
        print(f"{audit['robots']} robots x {audit['steps']} steps: coverage {audit['coverage']:.4f}, covered at every step "
              f"{audit['covered_robots']:.4f}, actually safe {audit['actually_safe']:.4f}, reached the goal {audit['reached_goal']:.4f}")
    return out


if __name__ == "__main__":
    main()
