"""Plans tracked by the legged robot: B plans from tube/plan.py handed to B simulated robots of the
trajectory env under a trained policy, recorded at the ROM rate on the device, and audited against the tube -- what the reference's
deep_tube_learning/evaluation/evaluate_tube_simple_oneshot_on_mpc_traj.py:75-132 does with its ROM stand-in, done with the robot
the tube was learned for.  ``tube/plan.py::track`` stays the ROM-on-ROM tracker; this module is its counterpart on the HIP env.

The env runs ``trajectory_generator.cls = 'PlanTrajectoryGenerator'`` (LG_TG_KIND_PLAN, this project's own generator class:
csrc/lg_traj.h): every env's ROM window is advanced with its own plan's inputs, one per ROM step.  The record is taken by
``k_traj_record`` (lg_traj_rec_begin / lg_traj_rec_step): one small launch after every env step, no device-to-host read.

Alignment.  The window's head runs Nw = trajectory_generator.N ROM steps ahead of ``trajectory[:, 0]``, the point the robot tracks,
so plan node j is recorder row Nw + j (j = 0..Np); rows 0..Nw - 1 are the lead-in on the start point.  A row is written on the env
step of the ROM step, after the env's clock moved on by env.dt, so ``z_ref`` sits env.dt into the interval past its node:
z_ref[j] = Z_j + (Z_{j+1} - Z_j) env.dt / rom.dt.  That is how ``collect()`` (scripts/collect_trajectory_data.py) records the data
the tube was trained on, so the audit measures the error the tube predicts.

Replanning.  ``closed_loop_env`` is ``plan.closed_loop`` with the robot as the tracker: at every ROM step
a new plan from window point 1, the node the robot is heading for, and ``traj_gen.replan`` (lg_traj_replan) rewrites the window
behind it.  There recorder row r sits env.dt into the interval past node r - 1 -- node k is row k + 1 -- and ``rom_schedule`` tells the
loop how many env steps each ROM step takes, so nothing is read back from the device inside it.
"""
import copy
import ctypes as C

from .. import capi
from .plan import audit, audit_closed_loop, shift_past, shift_plan

PLAN_KIND = capi.TG_KINDS["PlanTrajectoryGenerator"]


# ---------------------------------------------------------------- the recorder
def rec_refusal(rec, N, env_x_n):
    """lg_traj_rec_check on the host, in the library's words (without its "lg_traj_rec: " prefix): None, or why `rec` (a
    capi.lg_traj_rec) is refused for N envs whose state vector has env_x_n entries."""
    if N < 1:
        return f"N = {N} must be at least 1"
    if rec.rows_max < 2:
        return f"rows_max = {rec.rows_max} must be at least 2"
    for name in ("z", "pz_x", "v", "rows", "dead", "k_mark"):
        if not getattr(rec, name):
            return f"{name} is null"
    if rec.x and rec.x_n != env_x_n:
        return f"x_n = {rec.x_n} must be the env's {env_x_n}"
    if not rec.x and rec.x_n != 0:
        return f"x_n = {rec.x_n} must be 0 without x"
    return None


class TrajRecorder:
    """lg_traj_rec on one trajectory env (any generator kind): the caller-owned device buffers z, pz_x (N, rows_max, 2),
    v (N, rows_max - 1, 2), rows (N) int32, dead (N) uint8, k_mark (N) and, with want_x, x (N, rows_max, x_n) in get_state()'s
    layout.  begin() writes row 0; step() after every env step writes a row for every env whose ROM stepped, and marks an env
    that reset as dead.  Per-env ROM-rate recording: not collect()'s global "until every ROM has stepped" criterion."""

    def __init__(self, env, rows_max, want_x=False):
        import torch
        if getattr(env.setup, "traj", None) is None:
            raise ValueError("the recorder needs a trajectory env")
        N, dev = env.num_envs, env.device
        self.env, self.rows_max = env, int(rows_max)
        self.x_n = 13 + 2 * env.num_actions
        if self.rows_max < 2:
            raise ValueError(f"rows_max = {self.rows_max} must be at least 2")
        R = self.rows_max
        self.z, self.pz_x = torch.zeros(N, R, 2, device=dev), torch.zeros(N, R, 2, device=dev)
        self.v = torch.zeros(N, R - 1, 2, device=dev)
        self.rows = torch.zeros(N, dtype=torch.int32, device=dev)
        self.dead = torch.zeros(N, dtype=torch.uint8, device=dev)
        self.k_mark = torch.zeros(N, device=dev)
        self.x = torch.zeros(N, R, self.x_n, device=dev) if want_x else None
        r = capi.lg_traj_rec()
        r.rows_max, r.x_n = R, self.x_n if want_x else 0
        for name in ("z", "pz_x", "v", "rows", "dead", "k_mark"):
            setattr(r, name, getattr(self, name).data_ptr())
        r.x = self.x.data_ptr() if want_x else None
        why = rec_refusal(r, N, self.x_n)
        if why:
            raise ValueError(why)
        self.struct = r

    def begin(self):
        self.env.core.call("traj_rec_begin", C.byref(self.struct))

    def step(self):
        self.env.core.call("traj_rec_step", C.byref(self.struct))


# ---------------------------------------------------------------- configuration
def plan_env_cfg(task, B, push_robots=False):
    """(env_cfg, train_cfg) of `task` for tracking B plans: scripts/evaluate_tracking.py:66-76's overrides -- 20 s episodes, no
    randomisation, no ROM start offset, no curriculum -- with PlanTrajectoryGenerator and B envs, and pushes only on request."""
    from ..envs import task_registry                              # importing the package registers the tasks
    env_cfg, train_cfg = task_registry.get_cfgs(name=task)
    env_cfg, train_cfg = copy.deepcopy(env_cfg), copy.deepcopy(train_cfg)
    if not hasattr(env_cfg, "trajectory_generator"):
        raise ValueError(f"task {task!r} is not a trajectory-tracking task")
    if int(B) < 1:
        raise ValueError(f"B = {B} must be at least 1")
    env_cfg.env.num_envs = int(B)
    env_cfg.env.episode_length_s = 20
    env_cfg.trajectory_generator.cls = "PlanTrajectoryGenerator"
    dr = env_cfg.domain_rand
    dr.randomize_friction = dr.randomize_base_mass = dr.randomize_inv_base_mass = False
    dr.push_robots = bool(push_robots)
    if not push_robots:
        # the trajectory env pushes from per-env timers whatever push_robots says (as the reference does, legged_robot_trajectory.py:
        # 150-160): without the request the timers start beyond any horizon
        dr.time_between_pushes = [1e6, 1e6]
    rsp = dr.rigid_shape_properties
    rsp.randomize_restitution = rsp.randomize_compliance = rsp.randomize_thickness = False
    dr.randomize_rom_distance = False
    env_cfg.curriculum.use_curriculum = False
    return env_cfg, train_cfg


# ---------------------------------------------------------------- tracking
def rom_substeps(env):
    """S: env steps per ROM step."""
    return max(1, int(round(float(env.setup.traj["rom_dt"]) / float(env.dt))))


def horizon_steps(Nw, Np, S):
    """Env steps track_env takes: Nw lead-in rows, Np + 1 plan nodes, and S more for a ROM step that the generator's `- 1e-5`
    comparison delays by one env step."""
    return (Nw + Np + 1) * S + S


def check_track(env, v, z0, H_rev=0, allow_fast=False):
    """track_env's refusals (ValueError); returns (B, Np, Nw, S, steps).  v, z0: tensors."""
    from ..envs.base.obs_history import refuse_history
    refuse_history(env, "track_env")
    traj = getattr(env.setup, "traj", None)
    if traj is None or traj["kind"] != PLAN_KIND:
        raise ValueError("track_env needs an env with trajectory_generator.cls = 'PlanTrajectoryGenerator' (plan_env_cfg)")
    B = env.num_envs
    if v.dim() != 3 or v.shape[0] != B or v.shape[1] < 1 or v.shape[2] != 2:
        raise ValueError(f"v must be ({B}, Np >= 1, 2), one plan per env; got {tuple(v.shape)}")
    Np, Nw = int(v.shape[1]), int(traj["N"])
    if Np > capi.PLAN_MAX_N:
        raise ValueError(f"Np = {Np} exceeds LG_PLAN_MAX_N = {capi.PLAN_MAX_N}")
    if tuple(z0.shape) != (B, 2):
        raise ValueError(f"z0 must be {(B, 2)}; got {tuple(z0.shape)}")
    if not 0 <= H_rev <= Nw:
        raise ValueError(f"H_rev = {H_rev} must lie in 0..{Nw}: the robot's history is the {Nw} lead-in rows of the window")
    S = rom_substeps(env)
    steps = horizon_steps(Nw, Np, S)
    if steps + 1 > int(env.max_episode_length):                     # env.reset() leaves the episode at step 1
        raise ValueError(f"the horizon takes {steps} env steps after the reset's own; max_episode_length is {int(env.max_episode_length)}")
    if not allow_fast:
        import torch
        lo, hi = torch.as_tensor(env.rom.v_min).to(v.device, v.dtype), torch.as_tensor(env.rom.v_max).to(v.device, v.dtype)
        over = torch.maximum(v - hi, lo - v).amax()
        if float(over) > 1e-6:
            raise ValueError(f"the plans' inputs reach |v| = {float(v.abs().amax()):.4g} m/s; the env's rom.v_min / v_max are "
                             f"{[round(float(x), 6) for x in lo.tolist()]} / {[round(float(x), 6) for x in hi.tolist()]}: rebuild the problem "
                             "inside them (PlanProblem.named(name, rom_v_min=..., rom_v_max=...)) or pass allow_fast=True")
    return B, Np, Nw, S, steps


def align(rec_z, rec_pz, rows, dead, z0, Nw, Np, H_rev=0):
    """The recorder's raw rows (device tensors z, pz_x (B, Nw + Np + 1, 2), rows, dead (B)) as track()'s keys.  Plan node j is
    row Nw + j.  The plan's frame: world minus z of row 0 (the window's start point) plus z0, in float64 and rounded once."""
    import torch
    sl = slice(Nw, Nw + Np + 1)
    origin = rec_z[:, :1].double()
    shift = lambda t: ((t[:, sl].double() - origin) + z0.double()[:, None, :]).float()
    w_all = torch.linalg.vector_norm(rec_z - rec_pz, dim=-1)        # world coordinates: the collector's error, every row
    w_true = w_all[:, sl]
    completed = (rows == Nw + Np + 1) & (dead == 0)
    B = rec_z.shape[0]
    return {"pz_x": shift(rec_pz), "z_ref": shift(rec_z), "w_true": w_true.contiguous(), "completed": completed, "rows": rows,
            "dead": dead != 0, "e_past": w_all[:, Nw - H_rev:Nw].contiguous(), "v_prev": torch.zeros(B, H_rev, 2, device=rec_z.device),
            "w0": w_true[:, 0].contiguous()}


def track_env(env, policy, v, z0, H_rev=0, want=(), allow_fast=False):
    """The plans v (B, Np, 2) from z0 (B, 2), B == env.num_envs, tracked by the env's robots under `policy` (obs -> actions).
    env.reset(); set_plans(v); traj_gen.reset(root xy) -- every window restarts at its robot; the recorder begins; then
    (Nw + Np + 1) S + S env steps, each followed by one recorder launch and no device-to-host read.
    Returns device tensors with track()'s keys -- pz_x, z_ref (B, Np + 1, 2) in the plan's frame, w_true (B, Np + 1) = |z - pz_x| in
    world coordinates -- and completed (B) bool (rows == Nw + Np + 1 and not dead), rows, dead, and the robot's own history for the
    tube's item: e_past (B, H_rev) = w_true of rows Nw - H_rev .. Nw - 1, v_prev = zeros (B, H_rev, 2), w0 = w_true[:, 0]; feed
    those to HipPlanScorer.score(z0, v, e=, v_prev=, w0=).  want: "x" adds x (B, Np + 1, x_n), "rec" the TrajRecorder itself.
    A robot that falls or times out stops recording (dead): its later rows stay zero and it is not completed."""
    import torch
    bad = [k for k in want if k not in ("x", "rec")]
    if bad:
        raise ValueError(f"want {bad}: of x, rec")
    v = torch.as_tensor(v).to(env.device, torch.float32).contiguous()
    z0 = torch.as_tensor(z0).to(env.device, torch.float32).contiguous()
    B, Np, Nw, S, steps = check_track(env, v, z0, H_rev, allow_fast)
    rec = TrajRecorder(env, Nw + Np + 1, want_x="x" in want)
    with torch.no_grad():
        env.reset()
        env.traj_gen.set_plans(v)
        start = env.rom.proj_z(env.root_states).clone()
        env.traj_gen.reset(start)
        # lg_traj_reset leaves the observed trajectory to the next step callback; the window is constant at `start`, and so is
        # its interpolation: row 0 records the window's start point
        env.trajectory.copy_(start[:, None, :].expand_as(env.trajectory))
        rec.begin()
        obs = env.get_observations()
        for _ in range(steps):
            obs = env.step(policy(obs.detach()).detach())[0]
            rec.step()
    out = align(rec.z, rec.pz_x, rec.rows, rec.dead, z0, Nw, Np, H_rev)
    if "x" in want:
        out["x"] = rec.x[:, Nw:Nw + Np + 1]
    if "rec" in want:
        out["rec"] = rec
    return out


# ---------------------------------------------------------------- replanning on the robot
def clock_schedule(Nw, rom_dt, dt, n_rom_steps):
    """The generator's clock in float32, one rounding per operation: after tg_reset -- t = -Nw rom_dt and Nw sums t += rom_dt, k = 0 --
    every env step tests t >= k rom_dt - 1e-5 (a ROM step: k += 1) and then adds dt.  Returns, for each of the next n_rom_steps ROM
    steps, the env steps up to and including the one it falls on.  The first is 1; an entry above round(rom_dt / dt) is a ROM step
    that the comparison delays by one env step."""
    import numpy as np
    f32 = np.float32
    rom_dt, dt = f32(rom_dt), f32(dt)
    t = f32(f32(-int(Nw)) * rom_dt)
    for _ in range(int(Nw)):
        t = f32(t + rom_dt)
    if not (dt > 0 and rom_dt > 0):
        raise ValueError(f"the clock does not reach a ROM step: rom_dt = {float(rom_dt)}, dt = {float(dt)} must be positive")
    k, out, steps = f32(0), [], 0
    while len(out) < int(n_rom_steps):
        steps += 1
        if t >= f32(f32(k * rom_dt) - f32(1e-5)):
            k = f32(k + f32(1))
            out.append(steps)
            steps = 0
        t = f32(t + dt)
    return out


def rom_schedule(env, n_rom_steps):
    """How many env steps each of the next n_rom_steps ROM steps takes after traj_gen.reset (clock_schedule on the env's N, rom_dt and
    dt).  Every live env shares that clock, so the schedule is the same for all of them and a loop needs no device read to know when
    a recorder row was written."""
    tj = env.setup.traj
    return clock_schedule(int(tj["N"]) * int(tj["dN"]), tj["rom_dt"], env.setup.dt, n_rom_steps)


def check_closed_loop(env, problem, H, w0="zero", allow_fast=False):
    """closed_loop_env's refusals (ValueError); returns (B, Nw, schedule of H + 1 ROM steps)."""
    from ..envs.base.obs_history import refuse_history
    refuse_history(env, "closed_loop_env")
    traj = getattr(env.setup, "traj", None)
    if traj is None or traj["kind"] != PLAN_KIND:
        raise ValueError("closed_loop_env needs an env with trajectory_generator.cls = 'PlanTrajectoryGenerator' (plan_env_cfg)")
    if H < 1:
        raise ValueError(f"H = {H} must be at least 1")
    if w0 not in ("zero", "error"):
        raise ValueError(f"w0 = {w0!r}: 'zero' or 'error'")
    if float(problem.dt) != float(traj["rom_dt"]):
        raise ValueError(f"problem.dt = {problem.dt} is not the env's rom.dt = {traj['rom_dt']}: replanning happens at the ROM's rate")
    Nw = int(traj["N"])
    if int(problem.N) < Nw:
        raise ValueError(f"problem.N = {problem.N} is shorter than the env's window, trajectory_generator.N = {Nw}: the plan must fill the window")
    sched = rom_schedule(env, H + 1)
    if sum(sched) + 1 > int(env.max_episode_length):                # env.reset() leaves the episode at step 1
        raise ValueError(f"the horizon takes {sum(sched)} env steps after the reset's own; max_episode_length is {int(env.max_episode_length)}")
    if not allow_fast:
        lo, hi = [float(x) for x in env.rom.v_min], [float(x) for x in env.rom.v_max]
        if any(float(a) < b - 1e-6 for a, b in zip(problem.rom_v_min, lo)) or any(float(a) > b + 1e-6 for a, b in zip(problem.rom_v_max, hi)):
            raise ValueError(f"problem.rom_v_min / rom_v_max = {list(problem.rom_v_min)} / {list(problem.rom_v_max)} reach beyond the env's "
                             f"rom.v_min / v_max = {[round(x, 6) for x in lo]} / {[round(x, 6) for x in hi]}: rebuild the problem inside them "
                             "(PlanProblem.named(name, rom_v_min=..., rom_v_max=...)) or pass allow_fast=True")
    return env.num_envs, Nw, sched


def closed_loop_env(env, policy, planner, H, start=None, iters_first=None, keep_plans=False, w0="zero", allow_fast=False):
    """plan.closed_loop (trajopt/tube_planning_closed_loop.py:82-168, "TPCL") with the legged robot as the tracker, for
    B = env.num_envs robots: H times -- plan from window point 1, the node the robot is heading for; rewrite the window behind it
    (traj_gen.replan, skipping robots that reset); take the env steps of one ROM interval.  planner: HipMppiPlanner, HipGradPlanner or
    ChainedPlanner (with Scenes, robot b lives in scene b).  start (2,) or (B, 2): the plan frame's image of the robots' start
    points, None = problem.start; the plan frame is (world - start_world) + start in float64, rounded once.
    Row r of the recorder is written env.dt into the interval past node r - 1, so node k is row k + 1; the tube item's past is the
    robot's own record: e takes |z - pz_x| of row j + 1 (world coordinates), v_prev the committed input (TPCL:159-163).  The loop reads
    nothing back: the env steps per ROM interval come from rom_schedule.  After it one device read checks that every robot that did
    not reset has its H + 2 rows; RuntimeError naming the schedule otherwise.
    Returns device tensors z, pz_x (B, H+1, 2) -- recorder rows 1..H+1 in the plan frame --, z_node (B, H+1, 2) the nodes planned
    from (start, then every later window point 1), v (B, H, 2) the committed inputs, w (B, H+1) -- 0 or the first w0, then w_sol[:, 1]
    of each plan in force --, cost, min_clear, best_J, n_bad (B, H), completed (B) bool, rows, dead and, with keep_plans, plans_v,
    plans_z, plans_w as closed_loop returns them."""
    import torch
    p = planner.problem
    B, Nw, sched = check_closed_loop(env, p, H, w0, allow_fast)
    dev = env.device
    s_plan = torch.as_tensor(p.start if start is None else start, dtype=torch.float32).to(dev)
    s_plan = s_plan.reshape(-1, 2).expand(B, 2).contiguous() if s_plan.numel() == 2 else s_plan.reshape(-1, 2).contiguous()
    if tuple(s_plan.shape) != (B, 2):
        raise ValueError(f"start must be (2,) or {(B, 2)}; got {tuple(s_plan.shape)}")
    tg = env.traj_gen
    rec = TrajRecorder(env, H + 2)
    norm = lambda d: torch.linalg.vector_norm(d, dim=-1)
    with torch.no_grad():
        env.reset()
        tg.set_plans(torch.zeros(B, 0, 2, device=dev))
        s_world = env.rom.proj_z(env.root_states).clone()
        tg.reset(s_world)
        env.trajectory.copy_(s_world[:, None, :].expand_as(env.trajectory))      # as track_env: the window is constant at the start
        rec.begin()
        frame = lambda t: ((t.double() - s_world.double().reshape((B,) + (1,) * (t.dim() - 2) + (2,))) +
                           s_plan.double().reshape((B,) + (1,) * (t.dim() - 2) + (2,))).float()
        e, v_prev = torch.zeros(B, p.H_rev, device=dev), torch.zeros(B, p.H_rev, 2, device=dev)
        err = norm(rec.z[:, 0] - rec.pz_x[:, 0])
        w_start = (lambda: None) if w0 == "zero" else (lambda: err)
        nodes, v, w = [], [], [torch.zeros(B, device=dev) if w0 == "zero" else err]
        cost, clear, bestJ, nbad, plans = [], [], [], [], {"v": [], "z": [], "w": []}
        obs, warm = env.get_observations(), None
        for j in range(H + 1):
            origin = frame(tg.trajectory[:, 1]).contiguous()
            nodes.append(origin)
            if j < H:
                sol = planner.plan(origin, warm, e, v_prev, w_start(), iters=iters_first) if j == 0 else \
                    planner.plan(origin, warm, e, v_prev, w_start())
                v_sol = sol["v"]
                tg.replan(v_sol, skip=rec.dead)
                v.append(v_sol[:, 0]), w.append(sol["score"]["w"][:, 1])
                cost.append(sol["score"]["cost"]), clear.append(sol["score"]["min_clear"]), bestJ.append(sol["best_J"]), nbad.append(sol["n_bad"])
                if keep_plans:
                    plans["v"].append(v_sol), plans["z"].append(sol["score"]["z"]), plans["w"].append(sol["score"]["w"])
                warm = shift_plan(v_sol)
            for _ in range(sched[j]):
                obs = env.step(policy(obs.detach()).detach())[0]
                rec.step()
            if j < H:                                               # recorder row j + 1 now exists
                err = norm(rec.z[:, j + 1] - rec.pz_x[:, j + 1])    # world coordinates: the collector's error
                e, v_prev = shift_past(e, v_prev, err, v_sol[:, 0])
        rows, dead = rec.rows.cpu(), rec.dead.cpu()                 # the one device read
    short = ((dead == 0) & (rows != H + 2)).nonzero().flatten()
    if short.numel():
        raise RuntimeError(f"{short.numel()} robot(s) that did not reset have not H + 2 = {H + 2} recorder rows (robot {int(short[0])}: "
                           f"{int(rows[short[0]])}): the env steps per ROM step taken from rom_schedule, {sched}, are not the device's")
    out = {"z": frame(rec.z[:, 1:]), "z_node": torch.stack(nodes, 1), "v": torch.stack(v, 1), "w": torch.stack(w, 1),
           "pz_x": frame(rec.pz_x[:, 1:]), "cost": torch.stack(cost, 1), "min_clear": torch.stack(clear, 1), "best_J": torch.stack(bestJ, 1),
           "n_bad": torch.stack(nbad, 1), "completed": (rec.rows == H + 2) & (rec.dead == 0), "rows": rec.rows, "dead": rec.dead != 0}
    if keep_plans:
        out.update({"plans_" + k: torch.stack(t, 0) for k, t in plans.items()})
    return out


def audit_closed_loop_env(result, problem, goal_tol=0.1, scenes=None):
    """plan.audit_closed_loop over the completed robots, plus completed / terminated (robots that reset: fell or timed out) and
    covered_robots_of_all, in which a robot that did not complete counts as not covered.  "robots" counts all of them.  Strict JSON;
    with no completed robot the shares are None.  scenes: a plan.Scenes of S = all the robots; the completed ones keep their own."""
    import torch
    done = result["completed"].detach().cpu().bool()
    B, n, H = int(done.numel()), int(done.sum()), int(result["v"].shape[1])
    head = {"robots": B, "completed": n, "terminated": int(result["dead"].detach().cpu().bool().sum())}
    if n == 0:
        empty = {"steps": H, "coverage_by_step": None, "coverage": None, "covered_robots": None, "actually_safe": None, "predicted_safe": None,
                 "goal_tol": float(goal_tol), "reached_goal": None, "goal_distance_mean": None, "error_mean": None, "error_max": None}
        return {**empty, **head, "covered_robots_of_all": 0.0}
    idx = done.nonzero().flatten()
    picked = {k: result[k].detach().cpu()[idx] for k in ("z", "w", "pz_x", "min_clear")}
    res = audit_closed_loop(picked, problem, goal_tol=goal_tol, scenes=None if scenes is None else _completed_scenes(scenes, B, idx))
    err = torch.linalg.vector_norm(picked["z"].double() - picked["pz_x"].double(), dim=-1)
    covered = (picked["w"].double() >= err).all(dim=1)
    if "by_robot" in res:
        res["by_robot"]["robot"] = [int(i) for i in idx]
    return {**res, **head, "covered_robots_of_all": float(covered.sum()) / B}


# ---------------------------------------------------------------- audit
def _completed_scenes(scenes, B, idx):
    from .plan import scenes_check
    scenes_check(scenes, B)
    return scenes.take(idx.numpy())


def audit_env(score, trk, problem, scenes=None):
    """plan.audit over the completed plans, plus completed / terminated (robots that reset: fell or timed out) and
    covered_plans_of_all, in which a robot that did not complete counts as not covered.  "plans" counts all of them.  Strict JSON;
    with no completed plan the shares are None.  scenes: a plan.Scenes of S = all the plans; the completed ones keep their own."""
    import torch
    done = trk["completed"].detach().cpu().bool()
    B, n = int(done.numel()), int(done.sum())
    head = {"plans": B, "completed": n, "terminated": int(trk["dead"].detach().cpu().bool().sum())}
    if n == 0:
        empty = {"nodes": int(trk["w_true"].shape[1]), "coverage_by_node": None, "coverage": None, "covered_plans": None,
                 "predicted_safe": None, "actually_safe": None, "table": None, "w_true_mean": None, "w_true_max": None}
        return {**empty, **head, "covered_plans_of_all": 0.0}
    idx = done.nonzero().flatten()
    pick = lambda t: t.detach().cpu()[idx]
    res = audit({"w": pick(score["w"]), "min_clear": pick(score["min_clear"])},
                {"w_true": pick(trk["w_true"]), "pz_x": pick(trk["pz_x"])}, problem,
                scenes=None if scenes is None else _completed_scenes(scenes, B, idx))
    covered = (pick(score["w"]).double() >= pick(trk["w_true"]).double()).all(dim=1)
    return {**res, **head, "covered_plans_of_all": float(covered.sum()) / B}
