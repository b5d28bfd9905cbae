"""ROM trajectories tracked by a VELOCITY-COMMAND policy: the reference's
deep_tube_learning/data_collection_velocity.py:84-156 on the device.  A SingleInt2D reduced-order model at rom.dt = env.dt runs
beside a velocity-command env (anymal_c_flat, rough terrain, A1, ANYmal-B, Cassie); a proportional law turns its desired pose and
velocity into a body-frame velocity command, written over the command columns of the observation, and the velocity policy does the
rest.  ``HipCommandTracker`` is ``lg_cmdtrack_*`` (csrc/cmdtrack_kernels.hip): one launch per env step, one lane per env, nothing
read back; the law is spelled out in include/legged_hip.h.

``collect`` returns the epoch dicts of scripts/collect_trajectory_data.py::collect (z, v, pz_x, done [, x, u]), so the dataset
builders, trainers, calibration and audits run on data of any velocity task.  Records are ENV-MAJOR -- z, pz_x (N, T+1, 2),
v (N, T, 2), done (N, T) -- the layout of the epoch pickles and tube/device_data.from_records; the reference's velocity script is
time-major.  ``track_cmd`` is tube/plan.py::track with the legged robot under a velocity policy as the tracker.

The observation's command columns hold command x commands_scale (legged_robot.py:208-226), so ``cmd_scale`` defaults to the
env's commands_scale; the reference writes the command raw (a policy then sees a command of half the size), which is
``cmd_scale = (1, 1, 1)``, ``raw_commands=True``.  There is no fallback: without the library or a GPU the tracker raises.
"""
import ctypes as C
import dataclasses

from .. import capi

RANDOM, PLAN = capi.TG_KINDS["TrajectoryGenerator"], capi.TG_KINDS["PlanTrajectoryGenerator"]
CMD_COL = 9                                                     # base lin vel 3, ang vel 3, gravity 3, then the commands


@dataclasses.dataclass
class CmdTrackCfg:
    """lg_cmdtrack_cfg, field for field.  The reference ships no configuration for its velocity script (Kp, u_min, u_max and
    track_yaw come from a `default.yaml` that is not in its tree); the defaults here are Kp = I, yaw not tracked (the value its
    other data-generation configurations give), commands within +-1 and the trajectory tasks' generator (N = 10, hold 1..2 s,
    0.01..2 Hz)."""
    kind: int = RANDOM
    track_yaw: bool = False
    Kp: tuple = (1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0)   # row-major 3 x 3
    u_min: tuple = (-1.0, -1.0, -1.0)
    u_max: tuple = (1.0, 1.0, 1.0)
    cmd_scale: tuple = (1.0, 1.0, 1.0)
    cmd_col: int = CMD_COL
    rom_v_min: tuple = (-1.0, -1.0)
    rom_v_max: tuple = (1.0, 1.0)
    t_low: float = 1.0
    t_high: float = 2.0
    freq_low: float = 0.01
    freq_high: float = 2.0
    prob_stationary: float = 0.01
    weight_sampler: int = capi.TG_WEIGHT_SAMPLERS["UniformWeightSampler"]
    tg_N: int = 10
    seed: int = 0
    x_n: int = 0                                                # 0, or the env's 13 + 2 num_actions: the optional x record
    rom_dt: float = 0.0                                         # the env's dt (from_env); not a field of the C struct

    @classmethod
    def from_env(cls, env, raw_commands=False, want_x=False, **kw):
        """A configuration for `env`: cmd_scale = the env's commands_scale (ones with raw_commands), rom_dt = env.dt, x_n."""
        s = env.core.cfg_struct
        scale = (1.0, 1.0, 1.0) if raw_commands else (float(s.obs_scale_lin_vel), float(s.obs_scale_lin_vel), float(s.obs_scale_ang_vel))
        kw.setdefault("cmd_scale", scale)
        kw.setdefault("seed", int(getattr(env.setup, "seed", 0)))
        return cls(rom_dt=float(env.dt), x_n=13 + 2 * int(env.num_actions) if want_x else 0, **kw)

    def to_struct(self):
        c = capi.lg_cmdtrack_cfg()
        c.kind, c.track_yaw, c.cmd_col = int(self.kind), int(bool(self.track_yaw)), int(self.cmd_col)
        c.weight_sampler, c.tg_N, c.x_n, c.seed = int(self.weight_sampler), int(self.tg_N), int(self.x_n), int(self.seed)
        import numpy as np
        for name, n in (("Kp", 9), ("u_min", 3), ("u_max", 3), ("cmd_scale", 3), ("rom_v_min", 2), ("rom_v_max", 2)):
            vals = np.asarray(getattr(self, name), dtype=float).reshape(-1).tolist()       # Kp also as a 3 x 3
            if len(vals) != n:
                raise ValueError(f"{name} must have {n} entries; got {len(vals)}")
            getattr(c, name)[:] = vals
        c.t_low, c.t_high, c.freq_low, c.freq_high = float(self.t_low), float(self.t_high), float(self.freq_low), float(self.freq_high)
        c.prob_stationary = float(self.prob_stationary)
        return c

    def check(self, env_traj=False, num_obs=48, env_x_n=37, rec=None):
        """lg_cmdtrack_check on the host, in the library's words (without its "lg_cmdtrack: " prefix): ValueError naming the
        field.  rec: a capi.lg_cmdtrack_rec or None."""
        why = refusal(self.to_struct(), rec, env_traj, num_obs, env_x_n)
        if why:
            raise ValueError(why)


def refusal(c, rec, env_traj, num_obs, env_x_n):
    """lg_cmdtrack_check restated: None, or the C side's sentence for the structs c (lg_cmdtrack_cfg) and rec (or None)."""
    import math
    if c is None:
        return "cfg is null"
    if env_traj:
        return "the env is a trajectory env: its observation has no command columns (collect_trajectory_data.py serves it)"
    if c.kind not in (RANDOM, PLAN):
        return f"kind = {c.kind} must be LG_TG_KIND_RANDOM (0) or LG_TG_KIND_PLAN (4)"
    if c.cmd_col < 0 or c.cmd_col + 3 > num_obs:
        return f"cmd_col = {c.cmd_col}: cmd_col .. cmd_col + 2 must lie within the num_obs = {num_obs} observations"
    if c.x_n != 0 and c.x_n != env_x_n:
        return f"x_n = {c.x_n} must be 0 or the env's {env_x_n}"
    for j in range(9):
        if not math.isfinite(c.Kp[j]):
            return f"Kp[{j}] is not finite"
    for j in range(3):
        if not c.u_min[j] <= c.u_max[j]:
            return f"u_min[{j}] exceeds u_max[{j}] (or one is not a number)"
        if not math.isfinite(c.cmd_scale[j]):
            return f"cmd_scale[{j}] is not finite"
    if c.kind == RANDOM:
        if c.weight_sampler not in (0, 1):
            return f"weight_sampler = {c.weight_sampler} must be LG_TG_WSAMP_UNIFORM (0) or LG_TG_WSAMP_NO_RAMP (1)"
        if not 1 <= c.tg_N <= capi.TRAJ_MAX_PTS - 1:
            return f"tg_N = {c.tg_N} must lie in 1..{capi.TRAJ_MAX_PTS - 1}"
        if not c.t_low > 0 or not c.t_high >= c.t_low:
            return "t_low / t_high must satisfy 0 < t_low <= t_high"
        for d in range(2):
            if not c.rom_v_min[d] <= c.rom_v_max[d]:
                return f"rom_v_min[{d}] exceeds rom_v_max[{d}] (or one is not a number)"
    if rec is not None:
        if rec.T < 1:
            return f"T = {rec.T} must be at least 1"
        for name in ("z", "v", "pz_x", "done"):
            if not getattr(rec, name):
                return f"{name} is null"
        if rec.x and c.x_n == 0:
            return "x is given but x_n = 0"
    return None


def is_trajectory_env(env):
    return getattr(env.setup, "traj", None) is not None


class HipCommandTracker:
    """lg_cmdtrack on one velocity-command env.  begin(T, epoch) allocates the epoch's records (device tensors, env-major) and
    writes command 0 into env.obs_buf; step(t) after env step t records it and writes command t + 1; records() gives the dict.
    The tracker keeps the env object alive and hands its context to every call; the library side holds no pointer into it, so
    close() of either, in any order, leaves nothing dangling -- a call after env.close() is refused here."""

    def __init__(self, env, cfg=None):
        import torch
        from ..lib import LeggedHipError, device_tensor, load
        from ..envs.base.obs_history import refuse_history
        refuse_history(env, "HipCommandTracker")     # the command goes into obs[:, 9:12] after the step, hence after the history's launch
        self._err, self._device_tensor = LeggedHipError, device_tensor
        self.env = env
        self.cfg = cfg if cfg is not None else CmdTrackCfg.from_env(env)
        self.x_n_env = 13 + 2 * int(env.num_actions)
        self.cfg.check(is_trajectory_env(env), int(env.core.cfg_struct.num_obs), self.x_n_env)
        if self.cfg.rom_dt and abs(float(self.cfg.rom_dt) - float(env.dt)) > 1e-9:
            raise ValueError(f"rom_dt = {self.cfg.rom_dt} must be the env's dt = {env.dt}")
        self.lib = capi.declare_cmdtrack_api(load())
        self.device = torch.device(env.device)
        self.N = int(env.num_envs)
        self.ctx = C.c_void_p()
        st = self.cfg.to_struct()
        rc = self.lib.lg_cmdtrack_create(self._env_ctx(), C.byref(st), C.byref(self.ctx))
        if rc != 0:
            raise LeggedHipError(f"lg_cmdtrack_create failed ({rc}): {self.lib.lg_last_error().decode()}")
        self.rec, self.struct, self.t = None, None, {}
        self._views()

    def _env_ctx(self):
        ctx = getattr(self.env.core, "ctx", None)
        if not ctx:
            raise self._err("the tracker's env is closed")
        return ctx

    def _views(self):
        b = capi.lg_cmdtrack_buffers()
        self.lib.lg_cmdtrack_get_buffers(self.ctx, C.byref(b))
        n = self.N
        shapes = {"state": ((n, capi.CT_STATE), "f4"), "tg_state": ((n, capi.TG_STRIDE), "f4"), "plan": ((n, capi.PLAN_MAX_N, 2), "f4"),
                  "n_resample": ((n,), "i4"), "inject_overrun": ((n,), "i4")}
        if b.inject_K:
            shapes["inject"] = ((n, int(b.inject_K)), "f4")
        for name, (shape, dt) in shapes.items():
            ptr = C.cast(getattr(b, name), C.c_void_p).value
            if name not in self.t or self.t[name].data_ptr() != ptr or tuple(self.t[name].shape) != shape:
                self.t[name] = self._device_tensor(ptr, shape, dt, self, self.device)

    def _call(self, fn, *args):
        rc = getattr(self.lib, "lg_cmdtrack_" + fn)(self.ctx, *args)
        if rc != 0:
            raise self._err(f"lg_cmdtrack_{fn} failed ({rc}): {self.lib.lg_last_error().decode()}")

    def inject(self, enable, R=0):
        """Draws read from self.t['inject'] (N, 9 + 20 R) in lg_romsim_inject's block layout instead of Philox."""
        self._call("inject", int(bool(enable)), int(R))
        self._views()

    def inject_status(self):
        self._call("inject_status")

    def set_plans(self, v):
        """PLAN kind: v (N, n_nodes, 2), 0 <= n_nodes <= LG_PLAN_MAX_N; a stream-ordered copy."""
        import torch
        v = torch.as_tensor(v).to(self.device, torch.float32).contiguous()
        if v.dim() != 3 or v.shape[0] != self.N or v.shape[2] != 2:
            raise ValueError(f"v must be ({self.N}, n_nodes, 2), one plan per env; got {tuple(v.shape)}")
        self._plans = v
        self._call("set_plans", self._env_ctx(), C.c_void_p(v.data_ptr()) if v.shape[1] else None, int(v.shape[1]))

    def begin(self, T, epoch=0, want_u=False):
        """Allocate the records of an epoch of T steps and launch the begin: row 0, command 0 into the observation."""
        import torch
        T, n, dev = int(T), self.N, self.device
        if T < 1:
            raise ValueError(f"T = {T} must be at least 1")
        z = lambda *s: torch.zeros(*s, device=dev)
        rec = {"z": z(n, T + 1, 2), "v": z(n, T, 2), "pz_x": z(n, T + 1, 2), "done": torch.zeros(n, T, dtype=torch.uint8, device=dev)}
        if want_u:
            rec["u"] = z(n, T, 3)
        if self.cfg.x_n:
            rec["x"] = z(n, T + 1, int(self.cfg.x_n))
        r = capi.lg_cmdtrack_rec()
        r.T = T
        for k in ("z", "v", "pz_x", "done", "u", "x"):
            setattr(r, k, rec[k].data_ptr() if k in rec else None)
        self.rec, self.struct, self.T = rec, r, T
        self._call("begin", self._env_ctx(), C.byref(r), int(epoch))

    def step(self, t):
        """After env step t: its record, then command t + 1 into the observation.  t is a host integer; nothing is read back."""
        self._call("step", self._env_ctx(), C.byref(self.struct), int(t))

    def records(self):
        """The epoch's device tensors: z, v, pz_x, done (bool) [, u, x]."""
        import torch
        out = dict(self.rec)
        out["done"] = out["done"].view(torch.bool)
        return out

    def close(self):
        if getattr(self, "ctx", None):
            self.t = {}
            self.lib.lg_cmdtrack_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def collect(env, policy, tracker, epochs, T, first_epoch=0, want_u=False, to_host=True):
    """The reference's epoch loop (data_collection_velocity.py:85-156) with the tracker on the device: per epoch env.reset(),
    tracker.begin, then T times {policy, env.step, tracker.step}.  No host synchronisation inside an epoch; the records come to
    the host once at its end (to_host=False keeps them device tensors).  Returns the list of epoch dicts, in
    scripts/collect_trajectory_data.py::collect's layout: z, v, pz_x, done [, x with cfg.x_n, u with want_u]."""
    import torch
    out = []
    with torch.no_grad():
        for e in range(int(epochs)):
            env.reset()
            tracker.begin(T, epoch=first_epoch + e, want_u=want_u)
            obs = env.get_observations()
            for t in range(int(T)):
                obs = env.step(policy(obs.detach()).detach())[0]
                tracker.step(t)
            rec = tracker.records()
            out.append({k: v.cpu().numpy() for k, v in rec.items()} if to_host else rec)
    return out


def track_cmd(env, policy, z0, v, tracker=None, want=()):
    """tube/plan.py::track with the legged robot under a velocity policy as the tracker: the plans v (B, Np, 2) from z0 (B, 2),
    B == env.num_envs, one node per env step (the plan's dt is env.dt).  env.reset(); the ROM starts at each robot's root xy;
    Np env steps, each followed by one tracker launch.  Returns device tensors with track()'s keys -- pz_x (B, Np + 1, 2) in the
    plan's frame ((world - start) + z0, in float64 and rounded once), w_true (B, Np + 1) = |z - pz_x| in world coordinates -- and,
    as tube/plan_env.py::track_env marks them, z_ref, completed (B) bool, rows, dead: a robot that resets (falls or times out) is
    dead, not completed, and rows counts its rows up to the reset.  want: "x", "u" add the records, "rec" the raw dict.
    tracker: a PLAN-kind HipCommandTracker of this env to reuse, else one is made (Kp = I, yaw not tracked) and closed."""
    import torch
    bad = [k for k in want if k not in ("x", "u", "rec")]
    if bad:
        raise ValueError(f"want {bad}: of x, u, rec")
    v = torch.as_tensor(v).to(env.device, torch.float32).contiguous()
    z0 = torch.as_tensor(z0).to(env.device, torch.float32).contiguous()
    B = int(env.num_envs)
    if v.dim() != 3 or v.shape[0] != B or v.shape[1] < 1 or v.shape[2] != 2:
        raise ValueError(f"v must be ({B}, Np >= 1, 2), one plan per env; got {tuple(v.shape)}")
    Np = int(v.shape[1])
    if Np > capi.PLAN_MAX_N:
        raise ValueError(f"Np = {Np} exceeds LG_PLAN_MAX_N = {capi.PLAN_MAX_N}")
    if tuple(z0.shape) != (B, 2):
        raise ValueError(f"z0 must be {(B, 2)}; got {tuple(z0.shape)}")
    own = tracker is None
    if own:
        tracker = HipCommandTracker(env, CmdTrackCfg.from_env(env, kind=PLAN, want_x="x" in want))
    if tracker.cfg.kind != PLAN:
        raise ValueError("track_cmd needs a tracker of kind PLAN")
    if "x" in want and not tracker.cfg.x_n:
        raise ValueError("want x: the tracker was made without x_n (CmdTrackCfg.from_env(env, want_x=True))")
    try:
        with torch.no_grad():
            env.reset()
            tracker.set_plans(v)
            tracker.begin(Np, want_u="u" in want)
            obs = env.get_observations()
            for t in range(Np):
                obs = env.step(policy(obs.detach()).detach())[0]
                tracker.step(t)
            rec = tracker.records()
            out = align_cmd(rec["z"], rec["pz_x"], rec["done"], z0)
            for k in ("x", "u"):
                if k in want:
                    out[k] = rec[k]
            if "rec" in want:
                out["rec"] = rec
    finally:
        if own:
            tracker.close()
    return out


def align_cmd(rec_z, rec_pz, done, z0):
    """The tracker's records (z, pz_x (B, Np + 1, 2), done (B, Np) bool) as track()'s keys plus track_env's marks."""
    import torch
    Np = done.shape[1]
    origin = rec_z[:, :1].double()
    shift = lambda t: ((t.double() - origin) + z0.double()[:, None, :]).float()
    dead = done.any(dim=1)
    first = torch.where(dead, done.int().argmax(dim=1), torch.full_like(done[:, 0], Np, dtype=torch.int64))
    return {"pz_x": shift(rec_pz), "z_ref": shift(rec_z), "w_true": torch.linalg.vector_norm(rec_z - rec_pz, dim=-1).contiguous(),
            "completed": ~dead, "rows": (first + 1).to(torch.int32), "dead": dead}
