"""Plans against a tube: score a batch of ROM plans against a one-shot tube, track them on the ROM-on-ROM
model, and audit whether the tube held -- lg_plan_score / lg_plan_track in include/legged_hip.h, one launch each.

A plan is a start ``z0`` (2) and ``N`` inputs ``v`` (N, 2) of the SingleInt2D ROM.  The definitions are the reference planner's
(trajopt/tube_trajopt.py, "TT"): the one-shot tube query :561-568, the obstacle constraint inflated by the tube :59-97, the quadratic
objective :41-56,206-212, the analytic baseline tubes :489-540 and the problems ``gap``, ``right``, ``right_wide`` :11-21; the tracking
loop is deep_tube_learning/evaluation/evaluate_tube_simple_oneshot_on_mpc_traj.py:75-88.  The plans come from any solver, from
``warm_start`` and ``perturb``, or from the planners below -- the sampling ``HipMppiPlanner`` (section 10.10), the first-order
``HipGradPlanner`` (section 10.11), or one after the other (``ChainedPlanner``) -- in ``closed_loop`` or alone, which stand in
for the reference's NLP solve.  tube_kind "nn_step" (section 10.13) scores and plans with a flat one-step tube instead, rolled node
by node along the plan inside the kernels (w[k+1] = fw(w[k], v[k], ..), trajopt/old/rom_tube_planning.py:106-107).
`Scenes` (section 10.14) gives every plan of a launch, or every MPPI instance, a goal and obstacles of its own; `random_scenes` draws them.
There is no CPU fallback: scoring, planning and tracking need the library and a GPU.
"""
import ctypes as C
import dataclasses
import json
from typing import List, Optional

import numpy as np

from .. import capi

# TT:11-21 problem_dict, number for number (tests/golden/plan_track.npz records the reference's own)
PROBLEMS = {
    "gap": {"start": [0.3, 0.3], "goal": [1.5, 1.5], "obs_c": [[1.0, 0.0], [0.75, 1.5]], "obs_r": [0.5, 0.5],
            "vel_max": 0.2, "pos_max": 10.0, "dt": 0.1},
    "right": {"start": [0.5, 0.0], "goal": [2.0, 0.0], "obs_c": [[1.0, 1.0], [0.625, -0.625]], "obs_r": [0.5, 0.5],
              "vel_max": 1.0, "pos_max": 10.0, "dt": 0.1},
    "right_wide": {"start": [0.5, 0.0], "goal": [2.0, 0.0], "obs_c": [[1.0, 1.0], [1.25, -1.25]], "obs_r": [0.5, 0.5],
                   "vel_max": 1.0, "pos_max": 10.0, "dt": 0.1},
}
TUBE_KINDS = tuple(capi.PLAN_TUBE)
ROLLING = ("l1_rolling", "l2_rolling")
MODEL_KINDS = ("nn", "nn_step")                     # the kinds that query a tube model; the others are analytic
NO_GRADIENT = ("tube_kind 'nn_step' has no gradient planner: reverse mode through N chained MLP passes is not built "
               "(plan with HipMppiPlanner)")


def _eye(s):
    return [float(s), 0.0, 0.0, float(s)]


@dataclasses.dataclass
class PlanProblem:
    """lg_plan_problem, field for field, plus the start the warm starts leave from.  Q, Qf, R: 2 x 2 row-major (4 numbers);
    Qf None = Q (TT:200-201).  recursive: the row layout of an nn_step model (train_tube.py --recursive).  The defaults are the reference script's: N = 50, Q = R = 10 I, Qw = 0, w_max = 1."""
    N: int = 50
    dt: float = 0.1
    start: List[float] = dataclasses.field(default_factory=lambda: [0.0, 0.0])
    goal: List[float] = dataclasses.field(default_factory=lambda: [0.0, 0.0])
    obs_c: List[List[float]] = dataclasses.field(default_factory=list)
    obs_r: List[float] = dataclasses.field(default_factory=list)
    H_rev: int = 0
    tube_kind: str = "nn"
    scaling: float = 0.5
    window_size: int = 10
    recursive: bool = False
    w_max: float = 1.0
    Qw: float = 0.0
    Q: List[float] = dataclasses.field(default_factory=lambda: _eye(10))
    Qf: Optional[List[float]] = None
    R: List[float] = dataclasses.field(default_factory=lambda: _eye(10))
    rom_z_min: List[float] = dataclasses.field(default_factory=lambda: [-1e9, -1e9])
    rom_z_max: List[float] = dataclasses.field(default_factory=lambda: [1e9, 1e9])
    rom_v_min: List[float] = dataclasses.field(default_factory=lambda: [-1e9, -1e9])
    rom_v_max: List[float] = dataclasses.field(default_factory=lambda: [1e9, 1e9])

    @classmethod
    def named(cls, name, **kw):
        """One of PROBLEMS with the ROM bounds the reference builds from vel_max / pos_max (...on_mpc_traj.py:48-50)."""
        if name not in PROBLEMS:
            raise KeyError(f"problem {name!r}: one of {tuple(PROBLEMS)}")
        p = PROBLEMS[name]
        base = dict(dt=p["dt"], start=list(p["start"]), goal=list(p["goal"]), obs_c=[list(c) for c in p["obs_c"]], obs_r=list(p["obs_r"]),
                    rom_z_min=[-p["pos_max"]] * 2, rom_z_max=[p["pos_max"]] * 2, rom_v_min=[-p["vel_max"]] * 2, rom_v_max=[p["vel_max"]] * 2)
        return cls(**{**base, **kw})

    @classmethod
    def from_json(cls, path):
        with open(path) as f:
            d = json.load(f)
        names = {f.name for f in dataclasses.fields(cls)}
        bad = sorted(set(d) - names)
        if bad:
            raise ValueError(f"{path}: unknown problem field(s) {bad}; the fields are {sorted(names)}")
        return cls(**d)

    def to_json(self):
        return dataclasses.asdict(self)

    @property
    def n_obs(self):
        return len(self.obs_r)

    def to_struct(self):
        """The lg_plan_problem; a tube_kind outside TUBE_KINDS becomes -1 (refused by the C side)."""
        q = capi.lg_plan_problem()
        q.N, q.H_rev, q.n_obs, q.window_size = int(self.N), int(self.H_rev), int(self.n_obs), int(self.window_size)
        q.tube_kind = capi.PLAN_TUBE.get(self.tube_kind, -1)
        q.recursive = int(bool(self.recursive))
        q.dt, q.scaling, q.w_max, q.Qw = float(self.dt), float(self.scaling), float(self.w_max), float(self.Qw)
        for i in range(min(self.n_obs, capi.PLAN_MAX_OBS)):
            q.obs_c[i][0], q.obs_c[i][1], q.obs_r[i] = float(self.obs_c[i][0]), float(self.obs_c[i][1]), float(self.obs_r[i])
        q.goal[:] = [float(x) for x in self.goal]
        q.Q[:], q.R[:] = [float(x) for x in self.Q], [float(x) for x in self.R]
        q.Qf[:] = [float(x) for x in (self.Q if self.Qf is None else self.Qf)]
        for name in ("rom_z_min", "rom_z_max", "rom_v_min", "rom_v_max"):
            getattr(q, name)[:] = [float(x) for x in getattr(self, name)]
        return q


def check_envelope(problem, model=None, level=None):
    """The supported envelope (lg_plan_check refuses the same); ValueError naming the field outside it.  model: None or an object
    with horizon (None or (H_fwd, H_rev)), input_dim and level_input -- a HipTubeModel or HipTubeTrainer."""
    p = problem
    if not 1 <= p.N <= capi.PLAN_MAX_N:
        raise ValueError(f"N={p.N}: 1..{capi.PLAN_MAX_N}")
    if len(p.obs_c) != len(p.obs_r):
        raise ValueError(f"obs_c holds {len(p.obs_c)} centres and obs_r {len(p.obs_r)} radii")
    if not 0 <= p.n_obs <= capi.PLAN_MAX_OBS:
        raise ValueError(f"n_obs={p.n_obs}: 0..{capi.PLAN_MAX_OBS}")
    if not p.dt > 0:
        raise ValueError(f"dt={p.dt}: must be positive")
    for i, r in enumerate(p.obs_r):
        if not r >= 0:
            raise ValueError(f"obs_r[{i}]={r}: a radius is not negative")
    if p.tube_kind not in TUBE_KINDS:
        raise ValueError(f"tube_kind={p.tube_kind!r}: one of {TUBE_KINDS}")
    if p.tube_kind in ROLLING and p.window_size < 1:
        raise ValueError(f"window_size={p.window_size}: at least 1 for a rolling tube_kind")
    for name in ("Q", "R") + (("Qf",) if p.Qf is not None else ()):
        if len(getattr(p, name)) != 4:
            raise ValueError(f"{name}: a 2 x 2 matrix as 4 numbers, row-major")
    if p.tube_kind not in MODEL_KINDS:
        if level is not None:
            raise ValueError("level is given, but an analytic tube_kind has none")
        return
    if model is None:
        raise ValueError(f"tube_kind {p.tube_kind!r} needs a tube model (a handle)")
    dims = getattr(model, "dims", None)
    input_dim = dims[0] if dims else model.input_dim
    if p.tube_kind == "nn_step":
        return _check_step(p, model, input_dim, dims[1] if dims else model.output_dim, level)
    if model.horizon is None:
        raise ValueError("the tube model is not a horizon model: a plan is scored by a one-shot tube (dataset scalar_horizon)")
    Hf, Hr = model.horizon
    if Hf != p.N:
        raise ValueError(f"the model's H_fwd={Hf} differs from N={p.N}")
    if Hr != p.H_rev:
        raise ValueError(f"the model's H_rev={Hr} differs from the problem's H_rev={p.H_rev}")
    want = Hr + 2 * (Hr + Hf) + int(bool(model.level_input))
    if input_dim != want:
        raise ValueError(f"nz must be 0: the model's input_dim={input_dim} is not H_rev + 2 (H_rev + H_fwd)"
                         f"{' + 1' if model.level_input else ''} = {want} (the ROM is SingleInt2D: no state columns past the position)")
    if level is not None and not model.level_input:
        raise ValueError("level is given, but the model is not level-conditioned")
    if level is None and model.level_input:
        raise ValueError("level is missing: the model is level-conditioned")


def step_taps(input_dim, level_input, recursive):
    """Taps T of a flat scalar tube model: with I' = input_dim minus the level column, I' = 1 + 2 T (not
    recursive) or 3 T (recursive).  ValueError naming input_dim and recursive where I' fits the form in no T >= 1."""
    Ip = int(input_dim) - int(bool(level_input))
    T = Ip // 3 if recursive else (Ip - 1) // 2
    if Ip < 3 or (Ip % 3 if recursive else (Ip - 1) % 2):
        raise ValueError(f"the model's input_dim={input_dim}{' (one of them the level)' if level_input else ''} with recursive={bool(recursive)} "
                         f"is not {'3 T' if recursive else '1 + 2 T'}{' + 1' if level_input else ''} for any T >= 1 (the ROM is SingleInt2D: "
                         "no state columns past the position)")
    return T


_STEP_ROWS, _STEP_LDS = 32, 144 * 1024               # LG_TUBE_ROWS, LG_TUBE_ROLLOUT_LDS (csrc/tube_device.h)


def step_tile_bytes(input_dim, units, H_rev, N):
    """Dynamic LDS of k_plan_score_step's tile without the weights (plan_kernels.hip plan_step_floats)."""
    return 4 * _STEP_ROWS * (((2 * (H_rev + N)) | 1) + ((H_rev + N + 1) | 1) + input_dim + 2 * units + (((N + 1) * 3) | 1))


def _check_step(p, model, input_dim, output_dim, level):
    """check_envelope for tube_kind 'nn_step' (lg_plan_check refuses the same)."""
    if model.horizon is not None:
        raise ValueError("the tube model is a horizon model: nn_step rolls a flat one-step tube along the plan (dataset scalar)")
    if output_dim != 1:
        raise ValueError(f"the model's output_dim={output_dim} must be 1: nn_step rolls a scalar tube")
    T = step_taps(input_dim, model.level_input, p.recursive)
    if not 0 <= p.H_rev <= capi.PLAN_STEP_MAX_HREV or p.H_rev < T - 1:
        raise ValueError(f"H_rev={p.H_rev}: 0..{capi.PLAN_STEP_MAX_HREV} and at least T - 1 = {T - 1} (the delayed taps of node 0 come from "
                         "e and v_prev)")
    units = getattr(model, "dims", (0, 0, getattr(model, "num_units", 0)))[2]
    if step_tile_bytes(input_dim, units, p.H_rev, p.N) > _STEP_LDS:
        raise ValueError(f"the tile of input_dim={input_dim}, {units} units, H_rev={p.H_rev} and N={p.N} does not fit the dynamic LDS ceiling")
    if level is not None and not model.level_input:
        raise ValueError("level is given, but the model is not level-conditioned")
    if level is None and model.level_input:
        raise ValueError("level is missing: the model is level-conditioned")


def step_offsets(calibration, N, coverage=None, level=None, trajectory=False):
    """The offsets (N) float32 an nn_step plan adds to fw[0..N-1].  fw[k] is k fed-back steps after the seed w0, so an
    AgeCalibration gives offset_at(age = k, coverage) (ages past max_age - 1 share the last group; trajectory adds the margin), and
    a Calibration of kind 'flat' or 'levels' its one_step offset at k = 0 and its rollout offset at k >= 1."""
    import torch
    from .calibrate import AgeCalibration
    if isinstance(calibration, AgeCalibration):
        if coverage is None and len(calibration.coverages) == 1:
            coverage = calibration.coverages[0]
        if coverage is None:
            raise ValueError(f"a per-age calibration needs the coverage: one of {calibration.coverages}")
        off = calibration.offset_at(torch.arange(N), coverage, trajectory=trajectory)
        if off.shape[-1] != 1:
            raise ValueError(f"the per-age calibration holds {off.shape[-1]} columns; nn_step rolls a scalar tube")
        return off[:, 0].float().contiguous()
    if trajectory:
        raise ValueError("the trajectory margin belongs to a per-age calibration (calibrate_tube.py --by_age --trajectory)")
    if calibration.kind not in ("flat", "levels"):
        raise ValueError(f"a {calibration.kind!r} calibration holds offsets per step ahead of a one-shot tube; nn_step takes kind 'flat' or "
                         "'levels' (calibrate_tube.py on a scalar / scalar_level run) or a per-age one (--by_age)")
    if calibration.kind == "flat" and coverage is None and len(calibration.coverages) == 1:
        coverage = calibration.coverages[0]
    kw = dict(level=level) if calibration.kind == "levels" else dict(coverage=coverage)
    one, roll = calibration.offset(part="one_step", **kw), calibration.offset(part="rollout", **kw)
    if one.numel() != 1:
        raise ValueError(f"the calibration holds {one.numel()} columns; nn_step rolls a scalar tube")
    return torch.cat([one.reshape(1), roll.reshape(1).repeat(N - 1)]).float().contiguous()


def warm_start(kind, start, goal, N, dt):
    """TT:415-432 get_warm_start for 'start', 'goal' and 'interpolate': (z (N+1, 2), v (N, 2)) as float64 arrays."""
    start, goal = np.asarray(start, np.float64), np.asarray(goal, np.float64)
    if kind == "start":
        return np.repeat(start[None, :], N + 1, 0), np.zeros((N, 2))
    if kind == "goal":
        return np.repeat(goal[None, :], N + 1, 0), np.zeros((N, 2))
    if kind == "interpolate":
        z = np.outer(np.linspace(0, 1, N + 1), goal - start) + start
        return z, np.diff(z, axis=0) / dt
    if kind == "nominal":
        raise NotImplementedError("warm start 'nominal' solves the nominal NLP with CasADi / IPOPT, which this project does not have "
                                  "(DESIGN.md section 7): bring that plan from your solver (--plans) or use 'interpolate'")
    raise ValueError(f"warm start {kind!r}: one of start, goal, interpolate (nominal needs the NLP solver)")


def perturb(v, sigma, K, seed, v_min, v_max):
    """K perturbations of the plan v (N, 2): v + sigma * standard normal, clipped to [v_min, v_max]; drawn from a torch generator
    on the host, so the same (v, sigma, K, seed) gives the same plans everywhere.  Returns a float32 tensor (K, N, 2)."""
    import torch
    v = torch.as_tensor(np.asarray(v), dtype=torch.float32)
    if v.dim() != 2 or v.shape[1] != 2:
        raise ValueError(f"v must be (N, 2); got {tuple(v.shape)}")
    if K < 1 or sigma < 0:
        raise ValueError(f"K={K} must be at least 1 and sigma={sigma} not negative")
    g = torch.Generator().manual_seed(int(seed))
    noise = torch.randn((int(K),) + tuple(v.shape), generator=g, dtype=torch.float32)
    lo, hi = torch.as_tensor(v_min, dtype=torch.float32), torch.as_tensor(v_max, dtype=torch.float32)
    return torch.maximum(torch.minimum(v[None] + float(sigma) * noise, hi), lo)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---------------------------------------------------------------- per-plan scenes
SCENES_ERR = "lg_plan_scenes: "                     # the prefix of lg_plan_scenes_check's refusals


class Scenes:
    """lg_plan_scenes: a goal and an obstacle list of its own for each of S plans (scoring, gradient) or S instances (MPPI); the
    rest of the problem stays the PlanProblem's.  Host arrays, validated here: goal (S, 2) or None = the problem's goal; obs_c
    (S, M <= 8, 2), obs_r (S, M) and n_obs (S) in 0..M -- scene s has the first n_obs[s] obstacles; n_obs None = M each -- or all
    three None = the problem's obstacles.  Radii are finite and not negative; centres and goals finite.
    obs_v (S, M, 2) or None: the obstacles' velocities in m/s, finite in the live slots; obs_c then holds
    the centres "now", at node 0 of a plan, and obstacle i is at c_i + u_i * (k * dt) at node k.  None = every obstacle stands still."""

    def __init__(self, goal=None, obs_c=None, obs_r=None, n_obs=None, obs_v=None):
        if obs_v is not None and obs_c is None:
            raise ValueError("obs_v is given without obs_c and obs_r: a velocity belongs to an obstacle of the scenes' own")
        if goal is None and obs_c is None and obs_r is None and n_obs is None:
            raise ValueError("goal, obs_c, obs_r and n_obs are all None: the scenes say nothing (pass scenes=None)")
        if (obs_c is None) != (obs_r is None):
            raise ValueError("obs_c and obs_r are given together or not at all")
        if n_obs is not None and obs_c is None:
            raise ValueError("n_obs is given without obs_c and obs_r")
        self.goal = None if goal is None else np.ascontiguousarray(goal, np.float32)
        self.obs_c = None if obs_c is None else np.ascontiguousarray(obs_c, np.float32)
        self.obs_r = None if obs_r is None else np.ascontiguousarray(obs_r, np.float32)
        if self.goal is not None and (self.goal.ndim != 2 or self.goal.shape[1] != 2 or self.goal.shape[0] < 1):
            raise ValueError(f"goal must be (S >= 1, 2); got {self.goal.shape}")
        self.n_obs = None
        if self.obs_c is not None:
            c, r = self.obs_c, self.obs_r
            if c.ndim != 3 or c.shape[2] != 2 or c.shape[0] < 1 or c.shape[1] > capi.PLAN_MAX_OBS:
                raise ValueError(f"obs_c must be (S >= 1, M <= {capi.PLAN_MAX_OBS}, 2); got {c.shape}")
            if r.shape != c.shape[:2]:
                raise ValueError(f"obs_r must be {c.shape[:2]}, one radius per centre; got {r.shape}")
            n = np.full(c.shape[0], c.shape[1], np.int64) if n_obs is None else np.asarray(n_obs)
            if n.shape != (c.shape[0],) or not np.issubdtype(n.dtype, np.integer):
                raise ValueError(f"n_obs must be ({c.shape[0]},) integers; got {n.shape} {n.dtype}")
            if n.min() < 0 or n.max() > c.shape[1]:
                raise ValueError(f"n_obs must lie in 0..{c.shape[1]} (the slots of obs_c); got {int(n.min())}..{int(n.max())}")
            self.n_obs = np.ascontiguousarray(n, np.int32)
            live = np.arange(c.shape[1])[None, :] < self.n_obs[:, None]
            if not np.isfinite(r[live]).all() or (r[live] < 0).any():
                raise ValueError("obs_r: a radius is finite and not negative")
            if not np.isfinite(c[live]).all():
                raise ValueError("obs_c: a centre is finite")
            if self.goal is not None and self.goal.shape[0] != c.shape[0]:
                raise ValueError(f"goal holds {self.goal.shape[0]} scenes and obs_c {c.shape[0]}")
        self.obs_v = None if obs_v is None else np.ascontiguousarray(obs_v, np.float32)
        if self.obs_v is not None:
            if self.obs_v.shape != self.obs_c.shape:
                raise ValueError(f"obs_v must be {self.obs_c.shape}, one velocity per centre; got {self.obs_v.shape}")
            if not np.isfinite(self.obs_v[live]).all():
                raise ValueError("obs_v: a velocity is finite")
        if self.goal is not None and not np.isfinite(self.goal).all():
            raise ValueError("goal: a goal is finite")
        self._dev = {}

    @property
    def S(self):
        return int((self.goal if self.goal is not None else self.obs_c).shape[0])

    def __len__(self):
        return self.S

    @classmethod
    def repeat(cls, problem, S):
        """S copies of the problem's own scene."""
        M = problem.n_obs
        return cls(goal=np.tile(np.asarray(problem.goal, np.float32), (int(S), 1)),
                   obs_c=np.tile(np.asarray(problem.obs_c, np.float32).reshape(1, M, 2), (int(S), 1, 1)),
                   obs_r=np.tile(np.asarray(problem.obs_r, np.float32).reshape(1, M), (int(S), 1)))

    def take(self, idx):
        """The scenes idx (an index array or slice) as Scenes of their own; repeats are allowed (there is no plan-to-scene map)."""
        g = lambda a: None if a is None else a[idx]
        return Scenes(g(self.goal), g(self.obs_c), g(self.obs_r), g(self.n_obs), g(self.obs_v))

    def _live(self):
        return np.arange(self.obs_c.shape[1])[None, :] < self.n_obs[:, None]

    @property
    def moving(self):
        """Whether the scenes carry velocities (the device struct then has `vel`, and the kernels read moving rows)."""
        return self.obs_v is not None

    def at(self, t):
        """The host scenes advanced to time t: every centre c + u * t in float32 with the device's roundings (u * t, then c + ..);
        the velocities stay.  Without velocities: the same scenes."""
        if self.obs_v is None:
            return self.take(slice(None))
        t = np.float32(t)
        return Scenes(self.goal, self.obs_c + self.obs_v * t, self.obs_r, self.n_obs, self.obs_v)

    def problem(self, s, base):
        """Scene s as a plain PlanProblem: `base` with the scene's goal and obstacles (float32 values, as the kernels read them).
        ValueError for a scene with a live velocity that is not zero: a PlanProblem cannot express one (take([s]) can)."""
        if self.obs_v is not None and (self.obs_v[s, :int(self.n_obs[s])] != 0).any():
            raise ValueError(f"scene {s} has a moving obstacle, which a PlanProblem cannot express: plan against scenes.take([{s}])")
        kw = {}
        if self.goal is not None:
            kw["goal"] = [float(x) for x in self.goal[s]]
        if self.obs_c is not None:
            n = int(self.n_obs[s])
            kw["obs_c"] = [[float(x) for x in c] for c in self.obs_c[s, :n]]
            kw["obs_r"] = [float(x) for x in self.obs_r[s, :n]]
        return dataclasses.replace(base, **kw)

    def goals(self, problem):
        """(S, 2) float64: every scene's goal (the problem's where the scenes carry none)."""
        if self.goal is None:
            return np.tile(np.asarray(problem.goal, np.float64), (self.S, 1))
        return self.goal.astype(np.float64)

    def obstacles(self, problem, t=None):
        """(c (S, M, 2), r (S, M), live (S, M) bool) float64: every scene's obstacles (the problem's where the scenes carry none).
        t: a time, or an array (T) of times, one per node; c is then (S, T, M, 2) for the array, the centres c + u * t in float64."""
        if self.obs_c is None:
            M = problem.n_obs
            c = np.tile(np.asarray(problem.obs_c, np.float64).reshape(1, M, 2), (self.S, 1, 1))
            r, live, u = np.tile(np.asarray(problem.obs_r, np.float64).reshape(1, M), (self.S, 1)), np.ones((self.S, M), bool), None
        else:
            c, r, live, u = self.obs_c.astype(np.float64), self.obs_r.astype(np.float64), self._live(), self.obs_v
        if t is None:
            return c, r, live
        t = np.asarray(t, np.float64)
        u = np.zeros_like(c) if u is None else np.where(live[..., None], u.astype(np.float64), 0.0)
        if t.ndim == 0:
            return c + u * t, r, live
        return c[:, None] + u[:, None] * t[None, :, None, None], r, live

    def packed(self):
        """obs (S, 8, 3) float32 [cx, cy, r], zeros past n_obs, as the library reads it; None without obstacles of their own."""
        if self.obs_c is None:
            return None
        M = self.obs_c.shape[1]
        live = (np.arange(M)[None, :] < self.n_obs[:, None])[..., None]
        obs = np.zeros((self.S, capi.PLAN_MAX_OBS, 3), np.float32)
        obs[:, :M] = np.where(live, np.concatenate([self.obs_c, self.obs_r[..., None]], axis=2), np.float32(0))
        return obs

    def packed_vel(self):
        """vel (S, 8, 2) float32 [ux, uy], zeros past n_obs, as the library reads it; None without velocities."""
        if self.obs_v is None:
            return None
        M = self.obs_v.shape[1]
        vel = np.zeros((self.S, capi.PLAN_MAX_OBS, 2), np.float32)
        vel[:, :M] = np.where(self._live()[..., None], self.obs_v, np.float32(0))
        return vel

    def to(self, device):
        """The device copy: (lg_plan_scenes, the tensors it points to), kept per device."""
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            up = lambda a: None if a is None else torch.as_tensor(a).to(device).contiguous()
            t = (up(self.goal), up(self.packed()), up(self.n_obs), up(self.packed_vel()))
            st = capi.lg_plan_scenes()
            st.S = self.S
            st.goal, st.obs, st.n_obs, st.vel = (None if x is None else x.data_ptr() for x in t)
            if self.obs_v is not None:                  # set_time's sources: the centres at t = 0
                t = t + (t[1][:, :, :2].clone(),)
            self._dev[key] = (st, t)
        return self._dev[key]

    def set_time(self, device, t):
        """Rewrite the centres of the cached device `obs` in place as c0 + u * t (float32: u * t, then c0 + ..): "now" becomes t.
        The pointers stay, nothing is allocated for the scenes and nothing is read back.  Nothing to do without velocities."""
        import torch
        if self.obs_v is None:
            return
        _, (_, obs, _, vel, c0) = self.to(device)
        torch.add(c0, vel * float(np.float32(t)), out=obs[:, :, :2])

    def save(self, path):
        np.savez(path, **{k: getattr(self, k) for k in ("goal", "obs_c", "obs_r", "n_obs", "obs_v") if getattr(self, k) is not None})

    @classmethod
    def load(cls, path):
        with np.load(path) as d:
            bad = sorted(set(d.files) - {"goal", "obs_c", "obs_r", "n_obs", "obs_v"})
            if bad:
                raise ValueError(f"{path}: unknown scene array(s) {bad}; the arrays are goal, obs_c, obs_r, n_obs, obs_v")
            return cls(**{k: d[k] for k in d.files})


def scenes_check(scenes, count):
    """lg_plan_scenes_check on the host arrays' S, in its words: ValueError where S differs from the call's count."""
    if scenes is not None and scenes.S != count:
        raise ValueError(f"{SCENES_ERR}S = {scenes.S} differs from the call's count of plans or instances = {count}")


# ---------------------------------------------------------------- a fleet's scenes
@dataclasses.dataclass
class FleetCfg:
    """lg_fleet_cfg, field for field: every other robot within sense_radius is a disc of radius `separation` (centre to centre)
    that moves with the input its plan in force applies next; the max_neighbours nearest are kept."""
    separation: float = 0.2
    sense_radius: float = 1.0
    max_neighbours: int = 8

    def check(self):
        """ValueError in lg_plan_fleet_scenes' words, the field named."""
        for name in ("separation", "sense_radius"):
            x = float(getattr(self, name))
            if not (np.isfinite(x) and x >= 0):
                raise ValueError(f"{name} must be finite and not negative")
        if not 0 <= int(self.max_neighbours) <= capi.PLAN_MAX_OBS:
            raise ValueError(f"max_neighbours = {self.max_neighbours} must lie in 0..{capi.PLAN_MAX_OBS}")

    def to_struct(self):
        c = capi.lg_fleet_cfg()
        c.separation, c.sense_radius, c.max_neighbours = float(self.separation), float(self.sense_radius), int(self.max_neighbours)
        return c


def fleet_scenes(cfg, pos, vel, t=0.0, static=None, out=None):
    """lg_plan_fleet_scenes: one launch from the robots' device positions and velocities (P, 2).  static: None or the device
    tensors (obs (P, 8, 3), vel (P, 8, 2) or None, n (P) int32).  out: (obs, vel, n_obs) to write into, or None = new tensors.
    Returns (obs (P, 8, 3), obs_vel (P, 8, 2), n_obs (P) int32)."""
    import torch
    from ..lib import LeggedHipError, load
    cfg.check()
    if pos.device.type != "cuda":
        raise LeggedHipError("a fleet's scenes are built on a GPU device (no CPU fallback); got " + str(pos.device))
    P, dev, M = pos.shape[0], pos.device, capi.PLAN_MAX_OBS
    pos, vel = pos.to(torch.float32).contiguous(), vel.to(dev, torch.float32).contiguous()
    if tuple(pos.shape) != (P, 2) or tuple(vel.shape) != (P, 2) or P < 1:
        raise ValueError(f"pos and vel must be (P >= 1, 2); got {tuple(pos.shape)} and {tuple(vel.shape)}")
    if out is None:
        out = (torch.empty(P, M, 3, device=dev), torch.empty(P, M, 2, device=dev), torch.empty(P, device=dev, dtype=torch.int32))
    s_obs, s_vel, s_n = (None, None, None) if static is None else static
    for name, x, shape in (("obs", out[0], (P, M, 3)), ("obs_vel", out[1], (P, M, 2)), ("n_obs", out[2], (P,)),
                           ("static obs", s_obs, (P, M, 3)), ("static vel", s_vel, (P, M, 2)), ("n_static", s_n, (P,))):
        if x is not None and (tuple(x.shape) != shape or not x.is_contiguous() or x.device != dev):
            raise ValueError(f"{name} must be a contiguous {shape} tensor on {dev}")
    lib = load()
    torch.cuda.set_device(dev)
    rc = lib.lg_plan_fleet_scenes(C.byref(cfg.to_struct()), _ptr(pos), _ptr(vel), P, _ptr(s_obs), _ptr(s_vel), _ptr(s_n), float(t),
                                  _ptr(out[0]), _ptr(out[1]), _ptr(out[2]), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise LeggedHipError(f"lg_plan_fleet_scenes failed ({rc}): {lib.lg_last_error().decode()}")
    return out


class FleetScenes(Scenes):
    """The scenes of a fleet of P robots, rebuilt on the device from the fleet's own state (lg_plan_fleet_scenes): robot p's scene is
    its static obstacles, then its nearest neighbours as moving discs.  goal (P, 2) or None: a goal per robot.  static: a Scenes of
    S = P with obstacles (and velocities, maybe) of its own, or None.  The device tensors are persistent: to(device) always returns
    the same struct and pointers, and update(pos, vel, t) rewrites obs, vel and n_obs in one launch.  The host arrays (obs_c, ..) are
    the static part, which is what the audits test actual safety against; the robots themselves are audit_closed_loop(fleet=)'s."""

    def __init__(self, P, cfg, goal=None, static=None):
        cfg.check()
        if static is not None and static.obs_c is None:
            raise ValueError("static: a Scenes with obstacles of its own (obs_c, obs_r, n_obs)")
        if static is not None and static.goal is not None:
            raise ValueError("static carries goals: a fleet's goals are FleetScenes' own argument")
        s, self.P = static, int(P)
        if goal is not None or s is not None:
            Scenes.__init__(self, goal, *((None,) * 4 if s is None else (s.obs_c, s.obs_r, s.n_obs, s.obs_v)))
            if Scenes.S.fget(self) != int(P):
                raise ValueError(f"the goals or the static scenes hold {Scenes.S.fget(self)} scenes; the fleet has P = {P} robots")
        else:
            self.goal = self.obs_c = self.obs_r = self.n_obs = self.obs_v = None
            self._dev = {}
        self.cfg = cfg
        if self.P < 1:
            raise ValueError(f"P = {P} must be at least 1")

    @property
    def S(self):
        return self.P

    @property
    def moving(self):
        return True

    def take(self, idx):
        raise ValueError("a fleet's scenes depend on the whole fleet: take() has no meaning (build a FleetScenes of the robots you want)")

    def obstacles(self, problem, t=None):
        if self.obs_c is None:                          # no static part: the device scenes hold neighbours alone, not the problem's
            T = () if t is None or np.ndim(t) == 0 else (len(t),)
            return np.zeros((self.P,) + T + (0, 2)), np.zeros((self.P, 0)), np.zeros((self.P, 0), bool)
        return Scenes.obstacles(self, problem, t)

    def to(self, device):
        import torch
        key = str(torch.device(device))
        if key not in self._dev:
            M = capi.PLAN_MAX_OBS
            up = lambda a: None if a is None else torch.as_tensor(a).to(device).contiguous()
            static = None if self.obs_c is None else (up(self.packed()), up(self.packed_vel()), up(self.n_obs))
            zeros = lambda *s, **kw: torch.zeros(*s, device=device, **kw)
            t = (up(self.goal), zeros(self.P, M, 3), zeros(self.P, dtype=torch.int32), zeros(self.P, M, 2), static)
            if static is not None:                      # before the first update: the static part at t = 0
                t[1].copy_(static[0]), t[2].copy_(static[2])
                if static[1] is not None:
                    t[3].copy_(static[1])
            st = capi.lg_plan_scenes()
            st.S = self.P
            st.goal, st.obs, st.n_obs, st.vel = (None if x is None else x.data_ptr() for x in t[:4])
            self._dev[key] = (st, t)
        return self._dev[key]

    def set_time(self, device, t):
        raise ValueError("a fleet's scenes take their time in update(pos, vel, t)")

    def update(self, pos, vel, t=0.0):
        """The one launch: the scenes of the fleet at positions pos (P, 2) moving with vel (P, 2) (device tensors) at time t, into
        the persistent tensors of pos's device.  Returns (obs, vel, n_obs), the tensors the struct points to."""
        _, (_, obs, n, v, static) = self.to(pos.device)
        if tuple(pos.shape) != (self.P, 2):
            raise ValueError(f"pos must be {(self.P, 2)}; got {tuple(pos.shape)}")
        fleet_scenes(self.cfg, pos, vel, t, static=static, out=(obs, v, n))
        return obs, v, n

    def save(self, path):
        raise ValueError("a fleet's scenes are rebuilt from the fleet's state and have no file form: save the static part")


RANDOM_SCENES_TRIES = 1000                          # rejections per scene before random_scenes gives up


def random_scenes(S, seed, start, n_obs=(1, 3), centre_box=((0.0, 0.0), (2.0, 2.0)), radius=(0.1, 0.4),
                  goal_box=((1.5, 1.5), (2.5, 2.5)), margin=0.05, speed=None):
    """S random scenes from numpy's default_rng(seed): per scene n in n_obs = (lo, hi) inclusive, a goal uniform in goal_box
    ((x_lo, y_lo), (x_hi, y_hi)), n centres uniform in centre_box and radii uniform in radius = (lo, hi).  A draw is rejected
    unless `start` -- (2,) or (S, 2) -- and the goal lie at least `margin` outside every obstacle, taken in float64 on the float32
    values kept; after RANDOM_SCENES_TRIES rejections of one scene a ValueError names it.  speed = (lo, hi): every obstacle moves
     in a uniform direction at a uniform speed in [lo, hi] m/s, drawn after its scene is accepted, so
    speed=None draws the scenes it drew before speeds existed."""
    if speed is not None and not 0 <= speed[0] <= speed[1]:
        raise ValueError(f"speed = {tuple(speed)}: 0 <= lo <= hi")
    lo, hi = int(n_obs[0]), int(n_obs[1])
    if S < 1 or not 0 <= lo <= hi <= capi.PLAN_MAX_OBS:
        raise ValueError(f"S = {S} must be at least 1 and n_obs = {tuple(n_obs)} lie in 0..{capi.PLAN_MAX_OBS}, lo <= hi")
    if not 0 <= radius[0] <= radius[1]:
        raise ValueError(f"radius = {tuple(radius)}: 0 <= lo <= hi")
    start = np.broadcast_to(np.asarray(start, np.float32).astype(np.float64), (S, 2))
    rng = np.random.default_rng(int(seed))
    cb, gb = np.asarray(centre_box, np.float64), np.asarray(goal_box, np.float64)
    goal, c, r, cnt = np.zeros((S, 2), np.float32), np.zeros((S, hi, 2), np.float32), np.zeros((S, hi), np.float32), np.zeros(S, np.int32)
    u = None if speed is None else np.zeros((S, hi, 2), np.float32)
    for s in range(S):
        for _ in range(RANDOM_SCENES_TRIES):
            n = int(rng.integers(lo, hi + 1))
            g = rng.uniform(gb[0], gb[1]).astype(np.float32)
            cs = rng.uniform(cb[0], cb[1], (n, 2)).astype(np.float32)
            rs = rng.uniform(radius[0], radius[1], n).astype(np.float32)
            far = lambda q: (np.linalg.norm(q[None, :] - cs.astype(np.float64), axis=1) >= rs.astype(np.float64) + margin).all()
            if far(start[s]) and far(g.astype(np.float64)):
                goal[s], c[s, :n], r[s, :n], cnt[s] = g, cs, rs, n
                if speed is not None:
                    ang, mag = rng.uniform(0.0, 2.0 * np.pi, n), rng.uniform(speed[0], speed[1], n)
                    u[s, :n] = (mag[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)).astype(np.float32)
                break
        else:
            raise ValueError(f"random_scenes: scene {s} was rejected {RANDOM_SCENES_TRIES} times: no draw keeps the start and the goal "
                             f"{margin} outside every obstacle (n_obs={tuple(n_obs)}, radius={tuple(radius)}, centre_box={cb.tolist()})")
    return Scenes(goal=goal, obs_c=c, obs_r=r, n_obs=cnt, obs_v=u)


def _scene_safe(pz, problem, scenes):
    """actually_safe per plan: no node of pz (B, T, 2) float64 inside an obstacle of the plan's own scene; with velocities the
    obstacle is taken where it is at the node's time, node j at j * dt."""
    import torch
    scenes_check(scenes, pz.shape[0])
    if getattr(scenes, "obs_v", None) is not None:
        c, r, live = (torch.as_tensor(a) for a in scenes.obstacles(problem, t=np.arange(pz.shape[1]) * float(problem.dt)))
        if c.shape[2] == 0:
            return torch.ones(pz.shape[0], dtype=torch.bool)
        d = torch.linalg.vector_norm(pz[:, :, None, :] - c, dim=-1)
        return ~((d < r[:, None, :]) & live[:, None, :]).any(dim=2).any(dim=1)
    c, r, live = (torch.as_tensor(a) for a in scenes.obstacles(problem))
    if c.shape[1] == 0:
        return torch.ones(pz.shape[0], dtype=torch.bool)
    d = torch.linalg.vector_norm(pz[:, :, None, :] - c[:, None, :, :], dim=-1)
    return ~((d < r[:, None, :]) & live[:, None, :]).any(dim=2).any(dim=1)


def refuse_old_library(lib):
    """LeggedHipError for a library that capi.declare_plan_api marked as built before lg_plan_call."""
    if getattr(lib, "plan_api_old", False):
        from ..lib import LeggedHipError
        raise LeggedHipError("the library (LG_HIP_LIB) still exports lg_plan_score_scenes: it was built before lg_plan_call, its planning "
                             "entries take the older argument lists, and calling them from this tree would corrupt memory (rebuild it)")


class HipPlanScorer:
    """lg_plan_score on one problem.  model: a HipTubeModel / HipTubeTrainer of a one-shot horizon tube ('nn'), of a flat scalar
    tube ('nn_step'), or None for the analytic kinds.  calibration: a Calibration of kind 'horizon' (pick
    the set with `coverage`; a single set needs none) or 'horizon_levels' (the set of `level`); its offsets are added per step
    ahead.  For 'nn_step': an AgeCalibration (`coverage`; `trajectory` adds its margin) or a Calibration of kind 'flat' / 'levels'
    (step_offsets).  level: a level-conditioned model's level."""

    def __init__(self, model, problem, calibration=None, level=None, coverage=None, device=None, trajectory=False):
        import torch
        from ..lib import LeggedHipError, load
        check_envelope(problem, model, level)
        self.problem, self.level = problem, level
        self.model = model if problem.tube_kind in MODEL_KINDS else None
        self._err = LeggedHipError
        self.offset = None
        if calibration is not None and problem.tube_kind == "nn_step":
            self.offset = step_offsets(calibration, problem.N, coverage=coverage, level=level, trajectory=trajectory)
        elif calibration is not None:
            if trajectory:
                raise ValueError("the trajectory margin belongs to a per-age calibration on tube_kind 'nn_step'")
            if not hasattr(calibration, "kind"):
                raise ValueError("a per-age calibration does not fit a one-shot tube: it belongs to tube_kind 'nn_step'")
            if calibration.kind not in ("horizon", "horizon_levels"):
                raise ValueError(f"a {calibration.kind!r} calibration does not fit a plan: offsets per step ahead come from kind "
                                 "'horizon' or 'horizon_levels' (calibrate_tube.py on a scalar_horizon / scalar_horizon_level run)")
            if calibration.kind == "horizon_levels":
                off = calibration.offset(level=level)
            else:
                if coverage is None and len(calibration.coverages) == 1:
                    coverage = calibration.coverages[0]
                off = calibration.offset(coverage=coverage)
            if off.numel() != problem.N:
                raise ValueError(f"the calibration holds {off.numel()} steps ahead; the problem has N={problem.N}")
            self.offset = off
        self.device = torch.device(device if device is not None else (model.device if self.model is not None else "cuda:0"))
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise LeggedHipError("scoring plans needs a GPU device (no CPU fallback); got " + str(self.device))
        self.lib = load()
        refuse_old_library(self.lib)
        self.struct = problem.to_struct()
        if self.offset is not None:
            self.offset = self.offset.to(self.device, torch.float32).contiguous()
        self._handle = getattr(self.model, "_tr", self.model).h if self.model is not None else None

    def call(self, count, z0, e=None, v_prev=None, w0=None, scenes=None):
        """The lg_plan_call, by reference, of a launch over `count` plans or instances on the device's current stream, from the
        state tensors (None = zeros), the scorer's offset and level, and `scenes` (a Scenes of S = count, or None).  The tensors it
        points at are kept until the next call."""
        import torch
        scenes_check(scenes, count)
        torch.cuda.set_device(self.device)
        c = capi.lg_plan_call()
        c.z0, c.e, c.v_prev, c.w0, c.offset = (None if t is None else t.data_ptr() for t in (z0, e, v_prev, w0, self.offset))
        if scenes is not None:
            c.scenes = C.pointer(scenes.to(self.device)[0])
        c.count, c.has_level, c.level = count, int(self.level is not None), float(self.level if self.level is not None else 0.0)
        c.stream = torch.cuda.current_stream(self.device).cuda_stream
        self._keep = (z0, e, v_prev, w0, scenes)
        return C.byref(c)

    def score(self, z0, v, e=None, v_prev=None, w0=None, want=("fw", "z", "w"), scenes=None):
        """z0 (B, 2), v (B, N, 2); e (B, H_rev), v_prev (B, H_rev, 2), w0 (B) or None = zeros.  scenes: a Scenes of S = B, plan b
        scored against its own goal and obstacles.  Returns device tensors: cost (B),
        min_clear (B), worst_node (B) int32, n_viol (B, 4) int32 [obstacle nodes, input steps, state nodes, tube nodes] and
        whatever of fw (B, N), z (B, N+1, 2), w (B, N+1) `want` names."""
        import torch
        p, dev = self.problem, self.device
        f32 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.float32).contiguous()
        z0, v, e, v_prev, w0 = f32(z0), f32(v), f32(e), f32(v_prev), f32(w0)
        if v.dim() != 3 or tuple(v.shape[1:]) != (p.N, 2) or v.shape[0] < 1:
            raise ValueError(f"v must be (B >= 1, {p.N}, 2); got {tuple(v.shape)}")
        B = v.shape[0]
        for name, t, shape in (("z0", z0, (B, 2)), ("e", e, (B, p.H_rev)), ("v_prev", v_prev, (B, p.H_rev, 2)), ("w0", w0, (B,))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {shape}; got {tuple(t.shape)}")
        bad = [k for k in want if k not in ("fw", "z", "w")]
        if bad:
            raise ValueError(f"want {bad}: of fw, z, w")
        out = {"cost": torch.empty(B, device=dev), "min_clear": torch.empty(B, device=dev),
               "worst_node": torch.empty(B, device=dev, dtype=torch.int32), "n_viol": torch.empty(B, 4, device=dev, dtype=torch.int32)}
        opt = {"fw": (B, p.N), "z": (B, p.N + 1, 2), "w": (B, p.N + 1)}
        for k in want:
            out[k] = torch.empty(opt[k], device=dev)
        rc = self.lib.lg_plan_score(
            self._handle, C.byref(self.struct), self.call(B, z0, e, v_prev, w0, scenes), _ptr(v),
            _ptr(out["cost"]), _ptr(out["min_clear"]), _ptr(out["worst_node"]), _ptr(out["n_viol"]),
            _ptr(out.get("fw")), _ptr(out.get("z")), _ptr(out.get("w")))
        if rc != 0:
            raise self._err(f"lg_plan_score failed ({rc}): {self.lib.lg_last_error().decode()}")
        self._keep += (v,)
        return out


def track(sim, z, v, x0=None, rom_dt=None, want=("x", "u")):
    """lg_plan_track: the plans z (B, N+1, 2), v (B, N, 2) tracked by `sim`'s DoubleInt2D model under its own Kp / Kd law, x0 (B, 4)
    or None = (z[0], 0, 0).  rom_dt defaults to the simulator's rom.dt; S = rom_dt / model.dt model steps per node (refused by the
    library unless whole, 1..8).  Returns device tensors pz_x (B, N+1, 2), w_true (B, N+1) and, as `want` names, x (B, N+1, 4),
    u (B, N S, 2).  The simulator's own state is not touched."""
    import torch
    dev = sim.device
    f32 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.float32).contiguous()
    z, v, x0 = f32(z), f32(v), f32(x0)
    if v.dim() != 3 or v.shape[2] != 2 or v.shape[0] < 1 or v.shape[1] < 1:
        raise ValueError(f"v must be (B >= 1, N >= 1, 2); got {tuple(v.shape)}")
    B, N = v.shape[:2]
    if tuple(z.shape) != (B, N + 1, 2):
        raise ValueError(f"z must be {(B, N + 1, 2)}; got {tuple(z.shape)}")
    if x0 is not None and tuple(x0.shape) != (B, 4):
        raise ValueError(f"x0 must be {(B, 4)}; got {tuple(x0.shape)}")
    rom_dt = float(sim.cfg.rom.dt if rom_dt is None else rom_dt)
    S = max(1, int(round(rom_dt / float(sim.cfg.env.model.dt))))
    out = {"pz_x": torch.empty(B, N + 1, 2, device=dev), "w_true": torch.empty(B, N + 1, device=dev)}
    if "x" in want:
        out["x"] = torch.empty(B, N + 1, 4, device=dev)
    if "u" in want:
        out["u"] = torch.empty(B, N * S, 2, device=dev)
    sim.use_current_stream()
    rc = sim.lib.lg_plan_track(sim.ctx, _ptr(z), _ptr(v), _ptr(x0), B, N, S, rom_dt, _ptr(out["pz_x"]), _ptr(out["w_true"]),
                               _ptr(out.get("x")), _ptr(out.get("u")))
    if rc != 0:
        raise sim._err(f"lg_plan_track failed ({rc}): {sim.lib.lg_last_error().decode()}")
    return out


def audit(score, track, problem, scenes=None):
    """Did the tube hold?  score: HipPlanScorer.score's dict with 'w'; track: track()'s dict.  Plain Python numbers throughout, so
    that json.dumps(..., allow_nan=False) takes the result as it is.  scenes: a Scenes of S = the plans (the one the plans were
    scored with); actually_safe is then taken against each plan's own obstacles.
    coverage_by_node[k]: share of plans with w[k] >= w_true[k]; coverage: its mean (the reference script's "Total Success Rate");
    covered_plans: share covered at every node; predicted_safe: min_clear >= 0; actually_safe: no node of the realised path inside
    an obstacle (|pz_x - c_i| < r_i); table: the shares of (predicted, actual) in {safe, unsafe}^2."""
    import torch
    w, wt = score["w"].detach().cpu().double(), track["w_true"].detach().cpu().double()
    pz = track["pz_x"].detach().cpu().double()
    if w.shape != wt.shape:
        raise ValueError(f"score w {tuple(w.shape)} and track w_true {tuple(wt.shape)} differ")
    B = w.shape[0]
    cov = w >= wt
    pred = score["min_clear"].detach().cpu().double() >= 0
    act = torch.ones(B, dtype=torch.bool)
    if scenes is not None:
        act = _scene_safe(pz, problem, scenes)
    else:
        for c, r in zip(problem.obs_c, problem.obs_r):
            d = torch.linalg.vector_norm(pz - torch.tensor(c, dtype=torch.float64), dim=-1)
            act &= ~(d < float(r)).any(dim=1)
    share = lambda m: float(m.double().mean())
    res = {"plans": int(B), "nodes": int(w.shape[1]),
           "coverage_by_node": [float(x) for x in cov.double().mean(dim=0)], "coverage": share(cov),
           "covered_plans": share(cov.all(dim=1)), "predicted_safe": share(pred), "actually_safe": share(act),
           "table": {"safe_safe": share(pred & act), "safe_unsafe": share(pred & ~act), "unsafe_safe": share(~pred & act),
                     "unsafe_unsafe": share(~pred & ~act)},
           "w_true_mean": float(wt.mean()), "w_true_max": float(wt.max())}
    if scenes is not None:                              # the audit per scene: plan b lives in scene b
        res["by_plan"] = {"covered": [bool(x) for x in cov.all(dim=1)], "predicted_safe": [bool(x) for x in pred],
                          "actually_safe": [bool(x) for x in act]}
    return res


# ---------------------------------------------------------------- the sampling planner
@dataclasses.dataclass
class MppiCfg:
    """lg_mppi_cfg, field for field: MPPI in place of the reference's NLP solve (trajopt/tube_trajopt.py:460 solve_tube).
    K candidates per instance and iteration, drawn as clip(mean + sigma_it * standard normal) with sigma_it = sigma * sigma_decay^it;
    weights exp(-(J - Jmin) / lambda) on J = cost + rho_g pen_g + rho_w pen_w + rho_z pen_z (the hinge sums of the obstacle, tube and
    state constraints).  instance_offset: instance p draws as instance id instance_offset + p."""
    K: int = 256
    iters: int = 20
    seed: int = 0
    instance_offset: int = 0
    sigma: float = 0.3
    sigma_decay: float = 1.0
    lambda_: float = 1.0
    rho_g: float = 1e4
    rho_w: float = 0.0
    rho_z: float = 0.0

    def check(self, P=1):
        """ValueError in lg_mppi_check's words, the field named."""
        if self.K < 32 or self.K > capi.MPPI_MAX_K or self.K % 32:
            raise ValueError(f"K = {self.K} must be a multiple of 32 in 32..{capi.MPPI_MAX_K}")
        if self.iters < 1:
            raise ValueError(f"iters = {self.iters} must be at least 1")
        if not self.sigma > 0:
            raise ValueError("sigma must be positive")
        if not 0 < self.sigma_decay <= 1:
            raise ValueError("sigma_decay must lie in (0, 1]")
        if not self.lambda_ > 0:
            raise ValueError("lambda must be positive")
        for name in ("rho_g", "rho_w", "rho_z"):
            if not getattr(self, name) >= 0:
                raise ValueError(f"{name} must not be negative")
        if P < 1:
            raise ValueError(f"P = {P} must be at least 1")
        if P * self.K > 2 ** 31 - 1:
            raise ValueError(f"P * K = {P * self.K} must not exceed 2^31 - 1")

    def to_struct(self, iters=None):
        c = capi.lg_mppi_cfg()
        c.K, c.iters, c.seed, c.instance_offset = int(self.K), int(self.iters if iters is None else iters), int(self.seed), int(self.instance_offset)
        c.sigma, c.sigma_decay, c.lambda_ = float(self.sigma), float(self.sigma_decay), float(self.lambda_)
        c.rho_g, c.rho_w, c.rho_z = float(self.rho_g), float(self.rho_w), float(self.rho_z)
        return c

    def sigma_it(self, it):
        """sigma * sigma_decay^it as the library takes it: `it` float32 products."""
        s, d = np.float32(self.sigma), np.float32(self.sigma_decay)
        for _ in range(int(it)):
            s = np.float32(s * d)
        return s


class HipMppiPlanner:
    """lg_plan_mppi on one problem for P instances at once, built on a HipPlanScorer: the handle, offset, level and envelope checks
    are the scorer's.  The arguments after cfg are HipPlanScorer's."""

    def __init__(self, model, problem, cfg, calibration=None, level=None, coverage=None, device=None, trajectory=False, scenes=None):
        cfg.check()
        self.scorer = HipPlanScorer(model, problem, calibration=calibration, level=level, coverage=coverage, device=device,
                                    trajectory=trajectory)
        self.problem, self.cfg, self.device, self.lib = problem, cfg, self.scorer.device, self.scorer.lib
        self._err = self.scorer._err
        self.scenes = scenes                            # a Scenes of S = the P of every call: instance p plans in scene p

    def _fail(self, name, rc):
        raise self._err(f"{name} failed ({rc}): {self.lib.lg_last_error().decode()}")

    def _call(self, st):
        """The scorer's lg_plan_call for a state() and the planner's scenes."""
        return self.scorer.call(st["P"], st["z0"], st["e"], st["v_prev"], st["w0"], self.scenes)

    def _stream(self):
        import torch
        torch.cuda.set_device(self.device)
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def state(self, z0, vbar, e=None, v_prev=None, w0=None, want=()):
        """The device arrays of a run: the instances' z0 (P, 2), e, v_prev, w0 (None = zeros), the mean plans vbar (P, N, 2) (copied),
        J (P, K), best_J, best_v, n_bad and whatever of cost, min_clear (P, K), pen (P, K, 3) `want` names."""
        import torch
        p, dev, K = self.problem, self.device, self.cfg.K
        f32 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.float32).contiguous()
        z0, e, v_prev, w0 = f32(z0), f32(e), f32(v_prev), f32(w0)
        vbar = torch.as_tensor(vbar).to(dev, torch.float32).clone().contiguous()
        if z0.dim() != 2 or z0.shape[1] != 2 or z0.shape[0] < 1:
            raise ValueError(f"z0 must be (P >= 1, 2); got {tuple(z0.shape)}")
        P = z0.shape[0]
        self.cfg.check(P)
        for name, t, shape in (("vbar", vbar, (P, p.N, 2)), ("e", e, (P, p.H_rev)), ("v_prev", v_prev, (P, p.H_rev, 2)), ("w0", w0, (P,))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {shape}; got {tuple(t.shape)}")
        bad = [k for k in want if k not in ("cost", "min_clear", "pen")]
        if bad:
            raise ValueError(f"want {bad}: of cost, min_clear, pen")
        st = {"P": P, "z0": z0, "e": e, "v_prev": v_prev, "w0": w0, "vbar": vbar, "J": torch.empty(P, K, device=dev),
              "best_J": torch.empty(P, device=dev), "best_v": torch.empty(P, p.N, 2, device=dev),
              "n_bad": torch.zeros(P, device=dev, dtype=torch.int32)}
        opt = {"cost": (P, K), "min_clear": (P, K), "pen": (P, K, 3)}
        for k in want:
            st[k] = torch.empty(opt[k], device=dev)
        return st

    def candidates(self, vbar, it=0):
        """lg_plan_mppi_candidates: the (P, K, N, 2) candidates of iteration `it` around vbar (P, N, 2) (tests and tools)."""
        import torch
        p = self.problem
        vbar = torch.as_tensor(vbar).to(self.device, torch.float32).contiguous()
        if vbar.dim() != 3 or tuple(vbar.shape[1:]) != (p.N, 2) or vbar.shape[0] < 1:
            raise ValueError(f"vbar must be (P >= 1, {p.N}, 2); got {tuple(vbar.shape)}")
        out = torch.empty(vbar.shape[0], self.cfg.K, p.N, 2, device=self.device)
        rc = self.lib.lg_plan_mppi_candidates(C.byref(self.scorer.struct), C.byref(self.cfg.to_struct()), int(it), _ptr(vbar), vbar.shape[0],
                                              _ptr(out), self._stream())
        if rc != 0:
            self._fail("lg_plan_mppi_candidates", rc)
        return out

    def step(self, st, it, what=3, reset=False, hist_row=None):
        """lg_plan_mppi_step on a state(): what & 1 the score (writes J and the optional outputs), what & 2 the update (reads J;
        writes vbar, best_J, best_v, n_bad and hist_row (P, 2) where given)."""
        sc = self.scorer
        rc = self.lib.lg_plan_mppi_step(
            sc._handle, C.byref(sc.struct), C.byref(self.cfg.to_struct()), self._call(st), int(it), int(what), int(bool(reset)),
            _ptr(st["vbar"]), _ptr(st["J"]), _ptr(st.get("cost")), _ptr(st.get("min_clear")), _ptr(st.get("pen")),
            _ptr(st["best_J"]), _ptr(st["best_v"]), _ptr(hist_row), _ptr(st["n_bad"]))
        if rc != 0:
            self._fail("lg_plan_mppi_step", rc)
        return st

    def warm_start(self, z0):
        """The `interpolate` warm start (TT:415-432) from every instance's z0 to the goal -- with scenes, to its own scene's goal --,
        clipped to the input bounds: (P, N, 2)."""
        p = self.problem
        z0 = np.asarray(z0, np.float64).reshape(-1, 2)
        goal = np.asarray(p.goal, np.float64)
        if getattr(self, "scenes", None) is not None and self.scenes.goal is not None:
            scenes_check(self.scenes, z0.shape[0])
            goal = self.scenes.goals(p)
        z = np.linspace(0, 1, p.N + 1)[None, :, None] * (goal - z0)[:, None, :] + z0[:, None, :]
        v = np.diff(z, axis=1) / p.dt                                    # warm_start's arithmetic, every instance at once
        return np.clip(v, np.asarray(p.rom_v_min, np.float64), np.asarray(p.rom_v_max, np.float64)).astype(np.float32)

    def plan(self, z0, v_init=None, e=None, v_prev=None, w0=None, iters=None):
        """lg_plan_mppi from z0 (P, 2): cfg.iters (or `iters`) iterations from the mean plans v_init (P, N, 2) or (N, 2); None = the
        clipped `interpolate` warm start.  Returns device tensors: v (P, N, 2) the final mean plan, best_v, best_J (P), hist
        (iters, P, 2) = (J of the mean plan, smallest J) per iteration, n_bad (P) int32, and score / best_score: both plans through
        HipPlanScorer.score (with z and w)."""
        import torch
        z0 = torch.as_tensor(z0, dtype=torch.float32).reshape(-1, 2)
        if v_init is None:
            v_init = self.warm_start(z0.cpu().numpy())
        v_init = torch.as_tensor(v_init, dtype=torch.float32)
        if v_init.dim() == 2:
            v_init = v_init[None].repeat(z0.shape[0], 1, 1)
        iters = self.cfg.iters if iters is None else int(iters)
        if iters < 1:
            raise ValueError(f"iters = {iters} must be at least 1")
        st = self.state(z0, v_init, e, v_prev, w0)
        hist = torch.empty(iters, st["P"], 2, device=self.device)
        sc = self.scorer
        rc = self.lib.lg_plan_mppi(
            sc._handle, C.byref(sc.struct), C.byref(self.cfg.to_struct(iters)), self._call(st), _ptr(st["vbar"]), _ptr(st["J"]),
            _ptr(st["best_J"]), _ptr(st["best_v"]), _ptr(hist), _ptr(st["n_bad"]))
        if rc != 0:
            self._fail("lg_plan_mppi", rc)
        want = ("z", "w")
        return {"v": st["vbar"], "best_v": st["best_v"], "best_J": st["best_J"], "hist": hist, "n_bad": st["n_bad"],
                "score": sc.score(st["z0"], st["vbar"], st["e"], st["v_prev"], st["w0"], want=want, scenes=self.scenes),
                "best_score": sc.score(st["z0"], st["best_v"], st["e"], st["v_prev"], st["w0"], want=want, scenes=self.scenes)}


# ---------------------------------------------------------------- the gradient planner
@dataclasses.dataclass
class GradCfg:
    """lg_grad_cfg, field for field: projected Adam on J = cost + rho_g pen_g + rho_w pen_w + rho_z pen_z (MppiCfg's objective),
    whose gradient k_plan_grad makes by a reverse sweep in the scoring tile.  iters stepping launches; the projection is the clip
    to rom_v_min / rom_v_max."""
    iters: int = 100
    lr: float = 0.05
    beta1: float = 0.9
    beta2: float = 0.999
    eps: float = 1e-8
    rho_g: float = 1e4
    rho_w: float = 0.0
    rho_z: float = 0.0

    def check(self, B=1):
        """ValueError in lg_plan_grad_check's words, the field named."""
        if self.iters < 1:
            raise ValueError(f"iters = {self.iters} must be at least 1")
        if not self.lr > 0:
            raise ValueError("lr must be positive")
        for name in ("beta1", "beta2"):
            if not 0 <= getattr(self, name) < 1:
                raise ValueError(f"{name} must lie in [0, 1)")
        if not self.eps > 0:
            raise ValueError("eps must be positive")
        for name in ("rho_g", "rho_w", "rho_z"):
            if not getattr(self, name) >= 0:
                raise ValueError(f"{name} must not be negative")
        if B < 1:
            raise ValueError(f"B = {B} must be at least 1")
        if B > 2 ** 31 - 1:
            raise ValueError(f"B = {B} must not exceed 2^31 - 1")

    def to_struct(self, iters=None):
        c = capi.lg_grad_cfg()
        c.iters = int(self.iters if iters is None else iters)
        c.lr, c.beta1, c.beta2, c.eps = float(self.lr), float(self.beta1), float(self.beta2), float(self.eps)
        c.rho_g, c.rho_w, c.rho_z = float(self.rho_g), float(self.rho_w), float(self.rho_z)
        return c


class HipGradPlanner:
    """lg_plan_grad / lg_plan_descend on one problem for P plans at once, built on a HipPlanScorer the way HipMppiPlanner is: the
    handle, offset, level and envelope checks are the scorer's.  The arguments after cfg are HipPlanScorer's."""

    warm_start = HipMppiPlanner.warm_start
    _fail = HipMppiPlanner._fail
    _call = HipMppiPlanner._call
    needs_gradient = True

    def __init__(self, model, problem, cfg, calibration=None, level=None, coverage=None, device=None, scenes=None):
        cfg.check()
        if problem.tube_kind == "nn_step":
            raise ValueError(NO_GRADIENT)
        self.scorer = HipPlanScorer(model, problem, calibration=calibration, level=level, coverage=coverage, device=device)
        self.problem, self.cfg, self.device, self.lib = problem, cfg, self.scorer.device, self.scorer.lib
        self._err = self.scorer._err
        self.scenes = scenes                            # a Scenes of S = the B of every call: plan b descends in scene b

    def state(self, z0, v, e=None, v_prev=None, w0=None, want=()):
        """The device arrays of a run: z0 (P, 2), e, v_prev, w0 (None = zeros), the plans v (P, N, 2) (copied), J (P), the Adam
        moments m, s, best_J, best_v, n_bad and whatever of grad (P, N, 2), cost, min_clear (P), pen (P, 3) `want` names."""
        import torch
        p, dev = self.problem, self.device
        f32 = lambda t: None if t is None else torch.as_tensor(t).to(dev, torch.float32).contiguous()
        z0, e, v_prev, w0 = f32(z0), f32(e), f32(v_prev), f32(w0)
        v = torch.as_tensor(v).to(dev, torch.float32).clone().contiguous()
        if z0.dim() != 2 or z0.shape[1] != 2 or z0.shape[0] < 1:
            raise ValueError(f"z0 must be (P >= 1, 2); got {tuple(z0.shape)}")
        P = z0.shape[0]
        self.cfg.check(P)
        for name, t, shape in (("v", v, (P, p.N, 2)), ("e", e, (P, p.H_rev)), ("v_prev", v_prev, (P, p.H_rev, 2)), ("w0", w0, (P,))):
            if t is not None and tuple(t.shape) != shape:
                raise ValueError(f"{name} must be {shape}; got {tuple(t.shape)}")
        opt = {"grad": (P, p.N, 2), "cost": (P,), "min_clear": (P,), "pen": (P, 3)}
        bad = [k for k in want if k not in opt]
        if bad:
            raise ValueError(f"want {bad}: of grad, cost, min_clear, pen")
        st = {"P": P, "z0": z0, "e": e, "v_prev": v_prev, "w0": w0, "v": v, "J": torch.empty(P, device=dev),
              "m": torch.empty(P, p.N, 2, device=dev), "s": torch.empty(P, p.N, 2, device=dev), "best_J": torch.empty(P, device=dev),
              "best_v": torch.empty(P, p.N, 2, device=dev), "n_bad": torch.zeros(P, device=dev, dtype=torch.int32)}
        for k in want:
            st[k] = torch.empty(opt[k], device=dev)
        return st

    def gradient(self, z0, v, e=None, v_prev=None, w0=None, want=("cost", "min_clear", "pen")):
        """lg_plan_grad: J (B) and grad (B, N, 2) = dJ/dv of the plans v from z0 (B, 2), and whatever of cost, min_clear, pen
        (B, 3) `want` names, as device tensors."""
        st = self.state(z0, v, e, v_prev, w0, want=("grad",) + tuple(k for k in want if k != "grad"))
        sc = self.scorer
        rc = self.lib.lg_plan_grad(
            sc._handle, C.byref(sc.struct), C.byref(self.cfg.to_struct()), self._call(st), _ptr(st["v"]),
            _ptr(st["J"]), _ptr(st["grad"]), _ptr(st.get("cost")), _ptr(st.get("min_clear")), _ptr(st.get("pen")))
        if rc != 0:
            self._fail("lg_plan_grad", rc)
        self._keep = st
        return {k: st[k] for k in ("J", "grad", "cost", "min_clear", "pen") if k in st}

    def step(self, st, it, what=3, reset=False, hist_row=None):
        """lg_plan_descend_step on a state(): what = 1 evaluates (J, the optional outputs, the elite, hist_row (P, 2)); what = 3
        also steps v, m and s in place."""
        sc = self.scorer
        rc = self.lib.lg_plan_descend_step(
            sc._handle, C.byref(sc.struct), C.byref(self.cfg.to_struct()), self._call(st), int(it), int(what), int(bool(reset)),
            _ptr(st["v"]), _ptr(st["J"]), _ptr(st.get("grad")),
            _ptr(st.get("cost")), _ptr(st.get("min_clear")), _ptr(st.get("pen")), _ptr(st["m"]), _ptr(st["s"]),
            _ptr(st["best_J"]), _ptr(st["best_v"]), _ptr(hist_row), _ptr(st["n_bad"]))
        if rc != 0:
            self._fail("lg_plan_descend_step", rc)
        return st

    def plan(self, z0, v_init=None, e=None, v_prev=None, w0=None, iters=None):
        """lg_plan_descend from z0 (P, 2): cfg.iters (or `iters`) steps from the plans v_init (P, N, 2) or (N, 2); None = the clipped
        `interpolate` warm start.  HipMppiPlanner.plan's keys: v (P, N, 2) the last iterate, best_v, best_J (P) the elite over every
        iterate, hist (iters + 1, P, 2) = (J, max |dJ/dv|) per evaluation, n_bad (P) int32, score / best_score."""
        import torch
        z0 = torch.as_tensor(z0, dtype=torch.float32).reshape(-1, 2)
        if v_init is None:
            v_init = self.warm_start(z0.cpu().numpy())
        v_init = torch.as_tensor(v_init, dtype=torch.float32)
        if v_init.dim() == 2:
            v_init = v_init[None].repeat(z0.shape[0], 1, 1)
        iters = self.cfg.iters if iters is None else int(iters)
        if iters < 1:
            raise ValueError(f"iters = {iters} must be at least 1")
        st = self.state(z0, v_init, e, v_prev, w0)
        hist = torch.empty(iters + 1, st["P"], 2, device=self.device)
        sc = self.scorer
        rc = self.lib.lg_plan_descend(
            sc._handle, C.byref(sc.struct), C.byref(self.cfg.to_struct(iters)), self._call(st),
            _ptr(st["v"]), _ptr(st["J"]), _ptr(st["m"]), _ptr(st["s"]), _ptr(st["best_J"]), _ptr(st["best_v"]),
            _ptr(hist), _ptr(st["n_bad"]))
        if rc != 0:
            self._fail("lg_plan_descend", rc)
        want = ("z", "w")
        return {"v": st["v"], "best_v": st["best_v"], "best_J": st["best_J"], "hist": hist, "n_bad": st["n_bad"],
                "score": sc.score(st["z0"], st["v"], st["e"], st["v_prev"], st["w0"], want=want, scenes=self.scenes),
                "best_score": sc.score(st["z0"], st["best_v"], st["e"], st["v_prev"], st["w0"], want=want, scenes=self.scenes)}


class ChainedPlanner:
    """Two planners on one problem, one after the other: `plan` runs `first` (say MPPI, which finds the homotopy class), then
    `second` (say the gradient planner, which polishes) from `first`'s best_v.  The result is `second`'s, with `first`'s under
    the key "first"; closed_loop takes it like either planner."""

    def __init__(self, first, second):
        if first.problem is not second.problem and first.problem != second.problem:
            raise ValueError("the two planners of a chain must share one problem")
        if getattr(first.problem, "tube_kind", None) == "nn_step" and any(getattr(pln, "needs_gradient", False) for pln in (first, second)):
            raise ValueError(NO_GRADIENT)
        if getattr(first, "scenes", None) is not getattr(second, "scenes", None):
            raise ValueError("the two planners of a chain must carry the same scenes")
        self.first, self.second = first, second
        self.problem, self.device, self.scenes = first.problem, first.device, getattr(first, "scenes", None)

    def plan(self, z0, v_init=None, e=None, v_prev=None, w0=None, iters=None):
        """`iters` goes to `first` (closed_loop's iters_first); `second` always runs its own."""
        a = self.first.plan(z0, v_init, e, v_prev, w0, iters=iters)
        b = dict(self.second.plan(z0, a["best_v"], e, v_prev, w0))
        b["first"] = a
        return b


def shift_plan(v):
    """The receding-horizon shift of mean plans (P, N, 2): one step on, the last row repeated."""
    import torch
    return torch.cat([v[:, 1:], v[:, -1:]], dim=1)


def shift_past(e, v_prev, err, v_k):
    """The tube item's past one step on (TPCL:160-163, as a true shift): e (P, H_rev) drops its oldest value and takes err (P),
    v_prev (P, H_rev, 2) takes v_k (P, 2).  With H_rev = 0 both stay empty."""
    import torch
    if e.shape[1] == 0:
        return e, v_prev
    return torch.cat([e[:, 1:], err[:, None]], dim=1), torch.cat([v_prev[:, 1:], v_k[:, None]], dim=1)


def closed_loop(planner, sim, H, start, x0=None, iters_first=None, keep_plans=False, track_fn=None, w0="zero", fleet=None):
    """trajopt/tube_planning_closed_loop.py:82-168 ("TPCL") for P robots at once: plan, apply the first action, replan, H times.
    start (P, 2); x0 (P, 4) the robots' states, None = (start, 0, 0).  The first plan runs iters_first iterations (None = cfg.iters)
    from the warm start, every later one cfg.iters from the previous mean plan shifted by one step.
    Step k: the action comes from track() on the first two nodes of the plan in force (the final mean plan) -- reference point
    z_sol[0], feed-forward v_sol[1] (TPCL:91-96), from the robot's state; x[:, 1] and its actions are kept.  Recorded: v_k = v_sol[0],
    z_{k+1} = z_sol[1], w_{k+1} = w_sol[1], pz_x_{k+1}; then e and v_prev shift by one and take |z_k - pz_x_k| and v_k, and the next
    plan starts from the ROM's z_{k+1} (TPCL:159).  No plan is made after the last step.
    w0: "zero" starts every plan's tube at 0 (w0 = None); "error" at |z_k - pz_x_k|, the tracking error at the replanning instant --
    the quantity the first column of a one-step tube model (tube_kind 'nn_step') was trained on.
    Moving scenes: where planner.scenes carries velocities, scenes.set_time(device, k * dt) comes before
    the plan of control step k, and the scenes are put back to time 0 at the end.  fleet: None = a FleetScenes as planner.scenes is
    updated before the plan of step k with update(pz_x_k, v_k, k * dt), v_k being the input each robot's plan in force applies next:
    zeros before the first plan, shift_plan(v_sol)[:, 0] afterwards; False = it is left as it stands.
    Returns device tensors z (P, H+1, 2), v (P, H, 2), w (P, H+1), pz_x (P, H+1, 2), x (P, H+1, 4), u (P, H S, 2), cost, min_clear,
    best_J (P, H) of the plan in force, n_bad (P, H) and, with keep_plans, plans_v (H, P, N, 2), plans_z (H, P, N+1, 2), plans_w and,
    for a fleet, fleet_obs (H, P, 8, 3), fleet_vel (H, P, 8, 2), fleet_n (H, P) and fleet_v (H, P, 2): the scenes each plan ran
    against and the velocities they were built from."""
    import torch
    p = planner.problem
    track_fn = track if track_fn is None else track_fn
    dev = planner.device
    start = torch.as_tensor(start, dtype=torch.float32).reshape(-1, 2).to(dev)
    P = start.shape[0]
    if H < 1:
        raise ValueError(f"H = {H} must be at least 1")
    if w0 not in ("zero", "error"):
        raise ValueError(f"w0 = {w0!r}: 'zero' or 'error'")
    xk = torch.cat([start, torch.zeros(P, 2, device=dev)], dim=1) if x0 is None else torch.as_tensor(x0, dtype=torch.float32).to(dev)
    if tuple(xk.shape) != (P, 4):
        raise ValueError(f"x0 must be {(P, 4)}; got {tuple(xk.shape)}")
    e, v_prev = torch.zeros(P, p.H_rev, device=dev), torch.zeros(P, p.H_rev, 2, device=dev)
    zk = start
    z, v, w, pz, x, u = [zk], [], [torch.zeros(P, device=dev)], [xk[:, :2]], [xk], []
    cost, clear, bestJ, nbad, plans = [], [], [], [], {"v": [], "z": [], "w": []}
    w_start = (lambda: None) if w0 == "zero" else (lambda: torch.linalg.vector_norm(z[-1] - pz[-1], dim=1))
    scenes = getattr(planner, "scenes", None)
    if fleet not in (None, False, True) and fleet is not scenes:
        raise ValueError("fleet: None, False, or the FleetScenes that is planner.scenes")
    is_fleet = isinstance(scenes, FleetScenes) and fleet is not False
    if fleet is not None and fleet is not False and not is_fleet:
        raise ValueError("fleet is asked for, but planner.scenes is no FleetScenes")
    timed = scenes is not None and not isinstance(scenes, FleetScenes) and scenes.obs_v is not None
    built = {"obs": [], "vel": [], "n": [], "v": []}

    def scene_step(k, v_next):                          # the scenes of control step k, before its plan
        if timed:
            scenes.set_time(dev, k * p.dt)
        if is_fleet:
            got = scenes.update(xk[:, :2].contiguous(), v_next, k * p.dt)
            if keep_plans:
                built["obs"].append(got[0].clone()), built["vel"].append(got[1].clone()), built["n"].append(got[2].clone())
                built["v"].append(v_next.clone())
    scene_step(0, torch.zeros(P, 2, device=dev))
    sol = planner.plan(zk, None, e, v_prev, w_start(), iters=iters_first)
    for k in range(H):
        v_sol, z_sol, w_sol = sol["v"], sol["score"]["z"], sol["score"]["w"]
        ff = v_sol[:, min(1, p.N - 1)][:, None]
        t = track_fn(sim, z_sol[:, :2], ff, xk, rom_dt=p.dt)
        xk = t["x"][:, 1]
        v_k = v_sol[:, 0]
        err = torch.linalg.vector_norm(z[-1] - pz[-1], dim=1)
        v.append(v_k), z.append(z_sol[:, 1]), w.append(w_sol[:, 1]), pz.append(xk[:, :2]), x.append(xk), u.append(t["u"])
        cost.append(sol["score"]["cost"]), clear.append(sol["score"]["min_clear"]), bestJ.append(sol["best_J"]), nbad.append(sol["n_bad"])
        if keep_plans:
            plans["v"].append(v_sol), plans["z"].append(z_sol), plans["w"].append(w_sol)
        e, v_prev = shift_past(e, v_prev, err, v_k)
        if k + 1 < H:
            scene_step(k + 1, shift_plan(v_sol)[:, 0])
            sol = planner.plan(z[-1], shift_plan(v_sol), e, v_prev, w_start())
    if timed:
        scenes.set_time(dev, 0.0)
    out = {"z": torch.stack(z, 1), "v": torch.stack(v, 1), "w": torch.stack(w, 1), "pz_x": torch.stack(pz, 1), "x": torch.stack(x, 1),
           "u": torch.cat(u, 1), "cost": torch.stack(cost, 1), "min_clear": torch.stack(clear, 1), "best_J": torch.stack(bestJ, 1),
           "n_bad": torch.stack(nbad, 1)}
    if keep_plans:
        out.update({"plans_" + k: torch.stack(t, 0) for k, t in plans.items()})
        if is_fleet:
            out.update({"fleet_" + k: torch.stack(t, 0) for k, t in built.items()})
    return out


FLEET_AUDIT_CHUNK = 256                             # robots per block of pairs in fleet_separation


def fleet_separation(pz):
    """(P) float64: every robot's smallest distance to another robot at the same step, over all steps of pz (P, T, 2) float64; inf
    for a fleet of one.  Chunked over pairs: FLEET_AUDIT_CHUNK x P x T distances at a time."""
    import torch
    P = pz.shape[0]
    out = torch.full((P,), float("inf"), dtype=torch.float64)
    for a in range(0, P, FLEET_AUDIT_CHUNK):
        d = torch.linalg.vector_norm(pz[a:a + FLEET_AUDIT_CHUNK, None] - pz[None], dim=-1)      # (chunk, P, T)
        d[torch.arange(d.shape[0]), torch.arange(a, a + d.shape[0])] = float("inf")
        d = torch.nan_to_num(d, nan=float("inf"), posinf=float("inf"))
        out[a:a + FLEET_AUDIT_CHUNK] = d.reshape(d.shape[0], -1).min(dim=1).values
    return out


def audit_closed_loop(result, problem, goal_tol=0.1, scenes=None, fleet=None):
    """Did the tube hold in closed loop?  With moving scenes actual safety is taken against each obstacle where it is at step k's
    time, k * dt.  fleet: a FleetCfg; adds min_separation (the smallest distance between two robots at one step of the realised
    pz_x, float64; None for one robot), collision_free (the share of robots never closer than `separation` to another at the same
    step) and by_robot["collision_free"].   scenes: a Scenes of S = the robots; actually_safe and reached_goal are then taken against
    each robot's own obstacles and goal.  Plain Python numbers (strict JSON).  coverage_by_step[k]: share of robots with
    w_k >= |z_k - pz_x_k|; coverage: its mean; covered_robots: share covered at every step; actually_safe: share whose realised path
    pz_x enters no obstacle; predicted_safe: share whose plans in force all had min_clear >= 0; reached_goal: share whose ROM path
    ends within goal_tol of the goal; goal_distance_mean: the mean of that distance."""
    import torch
    f64 = lambda t: t.detach().cpu().double()
    z, w, pz = f64(result["z"]), f64(result["w"]), f64(result["pz_x"])
    err = torch.linalg.vector_norm(z - pz, dim=-1)
    cov = w >= err
    act = torch.ones(z.shape[0], dtype=torch.bool)
    goal = torch.tensor(problem.goal, dtype=torch.float64)
    if scenes is not None:
        act, goal = _scene_safe(pz, problem, scenes), torch.as_tensor(scenes.goals(problem))
    else:
        for c, r in zip(problem.obs_c, problem.obs_r):
            act &= ~(torch.linalg.vector_norm(pz - torch.tensor(c, dtype=torch.float64), dim=-1) < float(r)).any(dim=1)
    pred = (f64(result["min_clear"]) >= 0).all(dim=1)
    dist = torch.linalg.vector_norm(z[:, -1] - goal, dim=-1)
    share = lambda m: float(m.double().mean())
    res = {"robots": int(z.shape[0]), "steps": int(z.shape[1] - 1), "coverage_by_step": [float(v) for v in cov.double().mean(dim=0)],
           "coverage": share(cov), "covered_robots": share(cov.all(dim=1)), "actually_safe": share(act), "predicted_safe": share(pred),
           "goal_tol": float(goal_tol), "reached_goal": share(dist <= goal_tol), "goal_distance_mean": float(dist.mean()),
           "error_mean": float(err.mean()), "error_max": float(err.max())}
    if scenes is not None:                              # the audit per scene: robot p lives in scene p
        res["by_robot"] = {"covered": [bool(x) for x in cov.all(dim=1)], "predicted_safe": [bool(x) for x in pred],
                           "actually_safe": [bool(x) for x in act], "reached_goal": [bool(x) for x in dist <= goal_tol],
                           "goal_distance": [float(x) for x in dist]}
    if fleet is not None:
        sep = fleet_separation(pz)
        free = sep >= float(fleet.separation)
        res["min_separation"] = float(sep.min()) if bool(torch.isfinite(sep.min())) else None
        res["collision_free"] = share(free)
        res.setdefault("by_robot", {})["collision_free"] = [bool(x) for x in free]
    return res
