"""Plans against a tube: score a batch of ROM plans against a one-shot tube, track them on the ROM-on-ROM
model, and audit whether the tube held -- lg_plan_score / lg_plan_track in include/legged_hip.h, one launch each.

A plan is a start ``z0`` (2) and ``N`` inputs ``v`` (N, 2) of the SingleInt2D ROM.  The definitions are the reference planner's
(trajopt/tube_trajopt.py, "TT"): the one-shot tube query :561-568, the obstacle constraint inflated by the tube :59-97, the quadratic
objective :41-56,206-212, the analytic baseline tubes :489-540 and the problems ``gap``, ``right``, ``right_wide`` :11-21; the tracking
loop is deep_tube_learning/evaluation/evaluate_tube_simple_oneshot_on_mpc_traj.py:75-88.  No optimiser is part of this: the plans come
from any solver, or from ``warm_start`` and ``perturb``.  There is no CPU fallback: scoring and tracking need the library and a GPU.
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


def _eye(s):
    return [float(s), 0.0, 0.0, float(s)]


@dataclasses.dataclass
class PlanProblem:
    """lg_plan_problem, field for field, plus the start the warm starts leave from.  Q, Qf, R: 2 x 2 row-major (4 numbers);
    Qf None = Q (TT:200-201).  The defaults are the reference script's: N = 50, Q = R = 10 I, Qw = 0, w_max = 1."""
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
    if p.tube_kind != "nn":
        if level is not None:
            raise ValueError("level is given, but an analytic tube_kind has none")
        return
    if model is None:
        raise ValueError("tube_kind 'nn' needs a tube model (a handle)")
    dims = getattr(model, "dims", None)
    input_dim = dims[0] if dims else model.input_dim
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


class HipPlanScorer:
    """lg_plan_score on one problem.  model: a HipTubeModel / HipTubeTrainer of a one-shot horizon tube, or None for the analytic
    kinds.  calibration: a Calibration of kind 'horizon' (pick the set with `coverage`; a single set needs none) or
    'horizon_levels' (the set of `level`); its offsets are added per step ahead.  level: a level-conditioned model's level."""

    def __init__(self, model, problem, calibration=None, level=None, coverage=None, device=None):
        import torch
        from ..lib import LeggedHipError, load
        check_envelope(problem, model, level)
        self.problem, self.level = problem, level
        self.model = model if problem.tube_kind == "nn" else None
        self._err = LeggedHipError
        self.offset = None
        if calibration is not None:
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
        self.struct = problem.to_struct()
        if self.offset is not None:
            self.offset = self.offset.to(self.device, torch.float32).contiguous()
        self._handle = getattr(self.model, "_tr", self.model).h if self.model is not None else None

    def score(self, z0, v, e=None, v_prev=None, w0=None, want=("fw", "z", "w")):
        """z0 (B, 2), v (B, N, 2); e (B, H_rev), v_prev (B, H_rev, 2), w0 (B) or None = zeros.  Returns device tensors: cost (B),
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
        torch.cuda.set_device(dev)
        rc = self.lib.lg_plan_score(self._handle, C.byref(self.struct), _ptr(z0), _ptr(v), _ptr(e), _ptr(v_prev), _ptr(w0), _ptr(self.offset),
                                    int(self.level is not None), float(self.level if self.level is not None else 0.0), B,
                                    _ptr(out["cost"]), _ptr(out["min_clear"]), _ptr(out["worst_node"]), _ptr(out["n_viol"]),
                                    _ptr(out.get("fw")), _ptr(out.get("z")), _ptr(out.get("w")),
                                    C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        if rc != 0:
            raise self._err(f"lg_plan_score failed ({rc}): {self.lib.lg_last_error().decode()}")
        self._keep = (z0, v, e, v_prev, w0)
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


def audit(score, track, problem):
    """Did the tube hold?  score: HipPlanScorer.score's dict with 'w'; track: track()'s dict.  Plain Python numbers throughout, so
    that json.dumps(..., allow_nan=False) takes the result as it is.
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
    for c, r in zip(problem.obs_c, problem.obs_r):
        d = torch.linalg.vector_norm(pz - torch.tensor(c, dtype=torch.float64), dim=-1)
        act &= ~(d < float(r)).any(dim=1)
    share = lambda m: float(m.double().mean())
    return {"plans": int(B), "nodes": int(w.shape[1]),
            "coverage_by_node": [float(x) for x in cov.double().mean(dim=0)], "coverage": share(cov),
            "covered_plans": share(cov.all(dim=1)), "predicted_safe": share(pred), "actually_safe": share(act),
            "table": {"safe_safe": share(pred & act), "safe_unsafe": share(pred & ~act), "unsafe_safe": share(~pred & act),
                      "unsafe_unsafe": share(~pred & ~act)},
            "w_true_mean": float(wt.mean()), "w_true_max": float(wt.max())}
