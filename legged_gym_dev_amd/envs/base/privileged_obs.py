"""Privileged observations for an asymmetric critic: the buffer the reference allocates, clips and
returns but never fills (legged_robot_config.py:38 ``num_privileged_obs``; base_task.py:62-79,104-105; legged_robot.py:100-104).

``cfg.privileged_obs.terms`` lists the terms of the row in order; ``cfg.privileged_obs.scales.<term>`` is the term's scale.
Every entry is ``clip(raw * scale, +-normalization.clip_observations)``; what ``raw`` is per term stands in
include/legged_hip.h (lg_priv_obs_*).  The row is written by ONE launch after the env step (csrc/privobs_kernels.hip) into a
buffer the library owns; ``HipPrivilegedObs.buf`` is a zero-copy view of it.  There is no fallback: without the library or a
GPU the handle raises.
"""
import ctypes as C
import dataclasses

from legged_gym_dev_amd import capi

# name -> width, from the env's dimensions; the order is capi.PRIV_TERMS (a term's LG_PRIV_* kind is its index there)
TERM_WIDTH = {
    "obs": lambda d: d["num_obs"],                         # the policy observation before noise
    "friction": lambda d: 1,                               # per-env friction coefficient
    "base_mass": lambda d: 1,                              # per-env added base mass
    "material": lambda d: 4,                               # restitution, compliance, thickness, inverse base mass
    "feet_contact_forces": lambda d: 3 * d["num_feet"],
    "feet_contact": lambda d: d["num_feet"],               # contact_forces[feet, 2] > 1
    "feet_air_time": lambda d: d["num_feet"],
    "body_contact": lambda d: d["num_pen"],                # |contact_forces[penalised body]| > 0.1
    "torques": lambda d: d["num_actions"],
    "heights": lambda d: d["num_height_points"],           # the height block of obs; needs measure_heights
    "episode_progress": lambda d: 1,                       # episode_length / max_episode_length
}
assert list(TERM_WIDTH) == capi.PRIV_TERMS


def dims_of(setup):
    """The dimensions lg_priv_obs_check takes, from an EnvSetup."""
    mh = bool(setup.measure_heights)
    return {"num_obs": int(setup.cfg.env.num_observations), "num_actions": int(setup.num_dof), "num_feet": len(setup.feet_indices),
            "num_pen": len(setup.penalised_contact_indices), "num_height_points": int(setup.num_height_points) if mh else 0,
            "measure_heights": int(mh)}


@dataclasses.dataclass
class PrivilegedObsSpec:
    """The terms of the row, their scales and the env dimensions that give their widths."""
    terms: tuple = ()
    scales: tuple = ()
    dims: dict = dataclasses.field(default_factory=dict)

    @classmethod
    def from_cfg(cls, cfg, setup):
        """cfg.privileged_obs read with defaults: a cfg class without the section (the reference's) gives a spec of no terms.
        Raises ValueError naming the field for an unknown or repeated term, ``heights`` without the height scan, more than
        LG_PRIV_MAX_TERMS terms or a row wider than LG_PRIV_MAX_WIDTH."""
        sec = getattr(cfg, "privileged_obs", None)
        terms = tuple(getattr(sec, "terms", None) or ())
        sc = getattr(sec, "scales", None)
        unknown = [t for t in terms if t not in TERM_WIDTH]
        if unknown:
            raise ValueError(f"cfg.privileged_obs.terms: no term named {unknown}; the terms are {capi.PRIV_TERMS}")
        spec = cls(terms, tuple(float(getattr(sc, t, 1.0)) for t in terms), dims_of(setup))
        why = refusal(spec.to_struct(), **spec.dims) if terms else None
        if why:
            raise ValueError(f"cfg.privileged_obs: {why}")
        return spec

    def widths(self):
        """term -> width, in the row's order."""
        return {t: int(TERM_WIDTH[t](self.dims)) for t in self.terms}

    @property
    def width(self):
        return sum(self.widths().values())

    def offsets(self):
        """term -> first column."""
        out, off = {}, 0
        for t, w in self.widths().items():
            out[t] = off
            off += w
        return out

    def to_struct(self):
        c = capi.lg_priv_cfg()
        c.num_terms = len(self.terms)
        for k, (t, s) in enumerate(zip(self.terms[:capi.PRIV_MAX_TERMS], self.scales)):
            c.terms[k].kind, c.terms[k].scale = capi.PRIV_TERMS.index(t), float(s)
        return c

    def resolve_num_privileged_obs(self, declared):
        """cfg.env.num_privileged_obs against the row: None becomes the row's width; a number must be that width."""
        W = self.width
        if declared is not None and int(declared) != W:
            raise ValueError(f"cfg.env.num_privileged_obs = {declared} but cfg.privileged_obs.terms give {W} columns: "
                             + ", ".join(f"{t} {w}" for t, w in self.widths().items()))
        return W


def refusal(c, num_obs, num_actions, num_feet, num_pen, num_height_points, measure_heights):
    """lg_priv_obs_check (host code of the library, needs no GPU): None, or its sentence without the "lg_priv_obs: " prefix."""
    from legged_gym_dev_amd.lib import load
    lib = capi.declare_priv_obs_api(load())
    if lib.lg_priv_obs_check(C.byref(c), num_obs, num_actions, num_feet, num_pen, num_height_points, int(bool(measure_heights)), None) == 0:
        return None
    return lib.lg_last_error().decode().split("lg_priv_obs: ", 1)[-1]


class HipPrivilegedObs:
    """lg_priv_obs on one env core (lib.HipEnvCore).  ``buf`` is the (num_envs, W) view, zeros until the first compute();
    compute() is one launch on the env's stream, to be called after the env step.  The handle keeps the core object and hands its
    context to every call; the library side holds no pointer into the env, so close() of either, in any order, leaves nothing
    dangling -- a compute() after the core was closed is refused here."""

    def __init__(self, core, spec):
        import torch
        from legged_gym_dev_amd.lib import LeggedHipError, device_tensor, load
        self._err = LeggedHipError
        self.core, self.spec = core, spec
        self.lib = capi.declare_priv_obs_api(load())
        self.ctx = C.c_void_p()
        st = spec.to_struct()
        rc = self.lib.lg_priv_obs_create(self._env_ctx(), C.byref(st), C.byref(self.ctx))
        if rc != 0:
            raise LeggedHipError(f"lg_priv_obs_create failed ({rc}): {self.lib.lg_last_error().decode()}")
        ptr, W = C.c_void_p(), C.c_int32()
        self.lib.lg_priv_obs_buffer(self.ctx, C.byref(ptr), C.byref(W))
        if int(W.value) != spec.width:
            raise LeggedHipError(f"lg_priv_obs_buffer: width {W.value} but the spec gives {spec.width}")
        self.width = int(W.value)
        self.buf = device_tensor(ptr.value, (int(core.setup.num_envs), self.width), "f4", self, torch.device(core.device))

    def _env_ctx(self):
        ctx = getattr(self.core, "ctx", None)
        if not ctx:
            raise self._err("the env of these privileged observations is closed")
        return ctx

    def compute(self):
        rc = self.lib.lg_priv_obs_compute(self.ctx, self._env_ctx())
        if rc != 0:
            raise self._err(f"lg_priv_obs_compute failed ({rc}): {self.lib.lg_last_error().decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.buf = None
            self.lib.lg_priv_obs_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
