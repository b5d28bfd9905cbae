"""Observation history for a feed-forward actor: the other half of an asymmetric actor-critic.

``cfg.obs_history.length`` = H frames including the current one (1: off), ``cfg.obs_history.columns`` = None (all of obs) or up
to 8 ascending half-open ranges [lo, hi) of obs columns that the past frames keep, ``cfg.obs_history.reset`` = "repeat" | "zero".
Env i after step t holds, newest first,

    [ obs_t (all num_obs columns) | sel(obs_t-1) | ... | sel(obs_t-H+1) ]            W = num_obs + (H - 1) S columns

where a frame is obs_buf as the actor saw it.  A reset (the step's dones, or a reset_idx made outside step()) reinitialises the
env: every past frame becomes sel(obs_t) ("repeat") or zeros ("zero").  The row is advanced by ONE launch after the env step
(csrc/obshist_kernels.hip) in a buffer the library owns; ``HipObsHistory.buf`` is a zero-copy view of it.  There is no fallback:
without the library or a GPU the handle raises.
"""
import ctypes as C
import dataclasses

from legged_gym_dev_amd import capi


@dataclasses.dataclass(frozen=True)
class ObsHistorySpec:
    """length, the ranges of the columns past frames keep (() = all), the reset rule and the env's num_obs."""
    length: int = 1
    ranges: tuple = ()
    reset: str = "repeat"
    num_obs: int = 0

    @classmethod
    def from_cfg(cls, cfg, setup):
        """cfg.obs_history read with defaults: a cfg class without the section (the reference's) or a length of 1 gives "off".
        Raises ValueError with lg_obs_hist_check's sentence, which names the field, before any device work."""
        sec = getattr(cfg, "obs_history", None)
        length = getattr(sec, "length", 1)
        length = 1 if length is None else int(length)
        num_obs = int(setup.cfg.env.num_observations)
        if length == 1:
            return cls(1, (), "repeat", num_obs)
        cols = getattr(sec, "columns", None)
        try:
            ranges = tuple((int(lo), int(hi)) for lo, hi in (cols or ()))
        except (TypeError, ValueError):
            raise ValueError(f"cfg.obs_history.columns = {cols!r}: None or a list of [lo, hi) pairs of obs columns")
        reset = getattr(sec, "reset", "repeat")
        if reset not in capi.OBS_HIST_RESET:
            raise ValueError(f"cfg.obs_history.reset = {reset!r}: one of {capi.OBS_HIST_RESET}")
        spec = cls(length, ranges, reset, num_obs)
        why = refusal(spec.to_struct(), num_obs)
        if why:
            raise ValueError(f"cfg.obs_history: {why}")
        return spec

    @classmethod
    def from_dict(cls, d):
        """The checkpoint's entry (as_dict) back into a spec; None (a checkpoint without the key) means no history."""
        if not d:
            return cls()
        return cls(int(d["length"]), tuple((int(lo), int(hi)) for lo, hi in d["ranges"]), str(d["reset"]), int(d["num_obs"]))

    def as_dict(self):
        return {"length": self.length, "ranges": [list(r) for r in self.ranges], "reset": self.reset, "num_obs": self.num_obs}

    @property
    def enabled(self):
        return self.length > 1

    def same_row(self, other):
        """Whether two specs give the same row: two that are off always do."""
        if not self.enabled or not other.enabled:
            return self.enabled == other.enabled
        return self.as_dict() == other.as_dict()

    def columns(self):
        """The selected obs columns, in the order a past frame holds them."""
        if not self.ranges:
            return list(range(self.num_obs))
        return [c for lo, hi in self.ranges for c in range(lo, hi)]

    @property
    def num_selected(self):
        return len(self.columns())

    @property
    def width(self):
        return self.num_obs + (self.length - 1) * self.num_selected

    def frame_offsets(self):
        """First column of every frame, newest first: [0, num_obs, num_obs + S, ...] (length entries)."""
        return [0] + [self.num_obs + k * self.num_selected for k in range(self.length - 1)]

    def to_struct(self):
        c = capi.lg_obs_hist_cfg()
        c.length, c.num_ranges, c.reset_mode = self.length, len(self.ranges), capi.OBS_HIST_RESET.index(self.reset)
        for k, (lo, hi) in enumerate(self.ranges[:capi.OBS_HIST_MAX_RANGES]):
            c.lo[k], c.hi[k] = lo, hi
        return c

    def __str__(self):
        if not self.enabled:
            return "no history"
        cols = ",".join(f"{lo}:{hi}" for lo, hi in self.ranges) or "all"
        return f"length {self.length}, columns {cols}, reset {self.reset}, num_obs {self.num_obs}"


def parse_columns(text):
    """"lo:hi[,lo:hi...]" of the command line -> [[lo, hi], ...]."""
    out = []
    for part in str(text).split(","):
        lo, sep, hi = part.strip().partition(":")
        if not sep:
            raise ValueError(f"--obs_history_columns {text!r}: expected lo:hi[,lo:hi...]")
        out.append([int(lo), int(hi)])
    return out


def refusal(c, num_obs):
    """lg_obs_hist_check (host code of the library, needs no GPU): None, or its sentence without the "lg_obs_hist: " prefix."""
    from legged_gym_dev_amd.lib import load
    lib = capi.declare_obs_hist_api(load())
    if lib.lg_obs_hist_check(C.byref(c), int(num_obs), None) == 0:
        return None
    return lib.lg_last_error().decode().split("lg_obs_hist: ", 1)[-1]


def refuse_history(env, who):
    """For the consumers that hand ``obs`` to a policy themselves or write into it after the env step."""
    spec = getattr(env, "obs_history_spec", None)
    if spec is not None and spec.enabled:
        raise ValueError(f"{who} does not take an env with cfg.obs_history ({spec}): it reads or writes obs itself, behind the "
                         "history's launch")


class HipObsHistory:
    """lg_obs_hist on one env core (lib.HipEnvCore).  ``buf`` is the (num_envs, W) view, zeros until the first compute();
    compute() is one launch on the env's stream, to be called after the env step; mark(ids) asks the next compute() to
    reinitialise those envs (None: all).  The handle keeps the core object and hands its context to every call; the library side
    holds no pointer into the env, so close() of either, in any order, leaves nothing dangling -- a compute() after the core was
    closed is refused here."""

    def __init__(self, core, spec):
        import torch
        from legged_gym_dev_amd.lib import LeggedHipError, device_tensor, load
        self._err = LeggedHipError
        self.core, self.spec = core, spec
        self.lib = capi.declare_obs_hist_api(load())
        self.ctx = C.c_void_p()
        st = spec.to_struct()
        rc = self.lib.lg_obs_hist_create(self._env_ctx(), C.byref(st), C.byref(self.ctx))
        if rc != 0:
            raise LeggedHipError(f"lg_obs_hist_create failed ({rc}): {self.lib.lg_last_error().decode()}")
        ptr, W = C.c_void_p(), C.c_int32()
        self.lib.lg_obs_hist_buffer(self.ctx, C.byref(ptr), C.byref(W))
        if int(W.value) != spec.width:
            raise LeggedHipError(f"lg_obs_hist_buffer: width {W.value} but the spec gives {spec.width}")
        self.width = int(W.value)
        self._device = torch.device(core.device)
        self.buf = device_tensor(ptr.value, (int(core.setup.num_envs), self.width), "f4", self, self._device)
        self._ids = None

    def _env_ctx(self):
        ctx = getattr(self.core, "ctx", None)
        if not ctx:
            raise self._err("the env of this observation history is closed")
        return ctx

    def compute(self):
        rc = self.lib.lg_obs_hist_compute(self.ctx, self._env_ctx())
        if rc != 0:
            raise self._err(f"lg_obs_hist_compute failed ({rc}): {self.lib.lg_last_error().decode()}")

    def mark(self, ids=None):
        import torch
        if ids is None:
            ptr, n = None, 0
        else:
            self._ids = torch.as_tensor(ids, device=self._device).reshape(-1).to(torch.int32).contiguous()   # alive until the next call
            ptr, n = C.c_void_p(self._ids.data_ptr()), int(self._ids.numel())
            if n == 0:
                return
        rc = self.lib.lg_obs_hist_mark(self.ctx, self._env_ctx(), ptr, n)
        if rc != 0:
            raise self._err(f"lg_obs_hist_mark failed ({rc}): {self.lib.lg_last_error().decode()}")

    def close(self):
        if getattr(self, "ctx", None):
            self.buf = None
            self.lib.lg_obs_hist_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
