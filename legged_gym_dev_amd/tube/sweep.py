"""HipTubeSweep: K tube models of one shape trained on one dataset by the same two launches per step (lg_tube_sweep_* in
include/legged_hip.h; k_tube_rows_sweep / k_tube_adam_sweep in tube_kernels.hip, the members along the grid's y axis).

It is ``TubeTraining`` (trainer.py) with K members, as ``HipTubeTrainer`` is with one: the library runs both through one
trainer.  Member k is, bit for bit, the ``HipTubeTrainer`` built from member k's configuration and given the same
calls: same initial parameters (``initial_params(..., seed_k)``), same epoch permutations and window starts, same reduction order.
The surface is the trainer's, indexed by member where a member is meant.  There is no CPU fallback.
"""
import ctypes as C

import torch

from .. import capi
from .trainer import LEVEL_LOSSES, LOSSES, TubeTraining, initial_params, make_cfg

MEMBER_FIELDS = ("alpha", "delta", "activation", "softplus_beta", "lr", "gamma", "step_size", "seed",
                 "level_lo", "level_hi")                                                 # what members may differ in
DEFAULTS = dict(num_units=32, num_layers=2, activation="relu", softplus_beta=1.0, loss="scalar", alpha=0.8, delta=1.0, lr=1e-3,
                gamma=0.1, step_size=10000, batch_size=2048, seed=42, horizon=None, level_lo=0.0, level_hi=1.0)   # HipTubeTrainer's


class _Member:
    """Member k's side of a sweep with the trainer's own method names: what a loop written for one trainer reads."""

    def __init__(self, sweep, k):
        self.sweep, self.k = sweep, k

    log_cap = property(lambda self: self.sweep.log_cap)

    def read_log(self, first, last):
        return self.sweep.read_log(self.k, first, last)

    def state_dict(self):
        return self.sweep.state_dict(self.k)


class HipTubeSweep(TubeTraining):
    PREFIX, NOUN = "lg_tube_sweep_", "sweep"

    def __init__(self, input_dim, output_dim, members, final_activation=None, device="cuda:0", **shared):
        """members: one dict per model with any of MEMBER_FIELDS.  shared: HipTubeTrainer's keywords; a member field given here
        is the value of every member that does not set it.  Any other trainer keyword inside a member (num_units, loss,
        batch_size, ...) is passed on to the library, which refuses members that differ in it.  The constructor loads every
        member's initial parameters, one transposed-copy launch per member."""
        if final_activation is not None:
            raise NotImplementedError("final_activation other than None is not supported (no reference configuration uses one)")
        members = [dict(m) for m in members]
        bad = sorted(set(shared) - set(DEFAULTS))
        if bad:
            raise TypeError(f"unknown keyword {bad[0]!r}")
        for k, m in enumerate(members):
            bad = sorted(set(m) - set(DEFAULTS))
            if bad:
                raise TypeError(f"member {k}: unknown field {bad[0]!r}")
        self.configs = [{**DEFAULTS, **shared, **m} for m in members]
        self._open(device)
        cfgs = (capi.lg_tube_cfg * max(1, len(self.configs)))()
        for k, c in enumerate(self.configs):        # the model envelope is the library's to refuse: it names the member
            if c["activation"] not in capi.TUBE_ACT:
                raise ValueError(f"member {k}: activation {c['activation']!r}: one of {tuple(capi.TUBE_ACT)}")
            if c["loss"] not in LOSSES:
                raise ValueError(f"member {k}: loss {c['loss']!r}: one of {tuple(LOSSES)}")
            if c["loss"] != "error" and c["loss"] not in LEVEL_LOSSES and c["alpha"] is None:
                raise ValueError(f"member {k}: loss {c['loss']!r} needs alpha")
            cfgs[k] = make_cfg(input_dim, output_dim, c)
        c0 = self.configs[0] if self.configs else DEFAULTS      # no member: the library refuses K = 0
        self.dims = (input_dim, output_dim, c0["num_units"], c0["num_layers"])
        self.loss, self.horizon, self.batch_size = c0["loss"], c0["horizon"], c0["batch_size"]
        self.level_input = c0["loss"] in LEVEL_LOSSES
        self.data_dim = input_dim - int(self.level_input)
        self._create(len(self.configs), cfgs, len(self.configs))
        for k, c in enumerate(self.configs):
            self.load_state_dict(k, initial_params(*self.dims, c["seed"]))

    def _expose(self, views):           # per member, under the trainer's attribute names: self.params[k], self.adam_m[k], ...
        for n, v in views.items():
            setattr(self, n, v)

    def member(self, k):
        return _Member(self, self._index(k))

    def _index(self, k):
        if not 0 <= int(k) < self.K:
            raise IndexError(f"member {k}: 0..{self.K - 1}")
        return int(k)

    # ---------------------------------------------------------------- model state
    def state_dict(self, k):
        """Member k's parameters under the reference MLP's keys; loads into HipTubeModel and deep_tube_learning.models.MLP."""
        return self._state_of(self.params[self._index(k)])

    def load_state_dict(self, k, sd):
        k = self._index(k)
        self._load_params(self.params[k], sd)
        self._call("params_changed", k)

    def read_log(self, k, first, last):
        """Member k's [loss, lr after the step, grad_norm, rows] of the steps first..last (1-based), as a host tensor."""
        return self._log_rows(self.log[self._index(k)], first, last)

    def evaluate(self):
        """Launches the eval of every member over the test split; returns a device tensor (K, 4), row k = member k's
        [loss, fraction fw > w, mean |w - fw| where fw > w, rows] (a copy, valid once the stream reaches it)."""
        self._call("eval")
        return torch.stack(self.eval_buf)

    def eval_level(self, level):
        """Level-conditioned sweeps: evaluate() with every test row of every member at `level`; (K, 4), column 1 the coverage."""
        if not self.level_input:
            raise ValueError("eval_level: the sweep is not level-conditioned (loss scalar_level / vector_level)")
        self._call("eval_level", C.c_float(float(level)))
        return torch.stack(self.eval_buf)

    def read_levels(self, k, count):
        """Host copy of the levels member k drew for the first `count` rows of the last step or evaluation."""
        if not self.level_input:
            raise ValueError("read_levels: the sweep is not level-conditioned (loss scalar_level / vector_level)")
        return self.levels[self._index(k)][:count].cpu()
