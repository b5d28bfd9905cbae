"""HipTubeSweep: K tube models of one shape trained on one dataset by the same two launches per step (lg_tube_sweep_* in
include/legged_hip.h; k_tube_rows_sweep / k_tube_adam_sweep in tube_kernels.hip, the members along the grid's y axis).

Member k is, bit for bit, the ``HipTubeTrainer`` built from member k's configuration and given the same calls: same initial
parameters (``initial_params(..., seed_k)``), same epoch permutations and window starts, same reduction order.  The surface is the
trainer's, indexed by member where a member is meant.  There is no CPU fallback.
"""
import ctypes as C
from collections import OrderedDict

import torch

from .. import capi
from ..lib import LeggedHipError, device_tensor, load
from .trainer import LEVEL_LOSSES, LOSSES, _numel, check_window_dims, initial_params, param_shapes

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


class HipTubeSweep:
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
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise LeggedHipError("the tube sweep needs a GPU device (no CPU fallback); got " + str(device))
        self.lib = load()
        self.h = None
        self.K = len(self.configs)
        cfgs = (capi.lg_tube_cfg * max(1, self.K))()
        for k, c in enumerate(self.configs):        # the model envelope is the library's to refuse: it names the member
            if c["activation"] not in capi.TUBE_ACT:
                raise ValueError(f"member {k}: activation {c['activation']!r}: one of {tuple(capi.TUBE_ACT)}")
            if c["loss"] not in LOSSES:
                raise ValueError(f"member {k}: loss {c['loss']!r}: one of {tuple(LOSSES)}")
            if c["loss"] != "error" and c["loss"] not in LEVEL_LOSSES and c["alpha"] is None:
                raise ValueError(f"member {k}: loss {c['loss']!r} needs alpha")
            hz, lv = c["horizon"], c["loss"] in LEVEL_LOSSES
            cfgs[k] = capi.lg_tube_cfg(input_dim=input_dim, output_dim=output_dim, num_units=c["num_units"], num_layers=c["num_layers"],
                                       activation=capi.TUBE_ACT[c["activation"]], loss=capi.TUBE_LOSS[LOSSES[c["loss"]]],
                                       horizon=int(hz is not None), batch_size=c["batch_size"], H_fwd=hz[0] if hz else 0,
                                       H_rev=hz[1] if hz else 0, step_size=c["step_size"], seed=c["seed"],
                                       alpha=c["alpha"] if c["alpha"] is not None else 0.0, delta=c["delta"],
                                       softplus_beta=c["softplus_beta"], lr=c["lr"], gamma=c["gamma"], level_input=int(lv),
                                       level_lo=c["level_lo"] if lv else 0.0, level_hi=c["level_hi"] if lv else 0.0)
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        self._call("create", cfgs, self.K, C.byref(h), obj=False)
        self.h = h
        c0 = self.configs[0]
        self.dims = (input_dim, output_dim, c0["num_units"], c0["num_layers"])
        self.loss, self.horizon, self.batch_size = c0["loss"], c0["horizon"], c0["batch_size"]
        self.level_input = c0["loss"] in LEVEL_LOSSES
        self.data_dim = input_dim - int(self.level_input)
        self.use_current_stream()
        self._views()
        for k, c in enumerate(self.configs):
            self.load_state_dict(k, initial_params(*self.dims, c["seed"]))
        self._data = {}

    # ---------------------------------------------------------------- plumbing
    def _call(self, fn, *args, obj=True):
        rc = getattr(self.lib, "lg_tube_sweep_" + fn)(*((self.h,) if obj else ()), *args)
        if rc != 0:
            raise LeggedHipError(f"lg_tube_sweep_{fn} failed ({rc}): {self.lib.lg_last_error().decode()}")

    def use_current_stream(self):
        self._call("set_stream", C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def _views(self):
        """Per member, torch views of its buffers under the trainer's attribute names: self.params[k], self.adam_m[k], ..."""
        ptr = lambda p: C.cast(p, C.c_void_p).value
        names = ("params", "grads", "adam_m", "adam_v", "log", "eval_buf", "starts", "perm", "levels")
        for n in names:
            setattr(self, n, [])
        for k in range(self.K):
            b = capi.lg_tube_buffers()
            self._call("get_buffers", k, C.byref(b))
            P = int(b.num_params)
            self.num_params, self.log_cap, self.step_count = P, int(b.log_cap), int(b.step)
            for n in ("params", "grads", "adam_m", "adam_v"):
                getattr(self, n).append(device_tensor(ptr(getattr(b, n)), (P,), "f4", self, self.device))
            self.log.append(device_tensor(ptr(b.log), (self.log_cap, 4), "f4", self, self.device))
            self.eval_buf.append(device_tensor(ptr(b.eval), (4,), "f4", self, self.device))
            self.starts.append(device_tensor(ptr(b.starts), (int(b.starts_cap),), "i4", self, self.device) if b.starts_cap else None)
            self.perm.append(device_tensor(ptr(b.perm), (int(b.perm_cap),), "i4", self, self.device) if b.perm_cap else None)
            self.levels.append(device_tensor(ptr(b.levels), (int(b.levels_cap),), "f4", self, self.device) if b.levels_cap else None)
        offs, shp = (C.c_int64 * 16)(), (C.c_int64 * 32)()
        n = self.lib.lg_tube_sweep_param_layout(self.h, offs, shp, 16)
        self.layout = [(key, int(offs[i]), shape) for (key, shape), i in zip(param_shapes(*self.dims), range(n))]

    def member(self, k):
        return _Member(self, self._index(k))

    def _index(self, k):
        if not 0 <= int(k) < self.K:
            raise IndexError(f"member {k}: 0..{self.K - 1}")
        return int(k)

    # ---------------------------------------------------------------- model state
    def state_dict(self, k):
        """Member k's parameters under the reference MLP's keys; loads into HipTubeModel and deep_tube_learning.models.MLP."""
        p = self.params[self._index(k)]
        return OrderedDict((key, p[o:o + _numel(s)].view(s).detach().clone()) for key, o, s in self.layout)

    def load_state_dict(self, k, sd):
        k = self._index(k)
        want = [key for key, _, _ in self.layout]
        if list(sd.keys()) != want:
            raise KeyError(f"state dict keys {list(sd.keys())} != {want}")
        for key, o, s in self.layout:
            if tuple(sd[key].shape) != tuple(s):
                raise ValueError(f"{key}: shape {tuple(sd[key].shape)} != {tuple(s)}")
            self.params[k][o:o + _numel(s)].copy_(sd[key].reshape(-1).to(self.device, torch.float32))
        self._call("params_changed", k)

    # ---------------------------------------------------------------- data
    def set_data(self, train, test=None):
        """As HipTubeTrainer.set_data; the splits are shared by all members."""
        for which, ds in ((0, train), (1, test)):
            if ds is None:
                continue
            if self.horizon is not None:
                w, z, v = (t.to(self.device, torch.float32).contiguous() for t in (ds.w, ds.z, ds.v))
                if (ds.H_fwd, ds.H_rev) != tuple(self.horizon):
                    raise ValueError("dataset horizon != sweep horizon")
                check_window_dims(self.dims[0], self.horizon, z.shape[2], v.shape[2], self.level_input)
                self._data[which] = (w, z, v)
                self._call("set_data", which, C.c_void_p(w.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(v.data_ptr()),
                           w.shape[0], w.shape[1], z.shape[2], v.shape[2])
            else:
                x, y = (t.to(self.device, torch.float32).contiguous() for t in (ds.data, ds.target))
                if x.shape[1] != self.data_dim or y.shape[1] != self.dims[1]:
                    raise ValueError(f"dataset dims {(x.shape[1], y.shape[1])} != model dims {(self.data_dim, self.dims[1])}")
                self._data[which] = (x, y)
                self._call("set_data", which, C.c_void_p(x.data_ptr()), C.c_void_p(y.data_ptr()), None, x.shape[0], 0, 0, 0)
        self._views()

    def n_train(self):
        return int(self._data[0][0].shape[0])

    # ---------------------------------------------------------------- training
    def begin_epoch(self, epoch):
        self._call("begin_epoch", int(epoch))

    def step(self, count=None, rows=None):
        """One Adam step of every member: on the next `count` rows of each member's own epoch permutation, or on `rows`
        (int32 device tensor) shared by all members."""
        if rows is not None:
            rows = rows.to(self.device, torch.int32).contiguous()
            self._rows_keep = rows
            self._call("step", C.c_void_p(rows.data_ptr()), rows.numel())
        else:
            self._call("step", None, int(count))
        self.step_count += 1

    def set_step(self, step):
        self._call("set_step", int(step))
        self.step_count = int(step)

    def read_log(self, k, first, last):
        """Member k's [loss, lr after the step, grad_norm, rows] of the steps first..last (1-based), as a host tensor."""
        if last - first + 1 > self.log_cap:
            raise ValueError("more steps than the device log holds")
        idx = torch.arange(first - 1, last, device=self.device) % self.log_cap
        return self.log[self._index(k)][idx].cpu()

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

    def close(self):
        if getattr(self, "h", None):
            self.params = self.grads = self.adam_m = self.adam_v = self.log = self.eval_buf = self.starts = self.perm = self.levels = None
            self.lib.lg_tube_sweep_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
