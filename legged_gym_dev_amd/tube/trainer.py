"""HipTubeTrainer: the reference tube MLP trained and run by the HIP kernels of tube_kernels.hip (lg_tube_* in
include/legged_hip.h).  TubeTraining holds what it shares with sweep.HipTubeSweep -- handle, buffer views, data, the training
calls -- since a single trainer is a sweep of one member, in the library and here; HipTubeTrainer adds
member 0's views as attributes and the inference methods.

A step is two launches on the current stream -- fused forward / loss / backward over the minibatch, then the fixed-order gradient
reduction, Adam and StepLR -- and nothing in it waits for the device.  Loss, lr and gradient norm of every step stay in a device
log until ``read_log``.  A level-conditioned model (loss ``scalar_level`` / ``vector_level``) takes the
coverage level as its last input column: ``eval_level``, ``predict_levels`` and ``read_levels`` are its own, and on a horizon
dataset (section 10.8) ``predict_windows_levels``.  ``predict``, ``predict_windows``, ``rollout`` and ``rollout_window`` run the model as it stands (one launch
each, the roll-outs included) and return device tensors.  There is no CPU fallback: without the library or a GPU the constructor raises.
"""
import ctypes as C
from collections import OrderedDict

import torch

from .. import capi
from ..lib import LeggedHipError, device_tensor, load

ACTIVATIONS = tuple(capi.TUBE_ACT)
LOSSES = {"scalar": "scalar", "scalar_horizon": "scalar", "vector": "vector", "error": "mse",
          "scalar_level": "scalar", "vector_level": "vector"}                                   # reference loss -> kernel loss
LEVEL_LOSSES = ("scalar_level", "vector_level")     # level-conditioned: lg_tube_cfg.level_input, the last input column is the level


def check_envelope(input_dim, output_dim, num_units, num_layers, activation="relu", final_activation=None, loss=None,
                   horizon=None, level_input=False, level_lo=0.0, level_hi=1.0):
    """The supported model envelope (the C side refuses the same); raises ValueError / NotImplementedError outside it.
    level_input: the level-conditioned tube, with the loss, the horizon and the level range it is asked with.  A conditioned
    horizon model needs H_rev >= 1: the chosen edge of the envelope."""
    if level_input:
        if loss is not None and LOSSES.get(loss) == "mse":
            raise ValueError("level_input needs a tube loss (scalar or vector): the mse loss has no level")
        if horizon is not None and horizon[1] < 1:
            raise ValueError(f"level_input with a horizon dataset needs H_rev >= 1 (got {horizon[1]}): an item without a past error "
                             "carries no error history; the flat level kinds serve that case")
        if input_dim < 2:
            raise ValueError(f"input_dim={input_dim}: with level_input it counts the level column and must be at least 2")
        if not 0.0 <= level_lo < level_hi <= 1.0:
            raise ValueError(f"level range [{level_lo}, {level_hi}): 0 <= level_lo < level_hi <= 1")
    if final_activation is not None:
        raise NotImplementedError("final_activation other than None is not supported (no reference configuration uses one)")
    if activation not in ACTIVATIONS:
        raise ValueError(f"activation {activation!r}: one of {ACTIVATIONS}")
    if not (16 <= num_units <= capi.TUBE_MAX_UNITS and num_units % 16 == 0):
        raise ValueError(f"num_units={num_units}: 16..{capi.TUBE_MAX_UNITS} in steps of 16")
    if not 1 <= num_layers <= 4:
        raise ValueError(f"num_layers={num_layers}: 1..4")
    if not 1 <= input_dim <= capi.TUBE_MAX_IN:
        raise ValueError(f"input_dim={input_dim}: 1..{capi.TUBE_MAX_IN}")
    if not 1 <= output_dim <= capi.TUBE_MAX_OUT:
        raise ValueError(f"output_dim={output_dim}: 1..{capi.TUBE_MAX_OUT}")


def window_input_dim(horizon, nz, m, level_input=False):
    """Columns of a horizon model's item: H_rev + nz + (H_rev + H_fwd) m, plus the level column of a conditioned model."""
    Hf, Hr = horizon
    return Hr + nz + (Hr + Hf) * m + int(bool(level_input))


def check_window_dims(input_dim, horizon, nz, m, level_input=False):
    """ValueError unless arrays z (.., nz) and v (.., m) build items of the model's input_dim (the C side refuses the same)."""
    if input_dim != window_input_dim(horizon, nz, m, level_input):
        raise ValueError(f"input_dim {input_dim} != H_rev + nz + (H_rev + H_fwd) * m{' + 1 (the level column)' if level_input else ''} = "
                         f"{window_input_dim(horizon, nz, m, level_input)} for H_fwd, H_rev = {tuple(horizon)}, nz = {nz}, m = {m}")


def param_shapes(input_dim, output_dim, num_units, num_layers):
    """[(state-dict key, shape)] of the reference MLP: Linear layers at the even indices of `layers`."""
    dims = [input_dim] + [num_units] * num_layers + [output_dim]
    out = []
    for i in range(num_layers + 1):
        out += [(f"layers.{2 * i}.weight", (dims[i + 1], dims[i])), (f"layers.{2 * i}.bias", (dims[i + 1],))]
    return out


def initial_params(input_dim, output_dim, num_units, num_layers, seed):
    """nn.Linear's default initialisation, drawn in the reference MLP's construction order after torch.manual_seed(seed)."""
    torch.manual_seed(seed)
    dims = [input_dim] + [num_units] * num_layers + [output_dim]
    sd = OrderedDict()
    for i in range(num_layers + 1):
        lin = torch.nn.Linear(dims[i], dims[i + 1])
        sd[f"layers.{2 * i}.weight"] = lin.weight.detach().clone()
        sd[f"layers.{2 * i}.bias"] = lin.bias.detach().clone()
    return sd


def make_cfg(input_dim, output_dim, c):
    """The lg_tube_cfg of one model from the trainer's keywords in `c` (num_units .. level_hi, as HipTubeTrainer names them)."""
    hz, lv = c["horizon"], c["loss"] in LEVEL_LOSSES
    return capi.lg_tube_cfg(input_dim=input_dim, output_dim=output_dim, num_units=c["num_units"], num_layers=c["num_layers"],
                            activation=capi.TUBE_ACT[c["activation"]], loss=capi.TUBE_LOSS[LOSSES[c["loss"]]],
                            horizon=int(hz is not None), batch_size=c["batch_size"], H_fwd=hz[0] if hz else 0,
                            H_rev=hz[1] if hz else 0, step_size=c["step_size"], seed=c["seed"],
                            alpha=c["alpha"] if c["alpha"] is not None else 0.0, delta=c["delta"],
                            softplus_beta=c["softplus_beta"], lr=c["lr"], gamma=c["gamma"], level_input=int(lv),
                            level_lo=c["level_lo"] if lv else 0.0, level_hi=c["level_hi"] if lv else 0.0)


VIEWS = ("params", "grads", "adam_m", "adam_v", "log", "eval_buf", "starts", "perm", "levels")


class TubeTraining:
    """What HipTubeTrainer (one model) and HipTubeSweep (K models) share: the handle of one C family (PREFIX), the views of every
    member's buffers, the data and the training calls.  The library runs both through one trainer."""
    PREFIX = NOUN = None                # "lg_tube_" / "trainer", "lg_tube_sweep_" / "sweep"
    h = None

    def _open(self, device):
        self.device = torch.device(device)
        if self.device.type != "cuda" or not torch.cuda.is_available():
            raise LeggedHipError(f"the tube {self.NOUN} needs a GPU device (no CPU fallback); got " + str(device))
        self.lib = load()

    def _create(self, K, *args):
        """Creates the handle (args: what the family's create takes before the handle) with its stream and views.  Needs dims."""
        self.K = K
        torch.cuda.set_device(self.device)
        h = C.c_void_p()
        self._call("create", *args, C.byref(h), obj=False)
        self.h = h
        self.use_current_stream()
        self._views()
        self._data = {}

    def _call(self, fn, *args, obj=True):
        rc = getattr(self.lib, self.PREFIX + fn)(*((self.h,) if obj else ()), *args)
        if rc != 0:
            raise LeggedHipError(f"{self.PREFIX}{fn} failed ({rc}): {self.lib.lg_last_error().decode()}")

    def use_current_stream(self):
        self._call("set_stream", C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream))

    def _member_arg(self, k):
        """What the family's per-member entries take for member k."""
        return (k,)

    def _views(self):
        """Torch views of every member's buffers, {name of VIEWS: [per member]}, handed to _expose; the parameter layout."""
        ptr = lambda p: C.cast(p, C.c_void_p).value
        views = {n: [] for n in VIEWS}
        for k in range(self.K):
            b = capi.lg_tube_buffers()
            self._call("get_buffers", *self._member_arg(k), C.byref(b))
            P = int(b.num_params)
            self.num_params, self.log_cap, self.step_count = P, int(b.log_cap), int(b.step)
            for n, p, shape, dt in (("params", b.params, (P,), "f4"), ("grads", b.grads, (P,), "f4"), ("adam_m", b.adam_m, (P,), "f4"),
                                    ("adam_v", b.adam_v, (P,), "f4"), ("log", b.log, (self.log_cap, 4), "f4"),
                                    ("eval_buf", b.eval, (4,), "f4"), ("starts", b.starts, (int(b.starts_cap),), "i4"),
                                    ("perm", b.perm, (int(b.perm_cap),), "i4"), ("levels", b.levels, (int(b.levels_cap),), "f4")):
                views[n].append(device_tensor(ptr(p), shape, dt, self, self.device) if shape[0] else None)
        self._expose(views)
        offs, shp = (C.c_int64 * 16)(), (C.c_int64 * 32)()
        n = getattr(self.lib, self.PREFIX + "param_layout")(self.h, offs, shp, 16)
        self.layout = [(key, int(offs[i]), shape) for (key, shape), i in zip(param_shapes(*self.dims), range(n))]

    def _state_of(self, params):
        return OrderedDict((k, params[o:o + _numel(s)].view(s).detach().clone()) for k, o, s in self.layout)

    def _load_params(self, params, sd):
        want = [k for k, _, _ in self.layout]
        if list(sd.keys()) != want:
            raise KeyError(f"state dict keys {list(sd.keys())} != {want}")
        for k, o, s in self.layout:
            if tuple(sd[k].shape) != tuple(s):
                raise ValueError(f"{k}: shape {tuple(sd[k].shape)} != {tuple(s)}")
            params[o:o + _numel(s)].copy_(sd[k].reshape(-1).to(self.device, torch.float32))

    # ---------------------------------------------------------------- data
    def set_data(self, train, test=None):
        """train / test: TubeDataset-like (data, target) or ScalarHorizonTubeDataset-like (w, z, v); shared by all members."""
        for which, ds in ((0, train), (1, test)):
            if ds is None:
                continue
            if self.horizon is not None:
                w, z, v = (t.to(self.device, torch.float32).contiguous() for t in (ds.w, ds.z, ds.v))
                if (ds.H_fwd, ds.H_rev) != tuple(self.horizon):
                    raise ValueError(f"dataset horizon != {self.NOUN} horizon")
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

    def _log_rows(self, log, first, last):
        if last - first + 1 > self.log_cap:
            raise ValueError("more steps than the device log holds")
        idx = torch.arange(first - 1, last, device=self.device) % self.log_cap
        return log[idx].cpu()

    def close(self):
        if getattr(self, "h", None):
            for n in VIEWS:
                setattr(self, n, None)
            self._call("destroy")
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class HipTubeTrainer(TubeTraining):
    PREFIX, NOUN = "lg_tube_", "trainer"

    def __init__(self, input_dim, output_dim, num_units=32, num_layers=2, activation="relu", softplus_beta=1.0,
                 loss="scalar", alpha=0.8, delta=1.0, lr=1e-3, gamma=0.1, step_size=10000, batch_size=2048, seed=42,
                 horizon=None, final_activation=None, device="cuda:0", level_lo=0.0, level_hi=1.0):
        """horizon: None for the row datasets, (H_fwd, H_rev) for ScalarHorizonTubeDataset.  loss "scalar_level" /
        "vector_level": the level-conditioned tube -- input_dim counts the level column (the last one), the data has
        input_dim - 1 columns, every row of a step draws its level uniformly from [level_lo, level_hi), alpha is not read.
        With a horizon the window item gains the level as its last column and the row's H_fwd outputs share it in the loss."""
        if loss not in LOSSES:
            raise ValueError(f"loss {loss!r}: one of {tuple(LOSSES)}")
        self.level_input = loss in LEVEL_LOSSES
        check_envelope(input_dim, output_dim, num_units, num_layers, activation, final_activation, loss=loss, horizon=horizon,
                       level_input=self.level_input, level_lo=level_lo, level_hi=level_hi)
        if loss in ("scalar", "scalar_horizon", "vector") and alpha is None:
            raise ValueError(f"loss {loss!r} needs alpha")
        self._open(device)
        self.dims = (input_dim, output_dim, num_units, num_layers)
        self.activation, self.softplus_beta, self.loss = activation, softplus_beta, loss
        self.horizon = horizon
        cfg = make_cfg(input_dim, output_dim, dict(
            num_units=num_units, num_layers=num_layers, activation=activation, softplus_beta=softplus_beta, loss=loss, alpha=alpha,
            delta=delta, lr=lr, gamma=gamma, step_size=step_size, batch_size=batch_size, seed=seed, horizon=horizon,
            level_lo=level_lo, level_hi=level_hi))
        self.batch_size = batch_size
        self.data_dim = input_dim - int(self.level_input)          # columns of the data: the level column is not in it
        self._create(1, C.byref(cfg))
        self.load_state_dict(initial_params(input_dim, output_dim, num_units, num_layers, seed))

    def _member_arg(self, k):
        return ()

    def _expose(self, views):           # the one member's views as attributes: self.params, self.adam_m, ...
        for n, v in views.items():
            setattr(self, n, v[0])

    # ---------------------------------------------------------------- model state
    def state_dict(self):
        """The reference MLP's keys (layers.{0,2,4,...}.weight / .bias); loads into deep_tube_learning.models.MLP."""
        return self._state_of(self.params)

    def load_state_dict(self, sd):
        self._load_params(self.params, sd)
        self._call("params_changed")

    def read_log(self, first, last):
        """Host copy (rows = steps first..last, 1-based, at most log_cap of them) of [loss, lr after the step, grad_norm, rows]."""
        return self._log_rows(self.log, first, last)

    def evaluate(self):
        """Launches the eval over the test split; returns a device tensor [loss, fraction fw > w, mean |w - fw| where fw > w,
        rows] (a copy, valid once the stream reaches it)."""
        self._call("eval")
        return self.eval_buf.clone()

    def eval_level(self, level):
        """Level-conditioned models: evaluate() with every test row at `level` (0..1) instead of a drawn one; entry 1 is then
        the coverage at that level."""
        self._need_level("eval_level")
        self._call("eval_level", C.c_float(float(level)))
        return self.eval_buf.clone()

    def read_levels(self, count):
        """Host copy of the levels of the first `count` rows of the last step or evaluation (row order of that batch)."""
        self._need_level("read_levels")
        if self.levels is None or not 0 <= count <= self.levels.numel():
            raise ValueError(f"count={count}: 0..{0 if self.levels is None else self.levels.numel()} (set_data sizes the buffer)")
        return self.levels[:count].cpu()

    def _need_level(self, what):
        if not self.level_input:
            raise ValueError(f"{what}: the model is not level-conditioned (loss scalar_level / vector_level)")

    # ---------------------------------------------------------------- inference (reads the parameters, changes nothing)
    def predict_levels(self, x, levels, rows=None):
        """Level-conditioned models: MLP([x[rows], level]) for every level of `levels` (1..64 values) in one launch, as a device
        tensor (count, n_levels, output_dim); x (n, input_dim - 1) holds no level column.  Entry [i, l] equals, bit for bit,
        predict() on row i with levels[l] appended."""
        self._need_level("predict_levels")
        x = self._f32(x)
        if x.dim() != 2 or x.shape[1] != self.data_dim or x.shape[0] < 1:
            raise ValueError(f"x must be (n >= 1, {self.data_dim}); got {tuple(x.shape)}")
        levels = self._levels_arg(levels)
        rows, count, rp = self._rows_arg(rows, x.shape[0])
        out = torch.empty(count, levels.numel(), self.dims[1], device=self.device, dtype=torch.float32)
        self._call("predict_levels", C.c_void_p(x.data_ptr()), rp, count, C.c_void_p(levels.data_ptr()), levels.numel(),
                   C.c_void_p(out.data_ptr()))
        self._keep = (x, rows, levels)
        return out

    def predict(self, x, rows=None):
        """MLP(x[rows]) (every row of x in order when rows is None) as a device tensor (count, output_dim); flat models."""
        if self.horizon is not None:
            raise ValueError("a horizon model predicts windows: predict_windows(ds, env, start)")
        x = self._f32(x)
        if x.dim() != 2 or x.shape[1] != self.dims[0] or x.shape[0] < 1:
            raise ValueError(f"x must be (n >= 1, {self.dims[0]}); got {tuple(x.shape)}")
        rows, count, rp = self._rows_arg(rows, x.shape[0])
        out = torch.empty(count, self.dims[1], device=self.device, dtype=torch.float32)
        self._call("predict", C.c_void_p(x.data_ptr()), rp, count, C.c_void_p(out.data_ptr()))
        self._keep = (x, rows)
        return out

    def _windows(self, ds, env, start):
        """The checked arguments of a window query: (w, z, v, n, T, env, start) on the device."""
        Hf, Hr = self.horizon
        if (ds.H_fwd, ds.H_rev) != (Hf, Hr):
            raise ValueError("dataset horizon != model horizon")
        w, z, v = (self._f32(t) for t in (ds.w, ds.z, ds.v))
        n, T = w.shape
        if z.shape[:2] != (n, T) or v.shape[:2] != (n, T):
            raise ValueError("w, z and v differ in envs or time steps")
        check_window_dims(self.dims[0], self.horizon, z.shape[2], v.shape[2], self.level_input)
        env = torch.as_tensor(env).to(self.device, torch.int32).contiguous().reshape(-1)
        start = torch.as_tensor(start).to(self.device, torch.int32).contiguous().reshape(-1)
        if env.numel() != start.numel() or env.numel() < 1:
            raise ValueError("env and start must have the same positive length")
        if int(env.min()) < 0 or int(env.max()) >= n:
            raise IndexError(f"env must lie in 0..{n - 1}")
        if int(start.min()) < Hr or int(start.max()) + Hf > T:
            raise IndexError(f"window out of range: need {Hr} <= start and start + {Hf} <= {T}")
        return w, z, v, n, T, env, start

    def predict_windows(self, ds, env, start):
        """The H_fwd predictions of the ScalarHorizonTubeDataset items (env[i], start[i]) of `ds` (w, z, v padded in front by
        H_rev): a device tensor (count, H_fwd).  Every start must satisfy H_rev <= start and start + H_fwd <= T."""
        if self.horizon is None:
            raise ValueError("a flat model predicts rows: predict(x, rows)")
        if self.level_input:
            raise ValueError("predict_windows: the model is level-conditioned, a window holds no level: "
                             "predict_windows_levels(ds, env, start, levels)")
        w, z, v, n, T, env, start = self._windows(ds, env, start)
        out = torch.empty(env.numel(), self.horizon[0], device=self.device, dtype=torch.float32)
        self._call("predict_windows", C.c_void_p(w.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(v.data_ptr()), n, T,
                   z.shape[2], v.shape[2], C.c_void_p(env.data_ptr()), C.c_void_p(start.data_ptr()), env.numel(),
                   C.c_void_p(out.data_ptr()))
        self._keep = (w, z, v, env, start)
        return out

    def predict_windows_levels(self, ds, env, start, levels):
        """Level-conditioned horizon models: the H_fwd predictions of the items (env[i], start[i]) of `ds` at every level of
        `levels` (1..64 values) in one launch, a device tensor (count, n_levels, H_fwd).  Entry [i, l] equals, bit for bit,
        predict() of a flat conditioned model with these parameters on the item with levels[l] appended."""
        self._need_level("predict_windows_levels")
        if self.horizon is None:
            raise ValueError("predict_windows_levels: not a horizon model; a flat model predicts rows: predict_levels(x, levels)")
        levels = self._levels_arg(levels)
        w, z, v, n, T, env, start = self._windows(ds, env, start)
        out = torch.empty(env.numel(), levels.numel(), self.horizon[0], device=self.device, dtype=torch.float32)
        self._call("predict_windows_levels", C.c_void_p(w.data_ptr()), C.c_void_p(z.data_ptr()), C.c_void_p(v.data_ptr()), n, T,
                   z.shape[2], v.shape[2], C.c_void_p(env.data_ptr()), C.c_void_p(start.data_ptr()), env.numel(),
                   C.c_void_p(levels.data_ptr()), levels.numel(), C.c_void_p(out.data_ptr()))
        self._keep = (w, z, v, env, start, levels)
        return out

    def rollout(self, x, fb, reseed=None):
        """Closed loop over time in one launch.  x (n_seq, T, input_dim): the teacher rows in time order.  Returns out
        (n_seq, T, output_dim) with out[s, t] = MLP(x[s, t] with its leading fb columns replaced by out[s, t-1, :fb]); at t = 0
        and where reseed[s, t] (bool / uint8, (n_seq, T)) is set the row is taken as it is."""
        if self.horizon is not None:
            raise ValueError("a horizon model has no closed loop: predict_windows(ds, env, start)")
        x = self._f32(x)
        if x.dim() != 3 or x.shape[2] != self.dims[0] or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x must be (n_seq >= 1, T >= 1, {self.dims[0]}); got {tuple(x.shape)}")
        if not 0 <= int(fb) <= min(self.dims[:2]):
            raise ValueError(f"fb={fb}: 0..min(input_dim, output_dim) = {min(self.dims[:2])}")
        reseed, rp = self._reseed_arg(reseed, x)
        out = torch.empty(x.shape[0], x.shape[1], self.dims[1], device=self.device, dtype=torch.float32)
        self._call("rollout", C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], int(fb), rp, C.c_void_p(out.data_ptr()))
        self._keep = (x, reseed)
        return out

    def rollout_window(self, x, fb, taps, dN, stride, reseed=None):
        """Closed loop of a windowed model in one launch.  A row of x (n_seq, T, input_dim) is `taps` blocks of `stride` columns,
        block i the dataset row delayed by i * dN steps, and the leading fb columns of every block are fed back: with s0(t) the
        last step <= t that is 0 or has reseed[s, t] set, block i of x[s, t] takes out[s, t-1-i*dN, :fb] where t - i*dN > s0(t)
        and keeps the teacher's columns otherwise.  taps == 1 is rollout(x, fb, reseed)."""
        if self.horizon is not None:
            raise ValueError("a horizon model has no closed loop: predict_windows(ds, env, start)")
        x = self._f32(x)
        if x.dim() != 3 or x.shape[2] != self.dims[0] or x.shape[0] < 1 or x.shape[1] < 1:
            raise ValueError(f"x must be (n_seq >= 1, T >= 1, {self.dims[0]}); got {tuple(x.shape)}")
        fb, taps, dN, stride = int(fb), int(taps), int(dN), int(stride)
        if fb < 1 or taps < 1 or dN < 1:
            raise ValueError(f"fb={fb}, taps={taps}, dN={dN}: each at least 1")
        if fb > self.dims[1]:
            raise ValueError(f"fb={fb} exceeds output_dim {self.dims[1]}")
        if taps > 1 and stride < fb:
            raise ValueError(f"stride={stride} is below fb={fb}")
        if (taps - 1) * (stride if taps > 1 else 0) + fb > self.dims[0]:
            raise ValueError(f"(taps - 1) * stride + fb = {(taps - 1) * stride + fb} exceeds input_dim {self.dims[0]}")
        if ((taps - 1) * dN + 1) * fb > capi.TUBE_RING_MAX:
            raise ValueError(f"ring ((taps - 1) * dN + 1) * fb = {((taps - 1) * dN + 1) * fb} floats per sequence exceeds "
                             f"{capi.TUBE_RING_MAX}")
        reseed, rp = self._reseed_arg(reseed, x)
        out = torch.empty(x.shape[0], x.shape[1], self.dims[1], device=self.device, dtype=torch.float32)
        self._call("rollout_window", C.c_void_p(x.data_ptr()), x.shape[0], x.shape[1], fb, taps, dN, stride if taps > 1 else 0, rp,
                   C.c_void_p(out.data_ptr()))
        self._keep = (x, reseed)
        return out

    def _f32(self, t):
        return t.to(self.device, torch.float32).contiguous()

    def _rows_arg(self, rows, n):
        """The checked row list of a query over n rows: (rows on the device or None, count, pointer or None)."""
        if rows is None:
            return None, n, None
        rows = rows.to(self.device, torch.int32).contiguous().reshape(-1)
        if rows.numel() < 1:
            raise ValueError("rows is empty")
        if int(rows.min()) < 0 or int(rows.max()) >= n:
            raise IndexError(f"rows must lie in 0..{n - 1}")
        return rows, rows.numel(), C.c_void_p(rows.data_ptr())

    def _levels_arg(self, levels):
        levels = self._f32(torch.as_tensor(levels)).reshape(-1)
        if not 1 <= levels.numel() <= capi.TUBE_MAX_LEVELS:
            raise ValueError(f"{levels.numel()} levels: 1..{capi.TUBE_MAX_LEVELS}")
        return levels

    def _reseed_arg(self, reseed, x):
        """The checked reseed flags of a roll-out over x (n_seq, T, .): (uint8 on the device or None, pointer or None)."""
        if reseed is None:
            return None, None
        reseed = reseed.to(self.device).ne(0).to(torch.uint8).contiguous()
        if tuple(reseed.shape) != tuple(x.shape[:2]):
            raise ValueError(f"reseed must be {tuple(x.shape[:2])}; got {tuple(reseed.shape)}")
        return reseed, C.c_void_p(reseed.data_ptr())


def _numel(shape):
    n = 1
    for s in shape:
        n *= s
    return n
