"""Checkpoint and export formats of the reference stack, produced from / consumed into the flat HBM
parameter buffers of the HIP learner.

* ``model_<it>.pt`` (rsl_rl ``OnPolicyRunner.save``; read by scripts/play.py:69-76 through
  ``task_registry.make_alg_runner(resume=True)``, legged_gym/utils/task_registry.py:150-155):
  ``{"model_state_dict": ActorCritic.state_dict(), "optimizer_state_dict": torch.optim.Adam.state_dict(),
  "iter": int, "infos": ...}``.  The optimiser entry is written in torch's own Adam layout (per-parameter
  ``step / exp_avg / exp_avg_sq`` in ``ActorCritic.parameters()`` order) so either stack can resume the other's run.
* ``policy_1.pt``: TorchScript of the actor MLP (legged_gym/utils/helpers.py:274-285, play.py:78-82).
* ``policy_lstm_1.pt``: for ActorCriticRecurrent, TorchScript of memory_a + the actor MLP with the module surface of the reference's
  ``PolicyExporterLSTM`` (helpers.py:288-313): ``forward(x)`` carries ``hidden_state`` / ``cell_state`` buffers (1, 1, H) from call
  to call, ``reset_memory()`` zeroes them.

Pure torch/CPU code: nothing here is on the training path.
"""
import copy
import os
from collections import OrderedDict

import torch

ACTIVATIONS = {"elu": torch.nn.ELU, "selu": torch.nn.SELU, "relu": torch.nn.ReLU, "lrelu": torch.nn.LeakyReLU,
               "tanh": torch.nn.Tanh, "sigmoid": torch.nn.Sigmoid}


def parameter_order(state_dict):
    """Names in ``ActorCritic.parameters()`` order: std, actor.*, critic.* (registration order in rsl_rl); ActorCriticRecurrent
    continues with memory_a.rnn.* and memory_c.rnn.* (weight_ih, weight_hh, bias_ih, bias_hh)."""
    names = list(state_dict.keys())
    rnn = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

    def rank(n):
        if n.startswith("memory_"):
            return (3 if n.startswith("memory_a.") else 4, rnn.index(n.split(".")[-1]), 0)
        return (0 if n == "std" else 1 if n.startswith("actor.") else 2, int(n.split(".")[1]) if "." in n else 0,
                0 if n.endswith("weight") else 1)
    return sorted(names, key=rank)


def adam_state_to_torch(names, shapes, adam_m, adam_v, step, lr):
    """Flat first/second moments -> ``torch.optim.Adam.state_dict()`` (betas 0.9/0.999, eps 1e-8)."""
    state, off = {}, 0
    for i, n in enumerate(names):
        cnt = 1
        for d in shapes[n]:
            cnt *= d
        state[i] = {"step": torch.tensor(float(step)), "exp_avg": adam_m[off:off + cnt].reshape(shapes[n]).clone().cpu(),
                    "exp_avg_sq": adam_v[off:off + cnt].reshape(shapes[n]).clone().cpu()}
        off += cnt
    group = {"lr": float(lr), "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0, "amsgrad": False, "maximize": False,
             "foreach": None, "capturable": False, "differentiable": False, "fused": None,
             "params": list(range(len(names)))}
    return {"state": state, "param_groups": [group]}


def adam_state_from_torch(sd, names, shapes):
    """Inverse of :func:`adam_state_to_torch`; also accepts this package's first-round layout
    (``adam_m / adam_v / step / lr``).  Returns (m_flat, v_flat, step, lr); a fresh optimiser (empty state) gives zeros."""
    if "adam_m" in sd:
        return sd["adam_m"].float().flatten(), sd["adam_v"].float().flatten(), float(sd["step"]), float(sd["lr"])
    ms, vs, step = [], [], 0.0
    for i, n in enumerate(names):
        st = sd["state"].get(i, sd["state"].get(str(i)))
        if st is None:
            z = torch.zeros(shapes[n]).flatten()
            ms.append(z); vs.append(z.clone())
            continue
        if tuple(st["exp_avg"].shape) != tuple(shapes[n]):
            raise ValueError(f"optimizer state of parameter {i} ({n}) has shape {tuple(st['exp_avg'].shape)}, expected {tuple(shapes[n])}")
        ms.append(st["exp_avg"].float().flatten()); vs.append(st["exp_avg_sq"].float().flatten())
        step = max(step, float(st["step"]))
    return torch.cat(ms), torch.cat(vs), step, float(sd["param_groups"][0]["lr"])


def build_mlp(state_dict, prefix="actor", activation="elu"):
    """``nn.Sequential`` [Linear, act, ..., Linear] with rsl_rl's module indices (actor.0, actor.2, ...)."""
    act = ACTIVATIONS[activation]
    idx = sorted({int(k.split(".")[1]) for k in state_dict if k.startswith(prefix + ".")})
    layers = OrderedDict()
    for n, i in enumerate(idx):
        w = state_dict[f"{prefix}.{i}.weight"]
        lin = torch.nn.Linear(w.shape[1], w.shape[0])
        with torch.no_grad():
            lin.weight.copy_(w.detach().cpu())
            lin.bias.copy_(state_dict[f"{prefix}.{i}.bias"].detach().cpu())
        layers[str(i)] = lin
        if n + 1 < len(idx):
            layers[str(i + 1)] = act()
    return torch.nn.Sequential(layers)


class LSTMPolicy(torch.nn.Module):
    """memory_a's LSTM followed by the actor MLP, one observation row per call, the state kept in buffers (batch of 1)."""

    def __init__(self, state_dict, activation):
        super().__init__()
        w_ih = state_dict["memory_a.rnn.weight_ih_l0"]
        H = w_ih.shape[0] // 4
        self.memory = torch.nn.LSTM(w_ih.shape[1], H, 1)
        with torch.no_grad():
            for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
                getattr(self.memory, k).copy_(state_dict[f"memory_a.rnn.{k}"].detach().cpu())
        self.actor = build_mlp(state_dict, "actor", activation)
        self.register_buffer("hidden_state", torch.zeros(1, 1, H))
        self.register_buffer("cell_state", torch.zeros(1, 1, H))

    def forward(self, x):
        seq = x.reshape(1, x.shape[0], x.shape[1])                        # one time step of a batch of rows
        y, state = self.memory(seq, (self.hidden_state, self.cell_state))
        self.hidden_state.copy_(state[0])
        self.cell_state.copy_(state[1])
        return self.actor(y[0])

    @torch.jit.export
    def reset_memory(self):
        self.hidden_state.zero_()
        self.cell_state.zero_()


class HistoryPolicy(torch.nn.Module):
    """The actor MLP behind its observation history (envs/base/obs_history.py), one (1, num_obs) frame per call: ``history`` is the
    (1, W) row [obs_t | sel(obs_t-1) | ...], moved on by one frame per call and reinitialised on the first call and on the call
    after reset_memory() -- every past frame then sel(obs_t) ("repeat") or zeros ("zero").  The surface is LSTMPolicy's."""

    def __init__(self, state_dict, activation, spec):
        super().__init__()
        self.actor = build_mlp(state_dict, "actor", activation)
        self.num_obs, self.num_selected, self.length, self.width = int(spec.num_obs), int(spec.num_selected), int(spec.length), int(spec.width)
        self.zero = spec.reset == "zero"
        if self.actor[0].in_features != self.width:
            raise ValueError(f"the actor takes {self.actor[0].in_features} columns but the history ({spec}) gives {self.width}")
        self.register_buffer("columns", torch.tensor(spec.columns(), dtype=torch.long))
        self.register_buffer("history", torch.zeros(1, self.width))
        self.register_buffer("fresh", torch.ones(1, dtype=torch.bool))

    def forward(self, obs):
        sel = obs.index_select(1, self.columns)
        if bool(self.fresh.item()):
            past = torch.zeros(1, (self.length - 1) * self.num_selected) if self.zero else sel.repeat(1, self.length - 1)
            self.fresh.zero_()
        else:
            older = self.history[:, self.num_obs:self.width - self.num_selected]
            past = torch.cat([self.history[:, :self.num_obs].index_select(1, self.columns), older], 1)
        self.history.copy_(torch.cat([obs, past], 1))
        return self.actor(self.history)

    @torch.jit.export
    def reset_memory(self):
        self.fresh.fill_(True)


def fold_obs_normalizer(state_dict, norm):
    """The frozen normaliser y = (x - mean) / (std + eps) folded into the layer that reads the row, so that the exported module takes
    RAW rows: W' = W diag(1 / (std + eps)), b' = b - W' mean, in float64, rounded once.  The layer is ``actor.0`` (also behind a
    history: it reads the (1, W) history row), or ``memory_a.rnn.weight_ih_l0`` / ``bias_ih_l0`` of the recurrent policy.  ``norm``:
    the normaliser's state dict (``_mean``, ``_std`` of (1, W)), optionally with ``eps`` (default 1e-2).  Returns a new dict."""
    wk, bk = (("memory_a.rnn.weight_ih_l0", "memory_a.rnn.bias_ih_l0") if "memory_a.rnn.weight_ih_l0" in state_dict
              else ("actor.0.weight", "actor.0.bias"))
    w, b = state_dict[wk].detach().cpu().double(), state_dict[bk].detach().cpu().double()
    mean, std = norm["_mean"].detach().cpu().double().reshape(-1), norm["_std"].detach().cpu().double().reshape(-1)
    if mean.numel() != w.shape[1] or std.numel() != w.shape[1]:
        raise ValueError(f"the observation normaliser has {mean.numel()} columns but {wk} reads {w.shape[1]}")
    w2 = w / (std + float(norm.get("eps", 1e-2))).reshape(1, -1)
    out = {k: v for k, v in state_dict.items()}
    out[wk], out[bk] = w2.float(), (b - w2 @ mean).float()
    return out


def export_policy_as_jit(actor_critic, path, activation=None, obs_history=None, obs_normalizer=None):
    """helpers.py:274-285: ``<path>/policy_1.pt`` = torch.jit.script(actor MLP on CPU); a recurrent policy (memory_a.* in its
    state dict) goes to ``<path>/policy_lstm_1.pt`` instead (helpers.py:288-313).  With ``obs_history`` (an enabled
    ObsHistorySpec) the actor goes out behind its history as ``<path>/policy_hist_1.pt`` (HistoryPolicy).  With ``obs_normalizer``
    (the state dict of the actor row's frozen normaliser, rl/obs_norm.py) the module takes raw rows: the normaliser is folded into
    its first layer (fold_obs_normalizer); file names and module surfaces stay."""
    os.makedirs(path, exist_ok=True)
    sd = actor_critic.state_dict()
    if obs_normalizer is not None:
        sd = fold_obs_normalizer(sd, obs_normalizer)
    activation = activation or getattr(actor_critic, "activation", "elu")
    if obs_history is not None and obs_history.enabled:
        scripted = torch.jit.script(HistoryPolicy(sd, activation, obs_history).to("cpu"))
        out = os.path.join(path, "policy_hist_1.pt")
        scripted.save(out)
        return out
    if "memory_a.rnn.weight_ih_l0" in sd:
        scripted = torch.jit.script(LSTMPolicy(sd, activation).to("cpu"))
        out = os.path.join(path, "policy_lstm_1.pt")
        scripted.save(out)
        return out
    model = copy.deepcopy(build_mlp(sd, "actor", activation)).to("cpu")
    scripted = torch.jit.script(model)
    out = os.path.join(path, "policy_1.pt")
    scripted.save(out)
    return out
