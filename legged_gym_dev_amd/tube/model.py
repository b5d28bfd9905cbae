"""HipTubeModel: a trained tube MLP for inference only -- ``predict``, ``predict_windows``, ``rollout`` and
``rollout_window`` on the HIP kernels, and ``predict_levels`` / ``with_level`` for a level-conditioned model
(``predict_windows_levels`` where it is a horizon model).

It wraps the same ``lg_tube`` handle the trainer uses; the model's shape comes from the state dict, and what the state dict
cannot say (activation, Softplus beta, the horizon) from the run's ``config.json`` (train_tube.py writes it) or from keywords.
No optimiser setting is asked for: nothing here trains.
"""
import json
import os

import torch

from .data import HORIZON_KINDS
from .trainer import HipTubeTrainer

CONFIG_NAME = "config.json"
CHECKPOINTS = {"latest": "model.pth", "best": "model_best.pth"}


def shape_from_state_dict(sd):
    """(input_dim, output_dim, num_units, num_layers) of a reference-MLP state dict (layers.{0,2,...}.weight / .bias)."""
    ws = [k for k in sd if k.endswith(".weight")]
    if not ws or any(k != f"layers.{2 * i}.weight" for i, k in enumerate(ws)):
        raise KeyError(f"not a tube MLP state dict: {list(sd.keys())}")
    return int(sd[ws[0]].shape[1]), int(sd[ws[-1]].shape[0]), int(sd[ws[0]].shape[0]), len(ws) - 1


def read_config(run_dir):
    """The run's config.json as a dict; FileNotFoundError names the file when it is missing."""
    path = os.path.join(run_dir, CONFIG_NAME)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} is missing (train_tube.py writes it; runs older than that need the flags spelled out)")
    with open(path) as f:
        return json.load(f)


class HipTubeModel:
    def __init__(self, state_dict, activation="relu", softplus_beta=1.0, horizon=None, device="cuda:0", level_input=False):
        """horizon: None, or (H_fwd, H_rev) for a ScalarHorizonTubeDataset model.  level_input: a level-conditioned model, whose
        last input column is the coverage level (predict_levels, with_level; with a horizon predict_windows_levels)."""
        I, O, U, L = shape_from_state_dict(state_dict)
        self._tr = HipTubeTrainer(I, O, num_units=U, num_layers=L, activation=activation, softplus_beta=softplus_beta,
                                  loss="scalar_level" if level_input else "scalar", alpha=0.5, batch_size=32,
                                  horizon=tuple(horizon) if horizon else None, device=device)
        self._tr.load_state_dict(state_dict)
        self.level_input = bool(level_input)
        self.input_dim, self.output_dim, self.num_units, self.num_layers = I, O, U, L
        self.activation, self.softplus_beta, self.horizon, self.device = activation, softplus_beta, self._tr.horizon, self._tr.device

    @classmethod
    def load(cls, src, checkpoint="latest", activation=None, softplus_beta=None, horizon=None, device="cuda:0", level_input=None):
        """src: a train_tube.py run folder (its config.json supplies activation, softplus_beta, the horizon and level_input;
        keywords replace them) or a state dict (keywords, defaults relu / 1.0 / flat / unconditioned)."""
        cfg = {}
        if isinstance(src, (str, os.PathLike)):
            if checkpoint not in CHECKPOINTS:
                raise ValueError(f"checkpoint {checkpoint!r}: one of {tuple(CHECKPOINTS)}")
            if activation is None or os.path.isfile(os.path.join(src, CONFIG_NAME)):
                cfg = read_config(src)                       # without the activation a missing file is an error that names it
            sd = torch.load(os.path.join(src, CHECKPOINTS[checkpoint]), map_location="cpu")
        else:
            sd = src
        if horizon is None and cfg.get("dataset") in HORIZON_KINDS:
            horizon = (cfg["H_fwd"], cfg["H_rev"])
        return cls(sd, activation=activation or cfg.get("activation", "relu"),
                   softplus_beta=softplus_beta if softplus_beta is not None else cfg.get("softplus_beta", 1.0),
                   horizon=horizon, device=device,
                   level_input=bool(cfg.get("level_input", False)) if level_input is None else level_input)

    def predict(self, x, rows=None):
        return self._tr.predict(x, rows)

    def predict_levels(self, x, levels, rows=None):
        return self._tr.predict_levels(x, levels, rows)

    @staticmethod
    def with_level(x, level):
        """x (..., input_dim - 1) with the level column appended: the rows predict / rollout / rollout_window take on a
        level-conditioned model."""
        return torch.cat((x, torch.full_like(x[..., :1], float(level))), dim=-1)

    def predict_windows(self, ds, env, start):
        return self._tr.predict_windows(ds, env, start)

    def predict_windows_levels(self, ds, env, start, levels):
        return self._tr.predict_windows_levels(ds, env, start, levels)

    def rollout(self, x, fb, reseed=None):
        return self._tr.rollout(x, fb, reseed)

    def rollout_window(self, x, fb, taps, dN, stride, reseed=None):
        return self._tr.rollout_window(x, fb, taps, dN, stride, reseed)

    def state_dict(self):
        return self._tr.state_dict()

    def use_current_stream(self):
        self._tr.use_current_stream()

    def close(self):
        self._tr.close()
