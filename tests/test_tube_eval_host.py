"""Host side of the tube evaluation: sequences() against from_folder on the reference fixtures, feedback_width, the metrics on
hand-made inputs whose answers can be written down, and train_tube's config.json round trip."""
import json
import math
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from legged_gym_dev_amd.tube import data as td
from legged_gym_dev_amd.tube import evaluate as ev
from legged_gym_dev_amd.tube import model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("tube_fx")
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "tube_dataset.npz")))
    for k in (0, 1):
        with open(d / f"epoch_{k}.pickle", "wb") as f:
            pickle.dump({key: fx[f"e{k}_{key}"] for key in ("z", "pz_x", "v", "done")}, f)
    return str(d)


KINDS = [("scalar", {}), ("scalar", {"recursive": True}), ("vector", {}), ("error_dynamics", {})]


@pytest.mark.parametrize("N,dN", [(1, 1), (3, 2)])
@pytest.mark.parametrize("kind,extra", KINDS, ids=lambda k: str(k))
def test_sequences_minus_done_rows_is_from_folder(folder, kind, extra, N, dN):
    args = dict(N=N, dN=dN, **extra)
    data, target, done = td.sequences(kind, folder, **args)
    ds = td.DATASETS[kind].from_folder(folder, **args)
    E, T = done.shape
    assert data.shape == (E, T, ds.input_dim) and target.shape == (E, T, ds.output_dim)
    assert data.dtype == torch.float32 and target.dtype == torch.float32 and done.dtype == torch.bool
    keep = ~done.reshape(-1)
    assert 0 < int(keep.sum()) < E * T
    assert torch.equal(data.reshape(E * T, -1)[keep], ds.data)
    assert torch.equal(target.reshape(E * T, -1)[keep], ds.target)


def test_sequences_refuses_the_horizon_dataset(folder):
    with pytest.raises(ValueError):
        td.sequences("scalar_horizon", folder)


def test_feedback_width():
    assert td.feedback_width("scalar", 1, 1, False, 4) == 1
    assert td.feedback_width("scalar", 1, 1, True, 4) == 1
    assert td.feedback_width("scalar", 3, 2, False, 4) == 1          # the window holds only z and v
    assert td.feedback_width("vector", 1, 1, False, 4) == 4
    assert td.feedback_width("error_dynamics", 1, 1, False, 2) == 2
    for kind, rec in (("vector", False), ("error_dynamics", False), ("scalar", True)):
        with pytest.raises(NotImplementedError):
            td.feedback_width(kind, 2, 1, rec, 4)
    with pytest.raises(ValueError):
        td.feedback_width("scalar_horizon", 1, 1, False, 4)
    with pytest.raises(ValueError):
        td.feedback_width("vector", 1, 1, False, None)


def test_reseed_mask_and_age():
    done = torch.tensor([[0, 0, 1, 0, 0, 0, 0, 0], [0, 0, 0, 0, 0, 0, 0, 1]], dtype=torch.bool)
    r = ev.reseed_mask(done)
    assert r.tolist() == [[1, 0, 0, 1, 0, 0, 0, 0], [1, 0, 0, 0, 0, 0, 0, 0]]
    assert ev.steps_since(r).tolist() == [[0, 1, 2, 0, 1, 2, 3, 4], [0, 1, 2, 3, 4, 5, 6, 7]]
    r3 = ev.reseed_mask(done, 3)
    assert r3.tolist() == [[1, 0, 0, 1, 0, 0, 1, 0], [1, 0, 0, 1, 0, 0, 1, 0]]
    assert ev.steps_since(r3).tolist() == [[0, 1, 2, 0, 1, 2, 0, 1], [0, 1, 2, 0, 1, 2, 0, 1]]


def test_metrics_by_hand():
    # one env, five steps, one output; step 2 is done and not scored
    pred = torch.tensor([[[1.0], [0.5], [9.0], [2.0], [1.0]]])
    target = torch.tensor([[[0.5], [1.0], [0.0], [2.0], [3.0]]])
    done = torch.tensor([[0, 0, 1, 0, 0]], dtype=torch.bool)
    reseed = ev.reseed_mask(done)                                   # 1 0 0 1 0 -> ages 0 1 2 0 1
    m = ev.tube_metrics(pred, target, done, reseed)
    assert m["steps"] == 4 and m["elements"] == 4
    assert m["success_rate"] == 0.5                                 # steps 0 and 3 (equality covers: err >= 0)
    assert m["mean_excess"] == 0.25                                 # (0.5 + 0.0) / 2
    assert m["success_rate_by_age"] == [1.0, 0.0]                   # age 0: steps 0, 3; age 1: steps 1, 4; age 2 is the done step
    assert m["mean_excess_by_age"][0] == 0.25 and math.isnan(m["mean_excess_by_age"][1])
    one = ev.tube_metrics(pred, target, done)
    assert one["success_rate"] == 0.5 and one["success_rate_by_age"] == [0.5]


def test_error_dynamics_metrics_by_hand():
    pred = torch.tensor([[[3.0, 4.0], [0.0, 0.0], [1.0, 1.0]]])
    target = torch.zeros(1, 3, 2)
    done = torch.tensor([[0, 0, 1]], dtype=torch.bool)
    m = ev.tube_metrics(pred, target, done, None, error_dynamics=True)
    assert m["mse"] == 25.0 / 4 and m["mean_error_norm"] == 2.5
    assert m["success_rate"] == 1.0 and m["mean_excess"] == 7.0 / 4
    assert m["mse_by_age"] == [25.0 / 4] and m["mean_error_norm_by_age"] == [2.5]


def test_window_metrics_by_hand():
    pred = torch.tensor([[1.0, 1.0, 1.0], [0.0, 2.0, 0.0]])
    target = torch.tensor([[0.0, 2.0, 1.0], [1.0, 1.0, 1.0]])
    m = ev.window_metrics(pred, target)
    assert m["windows"] == 2 and m["success_rate"] == 0.5 and m["success_rate_by_step"] == [0.5, 0.5, 0.5]
    assert m["mean_excess"] == 2.0 / 3


def test_config_json_round_trip(tmp_path):
    import evaluate_tube
    import train_tube
    a = train_tube.parse_args(["--data", "d", "--dataset", "scalar_horizon", "--H_fwd", "8", "--H_rev", "3", "--loss", "scalar_horizon",
                               "--alpha", "0.9", "--num_units", "48", "--num_layers", "3", "--activation", "softplus",
                               "--softplus_beta", "5.0"])
    cfg = train_tube.run_config(a)
    (tmp_path / tm.CONFIG_NAME).write_text(json.dumps(cfg))
    back = tm.read_config(str(tmp_path))
    assert back == cfg
    for k, v in (("dataset", "scalar_horizon"), ("H_fwd", 8), ("H_rev", 3), ("loss", "scalar_horizon"), ("alpha", 0.9), ("num_units", 48),
                 ("num_layers", 3), ("activation", "softplus"), ("softplus_beta", 5.0), ("N", 1), ("dN", 1), ("recursive", False)):
        assert back[k] == v
    e = evaluate_tube.parse_args(["--run", str(tmp_path), "--data", "d", "--H_rev", "4"])
    got = evaluate_tube.resolve_config(e)
    assert got["H_rev"] == 4 and got["H_fwd"] == 8 and got["activation"] == "softplus"      # a flag replaces the file's value
    empty = tmp_path / "old_run"
    empty.mkdir()
    with pytest.raises(FileNotFoundError, match="config.json"):
        evaluate_tube.resolve_config(evaluate_tube.parse_args(["--run", str(empty), "--data", "d"]))
    with pytest.raises(FileNotFoundError, match="config.json"):
        tm.read_config(str(empty))
    old = evaluate_tube.resolve_config(evaluate_tube.parse_args(["--run", str(empty), "--data", "d", "--dataset", "vector",
                                                                  "--activation", "tanh"]))
    assert old["dataset"] == "vector" and old["activation"] == "tanh" and old["N"] == 1


def test_shape_from_state_dict():
    from legged_gym_dev_amd.tube.trainer import initial_params
    assert tm.shape_from_state_dict(initial_params(7, 3, 48, 4, 0)) == (7, 3, 48, 4)
    with pytest.raises(KeyError):
        tm.shape_from_state_dict({"fc.weight": torch.zeros(2, 2)})
