"""Level-conditioned one-shot tubes, host side (no GPU): the envelope on both sides of the C boundary with
its H_rev >= 1 edge, the input_dim both sides ask of a split, the dataset kind, the item restatement (tests/tube_horizon_level_ref.py)
against ScalarHorizonTubeDataset's recorded items, the horizon_levels calibration, level_crossings and the scripts' flags."""
import ctypes
import os
import pickle
import sys

import numpy as np
import pytest
import torch

from legged_gym_dev_amd.tube import data as td
from tests import tube_horizon_level_ref as hl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")


def _fx(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


def _lib():
    import torch  # noqa: F401
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    lib = ctypes.CDLL(L.SO_PATH)
    lib.lg_last_error.restype = ctypes.c_char_p
    return lib


def _cfg(**over):
    from legged_gym_dev_amd import capi
    base = dict(input_dim=20, output_dim=4, num_units=16, num_layers=1, activation=0, loss=capi.TUBE_LOSS["scalar"], horizon=1,
                batch_size=32, H_fwd=4, H_rev=3, step_size=10, seed=1, alpha=0.0, delta=1.0, softplus_beta=1.0, lr=1e-3, gamma=0.1,
                level_input=1, level_lo=0.0, level_hi=1.0)
    return capi.lg_tube_cfg(**{**base, **over})


@pytest.mark.parametrize("loss", ["scalar_level", "vector_level"])
@pytest.mark.parametrize("shape", [(3, 4, 20), (1, 2, 8), (10, 50, 131)], ids=lambda s: f"Hrev{s[0]}-Hfwd{s[1]}")
def test_both_sides_accept_a_conditioned_horizon_config(loss, shape):
    from legged_gym_dev_amd import capi
    from legged_gym_dev_amd.tube.trainer import LOSSES, check_envelope
    Hr, Hf, I = shape
    lib = _lib()
    c = _cfg(input_dim=I, output_dim=Hf, H_fwd=Hf, H_rev=Hr, loss=capi.TUBE_LOSS[LOSSES[loss]], num_units=128 if I > 100 else 16)
    assert lib.lg_tube_check_cfg(ctypes.byref(c)) == 0, lib.lg_last_error().decode()
    check_envelope(I, Hf, 16, 1, loss=loss, horizon=(Hf, Hr), level_input=True)


@pytest.mark.parametrize("Hf", [1, 4])
def test_both_sides_refuse_a_conditioned_horizon_without_history(Hf):
    from legged_gym_dev_amd.tube.trainer import check_envelope
    lib = _lib()
    assert lib.lg_tube_check_cfg(ctypes.byref(_cfg(H_fwd=Hf, output_dim=Hf, H_rev=0))) == -1
    assert "horizon" in lib.lg_last_error().decode() and "H_rev" in lib.lg_last_error().decode()
    with pytest.raises(ValueError, match="horizon.*H_rev >= 1"):
        check_envelope(20, Hf, 16, 1, loss="scalar_level", horizon=(Hf, 0), level_input=True)
    # the unconditioned horizon handle keeps H_rev = 0, and the mse loss stays refused with a level
    assert lib.lg_tube_check_cfg(ctypes.byref(_cfg(H_fwd=Hf, output_dim=Hf, H_rev=0, level_input=0, level_lo=0.0, level_hi=0.0))) == 0
    assert lib.lg_tube_check_cfg(ctypes.byref(_cfg(loss=2))) == -1 and "mse" in lib.lg_last_error().decode()


def test_window_input_dim_counts_the_level():
    """What set_data and the window queries ask of a split on the Python side; lg_tube_set_data's own refusal needs a handle and
    is checked on the GPU (tests/test_hip_tube_horizon_level.py::test_refusals)."""
    from legged_gym_dev_amd.tube.trainer import check_window_dims, window_input_dim
    assert window_input_dim((4, 3), 2, 2) == 19 and window_input_dim((4, 3), 2, 2, True) == 20
    assert window_input_dim((2, 1), 0, 2, True) == 8 and window_input_dim((50, 10), 0, 2, True) == 131
    check_window_dims(20, (4, 3), 2, 2, True)
    check_window_dims(19, (4, 3), 2, 2, False)
    for I, lv in ((19, True), (21, True), (20, False)):
        with pytest.raises(ValueError, match="input_dim"):
            check_window_dims(I, (4, 3), 2, 2, lv)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    fx = _fx("tube_dataset")
    d = tmp_path_factory.mktemp("rom")
    for k in (0, 1):
        with open(d / f"epoch_{k}.pickle", "wb") as f:
            pickle.dump({key: fx[f"e{k}_{key}"] for key in ("z", "pz_x", "v", "done")}, f)
    return str(d)


def test_dataset_kind(folder):
    assert td.DATASETS["scalar_horizon_level"] is td.LevelScalarHorizonTubeDataset and td.HORIZON_LEVEL_KIND == "scalar_horizon_level"
    assert "scalar_horizon_level" not in td.LEVEL_KINDS and td.HORIZON_KINDS == ("scalar_horizon", "scalar_horizon_level")
    fx = _fx("tube_horizon")
    ds = td.DATASETS["scalar_horizon_level"].from_folder(folder, H_fwd=8, H_rev=3)
    base = td.DATASETS["scalar_horizon"].from_folder(folder, H_fwd=8, H_rev=3)
    for name in ("w", "z", "v"):
        assert torch.equal(getattr(ds, name), torch.from_numpy(fx[name])) and torch.equal(getattr(ds, name), getattr(base, name))
    assert [ds.input_dim, ds.output_dim] == [int(fx["dims"][0]) + 1, int(fx["dims"][1])] == [base.input_dim + 1, 8]
    assert ds.conditioned is True and base.conditioned is False and (ds.H_fwd, ds.H_rev) == (8, 3)
    np.random.seed(3)
    tr, te = ds.random_split(0.8)
    assert type(tr) is type(ds) and tr.input_dim == ds.input_dim and te.conditioned and len(tr) + len(te) == len(ds)
    with pytest.raises(ValueError, match="no per-step rows"):
        td.sequences("scalar_horizon_level", folder)
    with pytest.raises(ValueError, match="no closed loop"):
        td.feedback_layout("scalar_horizon_level", 1, 1, False, 4, 2)


def test_item_restatement_against_the_recorded_items(folder):
    fx = _fx("tube_horizon")
    ds = td.DATASETS["scalar_horizon_level"].from_folder(folder, H_fwd=8, H_rev=3)
    for i, (idx, ind) in enumerate(fx["items"].tolist()):
        for level in (0.0, 0.37, 1.0):
            x, y = hl.item(fx["w"], fx["z"], fx["v"], idx, ind, 8, 3, level)
            assert x.dtype == np.float64 and x.shape == (ds.input_dim,) and y.shape == (8,)
            assert np.array_equal(x[:-1].astype(np.float32), fx[f"x{i}"]) and np.array_equal(x[:-1], fx[f"x{i}"].astype(np.float64))
            assert x[-1] == level and np.array_equal(y.astype(np.float32), fx[f"y{i}"])
            hx, hy = ds._get_item_helper(idx, ind)
            assert np.array_equal(x[:-1], hx.double().numpy()) and np.array_equal(y, hy.double().numpy())
        xs, ys = hl.items(ds, [idx, idx], [ind, ind], [0.2, 0.9])
        assert torch.equal(xs[0, :-1], xs[1, :-1]) and xs[:, -1].tolist() == [0.2, 0.9] and torch.equal(ys[0], ys[1])
    x, _ = hl.item(fx["w"], fx["z"], fx["v"], 0, 3, 8, 3)
    assert x.shape == (ds.input_dim - 1,)


def _calibration():
    from legged_gym_dev_amd.tube.calibrate import Calibration
    off = torch.tensor([[0.1, 0.2, 0.3], [0.4, float("inf"), 0.6]])
    return Calibration("horizon_levels", [0.5, 0.9], off, 17, [9, 17], {"run": "/x", "dataset": "scalar_horizon_level", "window_stride": 2})


def test_horizon_levels_calibration_round_trip(tmp_path):
    from legged_gym_dev_amd.tube.calibrate import Calibration
    c = _calibration()
    path = str(tmp_path / "calibration.json")
    c.save(path)
    assert "Infinity" not in open(path).read()
    d = Calibration.load(path)
    assert d.kind == "horizon_levels" and d.coverages == [0.5, 0.9] and d.n == 17 and d.ranks == [9, 17]
    assert torch.equal(d.offsets, c.offsets) and d.provenance == c.provenance and d.to_json()["parts"] is None
    fw, w = torch.zeros(7, 3), torch.full((7, 3), 0.25)
    assert d.apply(fw, level=0.5).shape == (7, 3) and torch.equal(d.apply(fw, level=0.5)[0], torch.tensor([0.1, 0.2, 0.3]))
    assert d.covers(fw, w, level=0.5).shape == (7, 3) and d.covers(fw, w, level=0.5)[0].tolist() == [False, False, True]
    assert d.covers(fw, w, level=0.9)[0].tolist() == [True, True, True]
    assert torch.equal(d.offset(level=0.9), d.offset(0.9)) and torch.equal(d.offset(0.9, level=0.9), c.offsets[1])
    with pytest.raises(KeyError, match="was not calibrated"):
        d.offset(level=0.7)
    with pytest.raises(ValueError, match="calibrated to coverage"):
        d.offset(0.5, level=0.9)
    with pytest.raises(ValueError, match="needs the level"):
        d.offset()
    assert len(d.lines()) == 6 and d.lines()[4] == "level 0.9, step ahead 2: rank 17 of n 17, offset inf"
    with pytest.raises(ValueError, match="do not fit"):
        Calibration("horizon_levels", [0.5, 0.9], torch.zeros(3, 4), 5, [3, 5])
    with pytest.raises(ValueError, match="NaN offset in set level 0.5, step ahead 2"):
        Calibration("horizon_levels", [0.5], torch.tensor([[0.0, float("nan")]]), 5, [3])
    # the other kinds are what they were
    h = Calibration("horizon", [0.9], torch.zeros(1, 3), 5, [5])
    with pytest.raises(ValueError, match="has no levels"):
        h.offset(0.9, level=0.9)
    assert h.to_json()["parts"] is None and Calibration("flat", [0.9], torch.zeros(2, 1, 1), 5, [5]).to_json()["parts"] == ["one_step", "rollout"]


def test_level_crossings():
    from legged_gym_dev_amd.tube.evaluate import level_crossings
    p = torch.tensor([[[1.0, 1.0], [2.0, 0.5], [3.0, 0.5]]])                  # (1 window, 3 levels, 2 steps)
    assert level_crossings(p, [0.1, 0.5, 0.9]) == 0.25                       # step 1 falls once over two pairs; a tie is no fall
    assert level_crossings(p[:, [2, 0, 1]], [0.9, 0.1, 0.5]) == 0.25         # the levels' order does not matter
    assert level_crossings(p.flip(1), [0.1, 0.5, 0.9]) == 0.5
    assert np.isnan(level_crossings(p[:, :1], [0.5]))


def test_script_flags(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
    import calibrate_tube
    import evaluate_tube
    import train_tube
    a = train_tube.parse_args(["--data", "d", "--dataset", "scalar_horizon_level", "--H_fwd", "4", "--H_rev", "3", "--level_hi", "0.99",
                               "--sweep", "seed=1,2"])
    assert (a.loss, a.level_input, a.level_lo, a.level_hi) == ("scalar_level", True, 0.0, 0.99)
    cfg = train_tube.run_config(a)
    assert cfg["dataset"] == "scalar_horizon_level" and cfg["level_input"] is True and (cfg["H_fwd"], cfg["H_rev"]) == (4, 3)
    a = train_tube.parse_args(["--data", "d", "--dataset", "scalar_horizon_level", "--loss", "vector_level"])
    assert a.loss == "vector_level"
    with pytest.raises(SystemExit):
        train_tube.parse_args(["--data", "d", "--dataset", "scalar_horizon_level", "--loss", "error"])
    with pytest.raises(SystemExit):
        train_tube.parse_args(["--data", "d", "--dataset", "scalar_horizon", "--level_lo", "0.2"])
    assert "level_input" not in train_tube.run_config(train_tube.parse_args(["--data", "d", "--dataset", "scalar_horizon"]))
    run = {"dataset": "scalar_horizon_level"}
    ca = calibrate_tube.parse_args(["--run", "r", "--sim", "--levels", "0.5,0.9"])
    assert calibrate_tube.check_kind(run, ca) == [0.5, 0.9]
    with pytest.raises(ValueError, match="--levels, not --coverage"):
        calibrate_tube.check_kind(run, calibrate_tube.parse_args(["--run", "r", "--sim", "--coverage", "0.9"]))
    with pytest.raises(ValueError, match="one shot"):
        calibrate_tube.check_by_age(run, calibrate_tube.parse_args(["--run", "r", "--sim", "--by_age"]))
    path = str(tmp_path / "calibration.json")
    _calibration().save(path)
    ea = evaluate_tube.parse_args(["--run", "r", "--sim", "--calibration", path])
    assert evaluate_tube.load_calibration(ea, run, None).kind == "horizon_levels"
    with pytest.raises(ValueError, match="the run is scalar_horizon"):
        evaluate_tube.load_calibration(ea, {"dataset": "scalar_horizon"}, None)
