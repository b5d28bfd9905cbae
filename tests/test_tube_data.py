"""Tube-learning host side (legged_gym_dev_amd/tube): datasets and construct_dataset against fixtures recorded from the
reference's deep_tube_learning/datasets.py (tools/gen_fixtures_tube.py), random_split, the loss restatement against the
reference losses, the state-dict layout, and every refusal of the supported envelope.  No GPU needed."""
import ctypes
import os
import pickle

import numpy as np
import pytest
import torch

from legged_gym_dev_amd.tube import data as td
from tests import tube_ref

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _fx(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """The fixture's synthetic epochs written as collect_trajectory_data.py writes them; epoch 10 and 2 on top so that glob
    order and numeric order differ."""
    fx = _fx("tube_dataset")
    d = tmp_path_factory.mktemp("rom")
    for k in (0, 1):
        with open(d / f"epoch_{k}.pickle", "wb") as f:
            pickle.dump({key: fx[f"e{k}_{key}"] for key in ("z", "pz_x", "v", "done")}, f)
    return str(d)


def test_construct_dataset_matches_reference(folder):
    fx = _fx("tube_dataset")
    ds = td.construct_dataset(folder)
    assert sorted(ds) == sorted(k[3:] for k in fx if k.startswith("cd_"))
    for k, v in ds.items():
        np.testing.assert_array_equal(v, fx["cd_" + k], err_msg=k)
        assert v.dtype == fx["cd_" + k].dtype
    # the reference's done[-1, :] = True: every step of the last env of each epoch, not the last step of every env
    N = fx["e0_done"].shape[0]
    assert ds["done"][N - 1].all() and ds["done"][2 * N - 1].all()
    assert not ds["done"][:, -1].all()
    assert not os.path.exists(os.path.join(folder, "dataset.pickle"))      # no cache written


def test_construct_dataset_numeric_epoch_order(tmp_path):
    for k in (10, 2, 0):
        rec = {"z": np.full((1, 3, 2), k, np.float32), "pz_x": np.zeros((1, 3, 2), np.float32),
               "v": np.zeros((1, 2, 2), np.float32), "done": np.zeros((1, 2), bool)}
        with open(tmp_path / f"epoch_{k}.pickle", "wb") as f:
            pickle.dump(rec, f)
    ds = td.construct_dataset(str(tmp_path))
    assert ds["z"][:, 0, 0].tolist() == [0, 2, 10]


@pytest.mark.parametrize("case", ["scalar_n1", "scalar_n3", "scalar_n3_rec", "vector_n2", "error_n2"])
def test_row_datasets_match_reference(folder, case):
    fx = _fx("tube_rows")
    make = {"scalar_n1": lambda s: td.ScalarTubeDataset.from_folder(s, N=1, dN=1),
            "scalar_n3": lambda s: td.ScalarTubeDataset.from_folder(s, N=3, dN=1, recursive=False),
            "scalar_n3_rec": lambda s: td.ScalarTubeDataset.from_folder(s, N=3, dN=1, recursive=True),
            "vector_n2": lambda s: td.VectorTubeDataset.from_folder(s, N=2, dN=2),
            "error_n2": lambda s: td.ErrorDynamicsDataset.from_folder(s, N=2, dN=1)}[case]
    ds = make(folder)
    np.testing.assert_array_equal(ds.data.numpy(), fx[case + "_data"])
    np.testing.assert_array_equal(ds.target.numpy(), fx[case + "_target"])
    assert [ds.input_dim, ds.output_dim] == fx[case + "_dims"].tolist()
    assert ds.data.dtype == torch.float32 and ds.target.dtype == torch.float32


def test_horizon_dataset_matches_reference(folder):
    fx = _fx("tube_horizon")
    ds = td.ScalarHorizonTubeDataset.from_folder(folder, H_fwd=8, H_rev=3)
    for k in ("w", "z", "v"):
        np.testing.assert_array_equal(getattr(ds, k).numpy(), fx[k], err_msg=k)
    assert [ds.input_dim, ds.output_dim] == fx["dims"].tolist()
    for i, (idx, ind) in enumerate(fx["items"]):
        x, y = ds._get_item_helper(int(idx), int(ind))
        np.testing.assert_array_equal(x.numpy(), fx[f"x{i}"])
        np.testing.assert_array_equal(y.numpy(), fx[f"y{i}"])
    torch.manual_seed(0)
    for _ in range(20):
        x, y = ds[3]
        assert x.shape == (ds.input_dim,) and y.shape == (ds.output_dim,)


def test_random_split_is_one_contiguous_train_piece():
    data = torch.arange(50, dtype=torch.float32).reshape(25, 2)
    ds = td.ScalarTubeDataset(data, data[:, :1].clone(), 2, 1)
    np.random.seed(5)
    tr, te = ds.random_split(0.8)
    np.random.seed(5)
    s = np.random.randint(25 - 20)
    assert len(tr) == 20 and len(te) == 5 and type(tr) is td.ScalarTubeDataset
    assert torch.equal(tr.data, data[s:s + 20])
    assert torch.equal(te.data, torch.vstack((data[:s], data[s + 20:])))
    assert torch.equal(te.target, torch.vstack((data[:s, :1], data[s + 20:, :1])))
    w = torch.arange(10, dtype=torch.float32)[:, None].repeat(1, 30)
    hz = td.ScalarHorizonTubeDataset(w, torch.zeros(10, 30, 0), torch.zeros(10, 30, 2), 5, 2, 2 + 14, 5)
    np.random.seed(1)
    a, b = hz.random_split(0.5)
    np.random.seed(1)
    s = np.random.randint(5)
    assert torch.equal(a.w[:, 0], torch.arange(s, s + 5, dtype=torch.float32)) and len(b) == 5


@pytest.mark.parametrize("name", ["scalar", "scalar_horizon", "vector", "error"])
def test_loss_restatement_matches_reference(name):
    fx = _fx("tube_losses")
    fw = torch.from_numpy(fx["fw"]).requires_grad_(True)
    val = tube_ref.loss(name, fw, torch.from_numpy(fx["w"]), float(fx["alpha"]), float(fx["delta"]))
    val.backward()
    np.testing.assert_array_equal(val.detach().numpy(), fx[f"{name}_value"])
    np.testing.assert_array_equal(fw.grad.numpy(), fx[f"{name}_grad"])
    if name != "error":
        assert (fx[f"{name}_grad"][0] == 0).all()               # r = 0 takes the |r| branch, gradient 0


def test_state_dict_layout_matches_reference_mlp():
    from legged_gym_dev_amd.tube import trainer as tt
    sd = tt.initial_params(7, 3, 32, 3, seed=4)
    torch.manual_seed(4)
    ref = tube_ref.MLP(7, 3, 32, 3, "relu")
    assert list(sd) == list(ref.state_dict())
    for k, v in ref.state_dict().items():
        assert torch.equal(sd[k], v), k
    assert [s for _, s in tt.param_shapes(7, 3, 32, 3)] == [tuple(v.shape) for v in ref.state_dict().values()]
    ref.load_state_dict(sd)


def test_refusals():
    from legged_gym_dev_amd.tube import trainer as tt
    for cls in (td.AlphaScalarTubeDataset, td.AlphaVectorTubeDataset):
        with pytest.raises(NotImplementedError, match="broadcasts"):
            cls.from_folder("x")
        with pytest.raises(NotImplementedError, match="broadcasts"):
            cls(None, None, 1, 1)
    with pytest.raises(NotImplementedError, match="final_activation"):
        tt.check_envelope(3, 1, 32, 2, "relu", final_activation=torch.nn.Softplus())
    tt.check_envelope(130, 50, 128, 4, "softplus")
    for bad in [dict(num_units=8), dict(num_units=136), dict(num_units=40), dict(num_layers=0), dict(num_layers=5),
                dict(input_dim=257), dict(input_dim=0), dict(output_dim=65), dict(activation="gelu")]:
        kw = dict(input_dim=3, output_dim=1, num_units=32, num_layers=2, activation="relu")
        kw.update(bad)
        with pytest.raises(ValueError):
            tt.check_envelope(**kw)


def test_c_side_refuses_the_same_envelope():
    """lg_tube_check_cfg (what lg_tube_create runs first) needs no GPU."""
    from legged_gym_dev_amd import capi
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    lib = ctypes.CDLL(L.SO_PATH)
    capi.declare_tube_api(lib)
    lib.lg_last_error.restype = ctypes.c_char_p

    def cfg(**kw):
        c = dict(input_dim=3, output_dim=1, num_units=32, num_layers=2, activation=0, loss=0, horizon=0, batch_size=2048,
                 H_fwd=0, H_rev=0, step_size=10, seed=1, alpha=0.8, delta=1.0, softplus_beta=1.0, lr=1e-3, gamma=0.1)
        c.update(kw)
        return capi.lg_tube_cfg(**c)
    assert lib.lg_tube_check_cfg(ctypes.byref(cfg())) == 0
    assert lib.lg_tube_check_cfg(ctypes.byref(cfg(input_dim=256, output_dim=64, num_units=128, num_layers=4))) == 0
    for bad in [dict(num_units=8), dict(num_units=144), dict(num_units=40), dict(num_layers=0), dict(num_layers=5),
                dict(input_dim=257), dict(output_dim=65), dict(activation=4), dict(loss=3),
                dict(horizon=1, H_fwd=8, output_dim=5)]:
        assert lib.lg_tube_check_cfg(ctypes.byref(cfg(**bad))) == -1, bad
        assert lib.lg_last_error().decode().startswith("lg_tube:")
