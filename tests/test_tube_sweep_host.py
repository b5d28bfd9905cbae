"""train_tube.py --sweep on the host: parsing, the cartesian product and the member folder names, the refusals by name, and the
unchanged configuration of a run without the flag."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))


def test_sweep_flags_parse_by_field_type():
    import train_tube
    a = train_tube.parse_args(["--data", "d", "--sweep", "alpha=0.8,0.95", "--sweep", "seed=1,2", "--sweep", "activation=relu,tanh",
                               "--sweep", "step_size=100"])
    assert a.sweep == [("alpha", [0.8, 0.95]), ("seed", [1, 2]), ("activation", ["relu", "tanh"]), ("step_size", [100])]
    assert all(isinstance(v, int) for v in a.sweep[1][1]) and all(isinstance(v, float) for v in a.sweep[0][1])
    assert set(train_tube.SWEEP_FIELDS) == {"alpha", "delta", "activation", "softplus_beta", "lr", "gamma", "step_size", "seed"}


def test_members_are_the_cartesian_product_first_flag_slowest():
    import train_tube
    members = train_tube.sweep_members(train_tube.parse_sweep(["alpha=0.8,0.95", "seed=1,2"]))
    assert [name for name, _ in members] == ["alpha=0.8,seed=1", "alpha=0.8,seed=2", "alpha=0.95,seed=1", "alpha=0.95,seed=2"]
    assert [m for _, m in members] == [{"alpha": 0.8, "seed": 1}, {"alpha": 0.8, "seed": 2}, {"alpha": 0.95, "seed": 1},
                                       {"alpha": 0.95, "seed": 2}]
    one = train_tube.sweep_members(train_tube.parse_sweep(["lr=0.001,0.01,0.1"]))
    assert [name for name, _ in one] == ["lr=0.001", "lr=0.01", "lr=0.1"]
    assert len(train_tube.sweep_members(train_tube.parse_sweep(["alpha=0.7,0.8,0.9", "delta=0.5,1.0", "seed=1,2"]))) == 12


@pytest.mark.parametrize("flag, word", [("units=16,32", "units"), ("num_units=16,32", "share num_units"), ("batch_size=64,128", "share batch_size"),
                                        ("loss=scalar,vector", "share loss"), ("alpha", "alpha=v1,v2"), ("alpha=0.8,,0.9", "alpha=v1,v2"),
                                        ("seed=1.5", "int"), ("activation=relu,gelu", "activation is one of"),
                                        ("alpha=0.8,0.8", "repeated")])
def test_bad_sweep_flags_are_refused_by_name(flag, word):
    import train_tube
    with pytest.raises(ValueError, match=word):
        train_tube.parse_sweep([flag])
    with pytest.raises(SystemExit):
        train_tube.parse_args(["--data", "d", "--sweep", flag])


def test_an_axis_given_twice_is_refused():
    import train_tube
    with pytest.raises(ValueError, match="alpha: given twice"):
        train_tube.parse_sweep(["alpha=0.8", "alpha=0.9"])


def test_without_the_flag_the_configuration_is_todays():
    import train_tube
    argv = ["--data", "d", "--dataset", "vector", "--N", "3", "--loss", "vector", "--alpha", "0.9", "--num_units", "64", "--seed", "7"]
    a = train_tube.parse_args(argv)
    assert a.sweep is None
    got = dict(vars(a))
    got.pop("sweep")
    # the flags and defaults of the script before --sweep existed
    assert got == {"data": "d", "dataset": "vector", "N": 3, "dN": 1, "recursive": False, "H_fwd": 50, "H_rev": 10, "loss": "vector",
                   "alpha": 0.9, "delta": 1.0, "num_units": 64, "num_layers": 2, "activation": "relu", "softplus_beta": 1.0,
                   "batch_size": 2048, "num_epochs": 10, "validation_split": 0.8, "lr": 1e-3, "gamma": 0.1, "step_size": 10000,
                   "seed": 7, "steps_per_model_checkpoint": 1000, "steps_per_model_evaluation": 100, "out": "tube_runs/run",
                   "device": "cuda:0"}
    assert train_tube.run_config(a) == {"dataset": "vector", "N": 3, "dN": 1, "recursive": False, "H_fwd": 50, "H_rev": 10,
                                        "loss": "vector", "alpha": 0.9, "delta": 1.0, "num_units": 64, "num_layers": 2,
                                        "activation": "relu", "softplus_beta": 1.0, "seed": 7, "validation_split": 0.8}
