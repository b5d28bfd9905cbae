"""The device dataset builder, host side (no GPU): the closed-form row rule (tests/tube_rows_ref.py, what csrc/tube_data_kernels.hip
implements) against tube/data.py and the reference-made rows of tests/golden/tube_rows.npz; lg_tube_rows_check / lg_tube_rows_dims,
which are host code; and train_tube.py's --data / --sim command line."""
import ctypes
import os
import sys

import numpy as np
import pytest

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.tube import data as td
from tests import tube_rows_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))

# case of tube_rows.npz -> (kind, N, dN, recursive)
CASES = {"scalar_n1": ("scalar", 1, 1, False), "scalar_n3": ("scalar", 3, 1, False), "scalar_n3_rec": ("scalar", 3, 1, True),
         "vector_n2": ("vector", 2, 2, False), "error_n2": ("error_dynamics", 2, 1, False)}


def _fx(name):
    return dict(np.load(os.path.join(GOLD, name + ".npz")))


@pytest.fixture(scope="module")
def cd():
    fx = _fx("tube_dataset")
    return {k[3:]: v for k, v in fx.items() if k.startswith("cd_")}


def _host(kind, cd, N, dN, recursive):
    kw = dict(N=N, dN=dN, **({"recursive": recursive} if kind == "scalar" else {}))
    return td.DATASETS[kind].from_folder(cd, **kw), td.sequences(kind, cd, **kw)


@pytest.mark.parametrize("case", sorted(CASES))
def test_closed_form_equals_data_py_and_the_reference_rows(cd, case):
    kind, N, dN, rec = CASES[case]
    fx = _fx("tube_rows")
    ds, (sd, st, _) = _host(kind, cd, N, dN, rec)
    data, target = ref.sequences(kind, cd["z"], cd["pz_x"], cd["v"], N, dN, rec)
    assert np.array_equal(data, sd.numpy()) and np.array_equal(target, st.numpy())
    x, y = ref.rows(kind, cd, N, dN, rec)
    assert np.array_equal(x, ds.data.numpy()) and np.array_equal(y, ds.target.numpy())
    assert np.array_equal(x, fx[case + "_data"]) and np.array_equal(y, fx[case + "_target"])
    assert x.shape[0] == 376
    assert list(ref.dims(kind, N, rec, cd["z"].shape[2], cd["v"].shape[2])) == fx[case + "_dims"].tolist()


def test_mark_last_env_is_construct_datasets_quirk(cd):
    fx = _fx("tube_dataset")
    raw = {k: np.concatenate([fx[f"e{e}_{k}"] for e in (0, 1)], axis=0) for k in ("z", "pz_x", "v", "done")}
    assert raw["done"].shape[0] == 12
    assert np.array_equal(ref.keep_mask(raw["done"], True, 6), np.logical_not(cd["done"]))
    x, _ = ref.rows("scalar", raw, mark_last_env=True, epoch_envs=6)
    assert np.array_equal(x, _fx("tube_rows")["scalar_n1_data"])


@pytest.mark.parametrize("T", [1, 2, 5, 7])
@pytest.mark.parametrize("N,dN", [(1, 1), (3, 1), (3, 2), (10, 3)])
def test_closed_form_on_short_episodes_and_wide_state(T, N, dN):
    """n = 3, m = 1 and windows longer than the episode (every delayed block padding)."""
    rng = np.random.default_rng(T * 100 + N * 10 + dN)
    E = 3
    rec = {"z": rng.standard_normal((E, T + 1, 3)).astype(np.float32), "pz_x": rng.standard_normal((E, T + 1, 3)).astype(np.float32),
           "v": rng.standard_normal((E, T, 1)).astype(np.float32), "done": rng.random((E, T)) < 0.3}
    rec["z_p1"], rec["pz_x_p1"] = rec["z"][:, 1:], rec["pz_x"][:, 1:]
    for kind, recursive in (("scalar", False), ("scalar", True), ("vector", False), ("error_dynamics", False)):
        ds, _ = _host(kind, rec, N, dN, recursive)
        x, y = ref.rows(kind, rec, N, dN, recursive)
        assert np.array_equal(x, ds.data.numpy()) and np.array_equal(y, ds.target.numpy()), (kind, recursive)


def test_horizon_restatement(cd):
    for H in (0, 1, 10):
        ds = td.ScalarHorizonTubeDataset.from_folder(cd, H_fwd=4, H_rev=H)
        for got, want in zip(ref.horizon(cd, H), (ds.w, ds.z, ds.v)):
            assert np.array_equal(got, want.numpy())


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    lib = ctypes.CDLL(L.SO_PATH)
    capi.declare_tube_data_api(lib)
    lib.lg_last_error.restype = ctypes.c_char_p
    return lib


def _spec(**kw):
    s = dict(kind=0, N=1, dN=1, recursive=0, n=2, m=2, T=20, n_env=12, compact=1, mark_last_env=1, epoch_envs=6)
    s.update(kw)
    return capi.lg_tube_rows_spec(**s)


def test_c_side_dims_equal_the_dataset_classes(lib, cd):
    def dims(**kw):
        i, o = ctypes.c_int32(), ctypes.c_int32()
        assert lib.lg_tube_rows_dims(ctypes.byref(_spec(**kw)), ctypes.byref(i), ctypes.byref(o)) == 0, lib.lg_last_error()
        return i.value, o.value
    rng = np.random.default_rng(0)
    wide = {"z": rng.standard_normal((2, 6, 3)).astype(np.float32), "pz_x": rng.standard_normal((2, 6, 3)).astype(np.float32),
            "v": rng.standard_normal((2, 5, 1)).astype(np.float32), "done": np.zeros((2, 5), bool)}
    wide["z_p1"], wide["pz_x_p1"] = wide["z"][:, 1:], wide["pz_x"][:, 1:]
    for rec, n, m in ((cd, 2, 2), (wide, 3, 1)):
        for kind, N, dN, recursive in CASES.values():
            ds, _ = _host(kind, rec, N, dN, recursive)
            got = dims(kind=capi.TUBE_ROWS_KIND[kind], N=N, dN=dN, recursive=int(recursive), n=n, m=m)
            assert got == (ds.input_dim, ds.output_dim), (kind, N, dN, recursive, n, m)
    assert dims(kind=2, N=32, n=3, m=2) == (256, 3)                     # the edge of the model envelope
    assert lib.lg_tube_rows_workspace(ctypes.byref(_spec(compact=0))) == 0
    assert lib.lg_tube_rows_workspace(ctypes.byref(_spec(T=65))) == 12 * 2 * 12      # 2 chunks per env: int64 offset + int32 count


@pytest.mark.parametrize("bad,field", [
    (dict(kind=3), "kind"), (dict(kind=-1), "kind"), (dict(n=1), "n "), (dict(n=7), "n "), (dict(m=0), "m "), (dict(m=5), "m "),
    (dict(N=0), "N "), (dict(dN=0), "dN"), (dict(recursive=2), "recursive"), (dict(kind=1, recursive=1), "recursive"), (dict(T=0), "T "),
    (dict(n_env=0), "n_env"), (dict(compact=2), "compact"), (dict(mark_last_env=-1), "mark_last_env"), (dict(epoch_envs=0), "epoch_envs"),
    (dict(epoch_envs=5), "epoch_envs"), (dict(kind=2, N=33, n=3, m=2), "input_dim"), (dict(n_env=1 << 30, T=64, epoch_envs=1), "n_env x T")])
def test_c_side_refuses_outside_the_envelope_naming_the_field(lib, bad, field):
    assert lib.lg_tube_rows_check(ctypes.byref(_spec())) == 0
    i, o = ctypes.c_int32(), ctypes.c_int32()
    for rc in (lib.lg_tube_rows_check(ctypes.byref(_spec(**bad))), lib.lg_tube_rows_dims(ctypes.byref(_spec(**bad)), ctypes.byref(i), ctypes.byref(o)),
               lib.lg_tube_rows_workspace(ctypes.byref(_spec(**bad)))):
        assert rc == -1, bad
        msg = lib.lg_last_error().decode()
        assert msg.startswith("lg_tube_rows: ") and field in msg, (bad, msg)


def test_horizon_build_refusals_need_no_gpu(lib):
    one = ctypes.c_void_p(8)            # never read: every call below is refused before a launch
    for bad, field in ((dict(n=1), "n "), (dict(m=5), "m "), (dict(T=0), "T "), (dict(H=-1), "H_rev"), (dict(n_env=0), "n_env")):
        a = dict(n_env=4, T=8, n=2, m=2, H=3)
        a.update(bad)
        assert lib.lg_tube_horizon_build(one, one, one, a["n_env"], a["T"], a["n"], a["m"], a["H"], one, one, one, None) == -1
        assert field in lib.lg_last_error().decode()


def test_train_tube_command_line():
    import train_tube
    before = ['H_fwd', 'H_rev', 'N', 'activation', 'alpha', 'batch_size', 'dN', 'data', 'dataset', 'delta', 'device', 'gamma', 'loss', 'lr',
              'num_epochs', 'num_layers', 'num_units', 'out', 'recursive', 'seed', 'softplus_beta', 'step_size',
              'steps_per_model_checkpoint', 'steps_per_model_evaluation', 'sweep', 'validation_split']
    a = train_tube.parse_args(["--data", "folder"])
    assert sorted(vars(a)) == before and a.data == "folder"
    assert "sim" not in train_tube.run_config(a)
    s = train_tube.parse_args(["--sim"])
    assert s.sim is True and s.data is None
    assert (s.sim_envs, s.sim_T, s.sim_seed, s.sim_resident, s.sim_refresh) == (8192, None, 0, 1, 1)
    cfg = train_tube.run_config(train_tube.parse_args(["--sim", "--sim_envs", "64", "--sim_T", "20", "--sim_refresh", "0", "--sim_resident", "2"]))
    assert {k: cfg[k] for k in ("sim", "sim_envs", "sim_T", "sim_seed", "sim_resident", "sim_refresh")} == \
        {"sim": True, "sim_envs": 64, "sim_T": 20, "sim_seed": 0, "sim_resident": 2, "sim_refresh": 0}
    s = train_tube.parse_args(["--sim", "--dataset", "scalar_level", "--sweep", "seed=1,2"])
    assert s.level_input and s.sweep == [("seed", [1, 2])]
    for bad in ([], ["--data", "folder", "--sim"], ["--data", "folder", "--sim_envs", "8"], ["--sim", "--sim_envs", "1"]):
        with pytest.raises(SystemExit):
            train_tube.parse_args(bad)


def test_evaluate_tube_command_line():
    import evaluate_tube
    a = evaluate_tube.parse_args(["--run", "r", "--sim"])
    assert a.sim and a.data is None
    f = evaluate_tube.sim_flags(a, {"seed": 1, "sim_seed": 2, "sim_envs": 64, "sim_T": 20})
    assert f == {"sim_envs": 64, "sim_T": 20, "sim_resident": 1, "sim_seed": 3}          # a seed the run did not train with
    assert evaluate_tube.sim_flags(a, {"seed": 42})["sim_seed"] == 1
    assert evaluate_tube.parse_args(["--run", "r", "--data", "d"]).sim is False
    for bad in (["--run", "r"], ["--run", "r", "--data", "d", "--sim"]):
        with pytest.raises(SystemExit):
            evaluate_tube.parse_args(bad)
