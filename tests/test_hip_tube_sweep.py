"""HipTubeSweep (k_tube_rows_sweep / k_tube_adam_sweep; lg_tube_sweep_*): member k of a sweep is, bit for bit, the single
HipTubeTrainer built from member k's configuration and given the same calls -- on every loss and activation path, the horizon
dataset, a tail step, explicit rows, K = 1 and K = LG_TUBE_SWEEP_MAX -- plus run-to-run determinism, the hand-over to
HipTubeModel, the refusals, and train_tube.py --sweep -> evaluate_tube.py end to end.  Both run on one host path (TubeTrainer in
tube_api.hip); test_regrown_buffers_reach_the_kernels says that the kernels see every buffer that set_data regrew, through the
host copy with one member and through the device copy of the member array with K.

Every comparison is on the bits (floats viewed as int32), so a nan in an eval vector compares like any other value.
"""
import json
import os
import pickle
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Flat:
    def __init__(self, x, y):
        self.data, self.target = x, y


class _Horizon:
    def __init__(self, w, z, v, H_fwd, H_rev):
        self.w, self.z, self.v, self.H_fwd, self.H_rev = w, z, v, H_fwd, H_rev


def _flat_data(I, O, n_train=70, n_test=33, seed=0):
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(n_train + n_test, I, generator=g), torch.rand(n_train + n_test, O, generator=g) * 2
    return _Flat(x[:n_train], y[:n_train]), _Flat(x[n_train:], y[n_train:])


def _sweep(I, O, members, **shared):
    from legged_gym_dev_amd.tube.sweep import HipTubeSweep
    return HipTubeSweep(I, O, members=members, device=DEV, **shared)


def _single(I, O, member, **shared):
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    return HipTubeTrainer(I, O, device=DEV, **{**shared, **member})


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _assert_member_is_single(sw, k, tr, steps, ev_sweep=None, ev_single=None, starts=None):
    for name in ("params", "adam_m", "adam_v", "grads"):
        _same(getattr(sw, name)[k], getattr(tr, name), f"member {k}: {name}")
    if tr.perm is not None:
        _same(sw.perm[k], tr.perm, f"member {k}: perm")
    _same(sw.read_log(k, 1, steps), tr.read_log(1, steps), f"member {k}: log")
    if ev_sweep is not None:
        _same(ev_sweep[k], ev_single, f"member {k}: eval")
    if starts is not None:
        _same(sw.starts[k][:starts], tr.starts[:starts], f"member {k}: starts")


def _epochs(obj, n, batch, steps):
    """`steps` steps through the epochs 0, 1, ... of n rows: full batches and the tail."""
    done, epoch = 0, 0
    while done < steps:
        obj.begin_epoch(epoch)
        for b in range(0, n, batch):
            if done == steps:
                break
            obj.step(min(batch, n - b))
            done += 1
        epoch += 1


def _check_against_singles(I, O, members, shared, train, test, steps, horizon_rows=None):
    sw = _sweep(I, O, members, **shared)
    singles = [_single(I, O, m, **shared) for m in members]
    n = (train.w if horizon_rows else train.data).shape[0]
    try:
        for obj in [sw] + singles:
            obj.set_data(train, test)
            _epochs(obj, n, shared["batch_size"], steps)
        torch.cuda.synchronize()
        if horizon_rows:                                              # the window starts of the last step, before the eval redraws them
            for k, tr in enumerate(singles):
                _same(sw.starts[k][:horizon_rows], tr.starts[:horizon_rows], f"member {k}: starts of the last step")
        ev = sw.evaluate()
        assert tuple(ev.shape) == (len(members), 4)
        for k, tr in enumerate(singles):
            _assert_member_is_single(sw, k, tr, steps, ev, tr.evaluate(), starts=test.w.shape[0] if horizon_rows else None)
    finally:
        for obj in [sw] + singles:
            obj.close()


MEMBERS3 = [dict(alpha=0.8, lr=1e-3, delta=1.0, seed=3), dict(alpha=0.9, lr=3e-3, delta=0.5, seed=4),
            dict(alpha=0.95, lr=1e-2, delta=0.25, seed=5)]


def test_bit_equal_to_single_runs():
    """3 -> 32 x 2 ReLU -> 1, scalar loss; 70 rows at batch 64: a two-tile step and a 6-row tail per epoch, 2 epochs."""
    train, test = _flat_data(3, 1)
    shared = dict(num_units=32, num_layers=2, activation="relu", loss="scalar", batch_size=64, gamma=0.5, step_size=3)
    _check_against_singles(3, 1, MEMBERS3, shared, train, test, steps=4)


PATHS = {
    "vector-tanh": (6, 2, dict(num_units=48, num_layers=4, activation="tanh", loss="vector", batch_size=64), MEMBERS3),
    "mse-elu": (6, 2, dict(num_units=16, num_layers=1, activation="elu", loss="error", batch_size=64), MEMBERS3),
    "mixed-activations": (6, 2, dict(num_units=32, num_layers=2, loss="scalar", batch_size=64),
                          [dict(activation="relu", alpha=0.8, seed=1), dict(activation="softplus", softplus_beta=5.0, alpha=0.9, seed=2),
                           dict(activation="tanh", alpha=0.7, seed=3)]),
}


@pytest.mark.parametrize("path", sorted(PATHS))
def test_every_loss_and_activation_path(path):
    I, O, shared, members = PATHS[path]
    train, test = _flat_data(I, O, seed=len(path))
    _check_against_singles(I, O, members, shared, train, test, steps=3)


def test_horizon_dataset():
    """H_fwd 4, H_rev 2, nz 2, m 2: 16 inputs, 4 outputs; T = 12 leaves 5 window starts; 40 envs at batch 32."""
    Hf, Hr, T = 4, 2, 12
    g = torch.Generator().manual_seed(7)
    w, z, v = torch.rand(60, T, generator=g), torch.randn(60, T, 2, generator=g), torch.randn(60, T, 2, generator=g)
    train, test = _Horizon(w[:40], z[:40], v[:40], Hf, Hr), _Horizon(w[40:], z[40:], v[40:], Hf, Hr)
    shared = dict(num_units=128, num_layers=2, activation="softplus", softplus_beta=5.0, loss="scalar_horizon", batch_size=32,
                  horizon=(Hf, Hr))
    _check_against_singles(Hr + 2 + (Hr + Hf) * 2, Hf, MEMBERS3, shared, train, test, steps=3, horizon_rows=32)


def test_step_with_explicit_rows():
    train, _ = _flat_data(3, 1)
    rows = torch.tensor([5, 5, 0, 69, 17] + list(range(20, 55)), dtype=torch.int32)        # 40 rows: two tiles, row 5 twice
    shared = dict(num_units=32, num_layers=2, loss="scalar", batch_size=64)
    sw = _sweep(3, 1, MEMBERS3, **shared)
    singles = [_single(3, 1, m, **shared) for m in MEMBERS3]
    try:
        for obj in [sw] + singles:
            obj.set_data(train)
            obj.step(rows=rows.to(DEV))
            obj.step(rows=rows[:7].to(DEV))
        torch.cuda.synchronize()
        for k, tr in enumerate(singles):
            _assert_member_is_single(sw, k, tr, 2)
    finally:
        for obj in [sw] + singles:
            obj.close()


def test_one_member_is_the_single_trainer():
    train, test = _flat_data(3, 1)
    shared = dict(num_units=32, num_layers=2, loss="scalar", batch_size=64)
    _check_against_singles(3, 1, MEMBERS3[1:2], shared, train, test, steps=2)


def test_largest_sweep():
    from legged_gym_dev_amd import capi
    K = capi.TUBE_SWEEP_MAX
    members = [dict(alpha=0.5 + 0.007 * k, lr=1e-3 * (1 + k), seed=100 + k) for k in range(K)]
    train, _ = _flat_data(3, 1)
    shared = dict(num_units=16, num_layers=1, loss="scalar", batch_size=64)
    sw = _sweep(3, 1, members, **shared)
    singles = {k: _single(3, 1, members[k], **shared) for k in (0, K - 1)}
    try:
        for obj in [sw] + list(singles.values()):
            obj.set_data(train)
            obj.begin_epoch(0)
            obj.step(64)
        torch.cuda.synchronize()
        for k, tr in singles.items():
            _assert_member_is_single(sw, k, tr, 1)
    finally:
        for obj in [sw] + list(singles.values()):
            obj.close()


LEVELS3 = [dict(lr=1e-3, delta=1.0, seed=3, level_lo=0.5, level_hi=1.0), dict(lr=3e-3, delta=0.5, seed=4),
           dict(lr=1e-2, delta=0.25, seed=5, level_lo=0.1, level_hi=0.9)]


@pytest.mark.parametrize("batch", [32, 8])
@pytest.mark.parametrize("kind", ["trainer", "sweep"])
def test_regrown_buffers_reach_the_kernels(kind, batch):
    """The training kernels read every buffer pointer from the trainer's member array: the host copy with one member, the device
    copy with K.  set_data frees and reallocates starts, levels, perm and evpart when a split outgrows them, so a copy left stale
    would send the next launch to freed memory.  A: a 16-env split (8 test envs), then the 40-env split (20 test envs): at batch 8 all four buffers regrow,
    at batch 32 starts and levels start at the batch's size.  B: the 40-env split alone.  Horizon vector_level shape of
    test_horizon_dataset with the level column.  Every buffer, the log and the eval vector are bit-equal."""
    Hf, Hr, T = 4, 2, 12
    g = torch.Generator().manual_seed(7)
    w, z, v = torch.rand(60, T, generator=g), torch.randn(60, T, 2, generator=g), torch.randn(60, T, 2, generator=g)
    split = lambda a, b: _Horizon(w[a:b], z[a:b], v[a:b], Hf, Hr)
    shared = dict(num_units=128, num_layers=2, activation="softplus", softplus_beta=5.0, loss="vector_level", batch_size=batch,
                  horizon=(Hf, Hr))
    I = Hr + 2 + (Hr + Hf) * 2 + 1
    make = (lambda: _single(I, Hf, LEVELS3[0], **shared)) if kind == "trainer" else (lambda: _sweep(I, Hf, LEVELS3, **shared))
    pick = (lambda a: [a]) if kind == "trainer" else (lambda a: list(a))
    A, B = make(), make()
    try:
        A.set_data(split(0, 16), split(40, 48))
        got = []
        for obj in (A, B):
            obj.set_data(split(0, 40), split(40, 60))
            obj.begin_epoch(0)
            obj.step(batch)
            obj.step(8)                                               # at batch 32 the epoch's tail
            torch.cuda.synchronize()
            state = {n: [_bits(t).clone() for t in pick(getattr(obj, n))]
                     for n in ("params", "grads", "adam_m", "adam_v", "perm", "starts", "levels")}
            state["log"] = [_bits(obj.read_log(1, 2))] if kind == "trainer" else [_bits(obj.read_log(k, 1, 2)) for k in range(3)]
            state["eval"] = [_bits(e) for e in pick(obj.evaluate())]
            got.append(state)
        for name in ("perm", "starts", "levels"):                    # A's did grow to the second split
            assert all(tuple(t.shape) == (40,) for t in got[0][name]), name
        for name in got[0]:
            for k, (a, b) in enumerate(zip(got[0][name], got[1][name])):
                assert a.shape == b.shape and torch.equal(a, b), f"{name} of member {k}"
    finally:
        A.close()
        B.close()


def _member_states(members, shared, train, test, steps=3):
    sw = _sweep(3, 1, members, **shared)
    try:
        sw.set_data(train, test)
        _epochs(sw, 70, shared["batch_size"], steps)
        ev = sw.evaluate()
        torch.cuda.synchronize()
        return [[_bits(sw.params[k]), _bits(sw.adam_m[k]), _bits(sw.adam_v[k]), _bits(sw.grads[k]), _bits(sw.perm[k]),
                 _bits(sw.read_log(k, 1, steps)), _bits(ev[k])] for k in range(len(members))]
    finally:
        sw.close()


def test_a_member_does_not_depend_on_its_neighbour():
    train, test = _flat_data(3, 1)
    shared = dict(num_units=32, num_layers=2, loss="scalar", batch_size=64)
    a = _member_states([MEMBERS3[0], MEMBERS3[1]], shared, train, test)
    b = _member_states([MEMBERS3[0], dict(alpha=0.6, lr=5e-2, delta=0.1, seed=77, activation="elu")], shared, train, test)
    assert all(torch.equal(p, q) for p, q in zip(a[0], b[0]))
    assert not torch.equal(a[1][0], b[1][0])


def test_two_sweeps_bit_identical():
    train, test = _flat_data(3, 1)
    shared = dict(num_units=32, num_layers=2, loss="scalar", batch_size=64)
    a, b = (_member_states(MEMBERS3, shared, train, test) for _ in range(2))
    for k in range(3):
        assert all(torch.equal(p, q) for p, q in zip(a[k], b[k])), k


def test_hand_over_to_model_and_back():
    from legged_gym_dev_amd.tube.model import HipTubeModel
    train, _ = _flat_data(3, 1)
    x = torch.randn(40, 3, generator=torch.Generator().manual_seed(9)).to(DEV)
    shared = dict(num_units=32, num_layers=2, loss="scalar", batch_size=64)
    sw = _sweep(3, 1, MEMBERS3, **shared)
    tr = _single(3, 1, MEMBERS3[2], **shared)
    model = None
    try:
        for obj in (sw, tr):
            obj.set_data(train)
            obj.begin_epoch(0)
            obj.step(64)
        model = HipTubeModel(sw.state_dict(2), activation="relu", device=DEV)
        _same(model.predict(x), tr.predict(x), "predict of member 2's state dict")
        # a foreign state dict into member 0 and into the single trainer with member 0's configuration, then a step
        sd = {k: v * 0.5 for k, v in sw.state_dict(1).items()}
        tr0 = _single(3, 1, MEMBERS3[0], **shared)
        try:
            tr0.set_data(train)
            tr0.begin_epoch(0)
            tr0.step(64)
            for load in (lambda: sw.load_state_dict(0, sd), lambda: tr0.load_state_dict(sd)):
                load()
            for obj in (sw, tr0):
                obj.step(6)
            torch.cuda.synchronize()
            _assert_member_is_single(sw, 0, tr0, 2)
        finally:
            tr0.close()
    finally:
        for obj in (sw, tr, model):
            if obj is not None:
                obj.close()


def test_refusals():
    from legged_gym_dev_amd import capi
    from legged_gym_dev_amd.lib import LeggedHipError
    shared = dict(num_units=32, num_layers=2, loss="scalar", batch_size=64)
    K = capi.TUBE_SWEEP_MAX
    for members, word in (([], "K = 0"), ([{}] * (K + 1), f"K = {K + 1}"),
                          ([{}, {"num_units": 64}], "num_units differs between member 0 and member 1"),
                          ([{}, {}, {"batch_size": 32}], "batch_size differs between member 0 and member 2"),
                          ([{}, {"loss": "vector"}], "loss differs between member 0 and member 1"),
                          ([{}, {"num_units": 24}], "member 1: num_units must be")):
        with pytest.raises(LeggedHipError, match=word):
            _sweep(3, 1, members, **shared)
    sw = _sweep(3, 1, MEMBERS3, **shared)
    try:
        with pytest.raises(LeggedHipError, match="set_data"):
            sw.step(rows=torch.zeros(4, dtype=torch.int32, device=DEV))
        with pytest.raises(LeggedHipError, match="set_data"):
            sw.begin_epoch(0)
    finally:
        sw.close()


def _fixture_folder(path):
    fx = dict(np.load(os.path.join(ROOT, "tests", "golden", "tube_dataset.npz")))
    path.mkdir()
    for k in (0, 1):
        with open(path / f"epoch_{k}.pickle", "wb") as f:
            pickle.dump({key: fx[f"e{k}_{key}"] for key in ("z", "pz_x", "v", "done")}, f)
    return str(path)


def test_train_tube_sweep_then_evaluate(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
    import evaluate_tube
    import train_tube
    data = _fixture_folder(tmp_path / "data")
    common = ["--data", data, "--num_epochs", "2", "--batch_size", "128", "--lr", "3e-3", "--steps_per_model_checkpoint", "2",
              "--steps_per_model_evaluation", "3"]
    out = tmp_path / "sweep"
    train_tube.main(common + ["--out", str(out), "--sweep", "alpha=0.8,0.95", "--sweep", "seed=1,2"])
    names = ["alpha=0.8,seed=1", "alpha=0.8,seed=2", "alpha=0.95,seed=1", "alpha=0.95,seed=2"]
    assert sorted(os.listdir(out)) == sorted(names + ["sweep.json"])
    summary = json.load(open(out / "sweep.json"))
    assert [m["name"] for m in summary["members"]] == names
    for m, (alpha, seed) in zip(summary["members"], [(0.8, 1), (0.8, 2), (0.95, 1), (0.95, 2)]):
        assert m["hyperparameters"]["alpha"] == alpha and m["hyperparameters"]["seed"] == seed
        assert np.isfinite(m["final_train_loss"]) and np.isfinite(m["test"]["loss"]) and m["test"]["rows"] > 0
    plain = tmp_path / "plain"
    train_tube.main(common + ["--out", str(plain), "--alpha", "0.8", "--seed", "1"])
    member = out / names[0]
    assert sorted(os.listdir(member)) == sorted(os.listdir(plain))
    for ck in ("model.pth", "model_best.pth"):
        a, b = torch.load(member / ck, map_location="cpu"), torch.load(plain / ck, map_location="cpu")
        assert list(a) == list(b)
        for key in a:
            _same(a[key], b[key], f"{ck}: {key}")
    assert open(member / "metrics.jsonl").read() == open(plain / "metrics.jsonl").read()
    assert json.load(open(member / "config.json")) == json.load(open(plain / "config.json"))
    evaluate_tube.main(["--run", str(out / names[3]), "--data", data, "--checkpoint", "latest"])
    saved = json.load(open(out / names[3] / "eval.json"))
    assert saved["dataset"] == "scalar" and 0.0 <= saved["one_step"]["success_rate"] <= 1.0
