"""Level-conditioned tubes on the GPU (k_tube_rows<., true>, k_tube_rows_sweep<., true>, k_tube_predict_levels; DESIGN.md section
10.4): one step's gradient at the levels the kernel drew against float64 autograd, the draws themselves, 20 Adam + StepLR steps,
eval_level against predict, predict_levels against predict on the bits, a sweep against its single trainers, the ordering a
trained model shows over the levels, the unconditioned path against the sweep path, and collect -> train -> evaluate end to end."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import tube_level_ref, tube_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Flat:
    def __init__(self, x, y):
        self.data, self.target = x, y


def _trainer(I, O, **kw):
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    return HipTubeTrainer(I, O, device=DEV, **kw)


def _ref_model(tr, dtype, activation, beta=1.0):
    I, O, U, L = tr.dims
    m = tube_ref.MLP(I, O, U, L, activation, beta).to(dtype)
    m.load_state_dict({k: v.to(dtype).cpu() for k, v in tr.state_dict().items()})
    return m


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what=""):
    assert a.shape == b.shape and torch.equal(_bits(a), _bits(b)), what


def _with(x, lv):
    """x (n, I - 1) and lv (n, 1) or a number -> rows of full input_dim."""
    lv = lv if torch.is_tensor(lv) else torch.full_like(x[:, :1], float(lv))
    return torch.cat((x, lv.to(x)), dim=1)


# ---------------------------------------------------------------- 1. gradients
# scalar: 3+1 -> 16 x 1 ReLU -> 1, batch 33: two tiles, a tail of one row.  vector: 6+1 -> 32 x 2 Softplus(5) -> 2, batch 64.
GRAD_CASES = [("scalar_level", "relu", 1.0, 33, 3, 1, 16, 1), ("vector_level", "softplus", 5.0, 64, 6, 2, 32, 2)]


@pytest.mark.parametrize("case", GRAD_CASES, ids=lambda c: c[0])
def test_step_gradient_at_the_drawn_levels(case):
    loss, act, beta, B, Ix, O, U, L = case
    g = torch.Generator().manual_seed(B + Ix)
    n = 90
    x, y = torch.randn(n, Ix, generator=g), torch.rand(n, O, generator=g) * 2
    tr = _trainer(Ix + 1, O, num_units=U, num_layers=L, activation=act, softplus_beta=beta, loss=loss, delta=0.5, lr=0.0,
                  batch_size=64, seed=3, level_lo=0.05, level_hi=0.95)
    try:
        tr.set_data(_Flat(x, y))
        rows = torch.randperm(n, generator=g)[:B].to(torch.int32)
        ref = _ref_model(tr, torch.float64, act, beta)
        tr.step(rows=rows.to(DEV))
        torch.cuda.synchronize()
        lv = tr.read_levels(B).double()[:, None]
        assert bool(((lv >= 0.05) & (lv < 0.95)).all()) and lv.unique().numel() > B // 2
        xb, yb = x[rows.long()].double(), y[rows.long()].double()
        val = tube_level_ref.loss(loss, ref(_with(xb, lv)), yb, lv, 0.5)
        val.backward()
        want = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
        got = tr.grads.cpu().double()
        assert float(want[:U * (Ix + 1)].reshape(U, Ix + 1)[:, -1].abs().max()) > 0      # the level column has a weight gradient
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=2e-4 * (float(want.abs().max()) + 1e-12))
        log = tr.read_log(1, 1)[0]
        np.testing.assert_allclose(float(log[0]), float(val), rtol=1e-4, atol=1e-7)
        np.testing.assert_allclose(float(log[2]), float(want.norm()), rtol=1e-3)
        assert int(log[3]) == B
    finally:
        tr.close()


# ---------------------------------------------------------------- 2. draws
def _draw_run(n, batches, seed=11):
    """Steps of the given batch sizes on explicit rows, each after set_step(0): the levels of every step."""
    g = torch.Generator().manual_seed(1)
    x, y = torch.randn(n, 2, generator=g), torch.rand(n, 1, generator=g)
    tr = _trainer(3, 1, num_units=16, num_layers=1, loss="scalar_level", lr=1e-3, batch_size=max(batches), seed=seed,
                  level_lo=0.1, level_hi=0.9)
    out = []
    try:
        tr.set_data(_Flat(x, y))
        for b in batches:
            tr.set_step(0)
            tr.step(rows=torch.arange(b, dtype=torch.int32, device=DEV))
            out.append(tr.read_levels(b))
        tr.step(rows=torch.arange(batches[-1], dtype=torch.int32, device=DEV))            # step 2: another key
        out.append(tr.read_levels(batches[-1]))
        state = (tr.params.cpu(), tr.adam_m.cpu(), tr.adam_v.cpu(), tr.read_log(1, 2))
    finally:
        tr.close()
    return out, state


def test_level_draws():
    (lv1, lv2), state = _draw_run(4096, [4096])
    assert bool(((lv1 >= 0.1) & (lv1 < 0.9)).all())
    assert abs(float(lv1.double().mean()) - 0.5) <= 0.0145               # 4 sigma of the mean of 4096 uniforms of width 0.8
    assert not torch.equal(lv1, lv2)                                     # step 1 and step 2 draw under different keys
    (a33, a64, _), _ = _draw_run(64, [33, 64])
    _same(a33, a64[:33], "a row's level depends on (seed, key, position), not on the batch or the tile")
    _same(a64, lv1[:64], "nor on the data")
    (b1, b2), state_b = _draw_run(4096, [4096])
    _same(lv1, b1), _same(lv2, b2)
    for p, q in zip(state, state_b):
        _same(p, q, "two fresh runs")
    (c1, _), _ = _draw_run(64, [64], seed=12)
    assert not torch.equal(c1, lv1[:64])


# ---------------------------------------------------------------- 3. Adam + StepLR
def test_adam_steplr_track_torch_on_the_recorded_levels():
    """20 steps with a StepLR boundary at 8 and 16; torch float64 on the levels the kernel recorded, test_adam_steplr_track_torch's
    bounds."""
    Ix, O, U, L, B, n = 5, 2, 32, 2, 96, 400
    g = torch.Generator().manual_seed(11)
    x, y = torch.randn(n, Ix, generator=g), torch.rand(n, O, generator=g)
    tr = _trainer(Ix + 1, O, num_units=U, num_layers=L, activation="tanh", loss="vector_level", delta=1.0, lr=3e-3, gamma=0.5,
                  step_size=8, batch_size=B, seed=5, level_lo=0.2, level_hi=1.0)
    try:
        tr.set_data(_Flat(x, y))
        ref = _ref_model(tr, torch.float64, "tanh")
        opt, sched = tube_ref.optimizer(ref, 3e-3, 0.5, 8)
        ref_log = []
        for s in range(20):
            rows = torch.randint(0, n, (B if s % 7 else B - 5,), generator=g)
            tr.step(rows=rows.to(torch.int32).to(DEV))
            lv = tr.read_levels(rows.numel()).double()[:, None]
            opt.zero_grad()
            val = tube_level_ref.loss("vector_level", ref(_with(x[rows].double(), lv)), y[rows].double(), lv, 1.0)
            val.backward()
            opt.step()
            sched.step()
            ref_log.append((float(val), sched.get_last_lr()[0]))
        log = tr.read_log(1, 20)
        want = torch.cat([p.detach().reshape(-1) for p in ref.parameters()])
        np.testing.assert_allclose(tr.params.cpu().numpy(), want.numpy(), rtol=1e-3, atol=5e-5)
        np.testing.assert_allclose(log[:, 0].numpy(), [a for a, _ in ref_log], rtol=2e-3, atol=1e-6)
        np.testing.assert_allclose(log[:, 1].numpy(), [b for _, b in ref_log], rtol=1e-6)
        assert float(log[7, 1]) == pytest.approx(1.5e-3) and float(log[6, 1]) == pytest.approx(3e-3)
    finally:
        tr.close()


# ---------------------------------------------------------------- 4. eval_level
def test_eval_level_against_predict():
    n, Ix, O = 333, 4, 3
    g = torch.Generator().manual_seed(4)
    x, y = torch.randn(n, Ix, generator=g), torch.rand(n, O, generator=g) * 0.5
    for loss in ("scalar_level", "vector_level"):
        tr = _trainer(Ix + 1, O, num_units=48, num_layers=3, activation="tanh", loss=loss, delta=0.3, batch_size=64, seed=8)
        try:
            tr.set_data(_Flat(x[:50], y[:50]), _Flat(x, y))
            for lv in (0.3, 0.9):
                ev = tr.eval_level(lv).cpu()
                _same(tr.read_levels(n), torch.full((n,), lv), "levels of a fixed-level eval")
                fw = tr.predict(_with(x, lv).to(DEV)).cpu().double()
                want = tube_ref.eval_metrics(loss[:-6], fw, y.double(), float(np.float32(lv)), 0.3)
                np.testing.assert_allclose(ev[:3].numpy(), want, rtol=1e-4, atol=1e-6)
                assert int(ev[3]) == n
            ev = tr.evaluate().cpu()                                     # a drawn level per row, as a step does
            lv = tr.read_levels(n).double()[:, None]
            assert lv.unique().numel() > n // 2
            fw = tr.predict(_with(x, lv.float()).to(DEV)).cpu().double()
            np.testing.assert_allclose(float(ev[0]), float(tube_level_ref.loss(loss, fw, y.double(), lv, 0.3)), rtol=1e-4)
        finally:
            tr.close()


def test_eval_level_is_monotone_on_a_model_that_rises_with_the_level():
    """w0's level column and the following weights positive, every other input weight zero: the output rises with the level."""
    n, Ix = 200, 3
    g = torch.Generator().manual_seed(6)
    x, y = torch.randn(n, Ix, generator=g), torch.rand(n, 1, generator=g)
    tr = _trainer(Ix + 1, 1, num_units=16, num_layers=1, loss="scalar_level", batch_size=32, seed=2)
    try:
        sd = tr.state_dict()
        sd["layers.0.weight"] = torch.zeros(16, Ix + 1)
        sd["layers.0.weight"][:, -1] = 0.1
        sd["layers.0.bias"] = torch.zeros(16)
        sd["layers.2.weight"] = torch.full((1, 16), 0.6)
        sd["layers.2.bias"] = torch.zeros(1)                             # output = 0.96 level
        tr.load_state_dict(sd)
        tr.set_data(_Flat(x, y), _Flat(x, y))
        lo, hi = float(tr.eval_level(0.1)[1]), float(tr.eval_level(0.9)[1])
        assert hi >= lo and hi > 0.5 > lo
    finally:
        tr.close()


# ---------------------------------------------------------------- 5. predict_levels
SHAPES = [(1, 1, 16, 1, "relu"), (5, 2, 48, 4, "tanh"), (255, 64, 128, 2, "elu")]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}+1-{s[2]}x{s[3]}-{s[1]}")
def test_predict_levels_equals_predict_on_the_bits(shape):
    Ix, O, U, L, act = shape
    g = torch.Generator().manual_seed(Ix)
    x = torch.randn(40, Ix, generator=g).to(DEV)
    tr = _trainer(Ix + 1, O, num_units=U, num_layers=L, activation=act, loss="scalar_level", batch_size=32, seed=4)
    try:
        for n_levels in (1, 5, 64):
            levels = torch.rand(n_levels, generator=g)
            for count, rows in ((1, None), (31, None), (33, None), (33, torch.tensor([7, 7] + list(range(39, 8, -1)), dtype=torch.int32))):
                xs = x[:count] if rows is None else x
                got = tr.predict_levels(xs, levels, rows=None if rows is None else rows.to(DEV))
                assert tuple(got.shape) == (count, n_levels, O)
                src = xs if rows is None else x[rows.long().to(DEV)]
                for l in ([0, n_levels - 1] if n_levels > 5 else range(n_levels)):
                    want = tr.predict(_with(src, float(levels[l])))
                    _same(got[:, l, :], want, f"count {count}, level {l} of {n_levels}, rows {rows is not None}")
    finally:
        tr.close()


def test_predict_levels_refusals():
    from legged_gym_dev_amd.lib import LeggedHipError
    x = torch.zeros(4, 3, device=DEV)
    plain = _trainer(4, 1, num_units=16, num_layers=1, loss="scalar", batch_size=32)
    tr = _trainer(4, 1, num_units=16, num_layers=1, loss="scalar_level", batch_size=32)
    try:
        with pytest.raises(ValueError, match="not level-conditioned"):
            plain.predict_levels(x, [0.5])
        with pytest.raises(ValueError, match="not level-conditioned"):
            plain.eval_level(0.5)
        out, lv = torch.zeros(4, 65, 1, device=DEV), torch.zeros(65, device=DEV)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        assert plain.lib.lg_tube_predict_levels(plain.h, ptr(x), None, 4, ptr(lv), 1, ptr(out)) == -1
        assert "not level-conditioned" in plain.lib.lg_last_error().decode()
        assert plain.lib.lg_tube_eval_level(plain.h, C.c_float(0.5)) == -1
        for bad in (0, 65):
            assert tr.lib.lg_tube_predict_levels(tr.h, ptr(x), None, 4, ptr(lv), bad, ptr(out)) == -1
            assert "n_levels must be 1..64" in tr.lib.lg_last_error().decode()
            with pytest.raises(ValueError, match="levels"):
                tr.predict_levels(x, torch.zeros(bad))
        with pytest.raises(LeggedHipError, match="0..1"):
            tr.eval_level(1.5)
        with pytest.raises(ValueError, match=r"\(n >= 1, 3\)"):
            tr.predict_levels(torch.zeros(4, 4, device=DEV), [0.5])
    finally:
        plain.close()
        tr.close()


# ---------------------------------------------------------------- 6. sweep
def test_sweep_members_equal_their_single_trainers():
    from legged_gym_dev_amd.lib import LeggedHipError
    from legged_gym_dev_amd.tube.sweep import HipTubeSweep
    g = torch.Generator().manual_seed(0)
    x, y = torch.randn(103, 3, generator=g), torch.rand(103, 1, generator=g) * 2
    train, test = _Flat(x[:70], y[:70]), _Flat(x[70:], y[70:])
    members = [dict(level_lo=0.0, level_hi=1.0, seed=3, activation="relu"), dict(level_lo=0.5, level_hi=0.99, seed=4, activation="tanh"),
               dict(level_lo=0.1, level_hi=0.6, seed=5, activation="softplus", softplus_beta=5.0)]
    shared = dict(num_units=32, num_layers=2, loss="scalar_level", batch_size=64, gamma=0.5, step_size=3)
    sw = HipTubeSweep(4, 1, members=members, device=DEV, **shared)
    singles = [_trainer(4, 1, **{**shared, **m}) for m in members]
    try:
        for obj in [sw] + singles:
            obj.set_data(train, test)
            for epoch in range(3):                                       # 70 rows at batch 64: a two-tile step and a 6-row tail
                obj.begin_epoch(epoch)
                obj.step(64)
                if epoch < 2:
                    obj.step(6)
        torch.cuda.synchronize()
        for k, tr in enumerate(singles):
            _same(sw.read_levels(k, 64), tr.read_levels(64), f"member {k}: levels of the last step")
            lv = tr.read_levels(64)
            assert bool(((lv >= members[k]["level_lo"]) & (lv < members[k]["level_hi"])).all())
        ev = sw.eval_level(0.8)
        for k, tr in enumerate(singles):
            for name in ("params", "adam_m", "adam_v", "grads"):
                _same(getattr(sw, name)[k], getattr(tr, name), f"member {k}: {name}")
            _same(sw.read_log(k, 1, 5), tr.read_log(1, 5), f"member {k}: log")
            _same(ev[k], tr.eval_level(0.8), f"member {k}: eval_level")
        ev = sw.evaluate()
        for k, tr in enumerate(singles):
            _same(ev[k], tr.evaluate(), f"member {k}: eval with drawn levels")
            _same(sw.read_levels(k, 33), tr.read_levels(33), f"member {k}: levels of the eval")
    finally:
        for obj in [sw] + singles:
            obj.close()
    with pytest.raises(LeggedHipError, match="level_input differs between member 0 and member 1"):
        HipTubeSweep(4, 1, members=[dict(loss="scalar"), dict(loss="scalar_level")], device=DEV, num_units=32, batch_size=64)


# ---------------------------------------------------------------- 7. learning: ordering only
def _learning_data():
    g = torch.Generator().manual_seed(1234)
    x = torch.rand(4096, 2, generator=g)
    e = torch.rand(4096, 1, generator=g)
    return x, (0.2 + x[:, :1]) * e


LEARN_STEPS = 320


def test_trained_model_orders_the_levels():
    """x ~ U(0,1)^2, y = (0.2 + x0) e, e ~ U(0,1); 2+1 -> 32 x 2 ReLU -> 1, batch 256, lr 3e-3, LEARN_STEPS steps.
    Reference figure: the float64 torch restatement (tests/tube_level_ref.py), trained for the same number of steps with levels
    drawn by numpy, reaches coverages 0.112 / 0.480 / 0.896 at the levels 0.1 / 0.5 / 0.9 on these rows (mean predicted widths
    0.080 / 0.340 / 0.620; 0.172 / 0.571 / 0.982 after 160 steps, 0.134 / 0.543 / 0.964 after 480): more than 0.1 apart.
    The loss is Huber over the pinball value, an expectile-like target below delta: coverage rises with the level but need not
    equal it, so only the ordering is asserted."""
    x, y = _learning_data()
    tr = _trainer(3, 1, num_units=32, num_layers=2, loss="scalar_level", lr=3e-3, batch_size=256, seed=7)
    try:
        tr.set_data(_Flat(x, y), _Flat(x, y))
        for s in range(LEARN_STEPS):
            if s % 16 == 0:
                tr.begin_epoch(s // 16)
            tr.step(256)
        cov = [float(tr.eval_level(lv)[1]) for lv in (0.1, 0.5, 0.9)]
        width = tr.predict_levels(x, [0.1, 0.5, 0.9]).mean(dim=(0, 2)).tolist()
        print("coverage", cov, "mean width", width)
        assert cov[0] < cov[1] < cov[2]
        assert width[0] < width[1] < width[2]
    finally:
        tr.close()


# ---------------------------------------------------------------- 8. the unconditioned path
def test_unconditioned_trainer_still_equals_the_sweep_path():
    from legged_gym_dev_amd.tube.sweep import HipTubeSweep
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(103, 6, generator=g), torch.rand(103, 2, generator=g) * 2
    train, test = _Flat(x[:70], y[:70]), _Flat(x[70:], y[70:])
    cfg = dict(num_units=32, num_layers=2, activation="softplus", softplus_beta=5.0, loss="vector", alpha=0.9, delta=0.5,
               batch_size=64, seed=3, lr=3e-3)
    sw = HipTubeSweep(6, 2, members=[{}], device=DEV, **cfg)
    tr = _trainer(6, 2, **cfg)
    try:
        assert tr.levels is None and sw.levels == [None] and not tr.level_input
        for obj in (sw, tr):
            obj.set_data(train, test)
            for epoch in range(3):
                obj.begin_epoch(epoch)
                obj.step(64)
                if epoch < 2:
                    obj.step(6)
        _same(sw.params[0], tr.params, "params")
        _same(sw.read_log(0, 1, 5), tr.read_log(1, 5), "log")
        _same(sw.evaluate()[0], tr.evaluate(), "eval")
    finally:
        sw.close()
        tr.close()


# ---------------------------------------------------------------- 9. end to end
def test_collect_train_evaluate_end_to_end(tmp_path):
    sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
    import collect_rom_sim_data
    import evaluate_tube
    import train_tube
    data, run = tmp_path / "data", tmp_path / "run"
    collect_rom_sim_data.main(["--num_envs", "64", "--epochs", "2", "--episode_length_s", "5", "--out", str(data), "--seed", "2"])
    train_tube.main(["--data", str(data), "--dataset", "scalar_level", "--num_epochs", "2", "--batch_size", "1024", "--lr", "3e-3",
                     "--steps_per_model_checkpoint", "5", "--steps_per_model_evaluation", "3", "--out", str(run)])
    cfg = json.load(open(run / "config.json"))
    assert cfg["level_input"] is True and (cfg["level_lo"], cfg["level_hi"], cfg["loss"]) == (0.0, 1.0, "scalar_level")
    recs = [json.loads(s) for s in open(run / "metrics.jsonl")]
    evs = [r for r in recs if "Test Loss (level drawn)" in r]
    assert evs and all(f"Proportion Correct, fw > w (level={lv:.2f})" in evs[0] for lv in (0.5, 0.8, 0.9, 0.95))
    evaluate_tube.main(["--run", str(run), "--data", str(data), "--checkpoint", "latest", "--horizon", "25"])
    saved = json.load(open(run / "eval.json"))
    assert [r["level"] for r in saved["levels"]] == [0.5, 0.8, 0.9, 0.95] and saved["dataset"] == "scalar_level"
    for r in saved["levels"]:
        for part in ("one_step", "rollout"):
            assert r[part]["steps"] > 0 and np.isfinite(r[part]["success_rate"]) and 0.0 <= r[part]["success_rate"] <= 1.0
            assert all(v is None or np.isfinite(v) for v in r[part]["success_rate_by_age"])
