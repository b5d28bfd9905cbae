"""Level-conditioned one-shot tubes on the GPU (k_tube_rows<., true> and k_tube_rows_sweep<., true> on horizon handles,
k_tube_predict_levels<true> = the window query of many levels): the window query against the flat
conditioned predict on the bits, one step's gradient at the drawn starts and levels against float64 autograd, the draws, eval_level
against the window query, a sweep against its single trainers, the calibration against torch.sort, the refusals, and
train -> calibrate -> evaluate end to end on the simulator."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import tube_horizon_level_ref as hl
from tests import tube_level_ref, tube_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
INF = float("inf")


def _trainer(ds, **kw):
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    kw.setdefault("loss", "scalar_level")
    return HipTubeTrainer(ds.input_dim, ds.output_dim, horizon=(ds.H_fwd, ds.H_rev), device=DEV, **kw)


def _ref_model(tr, activation, beta=1.0):
    I, O, U, L = tr.dims
    m = tube_ref.MLP(I, O, U, L, activation, beta).double()
    m.load_state_dict({k: v.double().cpu() for k, v in tr.state_dict().items()})
    return m


def _same(a, b, what=""):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b), what


def _windows(ds, count, seed):
    """count windows of ds: both ends of the start range first, then random ones; with 33 or more, window 32 repeats window 0."""
    g = torch.Generator().manual_seed(seed)
    n, T = ds.w.shape
    env = torch.randint(0, n, (count,), generator=g, dtype=torch.int32)
    start = torch.randint(ds.H_rev, T - ds.H_fwd + 1, (count,), generator=g, dtype=torch.int32)
    start[0] = ds.H_rev
    if count > 1:
        start[1] = T - ds.H_fwd
    if count > 32:
        env[32], start[32] = env[0], start[0]
    return env, start


# ---------------------------------------------------------------- 1. the window query on the bits
# (H_rev, H_fwd, nz, m, units, layers, activation, beta, envs, T, counts, level counts); the last is the reference one-shot shape
BITS = [(3, 4, 2, 2, 16, 1, "relu", 1.0, 5, 24, (1, 31, 33), (1, 5, 64)), (1, 2, 0, 2, 32, 2, "tanh", 1.0, 5, 24, (1, 31, 33), (1, 5, 64)),
        (10, 50, 0, 2, 128, 2, "softplus", 5.0, 5, 64, (33,), (5,))]


@pytest.mark.parametrize("case", BITS, ids=lambda c: f"Hrev{c[0]}-Hfwd{c[1]}-nz{c[2]}-{c[4]}x{c[5]}")
def test_window_levels_equal_the_flat_predict_on_the_bits(case):
    from legged_gym_dev_amd.tube.model import HipTubeModel
    Hr, Hf, nz, m, U, L, act, beta, n, T, counts, level_counts = case
    ds = hl.dataset(n, T, nz, m, Hf, Hr, seed=Hr + Hf)
    assert ds.input_dim == Hr + nz + (Hr + Hf) * m + 1
    tr = _trainer(ds, num_units=U, num_layers=L, activation=act, softplus_beta=beta, batch_size=32, seed=4)
    flat = HipTubeModel(tr.state_dict(), activation=act, softplus_beta=beta, device=DEV, level_input=True)
    try:
        g = torch.Generator().manual_seed(7)
        for n_levels in level_counts:
            levels = torch.rand(n_levels, generator=g)
            for count in counts:
                env, start = _windows(ds, count, seed=count)
                got = tr.predict_windows_levels(ds, env, start, levels)
                assert tuple(got.shape) == (count, n_levels, Hf)
                for l in ([0, n_levels - 1] if n_levels > 5 else range(n_levels)):
                    x, _ = hl.items(ds, env, start, float(levels[l]), dtype=torch.float32, targets=False)
                    assert x.shape[1] == ds.input_dim and float(x[0, -1]) == float(levels[l])
                    _same(got[:, l, :], flat.predict(x.to(DEV)), f"count {count}, level {l} of {n_levels}")
                if count > 32:                                           # the same window in tile 0 and in tile 1
                    _same(got[0], got[32], "a window's result does not depend on its place in the tile")
    finally:
        flat.close()
        tr.close()


# ---------------------------------------------------------------- 2. one training step
@pytest.mark.parametrize("loss", ["scalar_level", "vector_level"])
def test_step_gradient_at_the_drawn_starts_and_levels(loss):
    B = 33
    ds = hl.dataset(5, 24, 2, 2, 4, 3, seed=21)
    g = torch.Generator().manual_seed(3)
    tr = _trainer(ds, num_units=16, num_layers=2, activation="softplus", softplus_beta=5.0, loss=loss, delta=0.5, lr=0.0, batch_size=64,
                  seed=3, level_lo=0.05, level_hi=0.95)
    try:
        tr.set_data(ds)
        rows = torch.randint(0, 5, (B,), generator=g, dtype=torch.int32)
        ref = _ref_model(tr, "softplus", 5.0)
        tr.step(rows=rows.to(DEV))
        torch.cuda.synchronize()
        starts, lv = tr.starts[:B].cpu(), tr.read_levels(B).double()[:, None]
        assert bool(((starts >= 3) & (starts < 24 - 4 - 1)).all()) and starts.unique().numel() > 4
        assert bool(((lv >= 0.05) & (lv < 0.95)).all()) and lv.unique().numel() > B // 2
        xb, yb = hl.items(ds, rows, starts, lv.reshape(-1))
        val = tube_level_ref.loss(loss, ref(xb), yb, lv, 0.5)
        val.backward()
        want = torch.cat([p.grad.reshape(-1) for p in ref.parameters()])
        got = tr.grads.cpu().double()
        assert float(want[:16 * ds.input_dim].reshape(16, ds.input_dim)[:, -1].abs().max()) > 0   # the level column has a weight gradient
        np.testing.assert_allclose(got.numpy(), want.numpy(), rtol=1e-3, atol=2e-4 * (float(want.abs().max()) + 1e-12))
        log = tr.read_log(1, 1)[0]
        np.testing.assert_allclose(float(log[0]), float(val.detach()), rtol=1e-4)
        assert int(log[3]) == B
    finally:
        tr.close()


# ---------------------------------------------------------------- 3. draws
def _draws(ds, batches, **kw):
    """(starts, levels) of steps of the given batch sizes on rows 0, 1, ... mod envs, each after set_step(0)."""
    tr = _trainer(ds, num_units=16, num_layers=1, batch_size=64, **kw)
    out = []
    try:
        tr.set_data(ds)
        for b in batches:
            tr.set_step(0)
            tr.step(rows=(torch.arange(b, dtype=torch.int32) % len(ds)).to(DEV))
            out.append((tr.starts[:b].cpu().clone(), tr.read_levels(b)))
    finally:
        tr.close()
    return out


def test_draws_depend_on_seed_key_and_position_only():
    from legged_gym_dev_amd.tube.sweep import HipTubeSweep
    ds = hl.dataset(5, 24, 2, 2, 4, 3, seed=22)
    (s32, l32), (s33, l33) = _draws(ds, [32, 33], seed=11, level_lo=0.1, level_hi=0.9)
    _same(s32, s33[:32], "starts: batch 32 against 33"), _same(l32, l33[:32], "levels: batch 32 against 33")
    assert bool(((l33 >= 0.1) & (l33 < 0.9)).all()) and bool(((s33 >= 3) & (s33 < 19)).all())
    other = hl.dataset(7, 24, 2, 2, 4, 3, seed=23)                          # other data, more envs: the same draws
    (o33s, o33l), = _draws(other, [33], seed=11, level_lo=0.1, level_hi=0.9)
    _same(o33s, s33), _same(o33l, l33)
    (c33s, c33l), = _draws(ds, [33], seed=12, level_lo=0.1, level_hi=0.9)
    assert not torch.equal(c33s, s33) and not torch.equal(c33l, l33)
    sw = HipTubeSweep(ds.input_dim, ds.output_dim, members=[dict(seed=11, level_lo=0.1, level_hi=0.9), dict(seed=12, level_lo=0.5, level_hi=0.6)],
                      device=DEV, num_units=16, num_layers=1, batch_size=64, loss="scalar_level", horizon=(4, 3))
    try:
        sw.set_data(ds)
        sw.step(rows=(torch.arange(33, dtype=torch.int32) % 5).to(DEV))
        _same(sw.starts[0][:33], s33, "starts: sweep member against the single trainer")
        _same(sw.read_levels(0, 33), l33, "levels: sweep member against the single trainer")
        _same(sw.starts[1][:33], c33s, "member 1 draws under its own seed")
        l1 = sw.read_levels(1, 33)
        assert bool(((l1 >= 0.5) & (l1 < 0.6)).all())
    finally:
        sw.close()


# ---------------------------------------------------------------- 4. eval_level
def test_eval_level_against_the_window_query():
    ds = hl.dataset(37, 24, 2, 2, 4, 3, seed=24)                            # 37 test windows: a full tile and a tail of five
    n = len(ds)
    for loss in ("scalar_level", "vector_level"):
        tr = _trainer(ds, num_units=32, num_layers=2, activation="tanh", loss=loss, delta=0.3, batch_size=64, seed=8)
        try:
            tr.set_data(ds, ds)
            envs = torch.arange(n, dtype=torch.int32)
            for lv in (0.3, 0.9):
                ev = tr.eval_level(lv).cpu()
                _same(tr.read_levels(n), torch.full((n,), lv), "levels of a fixed-level eval")
                starts = tr.starts[:n].cpu()
                assert bool(((starts >= 3) & (starts < 19)).all())
                fw = tr.predict_windows_levels(ds, envs, starts, [lv])[:, 0, :].cpu().double()
                _, y = hl.items(ds, envs, starts)
                want = tube_ref.eval_metrics(loss[:-6], fw, y, float(np.float32(lv)), 0.3)
                np.testing.assert_allclose(ev[:3].numpy(), want, rtol=1e-4, atol=1e-6)
                assert int(ev[3]) == n
            ev = tr.evaluate().cpu()                                     # a drawn level per row, as a step does
            lv, starts = tr.read_levels(n), tr.starts[:n].cpu()
            assert lv.unique().numel() > n // 2
            fw = tr.predict_windows_levels(ds, envs, starts, lv).cpu().double()[torch.arange(n), torch.arange(n)]   # window i at level i
            _, y = hl.items(ds, envs, starts)
            np.testing.assert_allclose(float(ev[0]), float(tube_level_ref.loss(loss, fw, y, lv.double()[:, None], 0.3)), rtol=1e-4)
        finally:
            tr.close()


# ---------------------------------------------------------------- 5. sweep
def test_sweep_members_equal_their_single_trainers():
    from legged_gym_dev_amd.tube.sweep import HipTubeSweep
    train, test = hl.dataset(70, 24, 2, 2, 4, 3, seed=25), hl.dataset(33, 24, 2, 2, 4, 3, seed=26)
    members = [dict(level_lo=0.0, level_hi=1.0, seed=3, activation="relu"), dict(level_lo=0.5, level_hi=0.99, seed=4, activation="tanh")]
    shared = dict(num_units=32, num_layers=2, loss="vector_level", batch_size=64, gamma=0.5, step_size=2)
    sw = HipTubeSweep(train.input_dim, train.output_dim, members=members, device=DEV, horizon=(4, 3), **shared)
    singles = [_trainer(train, **{**shared, **m}) for m in members]
    try:
        for obj in [sw] + singles:
            obj.set_data(train, test)
            obj.begin_epoch(0)
            obj.step(64)                                                 # 70 envs at batch 64: a two-tile step and a 6-row tail
            obj.step(6)
            obj.begin_epoch(1)
            obj.step(64)
        torch.cuda.synchronize()
        for k, tr in enumerate(singles):
            for name in ("params", "adam_m", "adam_v", "grads"):
                _same(getattr(sw, name)[k], getattr(tr, name), f"member {k}: {name}")
            _same(sw.starts[k][:64], tr.starts[:64], f"member {k}: starts")
            _same(sw.read_levels(k, 64), tr.read_levels(64), f"member {k}: levels")
            _same(sw.read_log(k, 1, 3), tr.read_log(1, 3), f"member {k}: log")
            lv = tr.read_levels(64)
            assert bool(((lv >= members[k]["level_lo"]) & (lv < members[k]["level_hi"])).all())
        ev = sw.eval_level(0.8)
        for k, tr in enumerate(singles):
            _same(ev[k], tr.eval_level(0.8), f"member {k}: eval_level")
            _same(sw.starts[k][:33], tr.starts[:33], f"member {k}: starts of the eval")
    finally:
        for obj in [sw] + singles:
            obj.close()


# ---------------------------------------------------------------- 6. calibration
def _model(I, O, U, L, act, horizon, seed=5):
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    tr = HipTubeTrainer(I, O, num_units=U, num_layers=L, activation=act, loss="scalar_level", batch_size=32, seed=seed, horizon=horizon, device=DEV)
    try:
        sd = tr.state_dict()
    finally:
        tr.close()
    return HipTubeModel(sd, activation=act, horizon=horizon, device=DEV, level_input=True)


def test_calibration_offsets_per_level_and_step_ahead():
    import calibrate_tube
    import evaluate_tube
    E, T = 8, 40
    g = torch.Generator().manual_seed(3)
    raw = {"z": torch.randn(E, T + 1, 4, generator=g), "pz_x": torch.randn(E, T + 1, 4, generator=g), "v": torch.randn(E, T, 2, generator=g),
           "done": torch.zeros(E, T, dtype=torch.uint8)}
    raw = {k: v.to(DEV) for k, v in raw.items()}
    cfg = {"dataset": "scalar_horizon_level", "N": 1, "dN": 1, "recursive": False, "H_fwd": 5, "H_rev": 2, "activation": "relu", "softplus_beta": 1.0}
    levels = [0.5, 0.9, 0.99]                                            # 96 windows: 0.99 asks for rank 97 -> +inf, and is kept
    model = _model(2 + 2 + 7 * 2 + 1, 5, 32, 2, "relu", (5, 2))
    try:
        a = calibrate_tube.parse_args(["--run", "unused", "--sim", "--window_stride", "3"])
        c = calibrate_tube.calibrate(model, cfg, raw, a, levels, torch.device(DEV))
        res, series = evaluate_tube.evaluate_horizon_levels(model, cfg, raw, 3, torch.device(DEV), levels, calib=c)
    finally:
        model.close()
    fw, w = series["fw_levels"], series["target"]
    W = fw.shape[0]
    assert c.kind == "horizon_levels" and c.coverages == levels and c.n == W == E * res["windows_per_env"] == 96
    assert tuple(c.offsets.shape) == (3, 5) and c.ranks == [-(-(W + 1) // 2), -(-(W + 1) * 9 // 10), -(-(W + 1) * 99 // 100)] == [49, 88, 97]
    for l, (lv, rank) in enumerate(zip(levels, c.ranks)):
        s = torch.sort((w.cpu() - fw[:, l, :].cpu()), dim=0).values
        _same(c.offsets[l], s[rank - 1] if rank <= W else torch.full((5,), INF), f"level {lv}")
        covered = c.covers(fw[:, l, :], w, level=lv).sum(dim=0).tolist()
        assert all(v >= min(rank, W) for v in covered)
        m = res["levels"][l]
        assert m["level"] == lv and m["calibrated"]["rank"] == rank and m["calibrated"]["one_shot"]["covered_by_step"] == covered
        assert m["one_shot"]["windows"] == W
    assert bool(torch.isinf(c.offsets[2]).all()) and res["levels"][2]["calibrated"]["one_shot"]["offset"] == ["inf"] * 5
    assert 0.0 <= res["level_crossings"] <= 1.0


# ---------------------------------------------------------------- 7. refusals
def test_refusals():
    from legged_gym_dev_amd.lib import LeggedHipError
    ds = hl.dataset(5, 24, 2, 2, 4, 3, seed=27)
    plain_ds = hl.dataset(5, 24, 2, 2, 4, 3, seed=27, conditioned=False)
    tr = _trainer(ds, num_units=16, num_layers=1, batch_size=32)
    plain = _trainer(plain_ds, num_units=16, num_layers=1, batch_size=32, loss="scalar_horizon", alpha=0.9)
    flat = _trainer_flat()
    ptr = lambda t: C.c_void_p(t.data_ptr())
    w, z, v = (t.to(DEV) for t in (ds.w, ds.z, ds.v))
    env, start = torch.zeros(4, dtype=torch.int32, device=DEV), torch.full((4,), 3, dtype=torch.int32, device=DEV)
    lv, out = torch.zeros(65, device=DEV), torch.zeros(4, 65, 4, device=DEV)
    call = lambda t, nl, nz=2: t.lib.lg_tube_predict_windows_levels(t.h, ptr(w), ptr(z), ptr(v), 5, 24, nz, 2, ptr(env), ptr(start), 4, ptr(lv), nl, ptr(out))
    err = lambda t: t.lib.lg_last_error().decode()
    try:
        assert call(plain, 1) == -1 and "not level-conditioned" in err(plain) and "level_input" in err(plain)
        assert call(flat, 1) == -1 and "not a horizon handle" in err(flat) and "horizon" in err(flat)
        for bad in (0, 65):
            assert call(tr, bad) == -1 and "n_levels must be 1..64" in err(tr)
            with pytest.raises(ValueError, match="levels"):
                tr.predict_windows_levels(ds, env, start, torch.zeros(bad))
        assert call(tr, 1, nz=3) == -1 and "input_dim" in err(tr) and "+ 1" in err(tr)
        assert call(tr, 1) == 0
        assert tr.lib.lg_tube_predict_windows(tr.h, ptr(w), ptr(z), ptr(v), 5, 24, 2, 2, ptr(env), ptr(start), 4, ptr(out)) == -1
        assert "level_input" in err(tr) and "lg_tube_predict_windows_levels" in err(tr)
        with pytest.raises(ValueError, match="predict_windows_levels"):
            tr.predict_windows(ds, env, start)
        with pytest.raises(ValueError, match="not level-conditioned"):
            plain.predict_windows_levels(plain_ds, env, start, [0.5])
        with pytest.raises(ValueError, match="not a horizon model"):
            flat.predict_windows_levels(ds, env, start, [0.5])
        with pytest.raises(IndexError, match="window out of range"):
            tr.predict_windows_levels(ds, env, start + 18, [0.5])
        # a split whose arrays do not build input_dim columns: the Python side, then the library itself
        with pytest.raises(ValueError, match="input_dim"):
            tr.set_data(plain_ds.__class__(ds.w, ds.z, ds.v[:, :, :1], 4, 3, ds.input_dim, 4))
        assert tr.lib.lg_tube_set_data(tr.h, 0, ptr(w), ptr(z), ptr(v), 5, 24, 2, 1) == -1 and "input_dim" in err(tr) and "+ 1" in err(tr)
        assert plain.lib.lg_tube_set_data(plain.h, 0, ptr(w), ptr(z), ptr(v), 5, 24, 2, 2) == 0
        assert tr.lib.lg_tube_set_data(tr.h, 0, ptr(w), ptr(z), ptr(v), 5, 24, 2, 2) == 0
        with pytest.raises(ValueError, match="horizon.*H_rev >= 1"):
            _trainer(hl.dataset(5, 24, 2, 2, 4, 0, seed=1), num_units=16, num_layers=1, batch_size=32)
        with pytest.raises(LeggedHipError, match="0..1"):
            tr.eval_level(1.5)
    finally:
        for t in (tr, plain, flat):
            t.close()


def _trainer_flat():
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    return HipTubeTrainer(20, 4, num_units=16, num_layers=1, loss="scalar_level", batch_size=32, device=DEV)


# ---------------------------------------------------------------- 8. end to end
def test_train_calibrate_evaluate_end_to_end(tmp_path):
    import calibrate_tube
    import evaluate_tube
    import train_tube
    from legged_gym_dev_amd.tube.calibrate import Calibration, default_path
    run = str(tmp_path / "run")
    sim = ["--sim_envs", "64", "--sim_T", "50"]
    train_tube.main(["--sim", "--sim_seed", "0", "--sim_refresh", "0", "--dataset", "scalar_horizon_level", "--H_fwd", "5", "--H_rev", "3",
                     "--out", run, "--num_epochs", "8", "--batch_size", "16", "--lr", "3e-3", "--seed", "3", "--steps_per_model_checkpoint", "10",
                     "--steps_per_model_evaluation", "10", "--device", DEV] + sim)      # 64 envs, 51 of them train: 4 steps per epoch, 32 steps
    cfg = json.load(open(os.path.join(run, "config.json")))
    assert cfg["dataset"] == "scalar_horizon_level" and cfg["level_input"] is True and cfg["loss"] == "scalar_level"
    recs = [json.loads(s) for s in open(os.path.join(run, "metrics.jsonl"))]
    assert max(r["step"] for r in recs) == 32
    evs = [r for r in recs if "Test Loss (level drawn)" in r]
    assert evs and all(f"Proportion Correct, fw > w (level={lv:.2f})" in evs[0] for lv in (0.5, 0.8, 0.9, 0.95))
    common = ["--run", run, "--sim", "--checkpoint", "latest", "--levels", "0.5,0.9", "--device", DEV]
    c = calibrate_tube.main(common + sim)
    assert os.path.isfile(default_path(run))
    saved = Calibration.load(default_path(run))
    W = 64 * len(range(3, 53 - 5))
    assert saved.kind == "horizon_levels" and saved.coverages == [0.5, 0.9] and saved.n == W and saved.provenance["sim_seed"] == 101
    assert tuple(saved.offsets.shape) == (2, 5) and bool(torch.isfinite(saved.offsets).all()) and torch.equal(saved.offsets, c.offsets)
    res = evaluate_tube.main(common + ["--calibration"])
    assert os.path.isfile(os.path.join(run, "eval.json"))
    ev = json.load(open(os.path.join(run, "eval.json")))
    assert [r["level"] for r in ev["levels"]] == [0.5, 0.9] and ev["dataset"] == "scalar_horizon_level" and ev["sim_seed"] == 1
    assert np.isfinite(ev["level_crossings"]) and 0.0 <= ev["level_crossings"] <= 1.0 and res["level_crossings"] == ev["level_crossings"]
    for r in ev["levels"]:
        m = r["calibrated"]["one_shot"]
        assert r["one_shot"]["windows"] == W and len(m["covered_by_step"]) == 5 and all(np.isfinite(v) for v in m["offset"])
        # no bound is asserted: the windows of one env overlap, so the rows are not exchangeable
        print(f"fresh robots, level {r['level']}: coverage {m['success_rate']:.4f} calibrated, {r['one_shot']['success_rate']:.4f} raw; "
              f"offsets {m['offset']}")
    print(f"level crossings: {ev['level_crossings']}")
    with pytest.raises(ValueError, match="--sim_seed 101 is the seed"):
        evaluate_tube.main(common + ["--calibration", "--sim_seed", "101"])
