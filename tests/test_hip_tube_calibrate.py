"""Conformal calibration on the GPU (tube/calibrate.py on lg_select_kth, calibrate_tube.py, evaluate_tube.py --calibration; DESIGN.md
section 10.6).  Models are untrained but seeded; the offsets must equal, bit for bit, the torch.sort selection on the CPU over
target - prediction with the device predictions copied back."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
INF = float("inf")
E, T = 8, 40


def _model(I, O, U, L, act, beta=1.0, level=False, horizon=None, seed=5):
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    tr = HipTubeTrainer(I, O, num_units=U, num_layers=L, activation=act, softplus_beta=beta, loss="scalar_level" if level else "scalar",
                        batch_size=32, seed=seed, horizon=horizon, device=DEV)
    try:
        sd = tr.state_dict()
    finally:
        tr.close()
    return HipTubeModel(sd, activation=act, softplus_beta=beta, horizon=horizon, device=DEV, level_input=level)


def _records(seed, n=2, done_p=0.1):
    """Random records of 8 envs x 40 steps with n = m = 2: scalar rows are 3 wide, vector rows 6; about a tenth of the steps done."""
    g = torch.Generator().manual_seed(seed)
    rec = {"z": torch.randn(E, T + 1, n, generator=g), "pz_x": torch.randn(E, T + 1, n, generator=g), "v": torch.randn(E, T, 2, generator=g),
           "done": (torch.rand(E, T, generator=g) < done_p).to(torch.uint8)}
    return {k: v.to(DEV) for k, v in rec.items()}


def _cfg(kind, **kw):
    return {"dataset": kind, "N": 1, "dN": 1, "recursive": False, "H_fwd": 5, "H_rev": 2, "activation": "relu", "softplus_beta": 1.0, **kw}


def _cpu_offsets(fw, w, done, ranks):
    """(n_ranks, out): torch.sort over the kept rows of the fp32 score w - fw, on the CPU."""
    O = w.shape[-1]
    scores = (w.cpu() - fw.cpu()).reshape(-1, O)
    s = torch.sort(scores[~done.cpu().reshape(-1).bool()], dim=0).values
    return torch.stack([s[r - 1] if 1 <= r <= s.shape[0] else torch.full((O,), INF) for r in ranks])


def _same_bits(a, b, what=""):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), what


FLAT = [("scalar", 3, 1, 16, 1, "relu", 1.0), ("vector", 6, 2, 32, 2, "softplus", 5.0)]


@pytest.mark.parametrize("case", FLAT, ids=lambda c: c[0])
def test_flat_offsets_equal_the_cpu_selection(case):
    import calibrate_tube
    import evaluate_tube
    kind, I, O, U, L, act, beta = case
    raw = _records(1)
    done = raw["done"].ne(0)
    coverages = [0.07, 0.5, 0.9, 0.999]                                  # 0.999 needs more rows than 8 x 40 has: +inf
    model = _model(I, O, U, L, act, beta)
    try:
        a = calibrate_tube.parse_args(["--run", "unused", "--sim", "--horizon", "10"])
        c = calibrate_tube.calibrate(model, _cfg(kind), raw, a, coverages, torch.device(DEV))
        res, series = evaluate_tube.evaluate_flat(model, _cfg(kind), raw, 10, torch.device(DEV), calib=c)
    finally:
        model.close()
    n = int((~done).sum())
    assert c.kind == "flat" and c.n == n and 0 < n < E * T and tuple(c.offsets.shape) == (2, 4, O)
    assert c.ranks[-1] == n + 1 and c.ranks[0] == -(-(n + 1) * 7 // 100)
    w, keep = series["w"], ~done[:, :, None]
    for p, part in enumerate(("one_step", "rollout")):
        fw = series["fw_single" if part == "one_step" else "fw"]
        _same_bits(c.offsets[p], _cpu_offsets(fw, w, done, c.ranks), part)
        for i, (cv, rank) in enumerate(zip(c.coverages, c.ranks)):
            covered = (c.covers(fw, w, cv, part=part) & keep).sum(dim=(0, 1))
            m = res["calibrated"][part][i]
            assert m["covered"] == int(covered.sum())
            assert round(m["success_rate"] * m["elements"]) == int(((c.apply(fw, cv, part=part) >= w) & keep).sum())
            if rank <= n:
                assert covered.tolist() == [rank] * O, (part, cv)       # random targets: no ties
            else:
                assert bool(torch.isinf(c.offsets[p, i]).all()) and covered.tolist() == [n] * O and m["offset"] == ["inf"] * O
                assert bool(c.covers(fw, w, cv, part=part).all())
    # a done row's target belongs to the next episode: moving it must not move an offset
    model = _model(I, O, U, L, act, beta)
    try:
        spoiled = dict(raw)
        for k in ("z", "pz_x"):
            spoiled[k] = raw[k].clone()
        t_done = done.nonzero()
        spoiled["pz_x"][t_done[:, 0], t_done[:, 1] + 1] += 1e6
        spoiled["done"] = raw["done"] | torch.cat((torch.zeros_like(raw["done"][:, :1]), raw["done"][:, :-1]), dim=1)   # and the row it feeds
        ref = dict(raw, done=spoiled["done"])
        a = calibrate_tube.parse_args(["--run", "unused", "--sim"])
        c1 = calibrate_tube.calibrate(model, _cfg(kind), spoiled, a, [0.5, 0.9], torch.device(DEV))
        c2 = calibrate_tube.calibrate(model, _cfg(kind), ref, a, [0.5, 0.9], torch.device(DEV))
    finally:
        model.close()
    _same_bits(c1.offsets[0], c2.offsets[0], "one-step offsets with the done rows' targets moved")
    assert float(c1.offsets[0].max()) < 1e5


LEVEL = [("scalar_level", 3, 1, 16, 1, "relu", 1.0), ("vector_level", 6, 2, 32, 2, "softplus", 5.0)]


@pytest.mark.parametrize("case", LEVEL, ids=lambda c: c[0])
def test_level_offsets_per_level(case):
    import evaluate_tube
    from legged_gym_dev_amd.tube import calibrate as cal
    from legged_gym_dev_amd.tube import evaluate as ev
    from legged_gym_dev_amd.tube.data import feedback_layout
    kind, I, O, U, L, act, beta = case
    raw = _records(2)
    levels = [0.5, 0.8, 0.9, 0.95]
    cfg = _cfg(kind, activation=act, softplus_beta=beta)
    model = _model(I + 1, O, U, L, act, beta, level=True)
    try:
        data, target, done = evaluate_tube.rows(kind, raw, {"N": 1, "dN": 1, **({"recursive": False} if O == 1 else {})}, torch.device(DEV))
        layout = feedback_layout(kind, 1, 1, False, n=2, m=2)
        reseed = ev.reseed_mask(done, None)
        c, series = cal.calibrate_levels(model, data, target, done, layout, reseed, levels)
        _same_bits(series["fw_single"][2], model.predict(model.with_level(data, 0.9).reshape(E * T, I + 1)).reshape(E, T, O))
        res, last = evaluate_tube.evaluate_levels(model, cfg, raw, None, torch.device(DEV), levels, calib=c)
    finally:
        model.close()
    n = int((~done).sum())
    assert c.kind == "levels" and c.coverages == levels and tuple(c.offsets.shape) == (2, 4, O) and c.n == n
    keep = ~done[:, :, None]
    for p, name in enumerate(("fw_single", "fw")):
        for l, (lv, rank) in enumerate(zip(levels, c.ranks)):
            fw = series[name][l]
            _same_bits(c.offsets[p, l], _cpu_offsets(fw, target, done, [rank])[0], f"{name}, level {lv}")
            covered = (c.covers(fw, target, lv, level=lv, part=cal.PARTS[p]) & keep).sum(dim=(0, 1))
            assert covered.tolist() == [rank] * O
            m = res["levels"][l]["calibrated"][cal.PARTS[p]]
            assert m["covered"] == rank * O and res["levels"][l]["calibrated"]["rank"] == rank
            assert round(m["success_rate"] * m["elements"]) == int(((c.apply(fw, lv, part=cal.PARTS[p]) >= target) & keep).sum())
    _same_bits(last["fw"], series["fw"][-1])


def test_horizon_offsets_per_step_ahead():
    import calibrate_tube
    import evaluate_tube
    raw = _records(3, n=4, done_p=0.0)                                   # z without its position is 2 wide: input 2 + 2 + 7 * 2
    cfg = _cfg("scalar_horizon")
    model = _model(18, 5, 32, 2, "relu", horizon=(5, 2))
    try:
        a = calibrate_tube.parse_args(["--run", "unused", "--sim", "--window_stride", "3"])
        c = calibrate_tube.calibrate(model, cfg, raw, a, [0.5, 0.9, 0.99], torch.device(DEV))
        res, series = evaluate_tube.evaluate_horizon(model, cfg, raw, 3, torch.device(DEV), calib=c)
    finally:
        model.close()
    fw, w = series["fw"].reshape(-1, 5), series["w"].reshape(-1, 5)
    W = fw.shape[0]
    assert c.kind == "horizon" and c.n == W == E * res["windows_per_env"] and tuple(c.offsets.shape) == (3, 5)
    assert c.ranks == [-(-(W + 1) // 2), -(-(W + 1) * 9 // 10), -(-(W + 1) * 99 // 100)]
    _same_bits(c.offsets, _cpu_offsets(fw, w, torch.zeros(W, dtype=torch.bool), c.ranks))
    for i, (cv, rank) in enumerate(zip(c.coverages, c.ranks)):
        covered = c.covers(fw, w, cv).sum(dim=0).tolist()
        assert covered == [min(rank, W)] * 5 and res["calibrated"]["one_shot"][i]["covered_by_step"] == covered
        assert round(res["calibrated"]["one_shot"][i]["success_rate"] * W * 5) == int((c.apply(fw, cv) >= w).sum())


def test_scripts_end_to_end_on_the_simulator(tmp_path):
    import calibrate_tube
    import evaluate_tube
    import train_tube
    from legged_gym_dev_amd.tube.calibrate import Calibration, default_path
    from legged_gym_dev_amd.tube.model import HipTubeModel
    run = str(tmp_path / "run")
    sim = ["--sim_envs", "64", "--sim_T", "50"]
    train_tube.main(["--sim", "--sim_seed", "0", "--sim_refresh", "0", "--out", run, "--num_epochs", "3", "--batch_size", "256", "--seed", "3",
                     "--device", DEV] + sim)                             # 63 x 50 rows, 0.8 of them train: 10 steps per epoch
    c = calibrate_tube.main(["--run", run, "--sim", "--checkpoint", "latest"] + sim)
    saved = Calibration.load(default_path(run))
    assert saved.provenance["sim_seed"] == 101 and saved.provenance["source"] == "sim" and saved.provenance["checkpoint"] == "latest"
    assert saved.kind == "flat" and saved.coverages == [0.9, 0.95] and saved.n == 64 * 50 and torch.equal(saved.offsets, c.offsets)
    assert saved.ranks == [2881, 3041] and bool(torch.isfinite(saved.offsets).all())
    plain_out, cal_out = str(tmp_path / "plain"), str(tmp_path / "cal")
    common = ["--run", run, "--sim", "--checkpoint", "latest", "--device", DEV]
    evaluate_tube.main(common + ["--out", plain_out])
    res = evaluate_tube.main(common + ["--out", cal_out, "--calibration"])
    plain, withc = (json.load(open(os.path.join(d, "eval.json"))) for d in (plain_out, cal_out))
    assert sorted(set(withc) - set(plain)) == ["calibrated", "calibration"] and list(plain) == [k for k in withc if k in plain]
    for k in plain:
        assert plain[k] == withc[k], k
    assert withc["sim_seed"] == 1 and withc["calibrated"]["coverages"] == [0.9, 0.95]
    # the same predictions once more: the success rates are counts of fw + q >= w, "covered" counts of w - fw <= q
    flags = {k: withc[k] for k in ("sim_envs", "sim_T", "sim_seed", "sim_resident")}
    raw = evaluate_tube.sim_records(flags, DEV)
    model = HipTubeModel.load(run, checkpoint="latest", device=DEV)
    try:
        rcfg = evaluate_tube.resolve_config(evaluate_tube.parse_args(["--run", run, "--sim"]))
        _, s = evaluate_tube.evaluate_flat(model, rcfg, raw, None, torch.device(DEV))
    finally:
        model.close()
    for part, name in (("one_step", "fw_single"), ("rollout", "fw")):
        for i, cv in enumerate(saved.coverages):
            m = withc["calibrated"][part][i]
            q = saved.offset(cv, part=part).to(DEV)
            assert m["elements"] == 64 * 50 and m["offset"] == q.tolist()
            assert round(m["success_rate"] * m["elements"]) == int((s[name] + q >= s["w"]).sum())
            assert m["covered"] == int(((s["w"] - s[name]) <= q).sum())
            print(f"fresh robots, {part}, coverage {cv}: offset {q.tolist()}, covered {m['covered']} of {m['elements']} = "
                  f"{m['covered'] / m['elements']:.4f} (uncalibrated {withc[part]['success_rate']:.4f})")
    with pytest.raises(ValueError, match="--sim_seed 101 is the seed"):
        evaluate_tube.main(common + ["--out", cal_out, "--calibration", "--sim_seed", "101"])
    assert res["calibration"] == os.path.abspath(default_path(run))
