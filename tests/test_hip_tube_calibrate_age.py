"""Per-age and per-trajectory calibration on the GPU (tube/calibrate.py calibrate_by_age / calibrate_trajectory on lg_select_kth_grouped,
calibrate_tube.py --by_age --trajectory, evaluate_tube.py --age_calibration).  Models are untrained but seeded;
offsets, counts, ranks and margins must equal, bit for bit, the torch.sort restatement on the CPU over target - roll-out with the
device's roll-out copied back.  The refusals of the scripts need no GPU."""
import json
import os
import sys

import pytest
import torch

gpu = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
INF = float("inf")
E, T, K = 64, 40, 10
CASES = [("scalar", 3, 1, 32, 2, "relu"), ("vector", 6, 2, 16, 1, "tanh")]
COVERAGES = [0.5, 0.9, 0.999]                                # 0.999 needs more steps than an age has: +inf


def _model(I, O, U, L, act, seed=5):
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    tr = HipTubeTrainer(I, O, num_units=U, num_layers=L, activation=act, softplus_beta=1.0, loss="scalar", batch_size=32, seed=seed, device=DEV)
    try:
        sd = tr.state_dict()
    finally:
        tr.close()
    return HipTubeModel(sd, activation=act, softplus_beta=1.0, device=DEV)


def _rows(kind, seed):
    """64 envs x 40 steps with n = m = 2 (scalar rows 3 wide, vector rows 6), a few sparse dones, reseeded every 10 steps: 10 ages."""
    import evaluate_tube
    from legged_gym_dev_amd.tube import evaluate as ev
    from legged_gym_dev_amd.tube.data import feedback_layout
    g = torch.Generator().manual_seed(seed)
    raw = {"z": torch.randn(E, T + 1, 2, generator=g), "pz_x": torch.randn(E, T + 1, 2, generator=g), "v": torch.randn(E, T, 2, generator=g),
           "done": (torch.rand(E, T, generator=g) < 0.02).to(torch.uint8)}
    raw = {k: v.to(DEV) for k, v in raw.items()}
    data, target, done = evaluate_tube.rows(kind, raw, {"N": 1, "dN": 1, **({"recursive": False} if kind == "scalar" else {})}, torch.device(DEV))
    assert 0 < int(done.sum()) < E * T // 10
    return data, target, done, feedback_layout(kind, 1, 1, False, n=2, m=2), ev.reseed_mask(done, K)


def _cpu_by_age(scores, group, G, coverages):
    """scores (rows, out), group (rows) on the CPU -> offsets (coverages, G, out), counts (G), ranks (G, coverages) by torch.sort."""
    from legged_gym_dev_amd.tube.calibrate import conformal_rank
    O = scores.shape[1]
    q = torch.full((len(coverages), G, O), INF)
    counts, ranks = torch.zeros(G, dtype=torch.int64), torch.zeros(G, len(coverages), dtype=torch.int64)
    for a in range(G):
        s = torch.sort(scores[group == a], dim=0).values
        counts[a] = s.shape[0]
        for c, cv in enumerate(coverages):
            ranks[a, c] = conformal_rank(s.shape[0], cv)
            if ranks[a, c] <= s.shape[0]:
                q[c, a] = s[ranks[a, c] - 1]
    return q, counts, ranks


def _cpu_groups(done, reseed, G):
    from legged_gym_dev_amd.tube import evaluate as ev
    age = ev.steps_since(reseed.cpu())
    return torch.where(~done.cpu().bool(), age.clamp(max=G - 1), torch.full_like(age, -1))


def _same_bits(a, b, what=""):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    assert a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32)), what


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_offsets_per_age_equal_the_cpu_selection(case):
    from legged_gym_dev_amd.tube import calibrate as cal
    from legged_gym_dev_amd.tube import evaluate as ev
    kind, I, O, U, L, act = case
    data, target, done, layout, reseed = _rows(kind, 1)
    model = _model(I, O, U, L, act)
    try:
        q, counts, ranks = cal.calibrate_by_age(model, data, target, done, layout, reseed, COVERAGES, kind)
        q4, counts4, ranks4 = cal.calibrate_by_age(model, data, target, done, layout, reseed, COVERAGES, kind, max_age=4)
        some = torch.arange(5, E, 3)
        qe, countse, rankse = cal.calibrate_by_age(model, data, target, done, layout, reseed, COVERAGES, kind, envs=some.to(DEV))
        fw = model.rollout_window(data, *layout, reseed)
        fw_some = model.rollout_window(data[some.to(DEV)], *layout, reseed[some.to(DEV)])
    finally:
        model.close()
    assert tuple(q.shape) == (3, K, O) and tuple(counts.shape) == (K,) and tuple(ranks.shape) == (K, 3)
    scores = (target.cpu() - fw.cpu()).reshape(E * T, O)
    group = _cpu_groups(done, reseed, K)
    assert sorted(set(group.reshape(-1).tolist())) == [-1] + list(range(K))
    want = _cpu_by_age(scores, group.reshape(-1), K, COVERAGES)
    _same_bits(q, want[0], "offsets per age")
    assert torch.equal(counts.cpu(), want[1]) and torch.equal(ranks.cpu(), want[2])
    assert int(counts.sum()) == int((~done).sum()) and bool(torch.isinf(q[2]).all()) and bool(torch.isfinite(q[:2]).all())
    # on the calibration rows the offset of an age covers at least rank of that age's rows
    c = cal.AgeCalibration(COVERAGES, q, counts, ranks)
    age = ev.steps_since(reseed)
    for i, cv in enumerate(COVERAGES):
        covered = c.covers(fw, target, age, cv).cpu()
        for a in range(K):
            got = covered[group == a].sum(dim=0)
            need = min(int(ranks[a, i]), int(counts[a]))                 # an infinite offset covers the age's every row
            assert bool((got >= need).all()) and (i < 2 or got.tolist() == [int(counts[a])] * O), (cv, a)
            if i < 2:
                assert got.tolist() == [need] * O                        # random targets: no ties
    # max_age = 4: ages 3.. share group 3
    want4 = _cpu_by_age(scores, _cpu_groups(done, reseed, 4).reshape(-1), 4, COVERAGES)
    _same_bits(q4, want4[0], "max_age = 4")
    assert torch.equal(counts4.cpu(), want4[1]) and torch.equal(ranks4.cpu(), want4[2])
    assert torch.equal(counts4[:3], counts[:3]) and int(counts4[3]) == int(counts[3:].sum())
    _same_bits(q4[:, :3], q[:, :3], "the ages below the pooled group")
    # a subset of the envs
    sub = (target.cpu()[some] - fw_some.cpu()).reshape(-1, O)
    wante = _cpu_by_age(sub, group[some].reshape(-1), K, COVERAGES)
    _same_bits(qe, wante[0], "envs = 5, 8, 11, ...")
    assert torch.equal(countse.cpu(), wante[1]) and torch.equal(rankse.cpu(), wante[2])


@gpu
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0])
def test_trajectory_margin(case):
    from legged_gym_dev_amd.tube import calibrate as cal
    from legged_gym_dev_amd.tube import evaluate as ev
    kind, I, O, U, L, act = case
    data, target, done, layout, reseed = _rows(kind, 2)
    coverages = [0.5, 0.9, 0.99]                                         # 0.99 of 32 margin envs: rank 33, an infinite margin
    even, odd = torch.arange(0, E, 2), torch.arange(1, E, 2)
    model = _model(I, O, U, L, act)
    try:
        c = cal.calibrate_trajectory(model, data, target, done, layout, reseed, coverages, kind)
        q_even = cal.calibrate_by_age(model, data, target, done, layout, reseed, coverages, kind, envs=even.to(DEV))
        moved = target.clone()
        moved[odd.to(DEV)] += 3.0
        c_moved = cal.calibrate_trajectory(model, data, moved, done, layout, reseed, coverages, kind)
        fw_odd = model.rollout_window(data[odd.to(DEV)], *layout, reseed[odd.to(DEV)])
    finally:
        model.close()
    assert c.max_age == K and tuple(c.offsets.shape) == (3, K, O) and tuple(c.margin.shape) == (3, O)
    assert c.margin_n == E // 2 and c.margin_ranks == [17, 30, 33]
    # the offsets come from the even envs alone
    _same_bits(c.offsets, q_even[0], "q against calibrate_by_age on the even envs")
    assert c.counts == q_even[1].tolist() and c.ranks == q_even[2].tolist()
    _same_bits(c_moved.offsets, c.offsets, "an odd env's target moved")
    assert bool((c_moved.margin[:2] > c.margin[:2] + 2.9).all())
    # delta: the restatement on the CPU
    group = _cpu_groups(done, reseed, K)[odd]                            # (32, T)
    r = target.cpu()[odd] - fw_odd.cpu()                                 # (32, T, out)
    s = r[None] - c.offsets[:, group.clamp(min=0)]                       # (coverages, 32, T, out)
    s = torch.where((group >= 0)[None, :, :, None], s, torch.full_like(s, -INF)).amax(dim=2)
    srt = torch.sort(s, dim=1).values                                    # over the envs
    want = torch.stack([srt[i, k - 1] if k <= E // 2 else torch.full((O,), INF) for i, k in enumerate(c.margin_ranks)])
    _same_bits(c.margin, want, "delta")
    assert bool(torch.isinf(c.margin[2]).all()) and bool(torch.isfinite(c.margin[:2]).all())
    # on the margin half at least margin_rank envs lie inside fw + q + delta at every kept step
    age = ev.steps_since(reseed)[odd.to(DEV)]
    for i, cv in enumerate(coverages):
        covered = c.covers(fw_odd, target[odd.to(DEV)], age, cv, trajectory=True)
        whole = (covered | done[odd.to(DEV)][:, :, None]).all(dim=1).sum(dim=0).tolist()
        need = min(c.margin_ranks[i], E // 2)
        assert all(w >= need for w in whole) and (i == 2 or whole == [need] * O), (cv, whole)
        rate = ev.trajectory_metrics(covered, done[odd.to(DEV)])["trajectory_success_rate"]
        assert rate == [w / (E // 2) for w in whole]


@gpu
def test_scripts_end_to_end_on_the_simulator(tmp_path):
    import calibrate_tube
    import evaluate_tube
    import train_tube
    from legged_gym_dev_amd.tube.calibrate import AgeCalibration, default_age_path, default_path
    run = str(tmp_path / "run")
    sim = ["--sim_envs", "64", "--sim_T", "50"]
    train_tube.main(["--sim", "--sim_seed", "0", "--sim_refresh", "0", "--out", run, "--num_epochs", "3", "--batch_size", "256", "--seed", "3",
                     "--device", DEV] + sim)
    plain_dir = str(tmp_path / "plain")
    cal_args = ["--run", run, "--sim", "--checkpoint", "latest", "--horizon", "10"] + sim
    calibrate_tube.main(cal_args + ["--out", plain_dir])
    assert not os.path.exists(os.path.join(plain_dir, "calibration_age.json"))
    calibrate_tube.main(cal_args + ["--by_age", "--trajectory"])
    assert open(default_path(run), "rb").read() == open(os.path.join(plain_dir, "calibration.json"), "rb").read()
    c = AgeCalibration.load(default_age_path(run))
    assert c.coverages == [0.9, 0.95] and c.max_age == 10 and tuple(c.offsets.shape) == (2, 10, 1) and c.counts == [32 * 5] * 10
    assert c.ranks == [[145, 153]] * 10 and c.margin_n == 32 and c.margin_ranks == [30, 32] and tuple(c.margin.shape) == (2, 1)
    assert c.provenance["sim_seed"] == 101 and c.provenance["reseed_every"] == 10 and c.provenance["source"] == "sim"
    assert bool(torch.isfinite(c.offsets).all()) and bool(torch.isfinite(c.margin).all())
    plain_out, age_out = str(tmp_path / "eval_plain"), str(tmp_path / "eval_age")
    common = ["--run", run, "--sim", "--checkpoint", "latest", "--device", DEV, "--horizon", "10"]
    evaluate_tube.main(common + ["--out", plain_out])
    res = evaluate_tube.main(common + ["--out", age_out, "--age_calibration"])
    plain, witha = (json.load(open(os.path.join(d, "eval.json"))) for d in (plain_out, age_out))
    assert sorted(set(witha) - set(plain)) == ["age_calibration", "calibrated_by_age"] and list(plain) == [k for k in witha if k in plain]
    for k in plain:
        assert plain[k] == witha[k], k
    assert res["age_calibration"] == os.path.abspath(default_age_path(run))
    ba = witha["calibrated_by_age"]
    assert ba["coverages"] == [0.9, 0.95] and ba["max_age"] == 10 and sorted(ba["trajectory"]) == ["by_age", "by_age_margin", "raw"]
    assert len(ba["trajectory"]["raw"]["trajectory_success_rate"]) == 1 and ba["trajectory"]["raw"]["envs"] == 64
    for i, cv in enumerate(c.coverages):
        m = ba["rollout"][i]
        assert m["elements"] == 64 * 50 and sum(m["covered_by_age"]) == m["covered"] and len(m["covered_by_age"]) == 10
        by_age = " ".join(f"{n / 320:.3f}" for n in m["covered_by_age"])
        print(f"fresh robots, coverage {cv}: covered per age [{by_age}], overall {m['covered'] / m['elements']:.4f} "
              f"(uncalibrated {witha['rollout']['success_rate']:.4f}); whole trajectories: raw "
              f"{ba['trajectory']['raw']['trajectory_success_rate'][0]:.4f}, per age {ba['trajectory']['by_age'][i]['trajectory_success_rate'][0]:.4f}, "
              f"per age + margin {ba['trajectory']['by_age_margin'][i]['trajectory_success_rate'][0]:.4f}")
        r = [ba["trajectory"][k][i]["trajectory_success_rate"][0] for k in ("by_age", "by_age_margin")]
        assert all(0.0 <= v <= 1.0 for v in r)                            # no bound is asserted on the rates: 32 margin envs
    with pytest.raises(ValueError, match="--sim_seed 101 is the seed"):
        evaluate_tube.main(common + ["--out", age_out, "--age_calibration", "--sim_seed", "101"])


@pytest.mark.parametrize("dataset, reason", [("scalar_level", "level-conditioned"), ("vector_level", "level-conditioned"),
                                             ("scalar_horizon", "already has one offset per step ahead"),
                                             ("error_dynamics", "signed error, not a bound")])
def test_by_age_is_refused_with_a_reason(tmp_path, dataset, reason):
    import calibrate_tube
    with pytest.raises(ValueError, match="--by_age: .*" + reason):
        calibrate_tube.main(["--run", str(tmp_path / "none"), "--dataset", dataset, "--activation", "relu", "--sim", "--by_age"])
    assert not os.path.exists(str(tmp_path / "none"))


def test_trajectory_needs_by_age(tmp_path):
    import calibrate_tube
    import evaluate_tube
    base = ["--run", str(tmp_path / "none"), "--dataset", "scalar", "--activation", "relu", "--sim"]
    with pytest.raises(ValueError, match="--trajectory needs --by_age"):
        calibrate_tube.main(base + ["--trajectory"])
    with pytest.raises(ValueError, match="--max_age needs --by_age"):
        calibrate_tube.main(base + ["--max_age", "5"])
    with pytest.raises(ValueError, match="--max_age must be 1..1024"):
        calibrate_tube.main(base + ["--by_age", "--max_age", "1025"])
    assert not os.path.exists(str(tmp_path / "none"))
    with pytest.raises(ValueError, match="--age_calibration: per-age offsets exist for the roll-out of the flat kinds"):
        evaluate_tube.main(["--run", str(tmp_path / "none"), "--dataset", "scalar_horizon", "--activation", "relu", "--sim", "--age_calibration"])
