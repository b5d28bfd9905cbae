"""Conformal calibration without a GPU (tube/calibrate.py, calibrate_tube.py, evaluate_tube.py --calibration): the rank in exact
arithmetic, the Calibration container (JSON round trip, apply / covers broadcasting against a float64 restatement, the in-sample
property), and the argument handling of the two scripts."""
import json
import math
import os
import sys

import pytest
import torch

from legged_gym_dev_amd.tube import calibrate as cal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))


def test_conformal_rank():
    assert cal.conformal_rank(9, 0.9) == 9
    assert cal.conformal_rank(19, 0.95) == 19
    assert math.ceil(100 * 0.07) == 8                                    # the float64 product the exact form avoids
    assert cal.conformal_rank(99, 0.07) == 7
    assert cal.conformal_rank(8, 0.9) == 9                               # > n: the offset is +inf
    assert cal.conformal_rank(99, "0.07") == 7
    for bad in (0, 1, 1.2, 0.0, 1.0, -0.1):
        with pytest.raises(ValueError, match="coverage"):
            cal.conformal_rank(10, bad)


def _sorted_offset(scores, keep, rank):
    """torch.sort restatement: the rank-th smallest kept score per column of scores (rows, columns); +inf outside 1..n_kept."""
    kept = scores[keep]
    if rank < 1 or rank > kept.shape[0]:
        return torch.full((scores.shape[1],), float("inf"))
    return torch.sort(kept.double(), dim=0).values[rank - 1].float()             # float64 holds every fp32 score exactly


def _flat_calibration(g, E=7, T=11, O=2, coverages=(0.5, 0.9)):
    fw1, fw2, w = (torch.randn(E, T, O, generator=g) for _ in range(3))
    done = torch.rand(E, T, generator=g) < 0.2
    keep = ~done.reshape(-1)
    n = int(keep.sum())
    ranks = [cal.conformal_rank(n, c) for c in coverages]
    offs = torch.stack([torch.stack([_sorted_offset((w - fw).reshape(-1, O), keep, r) for r in ranks]) for fw in (fw1, fw2)])
    return cal.Calibration("flat", coverages, offs, n, ranks, {"run": "r", "source": "sim", "sim_seed": 101}), (fw1, fw2), w, done


def test_json_round_trip_with_an_inf_offset(tmp_path):
    c = cal.Calibration("horizon", [0.9, 0.99], torch.tensor([[0.25, -1.5, 3.0], [float("inf")] * 3]), 50, [46, 51],
                        {"run": "/x", "checkpoint": "best", "dataset": "scalar_horizon", "data": "/d"})
    path = str(tmp_path / cal.CALIBRATION_NAME)
    c.save(path)
    text = open(path).read()
    json.loads(text, parse_constant=lambda s: pytest.fail(f"not strict JSON: {s}"))
    assert '"inf"' in text
    d = cal.Calibration.load(path)
    assert d.kind == c.kind and d.coverages == c.coverages and d.n == 50 and d.ranks == [46, 51] and d.provenance == c.provenance
    assert torch.equal(d.offsets, c.offsets) and d.offsets.dtype == torch.float32
    assert bool(d.covers(torch.zeros(4, 3), torch.full((4, 3), 1e30), 0.99).all())
    with pytest.raises(ValueError, match="NaN offset in set coverage 0.9, step ahead 2"):
        cal.Calibration("horizon", [0.9], torch.tensor([[0.0, float("nan")]]), 5, [5])
    assert len(c.lines()) == 6 and "rank 51 of n 50, offset inf" in c.lines()[-1]


def test_apply_and_covers_broadcast_for_the_three_kinds():
    g = torch.Generator().manual_seed(0)
    c, (fw1, fw2), w, done = _flat_calibration(g)
    for part, fw in (("one_step", fw1), ("rollout", fw2)):
        for i, cv in enumerate(c.coverages):
            q = c.offsets[cal.PARTS.index(part), i]
            assert torch.equal(c.apply(fw, cv, part=part), fw + q[None, None, :])
            want = (w - fw).double() <= q.double()[None, None, :]                   # float64 restatement on the fp32 score
            assert torch.equal(c.covers(fw, w, cv, part=part), want)
    with pytest.raises(KeyError, match="0.7 was not calibrated"):
        c.apply(fw1, 0.7)
    with pytest.raises(ValueError, match="no levels"):
        c.apply(fw1, 0.9, level=0.9)
    # levels: level l is calibrated to coverage l
    L = cal.Calibration("levels", [0.5, 0.9], torch.arange(8.0).reshape(2, 2, 2), 10, [6, 10])
    fw = torch.zeros(3, 5, 2)
    assert torch.equal(L.apply(fw, 0.9, part="rollout")[1, 2], torch.tensor([6.0, 7.0]))
    assert torch.equal(L.apply(fw, 0.5, level=0.5)[0, 0], torch.tensor([0.0, 1.0]))
    with pytest.raises(ValueError, match="level 0.5 is calibrated to coverage 0.5"):
        L.apply(fw, 0.9, level=0.5)
    # horizon: (windows, H_fwd) + (H_fwd)
    H = cal.Calibration("horizon", [0.9], torch.tensor([[1.0, 2.0, 3.0]]), 10, [10])
    assert torch.equal(H.apply(torch.zeros(4, 3), 0.9), torch.tensor([1.0, 2.0, 3.0]).expand(4, 3))
    assert H.covers(torch.zeros(4, 3), torch.full((4, 3), 2.0), 0.9).tolist() == [[False, True, True]] * 4


def test_in_sample_covers_counts_at_least_rank():
    g = torch.Generator().manual_seed(1)
    c, (fw1, fw2), w, done = _flat_calibration(g, E=9, T=13, O=3, coverages=(0.1, 0.5, 0.9, 0.99))
    keep = ~done
    for part, fw in (("one_step", fw1), ("rollout", fw2)):
        for cv, rank in zip(c.coverages, c.ranks):
            covered = (c.covers(fw, w, cv, part=part) & keep[:, :, None]).sum(dim=(0, 1))
            assert bool((covered >= min(rank, c.n)).all()), (part, cv)
            assert bool((covered == rank).all()) or rank > c.n                       # random scores have no ties
    # ties: the count may exceed the rank, never fall below it
    w = torch.tensor([0.0, 1.0, 1.0, 1.0, 2.0]).reshape(1, 5, 1)
    fw = torch.zeros(1, 5, 1)
    q = _sorted_offset((w - fw).reshape(-1, 1), torch.ones(5, dtype=torch.bool), 2)
    t = cal.Calibration("flat", [0.3], q.reshape(1, 1, 1).repeat(2, 1, 1), 5, [2])
    assert int(t.covers(fw, w, 0.3).sum()) == 4


def test_calibrate_tube_refuses_what_is_not_a_bound():
    import calibrate_tube
    a = calibrate_tube.parse_args(["--run", "/nonexistent", "--sim", "--dataset", "error_dynamics", "--activation", "relu"])
    cfg = calibrate_tube.et.resolve_config(a)
    with pytest.raises(ValueError, match="signed error, not a bound"):
        calibrate_tube.check_kind(cfg, a)
    with pytest.raises(ValueError, match="only bounds are calibrated"):
        cal.calibrate_flat(None, torch.zeros(1, 2, 3), torch.zeros(1, 2, 1), torch.zeros(1, 2), (1, 1, 1, 1), None, [0.9], kind="error_dynamics")
    a = calibrate_tube.parse_args(["--run", "/nonexistent", "--sim", "--dataset", "scalar", "--activation", "relu", "--coverage", "0.9,1.0"])
    with pytest.raises(ValueError, match="coverage must lie inside"):
        calibrate_tube.check_kind(calibrate_tube.et.resolve_config(a), a)
    a = calibrate_tube.parse_args(["--run", "/nonexistent", "--sim", "--dataset", "scalar", "--activation", "relu", "--coverage", "0.07,0.9"])
    assert calibrate_tube.check_kind(calibrate_tube.et.resolve_config(a), a) == [0.07, 0.9]
    a = calibrate_tube.parse_args(["--run", "/nonexistent", "--sim", "--dataset", "scalar_level", "--activation", "relu"])
    assert calibrate_tube.check_kind(calibrate_tube.et.resolve_config(a), a) == [0.5, 0.8, 0.9, 0.95]
    with pytest.raises(ValueError, match="--levels is for level-conditioned runs"):
        b = calibrate_tube.parse_args(["--run", "/nonexistent", "--sim", "--dataset", "vector", "--activation", "relu", "--levels", "0.5"])
        calibrate_tube.check_kind(calibrate_tube.et.resolve_config(b), b)
    # the default seed: the smallest seed >= 1 the run did not train with, plus 100
    a = calibrate_tube.parse_args(["--run", "/nonexistent", "--sim", "--sim_envs", "8", "--sim_T", "5"])
    assert calibrate_tube.sim_flags(a, {"seed": 1, "sim_seed": 2})["sim_seed"] == 103
    a = calibrate_tube.parse_args(["--run", "/nonexistent", "--sim", "--sim_seed", "7"])
    assert calibrate_tube.sim_flags(a, {"seed": 1})["sim_seed"] == 7


def test_evaluate_tube_refuses_the_calibrations_own_rows(tmp_path):
    import evaluate_tube
    run, data = str(tmp_path / "run"), str(tmp_path / "data")
    os.makedirs(run)
    g = torch.Generator().manual_seed(2)
    c, _, _, _ = _flat_calibration(g)
    c.provenance = {"run": run, "dataset": "scalar", "source": "sim", "sim_seed": 101, "sim_envs": 8, "sim_T": 5, "sim_resident": 1}
    c.save(cal.default_path(run))
    cfg = {"dataset": "scalar"}
    flags = ["--run", run, "--dataset", "scalar", "--activation", "relu"]
    a = evaluate_tube.parse_args(flags + ["--sim", "--calibration"])
    assert a.calibration == "" and evaluate_tube.parse_args(flags + ["--sim"]).calibration is None
    with pytest.raises(ValueError, match="--sim_seed 101 is the seed .* was calibrated on"):
        evaluate_tube.load_calibration(a, cfg, {"sim_seed": 101})
    got = evaluate_tube.load_calibration(a, cfg, {"sim_seed": 1})
    assert torch.equal(got.offsets, c.offsets)
    assert evaluate_tube.load_calibration(evaluate_tube.parse_args(flags + ["--sim"]), cfg, {"sim_seed": 101}) is None
    c.provenance = {"run": run, "dataset": "scalar", "data": os.path.abspath(data)}
    other = str(tmp_path / "elsewhere.json")
    c.save(other)
    a = evaluate_tube.parse_args(flags + ["--data", data, "--calibration", other])
    with pytest.raises(ValueError, match="is the folder .* was calibrated on"):
        evaluate_tube.load_calibration(a, cfg, None)
    a = evaluate_tube.parse_args(flags + ["--data", data + "2", "--calibration", other])
    assert evaluate_tube.load_calibration(a, cfg, None).n == c.n
    with pytest.raises(ValueError, match="calibrates a scalar model; the run is scalar_horizon"):
        evaluate_tube.load_calibration(a, {"dataset": "scalar_horizon"}, None)
    with pytest.raises(FileNotFoundError, match="calibrate_tube.py"):
        evaluate_tube.load_calibration(evaluate_tube.parse_args(flags + ["--sim", "--calibration", str(tmp_path / "none.json")]), cfg, None)
    assert evaluate_tube._cal_safe({"a": [float("inf"), 1.0], "b": 2}) == {"a": ["inf", 1.0], "b": 2}
