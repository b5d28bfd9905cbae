"""Train a one-shot tube from the simulator, calibrate it, then score, track and audit perturbed plans against it (DESIGN.md section
10.9), at the smallest shape section 10.8's end-to-end test uses.  Structure and consistency only: the plans are straight lines and
perturbed straight lines, not the generator's sample-and-hold signals, so they are not exchangeable with the training rows and no
coverage is promised -- measuring it is the point of the tool."""
import json
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))


def test_train_calibrate_score_track_audit(tmp_path):
    import audit_plans
    import calibrate_tube
    import train_tube
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.calibrate import Calibration, default_path
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim
    run, out = str(tmp_path / "run"), str(tmp_path / "audit")
    sim_flags = ["--sim_envs", "64", "--sim_T", "50"]
    train_tube.main(["--sim", "--sim_seed", "0", "--sim_refresh", "0", "--dataset", "scalar_horizon_level", "--H_fwd", "5", "--H_rev", "3",
                     "--out", run, "--num_epochs", "8", "--batch_size", "16", "--lr", "3e-3", "--seed", "3", "--steps_per_model_checkpoint", "10",
                     "--steps_per_model_evaluation", "10", "--device", DEV] + sim_flags)             # 32 steps
    calibrate_tube.main(["--run", run, "--sim", "--checkpoint", "latest", "--levels", "0.5,0.9", "--device", DEV] + sim_flags)
    calib = Calibration.load(default_path(run))
    assert calib.kind == "horizon_levels" and tuple(calib.offsets.shape) == (2, 5)
    # a 5-node problem: half a second of the gap problem's first stretch, 0.1 and 0.12 per second, between two small obstacles
    prob = pl.PlanProblem.named("gap", N=5, H_rev=3, goal=[0.35, 0.36], obs_c=[[0.36, 0.28], [0.28, 0.37]], obs_r=[0.02, 0.03])
    pj = str(tmp_path / "problem.json")
    json.dump(prob.to_json(), open(pj, "w"))
    argv = ["--run", run, "--checkpoint", "latest", "--problem_json", pj, "--warm_start", "interpolate", "--perturb", "63", "--sigma", "0.05",
            "--seed", "4", "--level", "0.9", "--device", DEV]
    res = audit_plans.main(argv + ["--calibration", "--out", out])
    saved = json.load(open(os.path.join(out, "audit.json")))
    assert saved == json.loads(json.dumps(res, allow_nan=False)) == res                    # the strict-JSON round trip
    assert res["plans"] == 64 and res["nodes"] == 6 and res["calibrated"] is True and res["problem"]["N"] == 5 and res["problem"]["H_rev"] == 3

    # the same through the library
    a = audit_plans.parse_args(argv)
    p = audit_plans.build_problem(a, audit_plans.run_config(run))
    z0, v, _ = audit_plans.build_plans(a, p)
    assert tuple(v.shape) == (64, 5, 2) and float(v.abs().max()) <= 0.2 + 1e-7 and float(v[1:].std()) > 0.03
    model, sim = HipTubeModel.load(run, checkpoint="latest", device=DEV), HipRomSim(audit_plans.sim_config(a, p), device=DEV)
    try:
        cal = pl.HipPlanScorer(model, p, calibration=calib, level=0.9).score(z0, v)
        raw = pl.HipPlanScorer(model, p, level=0.9).score(z0, v)
        t = pl.track(sim, cal["z"], v)
        lib = pl.audit(cal, t, p)
        lib_raw = pl.audit(raw, t, p)
    finally:
        model.close()
        sim.close()
    for k, val in lib.items():
        assert res[k] == val, k                                                                # the script's audit.json is the library call
    for r in (lib, lib_raw):
        shares = r["coverage_by_node"] + [r["coverage"], r["covered_plans"], r["predicted_safe"], r["actually_safe"]] + list(r["table"].values())
        assert all(0.0 <= s <= 1.0 for s in shares) and len(r["coverage_by_node"]) == 6
        assert abs(sum(r["table"].values()) - 1.0) < 1e-12
        assert abs(r["table"]["safe_safe"] + r["table"]["safe_unsafe"] - r["predicted_safe"]) < 1e-12
        assert abs(r["table"]["safe_safe"] + r["table"]["unsafe_safe"] - r["actually_safe"]) < 1e-12
        assert r["w_true_max"] >= r["w_true_mean"] >= 0.0
        assert json.loads(json.dumps(r, allow_nan=False)) == r
    off = calib.offset(level=0.9)
    assert torch.equal(cal["fw"], raw["fw"]) and torch.equal(cal["z"], raw["z"])
    up = (off >= 0).nonzero().reshape(-1) + 1
    assert bool((cal["w"][:, up] >= raw["w"][:, up]).all()) and torch.equal(cal["w"][:, 0], raw["w"][:, 0])
    assert torch.equal(cal["w"][:, 1:], raw["fw"] + off.to(DEV))
    assert lib["coverage"] >= lib_raw["coverage"] or bool((off < 0).any())
    print(f"perturbed straight-line plans, level 0.9: coverage {lib['coverage']:.4f} calibrated, {lib_raw['coverage']:.4f} raw; per node "
          f"{[round(c, 3) for c in lib['coverage_by_node']]}; offsets {off.tolist()}; realised error mean {lib['w_true_mean']:.4f}")


def test_plans_from_a_file_are_audited_as_they_are(tmp_path):
    """--plans F.npz, the way plans from any solver come in: the count in audit.json is the number of plans, the file's name sits
    under "source", and the audit equals the library call on the file's arrays."""
    import numpy as np
    import audit_plans
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim
    B, N = 37, 9
    g = torch.Generator().manual_seed(6)
    z0 = 0.3 + 0.1 * torch.rand(B, 2, generator=g)
    v = 0.15 * (2 * torch.rand(B, N, 2, generator=g) - 1)
    f, out = str(tmp_path / "plans.npz"), str(tmp_path / "out")
    np.savez(f, z0=z0.numpy(), v=v.numpy())
    argv = ["--tube", "l1_rolling", "--window_size", "3", "--scaling", "0.4", "--N", str(N), "--problem", "gap", "--plans", f, "--device", DEV]
    res = audit_plans.main(argv + ["--out", out])
    saved = json.load(open(os.path.join(out, "audit.json")))
    assert saved == res and res["plans"] == B and res["nodes"] == N + 1 and res["source"] == {"plans_file": f} and res["tube"] == "l1_rolling"
    a = audit_plans.parse_args(argv)
    p = audit_plans.build_problem(a, None)
    sim = HipRomSim(audit_plans.sim_config(a, p), device=DEV)
    try:
        s = pl.HipPlanScorer(None, p, device=DEV).score(z0, v)
        lib = pl.audit(s, pl.track(sim, s["z"], v), p)
    finally:
        sim.close()
    for k, val in lib.items():
        assert res[k] == val, k
    assert res["best_plan"] == int(s["cost"].argmin()) and 0.0 < res["w_true_max"]
    np.savez(f, z0=z0.numpy())
    with pytest.raises(ValueError, match="'v'"):
        audit_plans.main(argv)
