"""The gradient planner on the GPU (k_plan_grad): the forward half against the audited kernels on the bits;
dJ/dv against the float64 autograd restatement (tests/plan_grad_ref.py) under the chain yardstick of sections 10.1 / 10.2, away from
kinks; batch independence; the fused Adam step, the projection and the elite; lg_plan_descend against its steps; that it plans; the
closed loop against the same steps composed by hand.

The inputs are tests/test_hip_mppi.py's `_instances`, called with its own dt argument at 0.105 while the problem's dt stays 0.1: at
dt = 0.1 instance 0's nodes land on rom_z_max[0] = 0.35 to within 1e-8 (node 7 of N = 8, node 56 of N = 64), a kink of the state hinge
that would exclude instance 0 from every comparison.  At 0.105 its mean plan still starts outside rom_z_min, crosses the first
obstacle's centre and passes rom_z_max, so the obstacle, tube and state hinges all bind on it, at a distance from their kinks.
Instance 0's vy is exactly 0: for the l1 kinds that is the stated tie sign(0) = 0, not a kink (tests/plan_grad_ref.py objective)."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import plan_grad_ref as gr
from tests.test_hip_mppi import _J_of, _analytic, _instances, _ref_problem, _same, _trainer, _yardstick

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
RHO = dict(rho_g=1e4, rho_w=30.0, rho_z=7.0)
KINK = 1e-4                                                              # a plan is compared where its smallest float64 margin is at least this
SHAPES = [(1, 1), (3, 8), (33, 8), (2, 64)]                              # B x N: one plan, a partial tile, a tile boundary, the longest horizon
# tube: (name, kind, H_rev, model (units, layers, activation, beta, level-conditioned with an offset) or None)
TUBES = [("l2", "l2", 0, None), ("l1_rolling", "l1_rolling", 0, None), ("softplus5-Hr1", "nn", 1, (16, 1, "softplus", 5.0, False)),
         ("softplus5-Hr3", "nn", 3, (16, 1, "softplus", 5.0, False)), ("tanh-2x32", "nn", 3, (32, 2, "tanh", 1.0, False)),
         ("level-offset", "nn", 3, (16, 1, "softplus", 5.0, True))]
CASES = [(f"{t[0]}-{B}x{N}", B, N) + t[1:] for t in TUBES for B, N in SHAPES] + [
    ("relu-33x8", 33, 8, "nn", 3, (16, 1, "relu", 1.0, False)), ("elu-33x8", 33, 8, "nn", 3, (16, 1, "elu", 1.0, False)),
    ("reference-shape-2x50", 2, 50, "nn", 10, (128, 2, "softplus", 5.0, False))]
# case name -> seed of its inputs where the default, 100 + B + N, puts more than a tenth of the plans within KINK of a kink
SEEDS = {"l2-2x64": 1, "softplus5-Hr1-2x64": 1, "softplus5-Hr3-2x64": 2, "tanh-2x32-1x1": 1}


def _setup(case, seed=None):
    """(trainer or None, problem, planner keywords, the instances) of a case."""
    from legged_gym_dev_amd.tube.calibrate import Calibration
    name, B, N, kind, Hr, m = case
    tr = _trainer(Hr, N, *m) if m else None
    p = _analytic(N, kind, H_rev=Hr)
    cond = bool(m and m[4])
    calib = Calibration("horizon", [0.9], torch.linspace(-0.01, 0.05, N)[None], 100, [91]) if cond else None
    kw = dict(calibration=calib, level=0.85 if cond else None, device=DEV)
    d = _instances(B, N, Hr, seed=SEEDS.get(name, 100 + B + N) if seed is None else seed, dt=0.105)
    return tr, p, kw, d


def _past(d, tr):
    return (d["e"], d["v_prev"]) if tr else (None, None)


def _ref_kw(tr, case, pln, d):
    """The restatement's keywords for a case: the device's own weights, the past, the level and the offset."""
    m = case[5]
    if not m:
        return dict(w0=d["w0"])
    off = pln.scorer.offset.cpu().numpy() if pln.scorer.offset is not None else None
    return dict(w0=d["w0"], model={"sd": tr.state_dict(), "act": m[2], "beta": m[3]}, e=d["e"], v_prev=d["v_prev"], level=pln.scorer.level, offset=off)


# ---------------------------------------------------------------- 1. the forward half
FORWARD = [c for c in CASES if c[0] in ("l2-3x8", "l1_rolling-2x64", "softplus5-Hr3-33x8", "level-offset-3x8", "reference-shape-2x50")]


@pytest.mark.parametrize("case", FORWARD, ids=[c[0] for c in FORWARD])
def test_forward_equals_the_sampling_kernel_and_the_scorer(case):
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner, HipMppiPlanner, MppiCfg
    tr, p, kw, d = _setup(case)
    try:
        gp = HipGradPlanner(tr, p, GradCfg(**RHO), **kw)
        mp = HipMppiPlanner(tr, p, MppiCfg(K=32, sigma=0.2, seed=5, **RHO), **kw)
        assert float(d["vbar"].abs().max()) <= 1.0                       # in bounds: candidate 0 is the mean plan itself
        got = gp.gradient(d["z0"], d["vbar"], *_past(d, tr), d["w0"])
        st = mp.step(mp.state(d["z0"], d["vbar"], *_past(d, tr), d["w0"], want=("cost", "min_clear", "pen")), 0, what=1)
        for k in ("J", "cost", "min_clear", "pen"):
            _same(got[k], st[k][:, 0], k)
        sc = gp.scorer.score(d["z0"], d["vbar"], *_past(d, tr), d["w0"], want=())
        _same(got["cost"], sc["cost"], "cost"), _same(got["min_clear"], sc["min_clear"], "min_clear")
        assert (got["pen"][0] > 0).all(), "all three hinge sums bind on instance 0"
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 2. the gradient
@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gradient_against_float64_autograd_under_the_chain_yardstick(case):
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner
    tr, p, kw, d = _setup(case)
    try:
        gp = HipGradPlanner(tr, p, GradCfg(**RHO), **kw)
        got = gp.gradient(d["z0"], d["vbar"], *_past(d, tr), d["w0"])
        rp, rho, rkw = _ref_problem(p), [RHO["rho_g"], RHO["rho_w"], RHO["rho_z"]], _ref_kw(tr, case, gp, d)
        J64, g64, parts = gr.value_and_grad(rp, rho, d["z0"], d["vbar"], torch.float64, **rkw)
        J32, g32, _ = gr.value_and_grad(rp, rho, d["z0"], d["vbar"], torch.float32, **rkw)
        ok = parts["margin"] >= KINK
        print(f"{case[0]}: {int(ok.sum())} of {len(ok)} plans compared (smallest margin {parts['margin'].min():.2e}); pen of instance 0 {parts['pen'][0]}")
        assert ok.sum() >= 0.9 * len(ok), "at least 90 % of the plans lie away from every kink"
        assert ok[0] and (parts["pen"][0] > 0).all(), "instance 0, where every hinge binds, is compared"
        _yardstick(f"{case[0]} J", got["J"].cpu().numpy()[ok], J32[ok], J64[ok])
        _yardstick(f"{case[0]} dJ/dv", got["grad"].cpu().numpy()[ok], g32[ok], g64[ok])
        assert np.abs(g64[ok]).max() > 1.0 and bool(torch.isfinite(got["grad"]).all())
    finally:
        if tr:
            tr.close()


@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("l1_rolling-33x8", "tanh-2x32-33x8")], ids=["l1_rolling", "tanh-2x32"])
def test_a_plan_does_not_depend_on_the_batch_or_its_place_in_a_tile(case):
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner
    tr, p, kw, d = _setup(case)
    try:
        gp = HipGradPlanner(tr, p, GradCfg(**RHO), **kw)
        e, vp = _past(d, tr)
        full = {k: t.clone() for k, t in gp.gradient(d["z0"], d["vbar"], e, vp, d["w0"]).items()}
        for j in (0, 5, 31, 32):
            s = slice(j, j + 1)
            one = gp.gradient(d["z0"][s], d["vbar"][s], e[s] if tr else None, vp[s] if tr else None, d["w0"][s])
            for k in ("J", "grad", "cost", "min_clear", "pen"):
                _same(one[k], full[k][s], f"plan {j} {k}")
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 3. the optimiser step
@pytest.mark.parametrize("case", [c for c in CASES if c[0] in ("l2-33x8", "softplus5-Hr3-3x8")], ids=["l2-33x8", "softplus5-Hr3-3x8"])
def test_step_is_adam_and_the_clip_on_the_devices_gradient_and_the_elite_is_exact(case):
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner
    tr, p, kw, d = _setup(case)
    try:
        p = dataclasses.replace(p, rom_v_min=[-0.4, -0.3], rom_v_max=[0.3, 0.45])   # tight, different per axis: a part of the steps is projected
        cfg = GradCfg(lr=0.2, **RHO)
        gp = HipGradPlanner(tr, p, cfg, **kw)
        lo, hi = np.float32(p.rom_v_min), np.float32(p.rom_v_max)
        B = case[1]
        st = gp.state(d["z0"], d["vbar"], *_past(d, tr), d["w0"], want=("grad",))
        hist = torch.empty(2, B, 2, device=DEV)
        m, s = torch.zeros_like(st["v"]).cpu().numpy(), torch.zeros_like(st["v"]).cpu().numpy()
        seen = []
        for it in range(2):
            v0 = st["v"].clone()
            gp.step(st, it, what=3, reset=it == 0, hist_row=hist[it])
            g, J = st["grad"].cpu().numpy(), st["J"].clone()
            plain = gp.gradient(d["z0"], v0, *_past(d, tr), d["w0"])
            _same(st["grad"], plain["grad"], "the stepping launch makes lg_plan_grad's gradient"), _same(J, plain["J"], "J")
            _same(hist[it], torch.stack([J, st["grad"].abs().reshape(B, -1).max(dim=1).values], dim=1), "hist")
            args = (it + 1, cfg.lr, cfg.beta1, cfg.beta2, cfg.eps, p.rom_v_min, p.rom_v_max)
            r32, r64 = (gr.adam_step(v0.cpu().numpy(), g, m, s, *args, D) for D in (np.float32, np.float64))
            for k, name in enumerate(("v", "m", "s")):
                _yardstick(f"{case[0]} step {it} {name}", st[name].cpu().numpy(), r32[k], r64[k])
            nv = st["v"].cpu().numpy()
            above, below = r64[3] > hi + 1e-6, r64[3] < lo - 1e-6         # the float64 step leaves the bounds by more than rounding can hide
            assert above.any() and below.any() and (B < 33 or (above.any(axis=(0, 1)) & below.any(axis=(0, 1))).all())   # 33 x 8: both bounds of both axes
            assert (nv >= lo).all() and (nv <= hi).all(), "the projection holds"
            assert (nv[above] == np.broadcast_to(hi, nv.shape)[above]).all() and (nv[below] == np.broadcast_to(lo, nv.shape)[below]).all(), "and is exact"
            m, s = st["m"].cpu().numpy(), st["s"].cpu().numpy()          # the next step starts from the device's own moments
            seen.append((J, v0))
        (J0, v0), (J1, v1) = seen
        win = J1 < J0
        _same(st["best_J"], torch.where(win, J1, J0), "best_J"), _same(st["best_v"], torch.where(win[:, None, None], v1, v0), "best_v")
        assert not st["n_bad"].any()
        # an elite that is already better stays, through an evaluation and through a step
        keep = st["best_v"].clone()
        st["best_J"].fill_(-1.0)
        gp.step(st, 2, what=1), gp.step(st, 2, what=3)
        _same(st["best_J"], torch.full((B,), -1.0)), _same(st["best_v"], keep)
    finally:
        if tr:
            tr.close()


def test_a_non_finite_plan_stays_and_is_counted():
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner
    B, N = 3, 8
    gp = HipGradPlanner(None, _analytic(N), GradCfg(lr=0.1, **RHO), device=DEV)
    d = _instances(B, N, 0, seed=3, dt=0.105)
    v = d["vbar"].clone()
    v[1, 2, 0] = float("nan")
    st = gp.step(gp.state(d["z0"], v, None, None, d["w0"]), 0, what=3, reset=True)
    assert st["n_bad"].tolist() == [0, 1, 0] and float(st["best_J"][1]) == float("inf") and bool(torch.isfinite(st["best_J"][[0, 2]]).all())
    _same(st["v"][1].view(torch.int32), v[1].view(torch.int32), "the plan is left as it is")
    assert not st["m"][1].any() and not st["s"][1].any()                 # a reset starts the moments, the refused step leaves them
    assert bool(torch.isfinite(st["v"][[0, 2]]).all()) and not torch.equal(st["v"][0].cpu(), v[0]) and not torch.equal(st["v"][2].cpu(), v[2])
    m1 = st["m"].clone()
    gp.step(st, 1, what=3)
    assert st["n_bad"].tolist() == [0, 2, 0]                             # counted per step
    _same(st["m"][1], m1[1]), _same(st["v"][1].view(torch.int32), v[1].view(torch.int32))
    gp.step(st, 2, what=1)
    assert st["n_bad"].tolist() == [0, 2, 0]                             # an evaluation refuses no step
    assert float(st["best_J"][1]) == float("inf")                        # a non-finite J never wins


@pytest.mark.parametrize("kind", ["l2", "nn"])
def test_lg_plan_descend_equals_its_steps_and_best_J_is_the_running_minimum(kind):
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner
    P, N, Hr, iters = 3, 5, 3 if kind == "nn" else 0, 6
    tr = _trainer(Hr, N, 16, 1, "relu") if kind == "nn" else None
    try:
        gp = HipGradPlanner(tr, _analytic(N, kind, H_rev=Hr), GradCfg(iters=iters, lr=0.05, **RHO), device=DEV)
        d = _instances(P, N, Hr, seed=2, dt=0.105)
        past = _past(d, tr)
        sol = gp.plan(d["z0"], d["vbar"], *past, d["w0"])
        st = gp.state(d["z0"], d["vbar"], *past, d["w0"])
        hist = torch.empty(iters + 1, P, 2, device=DEV)
        for it in range(iters + 1):
            gp.step(st, it, what=3 if it < iters else 1, reset=it == 0, hist_row=hist[it])
        for k, t in (("v", st["v"]), ("best_v", st["best_v"]), ("best_J", st["best_J"]), ("hist", hist), ("n_bad", st["n_bad"])):
            _same(sol[k], t, k)
        _same(sol["best_J"], sol["hist"][:, :, 0].min(dim=0).values, "best_J is the running minimum of hist")
        assert not torch.equal(sol["v"].cpu(), d["vbar"]) and bool((sol["best_J"] < sol["hist"][0, :, 0]).any())
        again = gp.plan(d["z0"], d["vbar"], *past, d["w0"])
        _same(again["v"], sol["v"], "the same bits on every run"), _same(again["hist"], sol["hist"])
        full = gp.scorer.score(d["z0"], sol["v"], *past, d["w0"], want=("z", "w"))
        for k in ("cost", "min_clear", "z", "w"):
            _same(sol["score"][k], full[k], f"score {k}")
        _same(sol["best_score"]["cost"], gp.scorer.score(d["z0"], sol["best_v"], *past, d["w0"], want=())["cost"])
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 4. it plans
def _small():
    from legged_gym_dev_amd.tube.plan import PlanProblem
    return PlanProblem(N=8, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], tube_kind="l2", scaling=0.02,
                       Q=[10.0, 0, 0, 10.0], R=[1.0, 0, 0, 1.0], rom_v_min=[-2.0, -2.0], rom_v_max=[2.0, 2.0])


def test_it_plans_on_the_small_problem():
    """The problem of tests/test_plan_grad_host.py, where the float64 restatement reaches J 42.7 and min_clear 0.019 from the warm
    start's 661.2 and -0.0310 in 101 evaluations; MPPI reaches J 39.4 in 5120 (tests/test_hip_mppi.py).  Four starts: the problem's
    and three beside it."""
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner
    p = _small()
    gp = HipGradPlanner(None, p, GradCfg(iters=100, lr=0.05, rho_g=1e4), device=DEV)
    z0 = torch.tensor(p.start).repeat(4, 1)
    z0[1:] += 0.01 * torch.randn(3, 2, generator=torch.Generator().manual_seed(0))
    warm = gp.scorer.score(z0, gp.warm_start(z0.numpy()), want=("z", "w"))
    assert float(warm["min_clear"][0]) == pytest.approx(-0.0310, abs=5e-5) and float(_J_of(warm, p, 1e4)[0]) == pytest.approx(661.2, abs=0.05)
    sol = gp.plan(z0)
    J = _J_of(sol["best_score"], p, 1e4)
    print(f"gradient planner: min_clear {sol['best_score']['min_clear'].tolist()}, J {J.tolist()} (MPPI: 39.4), best_J {sol['best_J'].tolist()}")
    assert bool((sol["best_score"]["min_clear"] >= 0).all()) and not sol["best_score"]["n_viol"][:, 0].any() and bool((J <= 0.1 * 661.2).all())
    assert not sol["n_bad"].any() and tuple(sol["hist"].shape) == (101, 4, 2)
    assert float(sol["hist"][0, 0, 0]) == pytest.approx(661.2, abs=0.05)


def test_the_gradient_polishes_what_mppi_found():
    from legged_gym_dev_amd.tube.plan import ChainedPlanner, GradCfg, HipGradPlanner, HipMppiPlanner, MppiCfg
    p = _small()
    mp = HipMppiPlanner(None, p, MppiCfg(K=64, iters=5, sigma=0.3, lambda_=1.0, rho_g=1e4, seed=2), device=DEV)
    gp = HipGradPlanner(None, p, GradCfg(iters=30, lr=0.02, rho_g=1e4), device=DEV)
    sol = ChainedPlanner(mp, gp).plan(torch.tensor(p.start).repeat(4, 1))
    before, after = sol["first"]["best_J"], sol["best_J"]
    print(f"mppi+grad: best_J {before.tolist()} -> {after.tolist()}")
    _same(sol["hist"][0, :, 0], before, "the polish starts from MPPI's elite, and scores it to the same bits")
    assert bool((after <= before).all())


@pytest.mark.parametrize("name", ["gap", "right"])
def test_clearance_on_the_reference_problems_is_reported(name):
    """Printed, not asserted: lr and the penalties are not tuned per problem."""
    from legged_gym_dev_amd.tube.plan import GradCfg, HipGradPlanner, PlanProblem
    p = PlanProblem.named(name, tube_kind="l1", N=50)
    gp = HipGradPlanner(None, p, GradCfg(iters=100, lr=0.05 * p.rom_v_max[0], rho_g=1e4), device=DEV)
    z0 = torch.tensor([p.start])
    warm = gp.scorer.score(z0, gp.warm_start(z0.numpy()), want=())
    sol = gp.plan(z0)
    print(f"{name}, l1 tube: min_clear {float(warm['min_clear'][0]):+.4f} -> {float(sol['best_score']['min_clear'][0]):+.4f}, "
          f"J {float(sol['hist'][0, 0, 0]):.1f} -> {float(sol['best_J'][0]):.1f}")
    assert bool(torch.isfinite(sol["best_J"]).all()) and not sol["n_bad"].any()


# ---------------------------------------------------------------- 5. the closed loop
def test_closed_loop_equals_the_steps_composed_by_hand():
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg
    p, P, H = _small(), 3, 4
    gp = pl.HipGradPlanner(None, p, pl.GradCfg(iters=8, lr=0.05, rho_g=1e4), device=DEV)
    sim = HipRomSim(RomSimCfg(), device=DEV)
    try:
        start = torch.tensor([[0.0, 0.0], [0.02, -0.03], [-0.05, 0.04]])
        res = pl.closed_loop(gp, sim, H, start, iters_first=12, keep_plans=True)
        s = start.to(DEV)
        xk, zk, vin = torch.cat([s, torch.zeros(P, 2, device=DEV)], 1), s, None
        e, vp = torch.zeros(P, 0, device=DEV), torch.zeros(P, 0, 2, device=DEV)
        for k in range(H):
            sol = gp.plan(zk, vin, e, vp, None, iters=12 if k == 0 else None)
            sc = gp.scorer.score(zk, sol["v"], e, vp, None, want=("z", "w"))
            t = pl.track(sim, sc["z"][:, :2], sol["v"][:, 1:2], xk, rom_dt=p.dt)
            _same(res["plans_v"][k], sol["v"], f"plan {k}"), _same(res["plans_z"][k], sc["z"]), _same(res["plans_w"][k], sc["w"])
            _same(res["v"][:, k], sol["v"][:, 0]), _same(res["z"][:, k], zk), _same(res["x"][:, k], xk)
            _same(res["z"][:, k + 1], sc["z"][:, 1]), _same(res["w"][:, k + 1], sc["w"][:, 1]), _same(res["x"][:, k + 1], t["x"][:, 1])
            _same(res["cost"][:, k], sc["cost"]), _same(res["min_clear"][:, k], sc["min_clear"]), _same(res["best_J"][:, k], sol["best_J"])
            xk, zk, vin = t["x"][:, 1], sc["z"][:, 1], torch.cat([sol["v"][:, 1:], sol["v"][:, -1:]], 1)
        assert not res["n_bad"].any()
        a = pl.audit_closed_loop(res, p)
        assert json.loads(json.dumps(a, allow_nan=False)) == a and a["robots"] == P and a["steps"] == H
    finally:
        sim.close()


def test_script_with_the_chained_planner_on_a_trained_level_conditioned_tube(tmp_path):
    """Section 10.8's smallest level-conditioned one-shot tube, as tests/test_hip_mppi.py trains it; plan_tube.py --planner mppi+grad
    in closed loop on it writes the library call's result."""
    import audit_plans
    import calibrate_tube
    import plan_tube
    import train_tube
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.calibrate import Calibration, default_path
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim
    run, out = str(tmp_path / "run"), str(tmp_path / "plan")
    sim_flags = ["--sim_envs", "64", "--sim_T", "50"]
    train_tube.main(["--sim", "--sim_seed", "0", "--sim_refresh", "0", "--dataset", "scalar_horizon_level", "--H_fwd", "5", "--H_rev", "3",
                     "--out", run, "--num_epochs", "8", "--batch_size", "16", "--lr", "3e-3", "--seed", "3", "--steps_per_model_checkpoint", "10",
                     "--steps_per_model_evaluation", "10", "--device", DEV] + sim_flags)
    calibrate_tube.main(["--run", run, "--sim", "--checkpoint", "latest", "--levels", "0.5,0.9", "--device", DEV] + sim_flags)
    prob = pl.PlanProblem.named("gap", N=5, H_rev=3, goal=[0.35, 0.36], obs_c=[[0.36, 0.28], [0.28, 0.37]], obs_r=[0.02, 0.03])
    pj = str(tmp_path / "problem.json")
    json.dump(prob.to_json(), open(pj, "w"))
    argv = ["--run", run, "--checkpoint", "latest", "--problem", pj, "--level", "0.9", "--calibration", "--K", "64", "--iters", "4", "--sigma", "0.05",
            "--rho_g", "1e4", "--starts", "3", "--start_noise", "0.01", "--seed", "4", "--closed_loop", "4", "--planner", "mppi+grad", "--lr", "0.01",
            "--grad_iters", "6", "--device", DEV]
    got = plan_tube.main(argv + ["--out", out])
    saved = json.load(open(os.path.join(out, "plan.json")))
    assert saved == json.loads(json.dumps(got, allow_nan=False)) == got
    assert got["planner"] == "mppi+grad" and got["grad"]["iters"] == 6 and got["grad"]["lr"] == 0.01 and got["mppi"]["K"] == 64
    assert got["closed_loop"] == 4 and got["audit"]["robots"] == 3 and np.asarray(got["hist"]).shape == (7, 3, 2)
    a = plan_tube.parse_args(argv)
    p = plan_tube.build_problem(a, audit_plans.run_config(run))
    model, sim = HipTubeModel.load(run, checkpoint="latest", device=DEV), HipRomSim(audit_plans.sim_config(a, p), device=DEV)
    try:
        kw = dict(calibration=Calibration.load(default_path(run)), level=0.9, device=DEV)
        pln = pl.ChainedPlanner(pl.HipMppiPlanner(model, p, plan_tube.mppi_cfg(a), **kw), pl.HipGradPlanner(model, p, plan_tube.grad_cfg(a), **kw))
        res = pl.closed_loop(pln, sim, 4, plan_tube.starts(a, p), keep_plans=True)
        assert pl.audit_closed_loop(res, p) == got["audit"]
        assert pln.plan(plan_tube.starts(a, p))["hist"].cpu().double().tolist() == got["hist"]
        np.testing.assert_array_equal(np.load(os.path.join(out, "plans.npz"))["v"], res["plans_v"].reshape(12, 5, 2).cpu().numpy())
    finally:
        model.close()
        sim.close()
