"""The sampling planner on the GPU (k_plan_sample_score, k_plan_mppi_update): the candidates' noise on its
own; the fused scores against lg_plan_score on the materialised candidates, on the bits; J on the bits and the hinge sums against the
float64 restatement (tests/mppi_ref.py) under the chain yardstick of sections 10.1 / 10.2; the update, the elite and the history;
lg_plan_mppi against its steps; that it plans; the closed loop against the same steps composed by hand."""
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import mppi_ref, plan_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))


def _trainer(Hr, N, U, L, act, beta=1.0, level=False, seed=4):
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    return HipTubeTrainer(Hr + 2 * (Hr + N) + int(level), N, num_units=U, num_layers=L, activation=act, softplus_beta=beta,
                          loss="scalar_level" if level else "scalar_horizon", alpha=0.9, batch_size=32, seed=seed, horizon=(N, Hr), device=DEV)


def _same(a, b, what=""):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert torch.equal(a, b), what


def _yardstick(name, got, r32, r64):
    """The chain yardstick of DESIGN.md sections 10.1 / 10.2: e32 = max |float32 restatement - float64|, the device within 4 e32."""
    e32 = float(np.abs(r32.astype(np.float64) - r64).max())
    ours = float(np.abs(np.asarray(got, np.float64) - r64).max())
    print(f"{name}: e32 = {e32:.3e}, device / e32 = {ours / e32 if e32 else 0:.2f}")
    if e32 == 0:
        assert ours == 0, name
    else:
        assert ours <= 4 * e32, (name, ours, e32)


def _analytic(N, kind="l2", **kw):
    from legged_gym_dev_amd.tube.plan import PlanProblem
    return PlanProblem(**{**dict(N=N, dt=0.1, goal=[1.0, 0.5], obs_c=[[0.2, 0.0], [0.5, 0.4]], obs_r=[0.1, 0.15], tube_kind=kind, scaling=0.5,
                                 window_size=3, w_max=0.02, Qw=2.0, rom_z_min=[0.01, -0.05], rom_z_max=[0.35, 0.3], rom_v_min=[-1.0, -1.0],
                                 rom_v_max=[1.0, 1.0]), **kw})


def _instances(P, N, Hr, seed, dt=0.1):
    """Instance 0 starts at the origin -- outside rom_z_min -- and its mean plan runs through the first obstacle's centre; the others
    start near the upper state bounds.  Every w0 lies above w_max = 0.02."""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    z0 = torch.tensor([0.34, 0.28]) + 0.04 * (r(P, 2) - 0.5)
    vbar = 0.6 * (2 * r(P, N, 2) - 1)
    z0[0] = 0.0
    vbar[0, :, 0], vbar[0, :, 1] = min(0.2 / (dt * max(N // 2, 1)), 1.0), 0.0
    return {"z0": z0, "vbar": vbar, "e": 0.1 * r(P, Hr), "v_prev": 0.2 * (2 * r(P, Hr, 2) - 1), "w0": 0.03 + 0.02 * r(P)}


def _ref_problem(p):
    d = p.to_json()
    d["Qf"] = d["Qf"] if d["Qf"] is not None else d["Q"]
    return d


# ---------------------------------------------------------------- 1. the candidates
@pytest.mark.parametrize("P,K,N", [(1, 32, 1), (2, 64, 8), (3, 96, 64)])
def test_candidate_zero_is_the_clipped_mean_and_all_lie_inside_the_bounds(P, K, N):
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    pln = HipMppiPlanner(None, _analytic(N), MppiCfg(K=K, sigma=0.7, sigma_decay=0.5, seed=11), device=DEV)
    vbar = 1.5 * (2 * torch.rand(P, N, 2, generator=torch.Generator().manual_seed(N)) - 1)          # a part of it outside +-1
    for it in (0, 2):
        c = pln.candidates(vbar, it)
        assert tuple(c.shape) == (P, K, N, 2)
        _same(c[:, 0], vbar.clamp(-1.0, 1.0), "candidate 0")
        assert float(c.min()) >= -1.0 and float(c.max()) <= 1.0 and (N == 1 or float((c.abs() == 1.0).float().mean()) > 0.05)
        _same(c, pln.candidates(vbar, it), "the same seed")
    other = HipMppiPlanner(None, _analytic(N), MppiCfg(K=K, sigma=0.7, sigma_decay=0.5, seed=12), device=DEV).candidates(vbar, 0)
    assert not torch.equal(other[:, 1:], pln.candidates(vbar, 0)[:, 1:])
    _same(other[:, 0], vbar.clamp(-1.0, 1.0))
    for j in range(P):                                                   # instance j of the batch = a batch of one at instance_offset j
        one = HipMppiPlanner(None, _analytic(N), MppiCfg(K=K, sigma=0.7, sigma_decay=0.5, seed=11, instance_offset=j), device=DEV)
        _same(one.candidates(vbar[j:j + 1], 2), pln.candidates(vbar, 2)[j:j + 1], f"instance {j}")


def test_the_noise_is_standard_normal_and_uncorrelated():
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    P, K, N, sigma = 4, 1024, 64, 0.5                                    # 4 x 1023 x 64 x 2 = 523 776 draws; sigma a power of two: eps is exact
    p = _analytic(N, rom_v_min=[-1e9, -1e9], rom_v_max=[1e9, 1e9])
    cfg = MppiCfg(K=K, sigma=sigma, sigma_decay=1.0, seed=2024)
    pln = HipMppiPlanner(None, p, cfg, device=DEV)
    vbar = torch.zeros(P, N, 2)
    eps = [((pln.candidates(vbar, it) - vbar.to(DEV)[:, None]) / float(cfg.sigma_it(it)))[:, 1:].double().cpu() for it in (0, 1)]
    z = eps[0]
    assert z.numel() >= 2 ** 18
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
    assert abs(float((z ** 3).mean())) < 0.05 and abs(float((z ** 4).mean()) - 3.0) < 0.15

    def corr(a, b):
        a, b = a.reshape(-1), b.reshape(-1)
        return abs(float(torch.corrcoef(torch.stack([a, b]))[0, 1])), 5.0 / np.sqrt(a.numel())
    for name, (a, b) in {"x and y": (z[..., 0], z[..., 1]), "candidates j and j + 1": (z[:, :-1], z[:, 1:]),
                         "nodes k and k + 1": (z[:, :, :-1], z[:, :, 1:]), "iterations it and it + 1": (eps[0], eps[1]),
                         "instances p and p + 1": (z[:-1], z[1:])}.items():
        c, bound = corr(a, b)
        print(f"|corr| {name}: {c:.2e} (bound {bound:.2e})")
        assert c < bound, name


# ---------------------------------------------------------------- 2. fused scoring
# (name, P, K, N, H_rev, model (units, layers, act, beta, level) or None, tube kind)
FUSED = [("l2-P3-K32-N8", 3, 32, 8, 0, None, "l2"), ("l1_rolling-P2-K96-N64", 2, 96, 64, 0, None, "l1_rolling"), ("l2-P1-K64-N1", 1, 64, 1, 0, None, "l2"),
         ("nn-plain", 2, 64, 5, 3, (16, 1, "relu", 1.0, False), "nn"), ("nn-conditioned-offset", 3, 96, 5, 3, (16, 1, "relu", 1.0, True), "nn"),
         ("nn-reference-shape", 1, 32, 50, 10, (128, 2, "softplus", 5.0, False), "nn")]


@pytest.mark.parametrize("case", FUSED, ids=[c[0] for c in FUSED])
def test_fused_scores_equal_lg_plan_score_on_the_candidates(case):
    from legged_gym_dev_amd.tube.calibrate import Calibration
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    name, P, K, N, Hr, m, kind = case
    tr = _trainer(Hr, N, *m) if m else None
    try:
        p = _analytic(N, kind, H_rev=Hr)
        cond = bool(m and m[4])
        calib = Calibration("horizon", [0.9], torch.linspace(-0.01, 0.05, N)[None], 100, [91]) if cond else None
        cfg = MppiCfg(K=K, sigma=0.2, sigma_decay=0.5, seed=5, rho_g=1e4, rho_w=30.0, rho_z=7.0, instance_offset=3)
        pln = HipMppiPlanner(tr, p, cfg, calibration=calib, level=0.85 if cond else None, device=DEV)
        d = _instances(P, N, Hr, seed=K + N)
        nn_args = (d["e"], d["v_prev"]) if m else (None, None)
        it = 1
        st = pln.step(pln.state(d["z0"], d["vbar"], *nn_args, d["w0"], want=("cost", "min_clear", "pen")), it, what=1)
        _same(st["vbar"], d["vbar"], "the score leaves the mean plans alone")
        cand = pln.candidates(d["vbar"], it)
        rep = lambda t: None if t is None else t.repeat_interleave(K, dim=0)
        sc = pln.scorer.score(rep(d["z0"]), cand.reshape(P * K, N, 2), rep(nn_args[0]), rep(nn_args[1]), rep(d["w0"]))
        _same(st["cost"].reshape(-1), sc["cost"], "cost")
        _same(st["min_clear"].reshape(-1), sc["min_clear"], "min_clear")
        # J: the stated float32 expression on the device's own cost and pen
        cost, pen = st["cost"].cpu(), st["pen"].cpu()
        rho = [torch.tensor(x, dtype=torch.float32) for x in (cfg.rho_g, cfg.rho_w, cfg.rho_z)]
        _same(st["J"], ((cost + rho[0] * pen[..., 0]) + rho[1] * pen[..., 1]) + rho[2] * pen[..., 2], "J")
        np.testing.assert_array_equal(st["J"].cpu().numpy(), mppi_ref.total(cost.numpy(), pen.numpy(), [cfg.rho_g, cfg.rho_w, cfg.rho_z]))
        # pen against the float64 restatement, on the device's candidates (and, for the MLP, the device's tube values)
        v, rp, res = cand.reshape(P * K, N, 2).cpu().numpy(), _ref_problem(p), {}
        off = pln.scorer.offset.cpu().numpy() if pln.scorer.offset is not None else None
        for D in (np.float32, np.float64):
            fw = sc["fw"].cpu().numpy() if m else plan_ref.analytic(kind, v, p.scaling, p.window_size, D)
            r = plan_ref.score(rp, rep(d["z0"]).numpy(), v, fw, rep(d["w0"]).numpy(), off, D)
            res[D] = mppi_ref.penalties(rp, r, D)
        got = st["pen"].reshape(P * K, 3).cpu().numpy()
        for c, col in enumerate(("pen_g", "pen_w", "pen_z")):
            _yardstick(f"{name} {col}", got[:, c], res[np.float32][:, c], res[np.float64][:, c])
            assert (got[:K, c] > 0).any(), f"{col} binds nowhere on instance 0"
        assert got[0, 0] > 0                                             # the mean plan of instance 0 crosses the obstacle's centre
    finally:
        if tr:
            tr.close()


def test_a_candidate_does_not_depend_on_P_or_K():
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    N = 8
    d = _instances(3, N, 0, seed=1)
    kw = dict(sigma=0.2, seed=9, rho_w=30.0, rho_z=7.0)
    big = HipMppiPlanner(None, _analytic(N), MppiCfg(K=96, **kw), device=DEV)
    sb = big.step(big.state(d["z0"], d["vbar"], None, None, d["w0"], want=("cost", "min_clear", "pen")), 0, what=1)
    one = HipMppiPlanner(None, _analytic(N), MppiCfg(K=32, instance_offset=2, **kw), device=DEV)
    so = one.step(one.state(d["z0"][2:], d["vbar"][2:], None, None, d["w0"][2:], want=("cost", "min_clear", "pen")), 0, what=1)
    for k in ("J", "cost", "min_clear", "pen"):
        _same(sb[k][2:, :32], so[k], k)


# ---------------------------------------------------------------- 3. the update
def _scored(P, K, N, kind="l2", lam=40.0, seed=3, it=1):
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    cfg = MppiCfg(K=K, sigma=0.2, sigma_decay=0.5, seed=seed, lambda_=lam, rho_g=50.0, rho_w=30.0, rho_z=7.0)
    pln = HipMppiPlanner(None, _analytic(N, kind), cfg, device=DEV)
    d = _instances(P, N, 0, seed=K + N)
    st = pln.step(pln.state(d["z0"], d["vbar"], None, None, d["w0"]), it, what=1)
    return pln, d, st, pln.candidates(d["vbar"], it)


def _check_update(name, lam, cand, J, old, new):
    """new vbar of every instance against the float64 restatement on the device's candidates and J."""
    for i in range(J.shape[0]):
        r32, r64 = (mppi_ref.update(cand[i], J[i], lam, D) for D in (np.float32, np.float64))
        if r64 is None:
            np.testing.assert_array_equal(new[i], old[i])
        else:
            _yardstick(f"{name} vbar[{i}]", new[i], r32, r64)


@pytest.mark.parametrize("P,K,N", [(1, 32, 1), (2, 64, 8), (3, 96, 64), (1, 4096, 8)])
def test_update_against_float64_and_the_elite_on_the_bits(P, K, N):
    pln, d, st, cand = _scored(P, K, N, "l1_rolling" if N == 64 else "l2")
    J = st["J"].clone()
    hist = torch.empty(P, 2, device=DEV)
    pln.step(st, 1, what=2, reset=True, hist_row=hist)
    Jn, cn = J.cpu().numpy(), cand.cpu().numpy()
    w = [mppi_ref.weights(Jn[i], 40.0, np.float64)[0] for i in range(P)]
    assert all((x > 1e-3).sum() >= 4 for x in w), "the weights are spread over several candidates"
    _check_update(f"P{P} K{K} N{N}", 40.0, cn, Jn, d["vbar"].numpy(), st["vbar"].cpu().numpy())
    idx = J.argmin(dim=1)                                                # torch: the first of equal minima
    assert all(int(idx[i]) == int(np.argmin(Jn[i])) for i in range(P))
    _same(st["best_J"], J.min(dim=1).values, "best_J")
    _same(st["best_v"], cand[torch.arange(P), idx], "best_v")
    _same(hist, torch.stack([J[:, 0], J.min(dim=1).values], dim=1), "hist")
    assert not st["n_bad"].any()
    # an elite that is already better stays; a worse one is replaced
    st["vbar"].copy_(d["vbar"].to(DEV))
    keep = st["best_v"].clone()
    st["best_J"].fill_(-1.0)
    pln.step(st, 1, what=2, reset=False)
    _same(st["best_J"], torch.full((P,), -1.0)), _same(st["best_v"], keep)
    st["vbar"].copy_(d["vbar"].to(DEV))
    st["best_J"].fill_(1e30), st["best_v"].zero_()
    pln.step(st, 1, what=2, reset=False)
    _same(st["best_J"], J.min(dim=1).values), _same(st["best_v"], cand[torch.arange(P), idx])


def test_non_finite_scores_get_weight_zero_and_an_all_bad_row_leaves_the_mean():
    P, K, N = 3, 96, 8
    pln, d, st, cand = _scored(P, K, N)
    J = st["J"]
    J[0, 5], J[0, 64], J[0, int(J[0].argmin())] = float("inf"), float("nan"), float("-inf")    # the best of instance 0 is lost too
    J[1, ::2], J[1, 1::2] = float("nan"), float("inf")
    Jn = J.clone()
    pln.step(st, 1, what=2, reset=True)
    new = st["vbar"].cpu()
    _check_update("injected", 40.0, cand.cpu().numpy(), Jn.cpu().numpy(), d["vbar"].numpy(), new.numpy())
    _same(new[1], d["vbar"][1], "an all-non-finite row leaves vbar as it is")
    assert bool(torch.isfinite(new).all()) and not torch.equal(new[0], d["vbar"][0])
    assert st["n_bad"].tolist() == [0, 1, 0]
    fin = torch.where(torch.isfinite(Jn), Jn, torch.full_like(Jn, float("inf")))
    _same(st["best_J"], fin.min(dim=1).values, "best_J skips the non-finite")
    assert float(st["best_J"][1]) == float("inf")
    _same(st["best_v"][1], d["vbar"][1], "a reset without a finite J: best_v is the mean")
    _same(st["best_v"][0], cand[0, int(fin[0].argmin())])
    st["J"].copy_(Jn)
    pln.step(st, 1, what=2, reset=False)
    assert st["n_bad"].tolist() == [0, 2, 0]                             # counted per iteration


@pytest.mark.parametrize("kind", ["l2", "nn"])
def test_lg_plan_mppi_equals_its_steps_and_the_history_is_the_elites_trace(kind):
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg
    P, N, Hr, iters = 3, 5, 3 if kind == "nn" else 0, 4
    tr = _trainer(Hr, N, 16, 1, "relu") if kind == "nn" else None
    try:
        cfg = MppiCfg(K=64, iters=iters, sigma=0.3, sigma_decay=0.7, seed=8, lambda_=5.0, rho_g=100.0, rho_w=3.0, rho_z=7.0)
        pln = HipMppiPlanner(tr, _analytic(N, kind, H_rev=Hr), cfg, device=DEV)
        d = _instances(P, N, Hr, seed=2)
        past = (d["e"], d["v_prev"]) if tr else (None, None)
        sol = pln.plan(d["z0"], d["vbar"], *past, d["w0"])
        st = pln.state(d["z0"], d["vbar"], *past, d["w0"])
        hist, trace = torch.empty(iters, P, 2, device=DEV), []
        for it in range(iters):
            pln.step(st, it, what=3, reset=it == 0, hist_row=hist[it])
            trace.append(st["best_J"].clone())
        for k, t in (("v", st["vbar"]), ("best_v", st["best_v"]), ("best_J", st["best_J"]), ("hist", hist), ("n_bad", st["n_bad"])):
            _same(sol[k], t, k)
        _same(sol["hist"][:, :, 1].cummin(dim=0).values, torch.stack(trace), "the running minimum of hist is best_J's trace")
        assert not torch.equal(sol["v"].cpu(), d["vbar"])
        again = pln.plan(d["z0"], d["vbar"], *past, d["w0"])
        _same(again["v"], sol["v"], "the same bits on every run"), _same(again["hist"], sol["hist"])
        full = pln.scorer.score(d["z0"], sol["v"], *past, d["w0"], want=("z", "w"))
        for k in ("cost", "min_clear", "z", "w"):
            _same(sol["score"][k], full[k], f"score {k}")
        _same(sol["best_score"]["cost"], pln.scorer.score(d["z0"], sol["best_v"], *past, d["w0"], want=())["cost"])
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 4. it plans
def _J_of(score, p, rho_g):
    """J of a scored plan from HipPlanScorer.score's cost, z and w, in float64 (no tube or state penalty in these problems)."""
    z, w = score["z"].double().cpu(), score["w"].double().cpu()
    pen = torch.zeros(z.shape[0], dtype=torch.float64)
    for c, r in zip(p.obs_c, p.obs_r):
        g = ((z - torch.tensor(c, dtype=torch.float64)) ** 2).sum(dim=-1) - (r + w) ** 2
        pen += (-g).clamp(min=0).sum(dim=1)
    return score["cost"].double().cpu() + rho_g * pen


def test_it_plans_on_the_small_problem():
    """The problem of tests/test_mppi_host.py, where a NumPy MPPI on the restatement reached min_clear 0.0177 .. 0.0220 and
    J 39.4 .. 39.6 from the warm start's -0.0310 and 661.2.  Four instances of one start: four noise streams."""
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg, PlanProblem
    p = PlanProblem(N=8, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], tube_kind="l2", scaling=0.02,
                    Q=[10.0, 0, 0, 10.0], R=[1.0, 0, 0, 1.0], rom_v_min=[-2.0, -2.0], rom_v_max=[2.0, 2.0])
    pln = HipMppiPlanner(None, p, MppiCfg(K=256, iters=20, sigma=0.3, sigma_decay=1.0, lambda_=1.0, rho_g=1e4), device=DEV)
    z0 = torch.tensor(p.start).repeat(4, 1)
    warm = pln.scorer.score(z0, pln.warm_start(z0.numpy()), want=("z", "w"))
    J0 = _J_of(warm, p, 1e4)
    assert float(warm["min_clear"][0]) == pytest.approx(-0.0310, abs=5e-5) and float(J0[0]) == pytest.approx(661.2, abs=0.05)
    sol = pln.plan(z0)
    J = _J_of(sol["score"], p, 1e4)
    print(f"min_clear {sol['score']['min_clear'].tolist()}, J {J.tolist()}, best_J {sol['best_J'].tolist()}")
    assert bool((sol["score"]["min_clear"] >= 0).all()) and bool((J <= 0.1 * J0).all()) and not sol["score"]["n_viol"][:, 0].any()
    assert not sol["n_bad"].any() and len({tuple(v.reshape(-1).tolist()) for v in sol["v"].cpu()}) == 4
    _same(sol["hist"][0, :, 0], torch.full((4,), float(sol["hist"][0, 0, 0])))         # iteration 0 scores the same warm start everywhere
    assert float(sol["hist"][0, 0, 0]) == pytest.approx(float(J0[0]), rel=1e-5)


def test_it_plans_through_the_gap():
    """The reference's gap with the l1 tube, N = 50: the warm start's clearance is -0.209; a NumPy MPPI on the restatement reached
    +0.011 .. +0.019 over three seeds."""
    from legged_gym_dev_amd.tube.plan import HipMppiPlanner, MppiCfg, PlanProblem
    p = PlanProblem.named("gap", tube_kind="l1", N=50)
    pln = HipMppiPlanner(None, p, MppiCfg(K=512, iters=30, sigma=0.05, sigma_decay=1.0, lambda_=1.0, rho_g=1e4), device=DEV)
    z0 = torch.tensor([p.start])
    warm = pln.scorer.score(z0, pln.warm_start(z0.numpy()), want=())
    assert float(warm["min_clear"][0]) == pytest.approx(-0.209, abs=5e-4)
    sol = pln.plan(z0)
    print(f"min_clear {sol['score']['min_clear'].tolist()}, best_J {sol['best_J'].tolist()}")
    assert float(sol["score"]["min_clear"][0]) >= 0 and int(sol["score"]["n_viol"][0, 0]) == 0


# ---------------------------------------------------------------- 5. the closed loop
def test_closed_loop_equals_the_steps_composed_by_hand():
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg
    p = pl.PlanProblem(N=8, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], tube_kind="l2", scaling=0.02,
                       Q=[10.0, 0, 0, 10.0], R=[1.0, 0, 0, 1.0], rom_v_min=[-2.0, -2.0], rom_v_max=[2.0, 2.0])
    P, H = 3, 6
    pln = pl.HipMppiPlanner(None, p, pl.MppiCfg(K=64, iters=3, sigma=0.3, lambda_=1.0, rho_g=1e4, seed=1), device=DEV)
    sim = HipRomSim(RomSimCfg(), device=DEV)
    try:
        assert round(p.dt / float(sim.cfg.env.model.dt)) == 2            # S = 2 at the default configuration
        sim.reset()
        sim.step(None)
        torch.cuda.synchronize()
        before = {k: sim.t[k].clone() for k in ("tg_state", "root_states", "tg_traj", "v_traj", "obs", "n_resample")}
        epoch = sim.lib.lg_romsim_get_epoch(sim.ctx)
        start = torch.tensor([[0.0, 0.0], [0.02, -0.03], [-0.05, 0.04]])
        res = pl.closed_loop(pln, sim, H, start, iters_first=5, keep_plans=True)
        torch.cuda.synchronize()
        for k, t in before.items():
            assert torch.equal(sim.t[k], t), k
        assert sim.lib.lg_romsim_get_epoch(sim.ctx) == epoch
        # the same by hand
        s = start.to(DEV)
        xk, zk, vin = torch.cat([s, torch.zeros(P, 2, device=DEV)], 1), s, None
        e, vp = torch.zeros(P, 0, device=DEV), torch.zeros(P, 0, 2, device=DEV)
        for k in range(H):
            sol = pln.plan(zk, vin, e, vp, None, iters=5 if k == 0 else None)
            sc = pln.scorer.score(zk, sol["v"], e, vp, None, want=("z", "w"))
            t = pl.track(sim, sc["z"][:, :2], sol["v"][:, 1:2], xk, rom_dt=p.dt)
            _same(res["plans_v"][k], sol["v"], f"plan {k}"), _same(res["plans_z"][k], sc["z"]), _same(res["plans_w"][k], sc["w"])
            _same(res["v"][:, k], sol["v"][:, 0]), _same(res["z"][:, k], zk), _same(res["x"][:, k], xk)
            _same(res["z"][:, k + 1], sc["z"][:, 1]), _same(res["w"][:, k + 1], sc["w"][:, 1])
            _same(res["x"][:, k + 1], t["x"][:, 1]), _same(res["pz_x"][:, k + 1], t["x"][:, 1, :2]), _same(res["u"][:, 2 * k:2 * k + 2], t["u"])
            _same(res["cost"][:, k], sc["cost"]), _same(res["min_clear"][:, k], sc["min_clear"]), _same(res["best_J"][:, k], sol["best_J"])
            xk, zk, vin = t["x"][:, 1], sc["z"][:, 1], torch.cat([sol["v"][:, 1:], sol["v"][:, -1:]], 1)
        assert tuple(res["u"].shape) == (P, 2 * H, 2) and not res["n_bad"].any()
        a = pl.audit_closed_loop(res, p)
        assert json.loads(json.dumps(a, allow_nan=False)) == a
        shares = a["coverage_by_step"] + [a[k] for k in ("coverage", "covered_robots", "actually_safe", "predicted_safe", "reached_goal")]
        assert all(0.0 <= x <= 1.0 for x in shares) and len(a["coverage_by_step"]) == H + 1 and a["robots"] == P and a["steps"] == H
        print(f"closed loop, l2 tube: coverage {a['coverage']:.3f} per step {[round(c, 2) for c in a['coverage_by_step']]}, actually safe "
              f"{a['actually_safe']:.2f}, predicted safe {a['predicted_safe']:.2f}")
    finally:
        sim.close()


def test_script_on_a_trained_level_conditioned_tube(tmp_path):
    """Section 10.8's smallest level-conditioned one-shot tube, as tests/test_hip_plan_audit.py trains it; plan_tube.py in closed loop
    on it.  plan.json is the library call; plans.npz goes through audit_plans.py --plans."""
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
            "--rho_g", "1e4", "--starts", "3", "--start_noise", "0.01", "--seed", "4", "--closed_loop", "4", "--device", DEV]
    got = plan_tube.main(argv + ["--out", out])
    saved = json.load(open(os.path.join(out, "plan.json")))
    assert saved == json.loads(json.dumps(got, allow_nan=False)) == got
    assert got["closed_loop"] == 4 and got["audit"]["robots"] == 3 and got["audit"]["steps"] == 4 and got["calibrated"] is True
    assert np.asarray(got["hist"]).shape == (4, 3, 2) and got["mppi"]["K"] == 64 and got["mppi"]["lambda"] == 1.0
    # the same through the library
    a = plan_tube.parse_args(argv)
    p = plan_tube.build_problem(a, audit_plans.run_config(run))
    model, sim = HipTubeModel.load(run, checkpoint="latest", device=DEV), HipRomSim(audit_plans.sim_config(a, p), device=DEV)
    try:
        pln = pl.HipMppiPlanner(model, p, plan_tube.mppi_cfg(a), calibration=Calibration.load(default_path(run)), level=0.9, device=DEV)
        res = pl.closed_loop(pln, sim, 4, plan_tube.starts(a, p), keep_plans=True)
        assert pl.audit_closed_loop(res, p) == got["audit"]
        assert pln.plan(plan_tube.starts(a, p))["hist"].cpu().double().tolist() == got["hist"]
    finally:
        model.close()
        sim.close()
    f = os.path.join(out, "plans.npz")
    z = np.load(f)
    assert z["z0"].shape == (12, 2) and z["v"].shape == (12, 5, 2)
    np.testing.assert_array_equal(z["v"], res["plans_v"].reshape(12, 5, 2).cpu().numpy())
    np.testing.assert_array_equal(z["z0"][:3], plan_tube.starts(a, p).numpy())
    aud = audit_plans.main(["--run", run, "--checkpoint", "latest", "--problem_json", pj, "--level", "0.9", "--calibration", "--plans", f,
                            "--device", DEV, "--out", str(tmp_path / "audit")])
    assert aud["plans"] == 12 and aud["nodes"] == 6 and aud["source"] == {"plans_file": f}
    print(f"closed loop on the trained tube: coverage {got['audit']['coverage']:.3f}, actually safe {got['audit']['actually_safe']:.2f}; "
          f"its plans audited open loop: coverage {aud['coverage']:.3f}")
