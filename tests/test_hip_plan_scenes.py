"""Per-plan scenes on the GPU.  The contracts are equalities on the bits:
  1. uniform scenes (Scenes.repeat) give every output of the entries without scenes;
  2. with heterogeneous scenes, plan b (MPPI instance p) is a call of one plan (instance) of the entry without scenes on scenes.problem(b);
  3. lg_plan_descend / lg_plan_mppi with scenes are their step entries composed by hand;
  4. independent of the old kernels: cost and min_clear against tests/plan_ref.py per plan in float64 under the chain yardstick
     (4 e32) and the margins (1e-5 on g, 1e-6 on a bound) of tests/test_hip_plan_score.py; counts and worst_node exact outside them;
  5. a fleet of 64 robots, each in its own scene, in closed loop; 6. the scripts."""
import dataclasses
import json
import os
import sys

import numpy as np
import pytest
import torch

from tests import plan_ref
from tests.test_hip_plan_score import _plans, _ref_problem, _same, _yardstick
from tests.test_hip_plan_score import _trainer as _oneshot
from tests.test_hip_plan_step import _trainer as _step

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))

RHO = dict(rho_g=1e4, rho_w=30.0, rho_z=7.0)
# name -> (tube_kind, H_rev, recursive, the model's maker from N or None).  The one-step kinds: T = 1 taps not recursive; T = 3 recursive,
# 2 x 32 units, whose weights are staged in LDS; T = 10 recursive, 4 x 128 units, 212 KB of weights, which the kernels read from wt.
TUBES = {"l1": ("l1", 0, False, None), "l2_rolling": ("l2_rolling", 0, False, None),
         "nn": ("nn", 3, False, lambda N: _oneshot(3, N, 16, 1, "relu")),
         "step": ("nn_step", 0, False, lambda N: _step(3, 16, 1, "relu")),
         "step-recursive-lds": ("nn_step", 2, True, lambda N: _step(9, 32, 2, "tanh")),
         "step-recursive-wt": ("nn_step", 9, True, lambda N: _step(30, 128, 4, "relu"))}


def _problem(name, N, **kw):
    from legged_gym_dev_amd.tube.plan import PlanProblem
    kind, Hr, rec, _ = TUBES[name]
    # bounds and a tube ceiling that a part of the plans crosses, so that every count and every hinge sum is exercised
    return PlanProblem.named("gap", **{**dict(N=N, H_rev=Hr, tube_kind=kind, recursive=rec, window_size=3, scaling=0.5, Qw=2.0, w_max=0.08,
                                             rom_z_min=[0.22, 0.22], rom_z_max=[0.4, 0.4], rom_v_min=[-0.15, -0.15], rom_v_max=[0.15, 0.15],
                                             goal=[0.6, 0.5], obs_c=[[0.36, 0.3], [0.28, 0.4]], obs_r=[0.05, 0.04]), **kw})


def _past(name, d, rows=slice(None)):
    """(e, v_prev, w0) as the kind takes them: the analytic kinds have no past."""
    if TUBES[name][3] is None:
        return None, None, d["w0"][rows]
    return d["e"][rows], d["v_prev"][rows], d["w0"][rows]


def _hetero(S, seed=0):
    """Random scenes around the plans of _plans (z0 near (0.3, 0.3), steps of up to 0.02): obstacles the paths run into."""
    from legged_gym_dev_amd.tube.plan import random_scenes
    return random_scenes(S, seed, [0.3, 0.3], n_obs=(0, 8), centre_box=((0.1, 0.1), (0.6, 0.6)), radius=(0.03, 0.12),
                         goal_box=((0.5, 0.4), (1.5, 1.5)), margin=0.0)


ROWS = (0, 5, 31, 32, 64)                                                # of B = 65: both tiles' edges and the one row of the third tile
HETERO_SEED = 2                                                          # rows 0, 5, 31, 32, 64 hold n_obs 0, 1 and 8 (asserted)


# ---------------------------------------------------------------- 1. uniform scenes are the entries without scenes
@pytest.mark.parametrize("N", [1, 5, 64])
@pytest.mark.parametrize("name", list(TUBES))
def test_uniform_scenes_are_the_entries_without_scenes(name, N):
    from legged_gym_dev_amd.tube import plan as pl
    tr = TUBES[name][3](N) if TUBES[name][3] else None
    try:
        p, Hr = _problem(name, N), TUBES[name][1]
        sc = pl.HipPlanScorer(tr, p, device=DEV)
        for B in (1, 31, 33, 65):
            d = _plans(B, N, Hr, seed=B)
            past, rep = _past(name, d), pl.Scenes.repeat(p, B)
            old, new = sc.score(d["z0"], d["v"], *past), sc.score(d["z0"], d["v"], *past, scenes=rep)
            assert sorted(old) == sorted(new) == ["cost", "fw", "min_clear", "n_viol", "w", "worst_node", "z"]
            for k in old:
                _same(old[k], new[k], f"score {k}, B {B}")
            if p.tube_kind != "nn_step":
                a = pl.HipGradPlanner(tr, p, pl.GradCfg(**RHO), device=DEV).gradient(d["z0"], d["v"], *past)
                b = pl.HipGradPlanner(tr, p, pl.GradCfg(**RHO), device=DEV, scenes=rep).gradient(d["z0"], d["v"], *past)
                assert sorted(a) == ["J", "cost", "grad", "min_clear", "pen"]
                for k in a:
                    _same(a[k], b[k], f"grad {k}, B {B}")
        P, cfg = 3, pl.MppiCfg(K=32, iters=1, sigma=0.1, seed=5, lambda_=5.0, **RHO)
        d = _plans(P, N, Hr, seed=77)
        got = []
        for scenes in (None, pl.Scenes.repeat(p, P)):
            pln = pl.HipMppiPlanner(tr, p, cfg, device=DEV, scenes=scenes)
            st = pln.state(d["z0"], d["v"], *_past(name, d))
            hist = torch.empty(P, 2, device=DEV)
            pln.step(st, 0, what=3, reset=True, hist_row=hist)
            got.append({**{k: st[k] for k in ("J", "vbar", "best_J", "best_v", "n_bad")}, "hist": hist})
        for k in got[0]:
            _same(got[0][k], got[1][k], f"mppi {k}")
        assert not torch.equal(got[0]["vbar"].cpu(), d["v"])
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 2. each plan sees its own scene
def _parts(sc):
    from legged_gym_dev_amd.tube.plan import Scenes
    return {"all": sc, "goals-only": Scenes(goal=sc.goal), "obstacles-only": Scenes(obs_c=sc.obs_c, obs_r=sc.obs_r, n_obs=sc.n_obs)}


@pytest.mark.parametrize("part", ["all", "goals-only", "obstacles-only"])
@pytest.mark.parametrize("name", ["l1", "nn", "step-recursive-lds"])
def test_each_plan_sees_its_own_scene(name, part):
    from legged_gym_dev_amd.tube import plan as pl
    N, B, Hr = 16, 65, TUBES[name][1]
    tr = TUBES[name][3](N) if TUBES[name][3] else None
    try:
        p = _problem(name, N)
        full = _hetero(B, HETERO_SEED)
        assert {0, 1, 8} <= set(full.n_obs[list(ROWS)].tolist()) and len(np.unique(full.goal, axis=0)) == B
        scenes = _parts(full)[part]
        d = _plans(B, N, Hr, seed=3)
        big = pl.HipPlanScorer(tr, p, device=DEV).score(d["z0"], d["v"], *_past(name, d), scenes=scenes)
        grad = p.tube_kind != "nn_step"
        if grad:
            gbig = pl.HipGradPlanner(tr, p, pl.GradCfg(**RHO), device=DEV, scenes=scenes).gradient(d["z0"], d["v"], *_past(name, d))
        for b in ROWS:
            row, q = slice(b, b + 1), scenes.problem(b, p)
            one = pl.HipPlanScorer(tr, q, device=DEV).score(d["z0"][row], d["v"][row], *_past(name, d, row))
            for k in one:
                _same(big[k][row], one[k], f"score {k}, plan {b}")
            if grad:
                gone = pl.HipGradPlanner(tr, q, pl.GradCfg(**RHO), device=DEV).gradient(d["z0"][row], d["v"][row], *_past(name, d, row))
                for k in gone:
                    _same(gbig[k][row], gone[k], f"grad {k}, plan {b}")
        if part == "all":                                                # the scenes matter: no two of the checked plans agree, and
            assert len({float(big["cost"][b]) for b in ROWS}) == len(ROWS)   # a scene without obstacles reports +inf and -1
            free = torch.as_tensor(full.n_obs == 0)
            assert bool(torch.isinf(big["min_clear"].cpu()[free]).all()) and bool((big["worst_node"].cpu()[free] == -1).all())
            assert bool(torch.isfinite(big["min_clear"].cpu()[~free]).all()) and bool((big["n_viol"].cpu()[:, 0] > 0).any())
        # MPPI: instance i of P = 3 is a call of one instance drawing as instance id i
        P, cfg = 3, pl.MppiCfg(K=32, iters=1, sigma=0.1, seed=5, lambda_=5.0, **RHO)
        sub = scenes.take(np.array([ROWS[0], ROWS[1], ROWS[4]]))
        m = _plans(P, N, Hr, seed=78)
        pln = pl.HipMppiPlanner(tr, p, cfg, device=DEV, scenes=sub)
        st = pln.state(m["z0"], m["v"], *_past(name, m), want=("cost", "min_clear", "pen"))
        hist = torch.empty(P, 2, device=DEV)
        pln.step(st, 0, what=3, reset=True, hist_row=hist)
        for i in range(P):
            row = slice(i, i + 1)
            one = pl.HipMppiPlanner(tr, sub.problem(i, p), dataclasses.replace(cfg, instance_offset=i), device=DEV)
            s1 = one.state(m["z0"][row], m["v"][row], *_past(name, m, row), want=("cost", "min_clear", "pen"))
            h1 = torch.empty(1, 2, device=DEV)
            one.step(s1, 0, what=3, reset=True, hist_row=h1)
            for k in ("J", "cost", "min_clear", "pen", "vbar", "best_J", "best_v", "n_bad"):
                _same(st[k][row], s1[k], f"mppi {k}, instance {i}")
            _same(hist[row], h1, f"mppi hist, instance {i}")
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 3. the loops are their steps
@pytest.mark.parametrize("name", ["l2_rolling", "nn"])
def test_the_scene_loops_equal_their_steps_composed_by_hand(name):
    from legged_gym_dev_amd.tube import plan as pl
    N, P, Hr = 5, 33, TUBES[name][1]
    tr = TUBES[name][3](N) if TUBES[name][3] else None
    try:
        p, scenes = _problem(name, N), _hetero(P, 4)
        d = _plans(P, N, Hr, seed=6)
        past = _past(name, d)
        mp = pl.HipMppiPlanner(tr, p, pl.MppiCfg(K=64, iters=3, sigma=0.1, sigma_decay=0.7, seed=8, lambda_=5.0, **RHO), device=DEV, scenes=scenes)
        sol = mp.plan(d["z0"], d["v"], *past)
        st, hist = mp.state(d["z0"], d["v"], *past), torch.empty(3, P, 2, device=DEV)
        for it in range(3):
            mp.step(st, it, what=3, reset=it == 0, hist_row=hist[it])
        for k, t in (("v", st["vbar"]), ("best_v", st["best_v"]), ("best_J", st["best_J"]), ("hist", hist), ("n_bad", st["n_bad"])):
            _same(sol[k], t, f"mppi {k}")
        for k, t in mp.scorer.score(d["z0"], sol["v"], *past, want=("z", "w"), scenes=scenes).items():
            _same(sol["score"][k], t, f"mppi score {k}")
        gp = pl.HipGradPlanner(tr, p, pl.GradCfg(iters=4, lr=0.02, **RHO), device=DEV, scenes=scenes)
        sol = gp.plan(d["z0"], d["v"], *past)
        st, hist = gp.state(d["z0"], d["v"], *past), torch.empty(5, P, 2, device=DEV)
        for it in range(5):
            gp.step(st, it, what=3 if it < 4 else 1, reset=it == 0, hist_row=hist[it])
        for k, t in (("v", st["v"]), ("best_v", st["best_v"]), ("best_J", st["best_J"]), ("hist", hist), ("n_bad", st["n_bad"])):
            _same(sol[k], t, f"descend {k}")
        assert not torch.equal(sol["v"].cpu(), d["v"])
        _same(sol["best_score"]["cost"], gp.scorer.score(d["z0"], sol["best_v"], *past, want=(), scenes=scenes)["cost"])
        # a mismatch of S is refused in lg_plan_scenes_check's words
        with pytest.raises(ValueError, match="lg_plan_scenes: S = 33 differs from the call's count of plans or instances = 2"):
            gp.plan(d["z0"][:2], d["v"][:2], *[t[:2] if t is not None else None for t in past])
    finally:
        if tr:
            tr.close()


def test_the_library_refuses_a_wrong_S_and_nn_step_gradients_with_scenes():
    import ctypes as C
    from legged_gym_dev_amd.tube import plan as pl
    p = _problem("l1", 5)
    sc = pl.HipPlanScorer(None, p, device=DEV)
    st, keep = _hetero(4, 0).to(DEV)
    d = _plans(5, 5, 0, seed=1)
    out = [torch.empty(5, device=DEV), torch.empty(5, device=DEV), torch.empty(5, dtype=torch.int32, device=DEV), torch.empty(5, 4, dtype=torch.int32, device=DEV)]
    ptr = lambda t: C.c_void_p(t.data_ptr())
    z0, v = d["z0"].to(DEV), d["v"].to(DEV)
    from legged_gym_dev_amd import capi
    call = capi.lg_plan_call(z0=z0.data_ptr(), count=5, scenes=C.pointer(st))
    rc = sc.lib.lg_plan_score(None, C.byref(sc.struct), C.byref(call), ptr(v), *[ptr(t) for t in out], None, None, None)
    assert rc == -1 and "lg_plan_scenes: S = 4 differs" in sc.lib.lg_last_error().decode()
    tr = TUBES["step"][3](5)
    try:
        with pytest.raises(ValueError, match="nn_step"):
            pl.HipGradPlanner(tr, _problem("step", 5), pl.GradCfg(), device=DEV, scenes=_hetero(5, 0))
    finally:
        tr.close()


# ---------------------------------------------------------------- 4. against the float64 restatement, plan by plan
def _per_plan_ref(p, scenes, d, fw, D):
    out = []
    for b in range(scenes.S):
        row = slice(b, b + 1)
        out.append(plan_ref.score(_ref_problem(scenes.problem(b, p)), d["z0"][row].numpy(), d["v"][row].numpy(), fw(b, D), d["w0"][row].numpy(), None, D))
    cat = lambda k: np.concatenate([o[k] for o in out])
    return {**{k: cat(k) for k in ("cost", "min_clear", "worst_node", "n_viol")}, "gmargin": np.concatenate([o["margin"][0] for o in out]),
            "bmargin": np.concatenate([o["margin"][1] for o in out]),
            "gap": np.array([(lambda s: s[1] - s[0] if len(s) > 1 else np.inf)(np.sort(o["g"][0].min(axis=1))) if o["g"].shape[2] else np.inf for o in out])}


@pytest.mark.parametrize("name", ["l1", "nn"])
def test_cost_clearance_and_counts_against_float64_per_plan(name):
    from legged_gym_dev_amd.tube import plan as pl
    N, B, Hr = 16, 65, TUBES[name][1]
    tr = TUBES[name][3](N) if TUBES[name][3] else None
    try:
        p, scenes = _problem(name, N), _hetero(B, HETERO_SEED)
        d = _plans(B, N, Hr, seed=3)
        got = {k: t.cpu().numpy() for k, t in pl.HipPlanScorer(tr, p, device=DEV).score(d["z0"], d["v"], *_past(name, d), scenes=scenes).items()}
        if name == "nn":                                                 # the MLP's values from the device: the walk is what is checked
            fw = lambda b, D: got["fw"][b:b + 1]
        else:
            fw = lambda b, D: plan_ref.analytic("l1", d["v"][b:b + 1].numpy(), p.scaling, p.window_size, D)
        r32, r64 = (_per_plan_ref(p, scenes, d, fw, D) for D in (np.float32, np.float64))
        for k in ("cost", "min_clear"):
            _yardstick(f"{name} {k}", got[k], r32[k], r64[k])
        keep = (r64["gmargin"] >= 1e-5) & (r64["bmargin"] >= 1e-6)
        print(f"{name}: {keep.mean():.3f} of the plans lie outside the margins")
        assert keep.mean() >= 0.9, f"the restatement leaves out {1 - keep.mean():.4f} of the plans"
        assert r64["gap"][keep].min() >= 1e-5, "two nodes tie for the smallest clearance: choose other plans"
        np.testing.assert_array_equal(got["n_viol"][keep], r64["n_viol"][keep])
        np.testing.assert_array_equal(got["worst_node"][keep], r64["worst_node"][keep])
        nv = r64["n_viol"][keep]
        assert all(len(np.unique(nv[:, j])) >= 3 for j in range(4)), "every count takes several values over the plans"
        if name == "l1":                                                 # the untrained MLP's tube peaks at two nodes, which take every arg-min
            assert len(np.unique(r64["worst_node"][keep])) > 4
    finally:
        if tr:
            tr.close()


# ---------------------------------------------------------------- 5. a fleet
def test_a_fleet_of_64_robots_each_in_its_own_scene():
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg
    S, H = 64, 3
    p = pl.PlanProblem(N=8, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], tube_kind="l1", scaling=0.02,
                       Q=[10.0, 0, 0, 10.0], R=[1.0, 0, 0, 1.0], rom_v_min=[-2.0, -2.0], rom_v_max=[2.0, 2.0])
    scenes = pl.random_scenes(S, 9, p.start, n_obs=(0, 3), centre_box=((0.2, -0.4), (0.8, 0.4)), radius=(0.05, 0.15),
                              goal_box=((0.8, -0.3), (1.2, 0.3)), margin=0.05)
    chain = pl.ChainedPlanner(pl.HipMppiPlanner(None, p, pl.MppiCfg(K=64, iters=4, sigma=0.3, seed=1), device=DEV, scenes=scenes),
                              pl.HipGradPlanner(None, p, pl.GradCfg(iters=10, lr=0.02), device=DEV, scenes=scenes))
    assert chain.scenes is scenes
    with pytest.raises(ValueError, match="same scenes"):
        pl.ChainedPlanner(chain.first, pl.HipGradPlanner(None, p, pl.GradCfg(), device=DEV))
    start = torch.tensor(p.start).repeat(S, 1)
    sol = chain.plan(start)
    assert bool((sol["best_J"] <= sol["first"]["best_J"]).all()), "the polish starts from MPPI's best plan and keeps an elite"
    assert bool((sol["best_J"] < sol["first"]["best_J"]).any())
    sim = HipRomSim(RomSimCfg(), device=DEV)
    try:
        res = pl.closed_loop(chain, sim, H, start, iters_first=6, keep_plans=True)
        again = pl.closed_loop(chain, sim, H, start, iters_first=6, keep_plans=True)
        torch.cuda.synchronize()
        for k in res:
            _same(res[k], again[k], f"rerun {k}")
        got = pl.audit_closed_loop(res, p, goal_tol=0.8, scenes=scenes)
        one = [pl.audit_closed_loop({k: t[i:i + 1] for k, t in res.items() if not k.startswith("plans_")}, scenes.problem(i, p), goal_tol=0.8)
               for i in range(S)]
        for key in ("actually_safe", "predicted_safe", "reached_goal"):
            assert got["by_robot"][key] == [o[key] == 1.0 for o in one], key
            assert got[key] == float(np.mean([o[key] for o in one])), key
        assert got["by_robot"]["covered"] == [o["covered_robots"] == 1.0 for o in one]
        assert got["by_robot"]["goal_distance"] == [o["goal_distance_mean"] for o in one]
        assert json.loads(json.dumps(got, allow_nan=False)) == got and got["robots"] == S and got["steps"] == H
        # every robot heads for its own goal: after H steps it is nearer to it than the start was
        d0 = np.linalg.norm(scenes.goals(p) - np.asarray(p.start), axis=1)
        assert (np.asarray(got["by_robot"]["goal_distance"]) < d0).all()
        print(f"fleet of {S}: predicted safe {got['predicted_safe']:.3f}, actually safe {got['actually_safe']:.3f}, coverage {got['coverage']:.3f}, "
              f"within 0.8 of the goal after {H} steps {got['reached_goal']:.3f}")
    finally:
        sim.close()


# ---------------------------------------------------------------- 6. the scripts
def test_scripts_with_scenes_reproduce_the_library_and_without_them_nothing_changes(tmp_path):
    import audit_plans
    import plan_tube
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim
    out = str(tmp_path / "plan")
    argv = ["--tube", "l1", "--scaling", "0.1", "--problem", "gap", "--N", "20", "--K", "64", "--iters", "4", "--sigma", "0.05", "--starts", "8",
            "--start_noise", "0.01", "--seed", "4", "--planner", "mppi+grad", "--grad_iters", "5", "--device", DEV]
    sflags = ["--scenes", "random", "--scene_seed", "3", "--scene_obs", "0,3"]
    got = plan_tube.main(argv + sflags + ["--out", out])
    assert json.load(open(os.path.join(out, "plan.json"))) == json.loads(json.dumps(got, allow_nan=False)) == got
    assert got["scenes"]["S"] == 8 and got["scenes"]["random"]["seed"] == 3 and len(got["audit"]["by_plan"]["actually_safe"]) == 8
    a = plan_tube.parse_args(argv + sflags)
    p = plan_tube.build_problem(a, None)
    scenes = plan_tube.build_scenes(a, p)[0]
    saved = pl.Scenes.load(os.path.join(out, "scenes.npz"))
    for k in ("goal", "obs_c", "obs_r", "n_obs"):
        np.testing.assert_array_equal(getattr(saved, k), getattr(scenes, k))
    sim = HipRomSim(audit_plans.sim_config(a, p), device=DEV)
    try:
        sol = plan_tube.make_planner(a, None, p, None, scenes).plan(plan_tube.starts(a, p))
        t = pl.track(sim, sol["score"]["z"], sol["v"])
        assert pl.audit(sol["score"], t, p, scenes=scenes) == got["audit"]
        np.testing.assert_array_equal(np.load(os.path.join(out, "plans.npz"))["v"], sol["v"].cpu().numpy())
        aud = audit_plans.main(["--tube", "l1", "--scaling", "0.1", "--problem", "gap", "--N", "20", "--plans", os.path.join(out, "plans.npz"),
                                "--scenes", os.path.join(out, "scenes.npz"), "--device", DEV, "--out", str(tmp_path / "audit")])
        for k, v in got["audit"].items():
            assert aud[k] == v, k
        assert aud["source"]["scenes_file"] == os.path.join(out, "scenes.npz")
        # without --scenes: plan.json is, byte for byte, what the script wrote before scenes existed
        plain = str(tmp_path / "plain")
        plan_tube.main(argv + ["--out", plain])
        a = plan_tube.parse_args(argv)
        z0 = plan_tube.starts(a, p)
        sol = plan_tube.make_planner(a, None, p, None).plan(z0)
        t = pl.track(sim, sol["score"]["z"], sol["v"])
        torch.cuda.synchronize()
        want = {"audit": pl.audit(sol["score"], t, p), "hist": sol["hist"].cpu().double().tolist(), "closed_loop": None, "starts": z0.double().tolist(),
                "mppi": {**{k: v for k, v in vars(plan_tube.mppi_cfg(a)).items() if k != "lambda_"}, "lambda": a.lambda_}, "problem": p.to_json(),
                "run": None, "tube": "l1", "level": None, "calibrated": False, "sim_cfg": [],
                "best_J": [float(x) for x in sol["best_J"].cpu()], "n_bad": [int(x) for x in sol["n_bad"].cpu()],
                "cost": [float(x) for x in sol["score"]["cost"].cpu()], "planner": "mppi+grad", "grad": vars(plan_tube.grad_cfg(a))}
        assert open(os.path.join(plain, "plan.json")).read() == json.dumps(want, indent=1, allow_nan=False)
        assert sorted(os.listdir(plain)) == ["plan.json", "plans.npz"]
    finally:
        sim.close()
