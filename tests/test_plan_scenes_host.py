"""Per-plan scenes, host side: lg_plan_scenes against the header, lg_plan_scenes_check's refusals and the
planning entries refusing a wrong S before a device is touched, Scenes' validation, round trips, random_scenes, the audits per scene
and the scripts' argument refusals.  No GPU."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
from legged_gym_dev_amd import capi  # noqa: E402
from legged_gym_dev_amd.tube import plan as pl  # noqa: E402


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd.lib import load
    return load()


def test_struct_matches_the_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu\\n",sizeof(lg_plan_scenes),' \
          'offsetof(lg_plan_scenes,S),offsetof(lg_plan_scenes,goal),offsetof(lg_plan_scenes,obs),offsetof(lg_plan_scenes,n_obs));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    T = capi.lg_plan_scenes
    assert out == [C.sizeof(T), T.S.offset, T.goal.offset, T.obs.offset, T.n_obs.offset]


def _struct(S, goal=1, obs=1, n_obs=1):
    """A struct whose pointers are never followed: the check is host code and reads the fields alone."""
    st = capi.lg_plan_scenes()
    st.S, st.goal, st.obs, st.n_obs = S, goal or None, obs or None, n_obs or None
    return st


CHECK = [(_struct(0), 0, "S = 0"), (_struct(-3), 3, "S = -3"), (_struct(4), 5, "S = 4 differs"), (_struct(4, obs=0), 4, "n_obs is given without obs"),
         (_struct(4, n_obs=0), 4, "obs is given without n_obs"), (_struct(4, 0, 0, 0), 4, "all NULL")]


@pytest.mark.parametrize("st,count,word", CHECK, ids=[c[2] for c in CHECK])
def test_check_refusals_name_the_field(lib, st, count, word):
    assert lib.lg_plan_scenes_check(C.byref(st), count) == -1
    msg = lib.lg_last_error().decode()
    assert msg.startswith("lg_plan_scenes: ") and word in msg


def test_check_accepts_each_valid_form(lib):
    for st in (_struct(4), _struct(4, obs=0, n_obs=0), _struct(4, goal=0)):
        assert lib.lg_plan_scenes_check(C.byref(st), 4) == 0


def test_every_entry_refuses_a_wrong_S_before_a_device_is_touched(lib):
    """Junk pointers everywhere: a launch, or any read of an array, would fault; the refusal comes first.  No GPU is present here."""
    p = pl.PlanProblem.named("gap", tube_kind="l1", N=5).to_struct()
    mc, gc = pl.MppiCfg(K=32, iters=2).to_struct(), pl.GradCfg(iters=2).to_struct()
    bad = _struct(4)
    j = C.c_void_p(64)
    pp = C.byref(p)
    call = lambda scenes: C.byref(capi.lg_plan_call(z0=64, count=5, scenes=C.pointer(scenes)))
    sc = call(bad)
    calls = {
        "lg_plan_score": (None, pp, sc, j, j, j, j, j, None, None, None),
        "lg_plan_mppi_step": (None, pp, C.byref(mc), sc, 0, 3, 1, j, j, None, None, None, j, j, None, j),
        "lg_plan_mppi": (None, pp, C.byref(mc), sc, j, j, j, j, None, j),
        "lg_plan_grad": (None, pp, C.byref(gc), sc, j, j, j, None, None, None),
        "lg_plan_descend_step": (None, pp, C.byref(gc), sc, 0, 3, 1, j, j, None, None, None, None, j, j, j, j, None, j),
        "lg_plan_descend": (None, pp, C.byref(gc), sc, j, j, j, j, j, j, None, j)}
    for name, args in calls.items():
        assert getattr(lib, name)(*args) == -1, name
        assert "lg_plan_scenes: S = 4 differs" in lib.lg_last_error().decode(), name
    # the gradient entries keep refusing nn_step in the same words with scenes as without, and the problem's own fields are still checked
    q = pl.PlanProblem.named("gap", tube_kind="nn_step", N=5).to_struct()
    ok = _struct(5)
    assert lib.lg_plan_grad(None, C.byref(q), C.byref(gc), call(ok), j, j, j, None, None, None) == -1
    assert "nn_step has no gradient planner" in lib.lg_last_error().decode()
    q = pl.PlanProblem.named("gap", tube_kind="l1", N=5).to_struct()
    q.obs_r[1] = -1.0
    assert lib.lg_plan_score(None, C.byref(q), call(ok), *calls["lg_plan_score"][3:]) == -1
    assert "obs_r[1]" in lib.lg_last_error().decode()


def test_a_library_from_before_the_call_struct_is_refused(lib):
    """A library that still has lg_plan_score_scenes takes the older positional lists: declare_plan_api marks it and leaves its six
    planning entries undeclared, and the scorer's helper refuses it -- host code, before any device work."""
    import types
    from legged_gym_dev_amd.lib import LeggedHipError
    entry = lambda: types.SimpleNamespace(argtypes=None)
    old = types.SimpleNamespace(lg_plan_score=entry(), lg_plan_score_scenes=entry(), lg_plan_check=entry(), lg_plan_scenes_check=entry())
    capi.declare_plan_api(old)
    assert old.plan_api_old is True and old.lg_plan_score.argtypes is None and old.lg_plan_score_scenes.argtypes is None
    assert len(old.lg_plan_check.argtypes) == 3 and len(old.lg_plan_scenes_check.argtypes) == 2      # unchanged entries stay usable
    with pytest.raises(LeggedHipError, match="lg_plan_score_scenes.*built before lg_plan_call"):
        pl.refuse_old_library(old)
    new = types.SimpleNamespace(lg_plan_score=entry(), lg_plan_check=entry())
    capi.declare_plan_api(new)
    assert new.plan_api_old is False and len(new.lg_plan_score.argtypes) == 11
    pl.refuse_old_library(new)
    assert lib.plan_api_old is False
    pl.refuse_old_library(lib)


G, OC, OR = np.zeros((3, 2)), np.zeros((3, 2, 2)), np.full((3, 2), 0.1)
BAD = [(dict(), "say nothing"), (dict(obs_c=OC), "together"), (dict(goal=G, n_obs=[1, 1, 1]), "n_obs is given without"),
       (dict(goal=np.zeros((3, 3))), r"goal must be"), (dict(goal=np.zeros((0, 2))), r"goal must be"),
       (dict(obs_c=np.zeros((3, 9, 2)), obs_r=np.zeros((3, 9))), "obs_c must be"), (dict(obs_c=OC, obs_r=np.zeros((3, 3))), "obs_r must be"),
       (dict(obs_c=OC, obs_r=OR, n_obs=[1, 3, 0]), r"n_obs must lie in 0\.\.2"), (dict(obs_c=OC, obs_r=OR, n_obs=[1, -1, 0]), "n_obs must lie"),
       (dict(obs_c=OC, obs_r=OR, n_obs=[1, 1]), "n_obs must be"), (dict(obs_c=OC, obs_r=OR, n_obs=[1.0, 1.0, 1.0]), "integers"),
       (dict(obs_c=OC, obs_r=np.array([[0.1, 0.1], [0.1, -0.1], [0.1, 0.1]])), "radius"),
       (dict(obs_c=OC, obs_r=np.array([[0.1, 0.1], [np.inf, 0.1], [0.1, 0.1]])), "radius"),
       (dict(obs_c=np.where(np.arange(12).reshape(3, 2, 2) == 5, np.nan, 0.0), obs_r=OR), "centre"),
       (dict(goal=np.array([[0, 0], [np.inf, 0], [0, 0]], float)), "goal is finite"), (dict(goal=np.zeros((4, 2)), obs_c=OC, obs_r=OR), "4 scenes")]


@pytest.mark.parametrize("kw,word", BAD, ids=[f"{i}-{w[:12]}" for i, (_, w) in enumerate(BAD)])
def test_scenes_validation(kw, word):
    with pytest.raises(ValueError, match=word):
        pl.Scenes(**kw)


def test_slots_past_n_obs_are_not_validated_and_pack_as_zeros():
    c, r = np.full((2, 3, 2), np.nan), np.full((2, 3), -1.0)
    c[0, 0], r[0, 0], c[1, :2], r[1, :2] = [1.0, 2.0], 0.5, [[3.0, 4.0], [5.0, 6.0]], [0.25, 0.75]
    sc = pl.Scenes(obs_c=c, obs_r=r, n_obs=[1, 2])
    obs = sc.packed()
    assert obs.shape == (2, 8, 3) and obs.dtype == np.float32 and sc.S == 2 and sc.goal is None
    assert obs[0, 0].tolist() == [1.0, 2.0, 0.5] and obs[1, 1].tolist() == [5.0, 6.0, 0.75] and not obs[0, 1:].any() and not obs[1, 2:].any()
    assert sc.n_obs.dtype == np.int32 and sc.n_obs.tolist() == [1, 2]


def test_problem_round_trip_save_load_and_repeat(tmp_path):
    base = pl.PlanProblem.named("gap", tube_kind="l1", N=7)
    sc = pl.random_scenes(9, 4, base.start, n_obs=(0, 8))
    assert {0, 8} <= set(sc.n_obs.tolist())
    for s in range(sc.S):
        q = sc.problem(s, base)
        n = int(sc.n_obs[s])
        assert q.n_obs == n and q.N == 7 and q.tube_kind == "l1" and q.start == base.start and q.rom_v_max == base.rom_v_max
        st = q.to_struct()
        assert [st.goal[0], st.goal[1]] == sc.goal[s].tolist() and st.n_obs == n
        assert [[st.obs_c[i][0], st.obs_c[i][1], st.obs_r[i]] for i in range(n)] == sc.packed()[s, :n].tolist()
        pl.check_envelope(q)
    assert base.goal == pl.PROBLEMS["gap"]["goal"]                       # the base is not touched
    goals = pl.Scenes(goal=sc.goal)
    assert goals.problem(2, base).obs_c == base.obs_c and goals.problem(2, base).goal == sc.goal[2].tolist() and goals.packed() is None
    f = str(tmp_path / "scenes.npz")
    sc.save(f)
    back = pl.Scenes.load(f)
    for k in ("goal", "obs_c", "obs_r", "n_obs"):
        np.testing.assert_array_equal(getattr(back, k), getattr(sc, k))
    goals.save(f)
    assert pl.Scenes.load(f).obs_c is None and sorted(np.load(f).files) == ["goal"]
    np.savez(f, goal=sc.goal, radius=sc.obs_r)
    with pytest.raises(ValueError, match="radius"):
        pl.Scenes.load(f)
    rep = pl.Scenes.repeat(base, 5)
    assert rep.S == 5 and all(rep.problem(s, base) == base for s in range(5)) and rep.n_obs.tolist() == [2] * 5
    free = pl.Scenes.repeat(dataclasses.replace(base, obs_c=[], obs_r=[]), 3)
    assert free.n_obs.tolist() == [0, 0, 0] and not free.packed().any()
    part = sc.take(np.array([3, 3, 0]))
    assert part.S == 3 and part.problem(1, base) == sc.problem(3, base) and part.problem(2, base) == sc.problem(0, base)


def test_random_scenes():
    start, kw = [0.3, 0.3], dict(n_obs=(0, 8), margin=0.07, radius=(0.1, 0.4))
    a, b, c = pl.random_scenes(256, 11, start, **kw), pl.random_scenes(256, 11, start, **kw), pl.random_scenes(256, 12, start, **kw)
    for k in ("goal", "obs_c", "obs_r", "n_obs"):
        np.testing.assert_array_equal(getattr(a, k), getattr(b, k))
    assert not np.array_equal(a.goal, c.goal) and not np.array_equal(a.obs_c, c.obs_c)
    assert set(a.n_obs.tolist()) == set(range(9)) and a.S == 256
    cc, rr, live = a.obstacles(None)
    assert cc.dtype == np.float64 and live.sum() == a.n_obs.sum()
    s64 = np.asarray(start, np.float32).astype(np.float64)
    for q in (np.broadcast_to(s64, (256, 2)), a.goal.astype(np.float64)):
        clear = np.linalg.norm(q[:, None, :] - cc, axis=2) - rr
        assert clear[live].min() >= 0.07
    assert (a.obs_r[live] >= np.float32(0.1)).all() and (a.obs_r[live] <= np.float32(0.4)).all() and len(np.unique(a.goal, axis=0)) == 256
    per = pl.random_scenes(4, 0, np.array([[0.0, 0.0], [2.0, 2.0], [0.0, 2.0], [2.0, 0.0]]), n_obs=(3, 3), margin=0.1)
    cc, rr, live = per.obstacles(None)
    assert (np.linalg.norm(np.array([[0.0, 0.0], [2.0, 2.0], [0.0, 2.0], [2.0, 0.0]])[:, None] - cc, axis=2) - rr).min() >= 0.1
    with pytest.raises(ValueError, match="scene 0 was rejected 1000 times"):
        pl.random_scenes(2, 0, [0.5, 0.5], n_obs=(1, 1), centre_box=((0.5, 0.5), (0.5, 0.5)), radius=(0.2, 0.2))
    for kw in (dict(n_obs=(2, 1)), dict(n_obs=(0, 9)), dict(radius=(0.3, 0.1))):
        with pytest.raises(ValueError):
            pl.random_scenes(2, 0, start, **kw)
    with pytest.raises(ValueError):
        pl.random_scenes(0, 0, start)


def _tracked(B, N, seed):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.rand(*s, generator=g)
    score = {"w": 0.1 * r(B, N + 1), "min_clear": r(B) - 0.3}
    track = {"w_true": 0.1 * r(B, N + 1), "pz_x": 0.3 + torch.cumsum(0.12 * r(B, N + 1, 2), dim=1)}
    return score, track


def test_audit_with_scenes_is_the_audit_of_each_plan_in_its_own_problem():
    B, N = 40, 12
    base = pl.PlanProblem.named("gap", tube_kind="l1", N=N)
    sc = pl.random_scenes(B, 2, base.start, n_obs=(0, 8), centre_box=((0.3, 0.3), (1.7, 1.7)))
    score, track = _tracked(B, N, 5)
    got = pl.audit(score, track, base, scenes=sc)
    one = [pl.audit({k: t[b:b + 1] for k, t in score.items()}, {k: t[b:b + 1] for k, t in track.items()}, sc.problem(b, base)) for b in range(B)]
    for key, name in (("actually_safe", "actually_safe"), ("predicted_safe", "predicted_safe"), ("covered", "covered_plans")):
        assert got["by_plan"][key] == [o[name] == 1.0 for o in one], key
        assert got[name] == float(np.mean([o[name] for o in one])), name
    assert 0.1 < got["actually_safe"] < 0.9, "the plans must split over safe and unsafe for the comparison to say something"
    assert got["actually_safe"] != pl.audit(score, track, base)["actually_safe"]
    assert json.loads(json.dumps(got, allow_nan=False)) == got
    # the problem's own scene for every plan is the audit without scenes, number for number
    plain, rep = pl.audit(score, track, base), pl.audit(score, track, base, scenes=pl.Scenes.repeat(base, B))
    assert {k: v for k, v in rep.items() if k != "by_plan"} == plain and "by_plan" not in plain
    with pytest.raises(ValueError, match="lg_plan_scenes: S = 40 differs"):
        pl.audit({k: t[:3] for k, t in score.items()}, {k: t[:3] for k, t in track.items()}, base, scenes=sc)
    # goals alone: the obstacles stay the problem's
    assert pl.audit(score, track, base, scenes=pl.Scenes(goal=sc.goal))["actually_safe"] == plain["actually_safe"]


def test_closed_loop_and_env_audits_with_scenes():
    P, H = 24, 9
    base = pl.PlanProblem.named("gap", tube_kind="l1", N=5)
    sc = pl.random_scenes(P, 6, base.start, n_obs=(0, 4), centre_box=((0.3, 0.3), (1.7, 1.7)))
    g = torch.Generator().manual_seed(1)
    z = 0.3 + torch.cumsum(0.15 * torch.rand(P, H + 1, 2, generator=g), dim=1)
    z[::3, -1] = torch.as_tensor(sc.goal[::3]) + 0.01                   # a third of the robots end at their own goal
    res = {"z": z, "w": 0.05 * torch.rand(P, H + 1, generator=g), "pz_x": z + 0.03 * (torch.rand(P, H + 1, 2, generator=g) - 0.5),
           "min_clear": torch.rand(P, H, generator=g) - 0.1}
    got = pl.audit_closed_loop(res, base, goal_tol=0.1, scenes=sc)
    one = [pl.audit_closed_loop({k: t[p:p + 1] for k, t in res.items()}, sc.problem(p, base), goal_tol=0.1) for p in range(P)]
    for key in ("actually_safe", "predicted_safe", "reached_goal"):
        assert got["by_robot"][key] == [o[key] == 1.0 for o in one], key
        assert got[key] == float(np.mean([o[key] for o in one])), key
    assert got["by_robot"]["goal_distance"] == [o["goal_distance_mean"] for o in one] and got["by_robot"]["covered"] == [o["covered_robots"] == 1.0 for o in one]
    assert got["reached_goal"] >= 1 / 3 and pl.audit_closed_loop(res, base)["reached_goal"] < got["reached_goal"]
    plain, rep = pl.audit_closed_loop(res, base), pl.audit_closed_loop(res, base, scenes=pl.Scenes.repeat(base, P))
    assert {k: v for k, v in rep.items() if k != "by_robot"} == plain
    assert json.loads(json.dumps(got, allow_nan=False)) == got
    # audit_env: the completed plans keep their own scenes
    from legged_gym_dev_amd.tube.plan_env import audit_env
    score, track = _tracked(P, H, 8)
    done = torch.arange(P) % 4 != 1
    trk = {**track, "completed": done, "dead": ~done}
    env = audit_env(score, trk, base, scenes=sc)
    idx = done.nonzero().flatten()
    want = pl.audit({k: t[idx] for k, t in score.items()}, {k: t[idx] for k, t in track.items()}, base, scenes=sc.take(idx.numpy()))
    assert {k: env[k] for k in want if k != "plans"} == {k: v for k, v in want.items() if k != "plans"} and env["plans"] == P
    assert audit_env(score, trk, base, scenes=pl.Scenes.repeat(base, P))["actually_safe"] == audit_env(score, trk, base)["actually_safe"]


def test_warm_start_goes_to_each_scenes_goal():
    base = pl.PlanProblem.named("right", tube_kind="l1", N=6)
    sc = pl.random_scenes(3, 1, base.start)
    stand_in = type("P", (), {"problem": base, "scenes": sc, "warm_start": pl.HipMppiPlanner.warm_start})()
    z0 = np.array([[0.5, 0.0], [0.4, 0.1], [0.6, -0.1]])
    v = stand_in.warm_start(z0)
    for s in range(3):
        want = np.clip(pl.warm_start("interpolate", z0[s], sc.goals(base)[s], 6, base.dt)[1], base.rom_v_min, base.rom_v_max).astype(np.float32)
        np.testing.assert_array_equal(v[s], want)
    stand_in.scenes = None
    np.testing.assert_array_equal(stand_in.warm_start(z0)[1], np.clip(pl.warm_start("interpolate", z0[1], base.goal, 6, base.dt)[1], -1, 1).astype(np.float32))
    stand_in.scenes = sc
    with pytest.raises(ValueError, match="lg_plan_scenes: S = 3 differs"):
        stand_in.warm_start(z0[:2])


def test_scripts_refuse_bad_scene_arguments(tmp_path, capsys):
    import audit_plans
    import plan_tube
    base = ["--tube", "l1", "--problem", "gap"]
    for extra, word in ((["--scene_seed", "3"], "--scene_seed belongs to --scenes random"), (["--scenes", "some.txt"], "random or a .npz"),
                        (["--scenes", "f.npz", "--scene_margin", "0.1"], "taken as it is"), (["--scenes", "random", "--scene_obs", "3"], "LO,HI"),
                        (["--scenes", "random", "--scene_obs", "2,9"], "<= 8"), (["--scenes", "random", "--scene_radius", "0.4,0.1"], "LO <= HI"),
                        (["--scenes", "random", "--scene_margin", "-1"], "negative")):
        with pytest.raises(SystemExit):
            plan_tube.parse_args(base + extra)
        assert word in capsys.readouterr().err, extra
    a = plan_tube.parse_args(base + ["--scenes", "random", "--starts", "4", "--scene_obs", "0,2"])
    assert a.scene_obs == (0, 2) and a.scene_radius == (0.1, 0.4) and a.scene_seed == 0 and a.scene_margin == 0.05
    assert plan_tube.parse_args(base).scenes is None and plan_tube.build_scenes(plan_tube.parse_args(base), None) == (None, None)
    p = pl.PlanProblem.named("gap", tube_kind="l1")
    sc, src = plan_tube.build_scenes(a, p)
    assert sc.S == 4 and src["S"] == 4 and src["random"]["seed"] == 0 and json.dumps(src, allow_nan=False)
    np.testing.assert_array_equal(sc.goal, plan_tube.build_scenes(a, p)[0].goal)
    f = str(tmp_path / "s.npz")
    sc.save(f)
    with pytest.raises(ValueError, match="holds 4 scenes; --starts is 3"):
        plan_tube.build_scenes(plan_tube.parse_args(base + ["--scenes", f, "--starts", "3"]), p)
    with pytest.raises(SystemExit):
        audit_plans.parse_args(base + ["--warm_start", "interpolate", "--scenes", "scenes.json"])
    assert "a .npz file" in capsys.readouterr().err
    plans = str(tmp_path / "plans.npz")
    np.savez(plans, z0=np.zeros((3, 2), np.float32), v=np.zeros((3, 50, 2), np.float32))
    with pytest.raises(ValueError, match="4 scenes and --plans .* 3 plans"):
        audit_plans.build_scene_plans(audit_plans.parse_args(base + ["--plans", plans, "--scenes", f]), p)
    z0, v, source, rep = audit_plans.build_scene_plans(audit_plans.parse_args(base + ["--warm_start", "interpolate", "--perturb", "2", "--scenes", f]), p)
    assert tuple(v.shape) == (12, 50, 2) and rep.S == 12 and source["scenes_file"] == f
    assert rep.problem(5, p) == sc.problem(1, p) and rep.problem(6, p) == sc.problem(2, p)
    np.testing.assert_array_equal(v[3].numpy(), pl.warm_start("interpolate", p.start, sc.goals(p)[1], 50, p.dt)[1].astype(np.float32))
    assert not torch.equal(v[4], v[3]) and not torch.equal(v[4], v[1])
