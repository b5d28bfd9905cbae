"""Plans tracked on the legged env, on the GPU: the plan-following generator's law and the recorder against
the float32 restatement (tests/plan_env_ref.py), the window's nodes against the scorer's on the bits, resets, track_env and the
--robot script end to end.  33 envs by default: two full post-step tiles of 16 and a ragged one."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.tube import plan as pl
from legged_gym_dev_amd.tube import plan_env as pe
from tests import harness
from tests import plan_env_ref as ref
from tests.test_eval_generators import GENS, TRAJ, _cfg, _setup, square_v

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
PLAN = "PlanTrajectoryGenerator"
OK, OT, OV = (capi.TG_FIELDS[k][0] for k in ("k", "t", "v"))
N_ENV, ROM_DT = 33, 0.1


def _handle(n=N_ENV, Nw=10, gen=PLAN, seed=3, vlim=None):
    cfg = _cfg(gen, n=n)
    cfg.trajectory_generator.N = Nw
    cfg.env.num_observations = 9 + 2 * Nw + 3 * 12
    cfg.domain_rand.randomize_rom_distance = False
    if vlim is not None:
        cfg.rom.v_min, cfg.rom.v_max = [-vlim, -vlim], [vlim, vlim]
    env = harness.HipHandle(_setup(cfg, seed=seed))
    env.set_step_counter(0)
    env.call("reset_all")
    env.sync()
    return env


def _post_step(env):
    """test_eval_generators._run_no_reset's pattern, one step: the post-step alone, contact forces zeroed, the episode young."""
    env.set("contact_forces", np.zeros(env.core.t["contact_forces"].shape, np.float32))
    env.set("episode_length", np.zeros(env.setup.num_envs, np.int64))
    env.call("post_physics_step")


def _set_plans(env, v):
    env._plans = torch.as_tensor(np.ascontiguousarray(v, np.float32)).to(DEV)
    env.call("traj_set_plans", C.c_void_p(env._plans.data_ptr()) if v.shape[1] else None, int(v.shape[1]))


def _traj_reset(env, z):
    env._z = torch.as_tensor(np.ascontiguousarray(z, np.float32)).to(DEV)
    env.call("traj_reset", C.c_void_p(env._z.data_ptr()))


def _law_from_env(env, plans, Nw):
    law = ref.PlanLaw(plans, Nw, ROM_DT, env.setup.dt)
    g = env.get("tg_state")
    law.k, law.t, law.win, law.v_in = g[:, OK].copy(), g[:, OT].copy(), env.get("tg_traj").copy(), g[:, OV:OV + 2].copy()
    return law


def _check(env, law, msg):
    g = env.get("tg_state")
    np.testing.assert_array_equal(g[:, OV:OV + 2], law.v_in, err_msg=msg + ": the input in force")
    np.testing.assert_array_equal(g[:, OK], law.k, err_msg=msg + ": k")
    np.testing.assert_array_equal(g[:, OT], law.t, err_msg=msg + ": t")
    np.testing.assert_array_equal(env.get("tg_traj"), law.win, err_msg=msg + ": the window")


# ------------------------------------------------------------------------------------------------ the C entries' refusals
def test_set_plans_refusals():
    from legged_gym_dev_amd.lib import LeggedHipError
    env = _handle(n=4)
    sq = _handle(n=4, gen=GENS["square"])
    z, meta = harness.load_fixture("anymal_c_flat")
    vel = harness.HipHandle(harness.make_setup("anymal_c_flat", z, meta)[0])
    v = torch.zeros(4, 3, 2, device=DEV)
    try:
        for h, args, word in ((env, (C.c_void_p(v.data_ptr()), 65), "n_nodes = 65 must lie in 0..64"), (env, (C.c_void_p(v.data_ptr()), -1), "n_nodes = -1"),
                              (env, (None, 3), "v is null"), (sq, (C.c_void_p(v.data_ptr()), 3), "not PlanTrajectoryGenerator"),
                              (vel, (C.c_void_p(v.data_ptr()), 3), "not a trajectory env")):
            with pytest.raises(LeggedHipError, match=word):
                h.call("traj_set_plans", *args)
        env.call("traj_set_plans", None, 0)                        # no node: allowed
        env.call("traj_set_plans", C.c_void_p(v.data_ptr()), 3)
        rec = capi.lg_traj_rec()
        with pytest.raises(LeggedHipError, match="rows_max = 0"):
            env.call("traj_rec_begin", C.byref(rec))
        with pytest.raises(LeggedHipError, match="not a trajectory env"):
            vel.call("traj_rec_step", C.byref(rec))
        with pytest.raises(LeggedHipError, match="unknown generator kind"):
            env.call("set_traj_generator", 5, 0)
        env.sync()
    finally:
        for h in (env, sq, vel):
            h.close()


# ------------------------------------------------------------------------------------------------ 1. the law
@pytest.mark.parametrize("Nw", [2, 10])
@pytest.mark.parametrize("n_nodes", [1, 5, 64])
def test_law_with_physics_out_of_the_way(Nw, n_nodes):
    """After every env step LG_TG_V, k, t and the whole window equal the restatement; after each ROM step the head equals the float32
    chain from the start.  Inputs are 0 before set_plans, during the pre-roll and for k >= n_nodes."""
    rng = np.random.default_rng(10 * Nw + n_nodes)
    env = _handle(Nw=Nw)
    try:
        S = round(ROM_DT / env.setup.dt)
        w = env.get("tg_traj")
        np.testing.assert_array_equal(w, np.repeat(w[:, -1:], Nw + 1, 1))         # the reset's pre-roll (t < 0): input 0, the window constant
        assert not env.get("tg_state")[:, OV:OV + 2].any() and not env.get("tg_state")[:, capi.TG_FIELDS["stationary"][0]].any()
        law = _law_from_env(env, np.zeros((N_ENV, 0, 2), np.float32), Nw)        # before any plan was set
        for s in range(S + 2):
            _post_step(env)
            law.step()
            _check(env, law, f"no plan, step {s}")
        np.testing.assert_array_equal(env.get("tg_traj"), w)
        plans = rng.uniform(-0.35, 0.35, (N_ENV, n_nodes, 2)).astype(np.float32)
        start = rng.uniform(-20, 20, (N_ENV, 2)).astype(np.float32)
        _set_plans(env, plans)
        _traj_reset(env, start)
        law = ref.PlanLaw(plans, Nw, ROM_DT, env.setup.dt)
        law.reset(np.arange(N_ENV), start)
        _check(env, law, "after reset(z)")
        nodes = ref.chain(start, plans, ROM_DT)
        m = 0
        for s in range((n_nodes + 2) * S + 1):
            _post_step(env)
            if law.step().all():
                m += 1
                want = nodes[:, min(m, n_nodes)]                               # past the plan the head stays on the last node
                np.testing.assert_array_equal(env.get("tg_traj")[:, -1], want, err_msg=f"head after ROM step {m}")
            _check(env, law, f"step {s}")
        assert m >= n_nodes + 2 and int(env.get("n_reset")[0]) == 0
        g = env.get("tg_state")
        assert not g[:, OV:OV + 2].any() and not g[:, capi.TG_FIELDS["stationary"][0]].any()      # k >= n_nodes: input 0
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ 2. the scored plan
@pytest.mark.parametrize("Np", [8, 50])
def test_the_robots_reference_is_the_scored_plan(Np):
    """problem.dt == rom.dt: the successive window heads are HipPlanScorer.score(...)['z'][:, 1:] on the bits."""
    p = pl.PlanProblem.named("gap", tube_kind="l2", N=Np)
    assert p.dt == ROM_DT
    g = torch.Generator().manual_seed(Np)
    v = (torch.rand(N_ENV, Np, 2, generator=g) * 0.4 - 0.2)
    z0 = torch.tensor(p.start, dtype=torch.float32).repeat(N_ENV, 1)
    env = _handle()
    try:
        z = pl.HipPlanScorer(None, p, device=DEV).score(z0, v, want=("z",))["z"]
        _set_plans(env, v.numpy())
        _traj_reset(env, z0.numpy())
        heads, k = [], env.get("tg_state")[:, OK].copy()
        for s in range(Np * 5 + 5):
            _post_step(env)
            kn = env.get("tg_state")[:, OK]
            assert np.all(kn == kn[0])
            if kn[0] != k[0] and len(heads) < Np:
                heads.append(env.core.t["tg_traj"][:, -1].clone())
            k = kn.copy()
        assert len(heads) == Np
        assert torch.equal(torch.stack(heads, 1), z[:, 1:])
        assert torch.equal(z[:, 0], z0.to(DEV))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ 3. resets
def test_reset_ids_replays_one_plan_and_leaves_the_others_alone():
    rng = np.random.default_rng(5)
    plans = rng.uniform(-0.35, 0.35, (N_ENV, 12, 2)).astype(np.float32)
    start = rng.uniform(-5, 5, (N_ENV, 2)).astype(np.float32)
    a, b = _handle(seed=9), _handle(seed=9)
    try:
        for env in (a, b):
            _set_plans(env, plans)
            _traj_reset(env, start)
        law = ref.PlanLaw(plans, 10, ROM_DT, a.setup.dt)
        law.reset(np.arange(N_ENV), start)
        for s in range(17):                                        # mid-plan: k = 4, between two ROM steps
            for env in (a, b):
                _post_step(env)
            law.step()
        _check(a, law, "before the reset")
        assert law.k[0] == 4 and law.v_in.any()
        who = 20
        ids = torch.tensor([who], dtype=torch.int32, device=DEV)
        a.call("reset_ids", C.c_void_p(ids.data_ptr()), 1)
        a.sync()
        xy = a.get("root_states")[who, :2]
        law.reset([who], xy[None])
        _check(a, law, "after reset_ids")                          # the others: k_traj_late left their v alone; env 20: k = 0, v = 0, window at its root
        others = np.arange(N_ENV) != who
        for s in range(12):
            for env in (a, b):
                _post_step(env)
            law.step()
            _check(a, law, f"after the reset, step {s}")
            for key in ("tg_state", "tg_traj"):
                np.testing.assert_array_equal(a.get(key)[others], b.get(key)[others], err_msg=key)
        assert law.k[who] == 3 and law.k[0] == 6
        np.testing.assert_array_equal(a.get("tg_traj")[who, -1], ref.chain(xy[None], plans[who:who + 1], ROM_DT)[0, 3])   # replayed from node 0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ product env helpers
def _product_env(n, Nw=None, push=False):
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.utils import get_args
    env_cfg, train_cfg = pe.plan_env_cfg(TRAJ, n, push_robots=push)
    if Nw is not None:
        env_cfg.trajectory_generator.N = Nw
        env_cfg.env.num_observations = 9 + 2 * Nw + 3 * 12
    args = get_args(["--task", TRAJ, "--num_envs", str(n), "--headless"])
    args.sim_device = args.rl_device = DEV
    env, _ = task_registry.make_env(name=TRAJ, args=args, env_cfg=env_cfg)
    return env, train_cfg, args


# ------------------------------------------------------------------------------------------------ 4. the recorder
@pytest.mark.parametrize("n", [17, 257])
def test_recorder_against_a_host_loop_on_the_same_env(n):
    """Full env.step calls with zero actions (the robot stands on its default pose), Nw = 2, Np = 6; env 3 times out mid-plan.  The
    test records by the three rules with torch indexing after every step; the device recorder runs beside it.  Everything is
    torch.equal, whatever set of envs ends up dead; separately: env 3 is dead with rows < rows_max and every other env completes."""
    Nw, Np = 2, 6
    R = Nw + Np + 1
    env, _, _ = _product_env(n, Nw=Nw)
    try:
        g = torch.Generator().manual_seed(n)
        v = (torch.rand(n, Np, 2, generator=g) * 0.4 - 0.2).to(DEV)
        B, Np_, Nw_, S, steps = pe.check_track(env, v, torch.zeros(n, 2, device=DEV))
        assert (Nw_, S, steps) == (Nw, 5, 50)
        zeros = torch.zeros(n, env.num_actions, device=DEV)
        env.reset()
        env.traj_gen.set_plans(v)
        start = env.rom.proj_z(env.root_states).clone()
        env.traj_gen.reset(start)
        env.trajectory.copy_(start[:, None, :].expand_as(env.trajectory))
        rec = pe.TrajRecorder(env, R, want_x=n == 17)
        rec.begin()
        tg = env.traj_gen
        z, pz, vv = torch.zeros(n, R, 2, device=DEV), torch.zeros(n, R, 2, device=DEV), torch.zeros(n, R - 1, 2, device=DEV)
        x = torch.zeros(n, R, rec.x_n, device=DEV)
        z[:, 0], pz[:, 0], x[:, 0] = env.trajectory[:, 0], env.rom.proj_z(env.root_states), env.get_state()
        rows, dead, k_mark = torch.ones(n, dtype=torch.long, device=DEV), torch.zeros(n, dtype=torch.bool, device=DEV), tg.k.clone()
        assert torch.equal(rec.z[:, 0], start) and torch.equal(rec.pz_x[:, 0], start) and torch.equal(rec.k_mark, k_mark)
        env.episode_length_buf[3] = env.max_episode_length - 24     # times out on env step 24 of 50
        for s in range(steps):
            _, _, _, dones, _ = env.step(zeros)
            rec.step()
            live = ~dead
            dead |= live & dones
            w = (live & ~dones & (tg.k != k_mark) & (rows < R)).nonzero().flatten()
            r = rows[w]
            z[w, r], pz[w, r], x[w, r] = env.trajectory[w, 0], env.rom.proj_z(env.root_states)[w], env.get_state()[w]
            vv[w, r - 1] = tg.v[w]
            rows[w] += 1
            k_mark[w] = tg.k[w]
        torch.cuda.synchronize()
        assert torch.equal(rec.rows.long(), rows) and torch.equal(rec.dead.bool(), dead)
        assert torch.equal(rec.z, z) and torch.equal(rec.pz_x, pz) and torch.equal(rec.v, vv)
        if rec.x is not None:
            assert torch.equal(rec.x, x) and bool(torch.isfinite(x).all())
        others = torch.arange(n, device=DEV) != 3
        assert bool(dead[3]) and 1 < int(rows[3]) < R
        assert not bool(dead[others].any()), f"standing robots terminated: {dead.nonzero().flatten().tolist()}"
        assert bool((rows[others] == R).all())
        # the recorded inputs are the plan's: the ROM step that wrote row m applied plan node m - 1 to the window's head
        assert torch.equal(rec.v[others][:, :Np], v[others])
        assert int(env.fault_total[0]) == 0
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ 5. track_env end to end
def test_track_env_with_a_fresh_policy_and_audit():
    """B = 33 under a freshly initialised policy: shapes, keys, the alignment against the recorder's raw rows, completed against
    rows and dead, audit_env as strict JSON.  Nothing is asserted about coverage: an untrained policy falls."""
    from legged_gym_dev_amd.envs import task_registry
    B, Np, Hr = N_ENV, 8, 3
    env, train_cfg, args = _product_env(B)
    runner = None
    try:
        train_cfg.runner.resume = False
        runner, _ = task_registry.make_alg_runner(env=env, name=TRAJ, args=args, train_cfg=train_cfg, log_root=None)
        policy = runner.get_inference_policy(device=env.device)
        p = pl.PlanProblem.named("gap", tube_kind="l2", N=Np, H_rev=Hr)
        g = torch.Generator().manual_seed(1)
        v = torch.rand(B, Np, 2, generator=g) * 0.4 - 0.2
        z0 = torch.tensor(p.start, dtype=torch.float32).repeat(B, 1)
        with pytest.raises(ValueError, match="allow_fast"):
            pe.track_env(env, policy, v * 10, z0)
        with pytest.raises(ValueError, match="set_plans"):
            env.traj_gen.set_plans(torch.zeros(B + 1, Np, 2))
        t = pe.track_env(env, policy, v, z0, H_rev=Hr, want=("rec", "x"))
        torch.cuda.synchronize()
        Nw, rec = 10, t["rec"]
        R = Nw + Np + 1
        assert rec.rows_max == R and tuple(rec.z.shape) == (B, R, 2)
        for k, shape in (("pz_x", (B, Np + 1, 2)), ("z_ref", (B, Np + 1, 2)), ("w_true", (B, Np + 1)), ("completed", (B,)), ("rows", (B,)),
                         ("dead", (B,)), ("e_past", (B, Hr)), ("v_prev", (B, Hr, 2)), ("w0", (B,)), ("x", (B, Np + 1, 37))):
            assert tuple(t[k].shape) == shape, k
        rows, dead = rec.rows.cpu().numpy(), rec.dead.cpu().numpy()
        assert np.all((rows >= 1) & (rows <= R))
        np.testing.assert_array_equal(t["completed"].cpu().numpy(), (rows == R) & (dead == 0))
        assert np.all((rows == R) | (dead == 1)), "an env that neither fell nor timed out must fill its rows within the horizon"
        want = ref.align(rec.z.cpu().numpy(), rec.pz_x.cpu().numpy(), rows, dead, z0.numpy(), Nw, Np, Hr)
        for k in ("pz_x", "z_ref"):
            np.testing.assert_array_equal(t[k].cpu().numpy(), want[k], err_msg=k)
        for k in ("w_true", "e_past", "w0"):
            np.testing.assert_allclose(t[k].cpu().numpy(), want[k], rtol=1e-6, atol=1e-7, err_msg=k)
        assert torch.equal(rec.z[:, 0], rec.pz_x[:, 0]) and not t["v_prev"].any()             # row 0: the window starts on the robot
        done = t["completed"].cpu().numpy()
        if done.any():                                             # a completed plan's reference is the plan, env.dt into each interval
            nodes = ref.chain(z0.numpy(), v.numpy(), ROM_DT)
            frac = np.float32(env.dt / ROM_DT)
            nxt = np.concatenate([nodes[:, 1:], nodes[:, -1:]], 1)
            np.testing.assert_allclose(t["z_ref"].cpu().numpy()[done], (nodes + (nxt - nodes) * frac)[done], rtol=0, atol=2e-5)
            assert torch.equal(rec.v[t["completed"]][:, :Np], v.to(DEV)[t["completed"]])
        s = pl.HipPlanScorer(None, p, device=DEV).score(z0, v, e=t["e_past"], v_prev=t["v_prev"], w0=t["w0"])
        res = pe.audit_env(s, t, p)
        assert json.loads(json.dumps(res, allow_nan=False)) == res
        assert res["plans"] == B and res["completed"] == int(done.sum()) and res["terminated"] == int(dead.sum()) and res["nodes"] == Np + 1
        print(f"fresh policy: {res['completed']} of {B} completed, {res['terminated']} terminated, coverage {res['coverage']}")
    finally:
        if runner is not None:
            runner.ppo.close()
        env.close()


def test_audit_script_on_the_robot_equals_the_library_calls(tmp_path):
    """audit_plans.py --robot on section 10.8's smallest trained tube: audit.json is track_env + score + audit_env."""
    import audit_plans
    import train_tube
    from legged_gym_dev_amd.tube.model import HipTubeModel
    run, out = str(tmp_path / "run"), str(tmp_path / "audit")
    train_tube.main(["--sim", "--sim_seed", "0", "--sim_refresh", "0", "--dataset", "scalar_horizon_level", "--H_fwd", "5", "--H_rev", "3",
                     "--out", run, "--num_epochs", "8", "--batch_size", "16", "--lr", "3e-3", "--seed", "3", "--steps_per_model_checkpoint", "10",
                     "--steps_per_model_evaluation", "10", "--device", DEV, "--sim_envs", "64", "--sim_T", "50"])
    # test_hip_plan_audit's 5-node problem: half a second of the gap problem's first stretch, 0.1 and 0.12 m/s, inside ANYmal's 0.35
    prob = pl.PlanProblem.named("gap", N=5, H_rev=3, goal=[0.35, 0.36], obs_c=[[0.36, 0.28], [0.28, 0.37]], obs_r=[0.02, 0.03])
    pj = str(tmp_path / "problem.json")
    json.dump(prob.to_json(), open(pj, "w"))
    argv = ["--run", run, "--checkpoint", "latest", "--problem_json", pj, "--warm_start", "interpolate", "--perturb", "32", "--sigma", "0.05",
            "--seed", "4", "--level", "0.9", "--device", DEV, "--robot"]
    res = audit_plans.main(argv + ["--out", out])
    saved = json.load(open(os.path.join(out, "audit.json")))
    assert saved == json.loads(json.dumps(res, allow_nan=False)) == res
    assert res["tracker"] == "robot" and res["plans"] == 33 and res["nodes"] == 6 and res["task"] == TRAJ and res["push_robots"] is False
    a = audit_plans.parse_args(argv)
    p = audit_plans.build_problem(a, audit_plans.run_config(run))
    z0, v, _ = audit_plans.build_plans(a, p)
    model = HipTubeModel.load(run, checkpoint="latest", device=DEV)
    try:
        s, lib, extra = audit_plans.main_robot(a, p, pl.HipPlanScorer(model, p, level=0.9, device=DEV), z0, v)
    finally:
        model.close()
    assert extra["tracker"] == "robot"
    for k, val in lib.items():
        assert res[k] == val, k


# ------------------------------------------------------------------------------------------------ 6. existing behaviour
def test_square_env_is_unchanged_on_the_bits():
    """One seed, 50 post-steps of a Square env against the restated Square law (test_eval_generators.square_v, here in float32 one
    rounding at a time): v, k, t and the window, bit for bit.  With +-4 m/s the first two corners (0.5 s, 0.75 s) fall inside."""
    vlim = 4.0
    env = _handle(gen=GENS["square"], vlim=vlim, seed=11)
    try:
        f32 = np.float32
        vmin, vmax = np.full(2, -vlim, f32), np.full(2, vlim, f32)
        g, win = env.get("tg_state"), env.get("tg_traj").copy()
        k, t = g[:, OK].copy(), g[:, OT].copy()
        dt, rom_dt = f32(env.setup.dt), f32(ROM_DT)
        seen = set()
        for s in range(50):
            _post_step(env)
            v = np.stack([square_v(t[i], vmin, vmax).astype(f32) for i in range(N_ENV)])
            for i in range(N_ENV):
                if t[i] >= f32(f32(k[i] * rom_dt) - f32(1e-5)):
                    head = (win[i, -1] + (rom_dt * v[i]).astype(f32)).astype(f32)
                    win[i, :-1] = win[i, 1:]
                    win[i, -1] = head
                    k[i] = f32(k[i] + f32(1))
                t[i] = f32(t[i] + dt)
            g = env.get("tg_state")
            np.testing.assert_array_equal(g[:, OV:OV + 2], v, err_msg=f"step {s}: v")
            np.testing.assert_array_equal(g[:, OK], k, err_msg=f"step {s}: k")
            np.testing.assert_array_equal(g[:, OT], t, err_msg=f"step {s}: t")
            np.testing.assert_array_equal(env.get("tg_traj"), win, err_msg=f"step {s}: window")
            seen |= {tuple(r) for r in v.tolist()}
        assert seen == {(0.0, 2.0), (4.0, 0.0), (0.0, -2.0)} and int(env.get("n_reset")[0]) == 0
    finally:
        env.close()
