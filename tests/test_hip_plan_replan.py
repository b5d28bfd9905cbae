"""Replanning on the legged env, on the GPU (lg_traj_replan, closed_loop_env): the replan law against the
float32 restatement (tests/plan_replan_ref.py) on the bits, replanning with the plan in force as a no-op under real physics, the
rewritten window against the scorer's nodes, resets, set_plans after a replan, the C entry's refusals, closed_loop_env against its
steps composed by hand, and the script.  33 envs: two full post-step tiles of 16 and a ragged one."""
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
from tests import plan_replan_ref as rr
from tests.test_eval_generators import GENS, TRAJ, _cfg, _setup

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
PLAN = "PlanTrajectoryGenerator"
OK, OT, OV = (capi.TG_FIELDS[k][0] for k in ("k", "t", "v"))
N_ENV, ROM_DT = 33, 0.1


def _handle(n=N_ENV, Nw=10, gen=PLAN, seed=3):
    cfg = _cfg(gen, n=n)
    cfg.trajectory_generator.N = Nw
    cfg.env.num_observations = 9 + 2 * Nw + 3 * 12
    cfg.domain_rand.randomize_rom_distance = False
    env = harness.HipHandle(_setup(cfg, seed=seed))
    env.set_step_counter(0)
    env.call("reset_all")
    env.sync()
    return env


def _post_step(env):
    """test_hip_plan_env._post_step: the post-step alone, contact forces zeroed, the episode young."""
    env.set("contact_forces", np.zeros(env.core.t["contact_forces"].shape, np.float32))
    env.set("episode_length", np.zeros(env.setup.num_envs, np.int64))
    env.call("post_physics_step")


def _set_plans(env, v):
    env._plans = torch.as_tensor(np.ascontiguousarray(v, np.float32)).to(DEV)
    env.call("traj_set_plans", C.c_void_p(env._plans.data_ptr()) if v.shape[1] else None, int(v.shape[1]))


def _traj_reset(env, z):
    env._z = torch.as_tensor(np.ascontiguousarray(z, np.float32)).to(DEV)
    env.call("traj_reset", C.c_void_p(env._z.data_ptr()))


def _replan(env, v, skip=None):
    env._rv = torch.as_tensor(np.ascontiguousarray(v, np.float32)).to(DEV)
    env._rs = None if skip is None else torch.as_tensor(np.ascontiguousarray(skip, np.uint8)).to(DEV)
    env.call("traj_replan", C.c_void_p(env._rv.data_ptr()), int(v.shape[1]), None if skip is None else C.c_void_p(env._rs.data_ptr()))


def _check(env, law, msg, traj=True):
    g = env.get("tg_state")
    np.testing.assert_array_equal(g[:, OV:OV + 2], law.v_in, err_msg=msg + ": the input in force")
    np.testing.assert_array_equal(g[:, OK], law.k, err_msg=msg + ": k")
    np.testing.assert_array_equal(g[:, OT], law.t, err_msg=msg + ": t")
    np.testing.assert_array_equal(env.get("tg_traj"), law.win, err_msg=msg + ": the window")
    if traj:
        np.testing.assert_array_equal(env.get("trajectory"), law.traj, err_msg=msg + ": the interpolated trajectory")


def _start(envs, plans, start, Nw):
    """set_plans + traj_reset on every handle; the restatement in the same state (its trajectory is the device's: traj_reset leaves it
    to the next step callback)."""
    for env in envs:
        _set_plans(env, plans)
        _traj_reset(env, start)
    law = rr.ReplanLaw(plans, Nw, ROM_DT, envs[0].setup.dt)
    law.reset(np.arange(N_ENV), start)
    law.traj[:] = envs[0].get("trajectory")
    return law


# ------------------------------------------------------------------------------------------------ 1. the law
@pytest.mark.parametrize("Nw", [1, 2, 10])
@pytest.mark.parametrize("n_nodes", [1, 5, 64])
def test_law_with_physics_out_of_the_way(Nw, n_nodes):
    """Replans right after traj_reset, on the env step of a ROM step and on the last env step of an interval, under one random skip
    mask: after every env step LG_TG_V, k, t, the window and the interpolated trajectory equal the restatement, and the skipped envs
    equal a second env that never saw the calls."""
    rng = np.random.default_rng(100 * Nw + n_nodes)
    a, b = _handle(Nw=Nw), _handle(Nw=Nw)
    try:
        S = round(ROM_DT / a.setup.dt)
        draw = lambda: rng.uniform(-0.35, 0.35, (N_ENV, n_nodes, 2)).astype(np.float32)
        skip = (rng.random(N_ENV) < 0.3).astype(np.uint8)
        assert 0 < skip.sum() < N_ENV
        start = rng.uniform(-20, 20, (N_ENV, 2)).astype(np.float32)
        law = _start((a, b), draw(), start, Nw)
        _check(a, law, "after reset(z)")

        def untouched(msg):
            for key in ("tg_state", "tg_traj", "trajectory"):
                np.testing.assert_array_equal(a.get(key)[skip != 0], b.get(key)[skip != 0], err_msg=f"{msg}: skipped envs, {key}")

        def replan(msg):
            u = draw()
            _replan(a, u, skip)
            law.replan(u, skip)
            _check(a, law, msg)
            untouched(msg)
        replan("replan right after reset(z)")
        s = 0
        for s_end, msg in ((S + 1, "replan on the env step of a ROM step"), (2 * S, "replan on the last env step of an interval"),
                           ((n_nodes + 4) * S, None)):
            while s < s_end:
                _post_step(a)
                _post_step(b)
                stepped = law.step()
                s += 1
                _check(a, law, f"step {s}")
                untouched(f"step {s}")
                assert stepped.all() == (s % S == 1) and stepped.any() == stepped.all()
            if msg:
                replan(msg)
        assert law.k[0] == n_nodes + 4 and int(a.get("n_reset")[0]) == 0
        g = a.get("tg_state")
        assert not g[skip == 0][:, OV:OV + 2].any()                                # past the plan: input 0
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 3. the scored plan
@pytest.mark.parametrize("N,Nw", [(8, 2), (64, 10), (8, 10)])
def test_the_rewritten_window_is_the_scored_plan(N, Nw):
    """After replan(u), window points 1.. are HipPlanScorer.score(z0 = point 1, u)['z'][:, :Nw] and the later heads z[:, Nw:], on the
    bits.  (8, 10): a plan shorter than the window -- the points past its last node stay on it."""
    p = pl.PlanProblem.named("gap", tube_kind="l2", N=N)
    assert p.dt == ROM_DT
    rng = np.random.default_rng(N + Nw)
    env = _handle(Nw=Nw)
    try:
        _start((env,), rng.uniform(-0.3, 0.3, (N_ENV, 12, 2)).astype(np.float32), rng.uniform(-2, 2, (N_ENV, 2)).astype(np.float32), Nw)
        for _ in range(7):                                                        # mid-interval, two ROM steps into the old plan
            _post_step(env)
        u = torch.as_tensor(rng.uniform(-0.2, 0.2, (N_ENV, N, 2)).astype(np.float32))
        z0 = env.core.t["tg_traj"][:, 1].clone()
        z = pl.HipPlanScorer(None, p, device=DEV).score(z0, u, want=("z",))["z"]
        _replan(env, u.numpy())
        env.sync()
        win = env.core.t["tg_traj"][:, 1:]
        m = min(Nw, N + 1)
        assert torch.equal(win[:, :m], z[:, :m]) and torch.equal(win[:, m:], z[:, -1:].expand(-1, Nw - m, -1))
        heads, k = [], env.get("tg_state")[:, OK].copy()
        for s in range((N + 1 - m) * 5 + 5):
            _post_step(env)
            kn = env.get("tg_state")[:, OK]
            if kn[0] != k[0] and len(heads) < N + 1 - m:
                heads.append(env.core.t["tg_traj"][:, -1].clone())
            k = kn.copy()
        assert len(heads) == N + 1 - m
        if heads:
            assert torch.equal(torch.stack(heads, 1), z[:, Nw:] if Nw <= N else z[:, -1:].expand(-1, len(heads), -1))
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ 4. resets, 5. set_plans
def test_reset_ids_mid_loop_and_set_plans_after_a_replan():
    """lg_reset_ids after a replan: the reset env's base is 0 -- it replays the plan in its buffer from node 0 at its new position --,
    every other env is bit-identical to a run without the reset.  Then set_plans: counter indexing again, on the bits."""
    rng = np.random.default_rng(5)
    Nw = 10
    plans = rng.uniform(-0.35, 0.35, (N_ENV, 12, 2)).astype(np.float32)
    start = rng.uniform(-5, 5, (N_ENV, 2)).astype(np.float32)
    a, b = _handle(seed=9), _handle(seed=9)
    try:
        law = _start((a, b), plans, start, Nw)
        u = rng.uniform(-0.35, 0.35, (N_ENV, 30, 2)).astype(np.float32)
        for s in range(17):                                                        # k = 4, between two ROM steps
            for env in (a, b):
                _post_step(env)
                if s == 7:
                    _replan(env, u)
            law.step()
            if s == 7:
                law.replan(u)
        _check(a, law, "before the reset")
        assert law.k[0] == 4 and law.k0[0] == 2 - (Nw - 1)
        who = 20
        ids = torch.tensor([who], dtype=torch.int32, device=DEV)
        a.call("reset_ids", C.c_void_p(ids.data_ptr()), 1)
        a.sync()
        xy = a.get("root_states")[who, :2]
        law.reset([who], xy[None])
        law.traj[who] = a.get("trajectory")[who]
        _check(a, law, "after reset_ids")
        others = np.arange(N_ENV) != who
        for s in range(12):
            for env in (a, b):
                _post_step(env)
            law.step()
            _check(a, law, f"after the reset, step {s}")
            for key in ("tg_state", "tg_traj", "trajectory"):
                np.testing.assert_array_equal(a.get(key)[others], b.get(key)[others], err_msg=key)
        assert law.k[who] == 3 and law.k[0] == 6 and law.k0[who] == 0
        np.testing.assert_array_equal(a.get("tg_traj")[who, -1], ref.chain(xy[None], u[who:who + 1], ROM_DT)[0, 3])   # the buffer's plan from node 0
        # set_plans after a replan: base 0 for everyone, the counter indexes the plan
        again = rng.uniform(-0.35, 0.35, (N_ENV, 12, 2)).astype(np.float32)
        _set_plans(a, again)
        law.set_plans(again)
        heads = a.get("tg_traj")[:, -1].copy()
        for s in range(6):
            _post_step(a)
            law.step()
            _check(a, law, f"after set_plans, step {s}")
        assert law.k[0] == 7 and not law.k0.any()
        want = (heads[0] + (np.float32(ROM_DT) * again[0, 6]).astype(np.float32)).astype(np.float32)
        np.testing.assert_array_equal(a.get("tg_traj")[0, -1], want)              # the ROM step 6 -> 7 took node 6
    finally:
        a.close()
        b.close()


# ------------------------------------------------------------------------------------------------ 6. the C entry's refusals
def test_replan_refusals():
    from legged_gym_dev_amd.lib import LeggedHipError
    env = _handle(n=4)
    sq = _handle(n=4, gen=GENS["square"])
    z, meta = harness.load_fixture("anymal_c_flat")
    vel = harness.HipHandle(harness.make_setup("anymal_c_flat", z, meta)[0])
    v = torch.zeros(4, 3, 2, device=DEV)
    vp = C.c_void_p(v.data_ptr())
    try:
        for h, args, word in ((env, (vp, 65, None), "lg_traj_replan: n_nodes = 65 must lie in 1..64"), (env, (vp, 0, None), "n_nodes = 0 must lie in 1..64"),
                              (env, (vp, -1, None), "n_nodes = -1"), (env, (None, 3, None), "lg_traj_replan: v is null"),
                              (sq, (vp, 3, None), "lg_traj_replan: the generator is not PlanTrajectoryGenerator"),
                              (vel, (vp, 3, None), "lg_traj_replan: not a trajectory env")):
            with pytest.raises(LeggedHipError, match=word):
                h.call("traj_replan", *args)
        before = env.get("tg_traj").copy()
        env.call("traj_replan", vp, 3, None)                                       # zero inputs from point 1 of a constant window: nothing moves
        np.testing.assert_array_equal(env.get("tg_traj"), before)
    finally:
        for h in (env, sq, vel):
            h.close()


# ------------------------------------------------------------------------------------------------ product env helpers
def _product_env(n, Nw=None):
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.utils import get_args
    env_cfg, train_cfg = pe.plan_env_cfg(TRAJ, n)
    if Nw is not None:
        env_cfg.trajectory_generator.N = Nw
        env_cfg.env.num_observations = 9 + 2 * Nw + 3 * 12
    args = get_args(["--task", TRAJ, "--num_envs", str(n), "--headless"])
    args.sim_device = args.rl_device = DEV
    env, _ = task_registry.make_env(name=TRAJ, args=args, env_cfg=env_cfg)
    return env, train_cfg, args


class _Pair:
    """Two product envs from one seed and one freshly initialised policy (the first env's runner; the policy is a function of the
    observation alone)."""

    def __init__(self, n, Nw=None):
        from legged_gym_dev_amd.envs import task_registry
        self.a = self.b = self.runner = None
        try:
            self.a, train_cfg, args = _product_env(n, Nw)
            train_cfg.runner.resume = False
            self.runner, _ = task_registry.make_alg_runner(env=self.a, name=TRAJ, args=args, train_cfg=train_cfg, log_root=None)
            self.policy = self.runner.get_inference_policy(device=self.a.device)
            self.b = _product_env(n, Nw)[0]
            self.b.reset()                                           # the runner reset its env once when it was made: the same draws
        except Exception:
            self.close()
            raise

    def close(self):
        if self.runner is not None:
            self.runner.ppo.close()
        for env in (self.a, self.b):
            if env is not None:
                env.close()


def _begin(env, v, rows):
    env.reset()
    env.traj_gen.set_plans(v)
    start = env.rom.proj_z(env.root_states).clone()
    env.traj_gen.reset(start)
    env.trajectory.copy_(start[:, None, :].expand_as(env.trajectory))
    rec = pe.TrajRecorder(env, rows)
    rec.begin()
    return start, rec


# ------------------------------------------------------------------------------------------------ 2. a replan with the plan in force
def test_replanning_with_the_plan_in_force_changes_nothing():
    """Real physics under a freshly initialised policy, twice from one seed: open loop on plans v, and with replan(v[:, j0:]) at every
    ROM interval, j0 = k - (Nw - 1) the base the law prescribes (nodes before 0 are the pre-roll's zero inputs).  Every recorder buffer
    is torch.equal; tg_traj, tg_state and root_states are torch.equal for every robot that did not reset -- a robot that falls replays
    the plan in its buffer from node 0, and the second run's buffer holds the tail last handed in, so such a robot is skipped from its
    reset on and compared through the recorder, which stops at the reset."""
    B, Nw, Np, R = N_ENV, 10, 12, 9
    pair = _Pair(B)
    try:
        g = torch.Generator().manual_seed(2)
        v = (torch.rand(B, Np, 2, generator=g) * 0.4 - 0.2).to(DEV)
        v_ext = torch.cat([torch.zeros(B, Nw - 1, 2, device=DEV), v], dim=1)
        sched = pe.rom_schedule(pair.a, R - 1)
        out = []
        with torch.no_grad():
            for env, closed in ((pair.a, False), (pair.b, True)):
                start, rec = _begin(env, v, R)
                obs = env.get_observations()
                for k, steps in enumerate(sched):                                  # k ROM steps have been taken: LG_TG_K = k
                    if closed:
                        env.traj_gen.replan(v_ext[:, k:k + capi.PLAN_MAX_N], skip=rec.dead)
                    for _ in range(steps):
                        obs = env.step(pair.policy(obs.detach()).detach())[0]
                        rec.step()
                torch.cuda.synchronize()
                out.append((start, rec, env.traj_gen.trajectory.clone(), env.core.t["tg_state"].clone(), env.root_states.clone()))
        (sa, ra, wa, ga, xa), (sb, rb, wb, gb, xb) = out
        assert torch.equal(sa, sb)
        for key in ("z", "pz_x", "v", "rows", "dead", "k_mark"):
            assert torch.equal(getattr(ra, key), getattr(rb, key)), key
        live = ra.dead == 0
        print(f"replan with the plan in force: {int(live.sum())} of {B} robots did not reset")
        assert bool(live.any()) and bool((ra.rows[live] == R).all())
        assert torch.equal(wa[live], wb[live]) and torch.equal(ga[live], gb[live]) and torch.equal(xa[live], xb[live])
        assert torch.equal(ra.v[live], v[live][:, :R - 1])                         # the inputs recorded are the plan's
    finally:
        pair.close()


# ------------------------------------------------------------------------------------------------ 7. closed_loop_env by hand
def _by_hand(env, policy, planner, H, iters_first, w0):
    """closed_loop_env's steps from the public pieces, as section 10.15 lists them."""
    p, B = planner.problem, env.num_envs
    sched = pe.rom_schedule(env, H + 1)
    norm = lambda d: torch.linalg.vector_norm(d, dim=-1)
    with torch.no_grad():
        s_world, rec = _begin(env, torch.zeros(B, 0, 2, device=DEV), H + 2)
        s_plan = torch.tensor(p.start, dtype=torch.float32, device=DEV).repeat(B, 1)
        frame = lambda t: ((t.double() - (s_world.double() if t.dim() == 2 else s_world.double()[:, None])) +
                           (s_plan.double() if t.dim() == 2 else s_plan.double()[:, None])).float()
        e, v_prev = torch.zeros(B, p.H_rev, device=DEV), torch.zeros(B, p.H_rev, 2, device=DEV)
        err = norm(rec.z[:, 0] - rec.pz_x[:, 0])
        nodes, vs, ws, sols = [], [], [torch.zeros(B, device=DEV) if w0 == "zero" else err], []
        obs, warm = env.get_observations(), None
        for j in range(H + 1):
            nodes.append(frame(env.traj_gen.trajectory[:, 1]))
            if j < H:
                sol = planner.plan(nodes[-1], warm, e, v_prev, None if w0 == "zero" else err, iters=iters_first if j == 0 else None)
                env.traj_gen.replan(sol["v"], skip=rec.dead)
                sols.append(sol), vs.append(sol["v"][:, 0]), ws.append(sol["score"]["w"][:, 1])
                warm = pl.shift_plan(sol["v"])
            for _ in range(sched[j]):
                obs = env.step(policy(obs.detach()).detach())[0]
                rec.step()
            if j < H:
                err = norm(rec.z[:, j + 1] - rec.pz_x[:, j + 1])
                e, v_prev = pl.shift_past(e, v_prev, err, sol["v"][:, 0])
        torch.cuda.synchronize()
    stack = lambda f: torch.stack([f(s) for s in sols], 1)
    return {"z": frame(rec.z[:, 1:]), "z_node": torch.stack(nodes, 1), "v": torch.stack(vs, 1), "w": torch.stack(ws, 1), "pz_x": frame(rec.pz_x[:, 1:]),
            "cost": stack(lambda s: s["score"]["cost"]), "min_clear": stack(lambda s: s["score"]["min_clear"]), "best_J": stack(lambda s: s["best_J"]),
            "n_bad": stack(lambda s: s["n_bad"]), "completed": (rec.rows == H + 2) & (rec.dead == 0), "rows": rec.rows, "dead": rec.dead != 0,
            "plans_v": torch.stack([s["v"] for s in sols], 0), "plans_z": torch.stack([s["score"]["z"] for s in sols], 0),
            "plans_w": torch.stack([s["score"]["w"] for s in sols], 0)}, sched


@pytest.mark.parametrize("Nw", [2, 10])
@pytest.mark.parametrize("kind", ["l1", "nn"])
def test_closed_loop_env_equals_its_steps_composed_by_hand(kind, Nw):
    """H = 6 on the gap problem with MPPI at K = 32, on two envs from one seed under one fresh policy: every returned tensor is
    torch.equal, rows match the host schedule.  Nothing is asserted about coverage: an untrained policy falls."""
    from tests.test_hip_mppi import _trainer
    H, B, N, Hr = 6, N_ENV, 10, 3 if kind == "nn" else 0
    tr = _trainer(Hr, N, 16, 1, "relu") if kind == "nn" else None
    pair = None
    try:
        pair = _Pair(B, Nw)
        p = pl.PlanProblem.named("gap", tube_kind=kind, N=N, H_rev=Hr)
        pln = pl.HipMppiPlanner(tr, p, pl.MppiCfg(K=32, iters=3, sigma=0.3, lambda_=1.0, rho_g=1e4, seed=1), device=DEV)
        w0 = "error" if kind == "nn" else "zero"
        got = pe.closed_loop_env(pair.a, pair.policy, pln, H, iters_first=5, keep_plans=True, w0=w0)
        want, sched = _by_hand(pair.b, pair.policy, pln, H, 5, w0)
        torch.cuda.synchronize()
        assert set(got) == set(want)
        for k in want:
            assert got[k].shape == want[k].shape and got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
        S = pe.rom_substeps(pair.a)
        print(f"{kind}, Nw = {Nw}: schedule {sched}, {sum(x > S for x in sched[1:])} late ROM step(s); "
              f"{int(got['completed'].sum())} of {B} completed, {int(got['dead'].sum())} reset")
        live = ~got["dead"]
        assert bool((got["rows"][live] == H + 2).all()) and torch.equal(got["completed"], live)
        for k, shape in (("z", (B, H + 1, 2)), ("z_node", (B, H + 1, 2)), ("v", (B, H, 2)), ("w", (B, H + 1)), ("pz_x", (B, H + 1, 2)),
                         ("cost", (B, H)), ("min_clear", (B, H)), ("best_J", (B, H)), ("n_bad", (B, H)), ("plans_v", (H, B, N, 2))):
            assert tuple(got[k].shape) == shape, k
        # every plan starts at the node the robot was heading for, which the previous plan put there
        assert torch.equal(got["plans_z"][:, :, 0], got["z_node"][:, :H].transpose(0, 1))
        done = got["completed"]
        if bool(done.any()):
            d = (got["plans_z"][:-1, :, 1] - got["plans_z"][1:, :, 0]).abs().transpose(0, 1)[done]
            assert float(d.max()) <= 4 * float(np.spacing(np.float32(64.0))), float(d.max())   # one world-frame rounding at the env origins' size
        res = pe.audit_closed_loop_env(got, p)
        assert json.loads(json.dumps(res, allow_nan=False)) == res and res["robots"] == B
    finally:
        if pair is not None:
            pair.close()
        if tr:
            tr.close()


# ------------------------------------------------------------------------------------------------ 8. the script
def test_script_on_the_robot_equals_the_library_calls(tmp_path):
    """plan_tube.py --closed_loop 5 --robot on the policy route of test_audit_script_on_the_robot_equals_the_library_calls (no
    checkpoint: a freshly initialised policy from the task's seed): plan.json is main_robot's audit and the library calls'."""
    import plan_tube
    out = str(tmp_path / "plan")
    argv = ["--tube", "l1", "--problem", "gap", "--N", "10", "--K", "32", "--iters", "3", "--sigma", "0.05", "--seed", "4", "--starts", str(N_ENV),
            "--start_noise", "0.01", "--closed_loop", "5", "--robot", "--device", DEV]
    res = plan_tube.main(argv + ["--out", out])
    saved = json.load(open(os.path.join(out, "plan.json")))
    assert saved == json.loads(json.dumps(res, allow_nan=False))
    assert res["tracker"] == "robot" and res["task"] == TRAJ and res["push_robots"] is False and res["closed_loop"] == 5
    assert res["audit"]["robots"] == N_ENV and res["audit"]["steps"] == 5
    assert {"completed", "terminated", "covered_robots_of_all"} <= set(res["audit"])
    npz = np.load(os.path.join(out, "plans.npz"))
    assert npz["z0"].shape == (5 * N_ENV, 2) and npz["v"].shape == (5 * N_ENV, 10, 2)
    a = plan_tube.parse_args(argv)
    p = plan_tube.build_problem(a, None)
    z0 = plan_tube.starts(a, p)
    planner = plan_tube.make_planner(a, None, p, None)
    lib_res, audit, extra = plan_tube.main_robot(a, planner, z0)
    assert extra["tracker"] == "robot" and audit == res["audit"]
    np.testing.assert_array_equal(lib_res["plans_v"].reshape(-1, 10, 2).cpu().numpy(), npz["v"])
    assert audit == pe.audit_closed_loop_env(lib_res, p, goal_tol=a.goal_tol)
