"""Replanning on the legged env, the part that needs no GPU: the clock schedule and the replan law by hand
(tests/plan_replan_ref.py), closed_loop_env on a stub env, recorder and planner in CPU torch -- call order, origins, shifts, alignment,
the RuntimeError --, every refusal, audit_closed_loop_env on hand-made records, the script's flags, the C entry in capi."""
import ctypes as C
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.tube import plan as pl
from legged_gym_dev_amd.tube import plan_env as pe
from tests import plan_env_ref as ref
from tests import plan_replan_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
f32 = np.float32


# ------------------------------------------------------------------------------------------------ the schedule
def test_schedule_by_hand():
    """Binary-exact clocks first: the ROM step falls on the first env step after a reset, then on every S-th.  Then a pair whose
    float32 sums drift: rom_dt = 2.1, dt = 0.3 (S = 7) -- ROM step 12 comes one env step late (8) and step 36 one early (6), the
    case test_plan_env_host.py's recorder script builds by hand.  Library, restatement and a direct float32 loop agree."""
    assert pe.clock_schedule(2, 0.5, 0.25, 5) == [1, 2, 2, 2, 2] == rr.clock_schedule(2, 0.5, 0.25, 5)
    assert pe.clock_schedule(1, 0.5, 0.5, 4) == [1, 1, 1, 1]
    assert pe.clock_schedule(10, 0.1, 0.02, 30) == [1] + [5] * 29               # the product env over any horizon of these tests
    got = pe.clock_schedule(1, 2.1, 0.3, 40)
    assert got == rr.clock_schedule(1, 2.1, 0.3, 40)
    assert got[0] == 1 and got[12] == 8 and got[36] == 6 and all(x == 7 for i, x in enumerate(got) if i not in (0, 12, 36))
    t, k, steps, late = f32(f32(-1) * f32(2.1)) + f32(2.1), f32(0), 0, []       # the loop itself, by hand
    t = f32(t)
    for s in range(sum(got)):
        steps += 1
        if t >= f32(f32(k * f32(2.1)) - f32(1e-5)):
            late.append(steps)
            k, steps = f32(k + f32(1)), 0
        t = f32(t + f32(0.3))
    assert late == got
    env = types.SimpleNamespace(setup=types.SimpleNamespace(traj={"N": 1, "dN": 1, "rom_dt": 2.1}, dt=0.3))
    assert pe.rom_schedule(env, 40) == got
    with pytest.raises(ValueError, match="does not reach"):
        pe.clock_schedule(1, 0.5, 0.0, 3)


# ------------------------------------------------------------------------------------------------ the law by hand
def _law(Nw, plans):
    law = rr.ReplanLaw(f32(plans), Nw=Nw, rom_dt=0.5, dt=0.5)                     # one env step per ROM step, exact in binary
    law.reset(np.arange(law.n), [[0, 0]] * law.n)
    return law


def test_law_by_hand_Nw_1():
    """Nw = 1: the window is points 0 and 1, both kept; only the base moves, so the next head advance takes the new plan's node 0."""
    law = _law(1, [[[1, 0], [1, 0], [1, 0]]])
    law.step()
    assert law.win[0].tolist() == [[0, 0], [0.5, 0]] and law.k[0] == 1 and law.v_in[0].tolist() == [1, 0]
    law.replan(f32([[[0, 2], [0, 4]]]))
    assert law.win[0].tolist() == [[0, 0], [0.5, 0]] and law.k0[0] == 1 and law.v_in[0].tolist() == [1, 0] and law.k[0] == 1     # LG_TG_V unchanged
    law.step()
    assert law.win[0].tolist() == [[0.5, 0], [0.5, 1]] and law.v_in[0].tolist() == [0, 2]
    law.step()
    assert law.win[0].tolist() == [[0.5, 1], [0.5, 3]]
    law.step()                                                                   # past the plan: input 0
    assert law.win[0].tolist() == [[0.5, 3], [0.5, 3]] and law.v_in[0].tolist() == [0, 0]


def test_law_by_hand_Nw_2_with_skip_and_reset():
    law = _law(2, [[[1, 0]] * 4, [[1, 0]] * 4])
    law.step()
    law.step()
    assert law.win[0].tolist() == [[0, 0], [0.5, 0], [1, 0]] and law.k.tolist() == [2, 2]
    law.replan(f32([[[0, 2], [0, 4], [0, 8]]] * 2), skip=[0, 1])
    # env 0: points 0, 1 kept; point 2 = point 1 + 0.5 * (0, 2); LG_TG_V = node Nw - 2 = 0; base = k - (Nw - 1) = 1.  env 1: untouched
    assert law.win[0].tolist() == [[0, 0], [0.5, 0], [0.5, 1]] and law.v_in[0].tolist() == [0, 2] and law.k0.tolist() == [1, 0]
    assert law.win[1].tolist() == [[0, 0], [0.5, 0], [1, 0]] and law.v_in[1].tolist() == [1, 0] and law.plans[1, :3].tolist() == [[1, 0]] * 3
    assert law.traj[0].tolist() == [[0.5, 0], [0.5, 1]]                          # re-interpolated at t = 1, k = 2: frac = rom_dt, points 1 and 2
    law.step()                                                                   # the head takes node Nw - 1 = 1; env 1 its old node k = 2
    assert law.win[0].tolist() == [[0.5, 0], [0.5, 1], [0.5, 3]] and law.win[1, -1].tolist() == [1.5, 0]
    law.step()
    assert law.win[0, -1].tolist() == [0.5, 7] and law.win[1, -1].tolist() == [1.5, 0]      # env 1: k = 3 = the new node count: 0
    law.step()
    assert law.win[0, -1].tolist() == [0.5, 7] and law.v_in[0].tolist() == [0, 0]           # j = 3: past the plan
    law.reset([0], [[10, 10]])                                                   # base 0: the buffer's plan replays from node 0
    law.step()
    assert law.k0.tolist() == [0, 0] and law.win[0, -1].tolist() == [10, 11] and law.k[0] == 1
    law.replan(f32([[[1, 1]]] * 2))                                              # a plan shorter than the window's tail is padded with 0
    law.set_plans(f32([[[2, 2], [4, 4]]] * 2))                                   # set_plans puts the base back: counter indexing
    assert law.k0.tolist() == [0, 0]
    law.step()
    assert law.win[0, -1].tolist() == [12.5, 12.5]                               # k = 1: node 1 of the set plan, on the replanned point (10.5, 10.5)


def test_law_by_hand_Nw_3_and_a_short_plan():
    law = _law(3, [[[1, 0]] * 6])
    for _ in range(3):
        law.step()
    assert law.win[0].tolist() == [[0, 0], [0.5, 0], [1, 0], [1.5, 0]] and law.k[0] == 3
    law.replan(f32([[[0, 2], [0, 4], [2, 0], [4, 0]]]))
    assert law.win[0].tolist() == [[0, 0], [0.5, 0], [0.5, 1], [0.5, 3]] and law.v_in[0].tolist() == [0, 4] and law.k0[0] == 1
    law.step()
    assert law.win[0, -1].tolist() == [1.5, 3] and law.v_in[0].tolist() == [2, 0]           # node Nw - 1 = 2
    law.replan(f32([[[8, 0]]]))                                                  # one node for two rewritten points: the second gets input 0
    assert law.win[0].tolist() == [[0.5, 0], [0.5, 1], [4.5, 1], [4.5, 1]] and law.v_in[0].tolist() == [0, 0] and law.k0[0] == 2
    law.step()
    assert law.win[0, -1].tolist() == [4.5, 1]                                   # node 2 of a one-node plan: 0
    np.testing.assert_array_equal(law.win[0, 0:2], ref.chain(f32([[0.5, 1]]), f32([[[8, 0]]]), 0.5)[0])


# ------------------------------------------------------------------------------------------------ closed_loop_env on stubs
class _StubEnv:
    """B robots that close half the gap to trajectory[:, 0] every env step, on rr.ReplanLaw.  world: the robots' spawn points.
    env_dt: the clock the "device" really runs; setup.dt is what rom_schedule is told."""

    def __init__(self, log, B=3, Nw=2, rom_dt=0.5, dt=0.25, env_dt=None, falls=None, max_len=1000, kind=4, vlim=1.0):
        self.log, self.num_envs, self.device, self.num_actions, self.dt, self.max_episode_length = log, B, "cpu", 1, dt, max_len
        self.setup = types.SimpleNamespace(traj={"kind": kind, "N": Nw, "dN": 1, "rom_dt": rom_dt}, dt=dt)
        self.rom = types.SimpleNamespace(v_min=torch.tensor([-vlim, -vlim]), v_max=torch.tensor([vlim, vlim]), proj_z=lambda x: x[..., :2], dt=rom_dt)
        self.law = rr.ReplanLaw(np.zeros((B, 0, 2), f32), Nw, rom_dt, dt if env_dt is None else env_dt)
        self.world = torch.tensor([[8.0, 16.0], [-4.0, 2.0], [32.0, -8.0]])[:B]
        self.root_states = torch.zeros(B, 13)
        self.trajectory = torch.from_numpy(self.law.traj)
        self.reset_buf = np.zeros(B, bool)
        self.falls, self.steps = falls or {}, 0
        env = self

        class TG:
            @property
            def trajectory(self):
                return torch.from_numpy(env.law.win)

            def set_plans(self, v):
                log.append(("set_plans", tuple(v.shape)))
                env.law.set_plans(v.numpy())

            def reset(self, z):
                log.append(("traj_reset",))
                env.law.reset(np.arange(B), z.numpy())

            def replan(self, v, skip=None):
                log.append(("replan", v.clone(), skip.clone()))
                env.law.replan(v.numpy(), skip.numpy())
        self.traj_gen = TG()

    def reset(self):
        self.log.append(("reset",))
        self.root_states[:, :2] = self.world

    def get_observations(self):
        return self.root_states[:, :2].clone()

    def step(self, actions):
        self.log.append(("step",))
        self.steps += 1
        self.law.step()
        self.root_states[:, :2] += 0.5 * (self.trajectory[:, 0] - self.root_states[:, :2])
        self.reset_buf[:] = [self.falls.get(i) == self.steps for i in range(self.num_envs)]
        return (self.get_observations(),)


def _stub_recorder(log):
    class Rec:
        def __init__(self, env, rows_max, want_x=False):
            self.env, self.rows_max, self.r = env, rows_max, ref.Recorder(env.num_envs, rows_max)
            for k in ("z", "pz_x", "v", "rows", "dead", "k_mark"):
                setattr(self, k, torch.from_numpy(getattr(self.r, k)))
            log.append(("rec", rows_max))

        def begin(self):
            log.append(("rec_begin",))
            e = self.env
            self.r.begin(e.trajectory[:, 0].numpy(), e.root_states[:, :2].numpy(), e.law.k.copy())

        def step(self):
            log.append(("rec_step",))
            e = self.env
            self.r.step(e.reset_buf, e.trajectory[:, 0].numpy(), e.root_states[:, :2].numpy(), e.law.k.copy(), e.law.v_in.copy())
    return Rec


class _StubPlanner:
    """Plan c (the c-th call) holds input (0.25 (c + 1), 0.5 b) at every node for robot b; z is the chain, w[:, n] = c + n / 8."""

    def __init__(self, log, problem, B=3):
        self.log, self.problem, self.B, self.calls = log, problem, B, 0

    def plan(self, z0, v_init=None, e=None, v_prev=None, w0=None, iters=None):
        p, c = self.problem, self.calls
        self.log.append(("plan", z0.clone(), None if v_init is None else v_init.clone(), e.clone(), v_prev.clone(), None if w0 is None else w0.clone(), iters))
        self.calls += 1
        v = torch.zeros(self.B, p.N, 2)
        v[:, :, 0], v[:, :, 1] = 0.25 * (c + 1), 0.5 * torch.arange(self.B)[:, None]
        z = torch.from_numpy(ref.chain(z0.numpy(), v.numpy(), p.dt))
        w = c + torch.arange(p.N + 1) / 8.0 + torch.zeros(self.B, 1)
        return {"v": v, "best_J": torch.full((self.B,), float(c)), "n_bad": torch.full((self.B,), c, dtype=torch.int32),
                "score": {"z": z, "w": w, "cost": torch.full((self.B,), 10.0 + c), "min_clear": torch.full((self.B,), 1.0 - c)}}


def _run(monkeypatch, H=4, Nw=2, w0="zero", falls=None, env_dt=None, keep_plans=True, H_rev=2, N=4, start=None):
    log = []
    monkeypatch.setattr(pe, "TrajRecorder", _stub_recorder(log))
    env = _StubEnv(log, Nw=Nw, falls=falls, env_dt=env_dt)
    p = pl.PlanProblem(N=N, dt=0.5, H_rev=H_rev, start=[1.0, 2.0], rom_v_min=[-1.0, -1.0], rom_v_max=[1.0, 1.0])
    planner = _StubPlanner(log, p)
    out = pe.closed_loop_env(env, lambda obs: obs[:, :1], planner, H, start=start, iters_first=7, keep_plans=keep_plans, w0=w0)
    return env, p, log, out


@pytest.mark.parametrize("Nw", [1, 2, 3])
def test_closed_loop_env_on_a_stub(monkeypatch, Nw):
    H, B = 4, 3
    env, p, log, out = _run(monkeypatch, H=H, Nw=Nw)
    sched = pe.rom_schedule(env, H + 1)
    assert sched == [1, 2, 2, 2, 2]
    # the call order
    names = [ev[0] for ev in log]
    want = ["rec", "reset", "set_plans", "traj_reset", "rec_begin"]
    for j in range(H):
        want += ["plan", "replan"] + ["step", "rec_step"] * sched[j]
    want += ["step", "rec_step"] * sched[H]
    assert names == want and log[0] == ("rec", H + 2) and log[2] == ("set_plans", (B, 0, 2))
    plans = [ev for ev in log if ev[0] == "plan"]
    replans = [ev for ev in log if ev[0] == "replan"]
    assert [ev[6] for ev in plans] == [7, None, None, None]                      # iters_first, then the planner's own
    assert plans[0][2] is None                                                   # ... and its own warm start
    start = torch.tensor([[1.0, 2.0]] * B)
    # the origins: plan j starts at the window point the robot is heading for, which is node 1 of plan j - 1; all exact in binary
    node = start
    for j in range(H):
        assert torch.equal(plans[j][1], node) and torch.equal(out["z_node"][:, j], node), j
        v_j = replans[j][1]
        assert torch.equal(out["v"][:, j], v_j[:, 0]) and not replans[j][2].any()
        if j:
            assert torch.equal(plans[j][2], pl.shift_plan(replans[j - 1][1]))     # the warm start: the previous plan shifted
        node = node + 0.5 * v_j[:, 0]
    assert torch.equal(out["z_node"][:, H], node)
    # the alignment: recorder row k + 1 is env.dt into the interval past node k (dt / rom_dt = 1 / 2)
    nodes = out["z_node"]
    assert torch.equal(out["z"][:, :H], nodes[:, :H] + 0.5 * (nodes[:, 1:] - nodes[:, :H]))
    # the tube item's past: e takes |z - pz_x| of row j + 1 in world coordinates, v_prev the committed input
    rec_err = torch.linalg.vector_norm(out["z"] - out["pz_x"], dim=-1)           # the frame is a translation by binary-exact numbers
    e, vp = torch.zeros(B, 2), torch.zeros(B, 2, 2)
    for j in range(H):
        assert torch.equal(plans[j][3], e) and torch.equal(plans[j][4], vp) and plans[j][5] is None, j
        e, vp = pl.shift_past(e, vp, rec_err[:, j], out["v"][:, j])
    assert bool((rec_err[:, 1:] > 0).all())                                      # the stub robot lags: the errors are not trivially 0
    assert torch.equal(out["w"], torch.tensor([[0.0, 0.125, 1.125, 2.125, 3.125]] * B))
    assert torch.equal(out["cost"], torch.tensor([[10.0, 11.0, 12.0, 13.0]] * B)) and torch.equal(out["best_J"], torch.tensor([[0.0, 1.0, 2.0, 3.0]] * B))
    assert torch.equal(out["min_clear"], torch.tensor([[1.0, 0.0, -1.0, -2.0]] * B)) and out["n_bad"].tolist() == [[0, 1, 2, 3]] * B
    assert out["completed"].tolist() == [True] * B and out["rows"].tolist() == [H + 2] * B and out["dead"].tolist() == [False] * B
    for k, shape in (("z", (B, H + 1, 2)), ("z_node", (B, H + 1, 2)), ("v", (B, H, 2)), ("w", (B, H + 1)), ("pz_x", (B, H + 1, 2)),
                     ("plans_v", (H, B, 4, 2)), ("plans_z", (H, B, 5, 2)), ("plans_w", (H, B, 5))):
        assert tuple(out[k].shape) == shape, k
    assert torch.equal(out["plans_z"][:, :, 0], out["z_node"][:, :H].transpose(0, 1))
    # the window the robot saw is the plan in force: after the last replan, points 1.. are that plan's nodes (in the world frame)
    res = pe.audit_closed_loop_env(out, p)
    assert res["robots"] == B and res["completed"] == B and res["steps"] == H and json.loads(json.dumps(res, allow_nan=False)) == res


def test_closed_loop_env_w0_error_start_and_a_fallen_robot(monkeypatch):
    """w0 = 'error': every plan's tube starts at the row's error (0 at the start).  Robot 1 resets on env step 3: it is skipped by every
    later replan, is not completed, and does not trip the row check.  start (B, 2): each robot its own plan frame."""
    H, B = 4, 3
    start = torch.tensor([[1.0, 2.0], [0.0, 0.0], [-2.0, 4.0]])
    env, p, log, out = _run(monkeypatch, H=H, w0="error", falls={1: 3}, keep_plans=False, start=start)
    plans = [ev for ev in log if ev[0] == "plan"]
    replans = [ev for ev in log if ev[0] == "replan"]
    assert torch.equal(plans[0][1], start) and torch.equal(out["z_node"][:, 0], start)
    err = torch.linalg.vector_norm(out["z"] - out["pz_x"], dim=-1)
    assert not plans[0][5].any() and all(torch.equal(plans[j][5], err[:, j - 1]) for j in range(1, H))
    assert torch.equal(out["w"][:, 0], torch.zeros(B))
    assert [ev[2].tolist() for ev in replans] == [[0, 0, 0], [0, 0, 0], [0, 1, 0], [0, 1, 0]]      # env step 3 ends ROM interval 1: its ROM step writes no row
    assert out["completed"].tolist() == [True, False, True] and out["dead"].tolist() == [False, True, False] and out["rows"].tolist() == [6, 2, 6]
    assert "plans_v" not in out
    res = pe.audit_closed_loop_env(out, p)
    assert (res["robots"], res["completed"], res["terminated"]) == (3, 2, 1)


def test_closed_loop_env_raises_when_rows_disagree_with_the_schedule(monkeypatch):
    """The "device" clock runs at half the dt the schedule was made from: live robots end with fewer than H + 2 rows."""
    with pytest.raises(RuntimeError, match=r"rom_schedule, \[1, 2, 2, 2, 2\]"):
        _run(monkeypatch, env_dt=0.125)


# ------------------------------------------------------------------------------------------------ refusals
def test_closed_loop_env_refusals(monkeypatch):
    log = []
    mk = lambda **kw: _StubEnv(log, **kw)
    P = lambda **kw: pl.PlanProblem(**{**dict(N=4, dt=0.5, rom_v_min=[-1.0, -1.0], rom_v_max=[1.0, 1.0]), **kw})
    assert pe.check_closed_loop(mk(), P(), 3) == (3, 2, [1, 2, 2, 2])
    for env, p, H, kw, word in (
            (mk(kind=2), P(), 3, {}, "PlanTrajectoryGenerator"),
            (types.SimpleNamespace(setup=types.SimpleNamespace(traj=None)), P(), 3, {}, "PlanTrajectoryGenerator"),
            (mk(), P(), 0, {}, "H = 0 must be at least 1"),
            (mk(), P(dt=0.1), 3, {}, r"problem.dt = 0.1 is not the env's rom.dt = 0.5"),
            (mk(Nw=5), P(), 3, {}, r"problem.N = 4 is shorter than the env's window, trajectory_generator.N = 5"),
            (mk(max_len=7), P(), 3, {}, "7 env steps after the reset's own; max_episode_length is 7"),
            (mk(vlim=0.35), P(), 3, {}, "allow_fast"),
            (mk(), P(rom_v_max=[1.0, 1.5]), 3, {}, r"rom_v_min / rom_v_max"),
            (mk(), P(), 3, {"w0": "tube"}, "w0 = 'tube': 'zero' or 'error'")):
        with pytest.raises(ValueError, match=word):
            pe.check_closed_loop(env, p, H, **kw)
    assert pe.check_closed_loop(mk(max_len=8), P(), 3)[2] == [1, 2, 2, 2]
    assert pe.check_closed_loop(mk(vlim=0.35), P(), 3, allow_fast=True)[0] == 3
    monkeypatch.setattr(pe, "TrajRecorder", _stub_recorder(log))
    with pytest.raises(ValueError, match=r"start must be \(2,\) or \(3, 2\)"):
        pe.closed_loop_env(mk(), None, _StubPlanner(log, P()), 2, start=torch.zeros(2, 2))
    with pytest.raises(ValueError, match="H = -1"):
        pe.closed_loop_env(mk(), None, _StubPlanner(log, P()), -1)


# ------------------------------------------------------------------------------------------------ the audit
def _records():
    p = pl.PlanProblem(N=2, goal=[2.0, 0.0], obs_c=[[5.0, 5.0]], obs_r=[1.0])
    z = torch.tensor([[[0, 0], [1, 0], [2, 0]]] * 4, dtype=torch.float32)
    pz = z.clone()
    pz[0, 1, 1] = 0.1                                            # robot 0: error 0.1 at step 1, covered by w = 0.2
    pz[1, 1] = torch.tensor([5.0, 5.5])                          # robot 1: enters the obstacle, far outside its tube
    pz[3, 2, 0] = 2.5                                            # robot 3: error 0.5 at step 2 against w = 0.3
    res = {"z": z, "pz_x": pz, "w": torch.tensor([[0.0, 0.2, 0.2], [0.0, 0.1, 0.1], [0.0, 0.5, 0.5], [0.0, 0.3, 0.3]]),
           "v": torch.zeros(4, 2, 2), "min_clear": torch.tensor([[0.5, 0.5], [0.5, -0.1], [0.3, 0.3], [0.2, 0.2]]),
           "completed": torch.tensor([True, True, False, True]), "dead": torch.tensor([False, False, True, False])}
    return p, res


def test_audit_closed_loop_env_by_hand():
    p, res = _records()
    r = pe.audit_closed_loop_env(res, p)
    assert (r["robots"], r["completed"], r["terminated"], r["steps"]) == (4, 3, 1, 2)
    # completed robots 0, 1, 3: robot 0 covered and safe; robot 1 uncovered at step 1, predicted unsafe, enters the obstacle; robot 3 uncovered
    # at step 2; the fallen robot 2 counts only in covered_robots_of_all
    assert r["coverage_by_step"] == [1.0, pytest.approx(2 / 3), pytest.approx(2 / 3)] and r["covered_robots"] == pytest.approx(1 / 3)
    assert r["covered_robots_of_all"] == 0.25 and r["predicted_safe"] == pytest.approx(2 / 3) and r["actually_safe"] == pytest.approx(2 / 3)
    assert r["reached_goal"] == 1.0 and r["goal_distance_mean"] == 0.0 and r["error_max"] == pytest.approx(float(np.hypot(4.0, 5.5)))
    assert json.loads(json.dumps(r, allow_nan=False)) == r
    everyone = dict(res, completed=torch.ones(4, dtype=torch.bool), dead=torch.zeros(4, dtype=torch.bool))
    full, base = pe.audit_closed_loop_env(everyone, p), pl.audit_closed_loop(everyone, p)
    assert all(full[k] == base[k] for k in base) and full["covered_robots_of_all"] == full["covered_robots"] == 0.5
    sc = pl.Scenes.repeat(p, 4)
    with_scenes = pe.audit_closed_loop_env(res, p, scenes=sc)
    assert with_scenes["by_robot"]["robot"] == [0, 1, 3] and with_scenes["by_robot"]["covered"] == [True, False, False]
    assert with_scenes["actually_safe"] == r["actually_safe"]


def test_audit_closed_loop_env_with_nobody_completed():
    p, res = _records()
    res = dict(res, completed=torch.zeros(4, dtype=torch.bool), dead=torch.ones(4, dtype=torch.bool))
    r = pe.audit_closed_loop_env(res, p, goal_tol=0.2)
    assert (r["robots"], r["completed"], r["terminated"], r["steps"], r["covered_robots_of_all"], r["goal_tol"]) == (4, 0, 4, 2, 0.0, 0.2)
    assert all(r[k] is None for k in ("coverage", "coverage_by_step", "covered_robots", "predicted_safe", "actually_safe", "reached_goal",
                                      "goal_distance_mean", "error_mean", "error_max"))
    text = json.dumps(r, allow_nan=False)
    assert "null" in text and json.loads(text) == r
    assert set(r) == set(pe.audit_closed_loop_env(_records()[1], p))             # the same keys either way


# ------------------------------------------------------------------------------------------------ the script's flags
def test_script_robot_flags(capsys):
    import plan_tube
    ok = ["--tube", "l1", "--problem", "gap"]
    a = plan_tube.parse_args(ok + ["--closed_loop", "5"])
    assert a.robot is False and a.task is None and a.push_robots is False and a.allow_fast is False
    a = plan_tube.parse_args(ok + ["--closed_loop", "5", "--robot", "--task", "anymal_c_flat_trajectory", "--load_run", "r", "--policy_checkpoint",
                                   "40", "--push_robots", "--allow_fast"])
    assert a.robot and a.policy_checkpoint == 40 and a.load_run == "r" and a.push_robots and a.allow_fast and a.checkpoint == "best"
    for argv, word in ((ok + ["--robot"], "audit_plans.py --robot"), (ok + ["--robot"], "--robot belongs to --closed_loop"),
                       (ok + ["--closed_loop", "5", "--task", "anymal_c_flat_trajectory"], "--task belongs to --robot"),
                       (ok + ["--closed_loop", "5", "--push_robots"], "--push_robots belongs"), (ok + ["--load_run", "r"], "--load_run belongs"),
                       (ok + ["--policy_checkpoint", "3"], "--policy_checkpoint belongs"), (ok + ["--allow_fast"], "--allow_fast belongs"),
                       (ok + ["--closed_loop", "5", "--robot", "--sim_cfg", "controller.Kp=10"], "--sim_cfg configures")):
        with pytest.raises(SystemExit):
            plan_tube.parse_args(argv)
        assert word in capsys.readouterr().err


# ------------------------------------------------------------------------------------------------ the C entry
def test_capi_exposes_lg_traj_replan_with_the_headers_signature():
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    lib = L.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "legged_hip.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+lg_traj_replan\s*\(([^)]*)\)\s*;", text)
    assert m, "include/legged_hip.h does not declare lg_traj_replan"
    params = [" ".join(x.split()) for x in m.group(1).split(",")]
    assert params == ["lg_ctx *ctx", "const float *v", "int32_t n_nodes", "const uint8_t *skip"]
    as_ctypes = [C.c_void_p if "*" in x else {"int32_t": C.c_int32, "int": C.c_int}[x.split()[0]] for x in params]
    assert list(lib.lg_traj_replan.argtypes) == as_ctypes
    v = (C.c_float * 2)()
    assert lib.lg_traj_replan(None, C.cast(v, C.c_void_p), 1, None) == -1 and "null argument" in lib.lg_last_error().decode()
    assert hasattr(capi, "PLAN_MAX_N") and capi.PLAN_MAX_N == 64


def test_replan_view_refusals():
    """traj_gen.replan's shape checks, beside set_plans': before any library call."""
    from legged_gym_dev_amd.envs.base.legged_robot_trajectory import _TrajGenView
    calls = []
    view = _TrajGenView.__new__(_TrajGenView)
    view._kind, view._t = capi.TG_KINDS["PlanTrajectoryGenerator"], {"tg_traj": torch.zeros(3, 3, 2)}
    view._core = types.SimpleNamespace(call=lambda *a: calls.append(a))
    for v, skip, word in ((torch.zeros(4, 5, 2), None, r"v must be \(3, n_nodes, 2\)"), (torch.zeros(3, 5, 3), None, "v must be"),
                          (torch.zeros(3, 0, 2), None, r"n_nodes = 0 must lie in 1\.\.LG_PLAN_MAX_N = 64"), (torch.zeros(3, 65, 2), None, "n_nodes = 65"),
                          (torch.zeros(3, 5, 2), torch.zeros(4, dtype=torch.uint8), "skip must be"),
                          (torch.zeros(3, 5, 2), torch.zeros(3, dtype=torch.int32), "skip must be")):
        with pytest.raises(ValueError, match=word):
            view.replan(v, skip)
    assert not calls
    view.replan(torch.zeros(3, 5, 2), torch.tensor([0, 1, 0], dtype=torch.uint8))
    view.replan(torch.zeros(3, 64, 2))
    assert [c[0] for c in calls] == ["traj_replan", "traj_replan"] and calls[0][2] == 5 and calls[1][3] is None
    view._kind = capi.TG_KINDS["TrajectoryGenerator"]
    with pytest.raises(ValueError, match="not 'PlanTrajectoryGenerator'"):
        view.replan(torch.zeros(3, 5, 2))
