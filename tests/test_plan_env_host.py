"""Plans tracked on the legged env, the part that needs no GPU (legged_gym_dev_amd/tube/plan_env.py, lg_traj_rec_check; DESIGN.md
section 10.12): the configuration, every refusal, lg_traj_rec against the header and its check's words on both sides, the
restatement (tests/plan_env_ref.py) by hand, the row alignment on a stub, audit_env on hand-made records, the script's flags."""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.tube import plan as pl
from legged_gym_dev_amd.tube import plan_env as pe
from tests import plan_env_ref as ref
from tests.test_eval_generators import _cfg, _setup

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
PLAN = "PlanTrajectoryGenerator"


@pytest.fixture(scope="module")
def lib():
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    return L.load()


# ------------------------------------------------------------------------------------------------ configuration
def test_plan_generator_constructs_with_kind_4_and_the_default_stays():
    assert capi.TG_KINDS[PLAN] == 4
    s = _setup(_cfg(PLAN))
    assert (s.traj["kind"], s.traj["weight_sampler"]) == (4, 0)
    s = _setup(_cfg())
    assert (s.traj["kind"], s.traj["weight_sampler"]) == (0, 0)


def test_plan_env_cfg_carries_the_evaluation_overrides():
    env_cfg, train_cfg = pe.plan_env_cfg("anymal_c_flat_trajectory", 33)
    dr = env_cfg.domain_rand
    assert env_cfg.trajectory_generator.cls == PLAN and env_cfg.env.num_envs == 33 and env_cfg.env.episode_length_s == 20
    assert not (dr.randomize_friction or dr.randomize_base_mass or dr.randomize_inv_base_mass or dr.push_robots or dr.randomize_rom_distance)
    rsp = dr.rigid_shape_properties
    assert not (rsp.randomize_restitution or rsp.randomize_compliance or rsp.randomize_thickness) and not env_cfg.curriculum.use_curriculum
    assert dr.time_between_pushes == [1e6, 1e6]                 # the env's push timers are not gated by push_robots: parked beyond any horizon
    pushed = pe.plan_env_cfg("anymal_c_flat_trajectory", 2, push_robots=True)[0].domain_rand
    assert pushed.push_robots is True and pushed.time_between_pushes == [0.5, 10.0]
    from legged_gym_dev_amd.envs import task_registry
    assert task_registry.get_cfgs(name="anymal_c_flat_trajectory")[0].trajectory_generator.cls == "TrajectoryGenerator"   # a copy was changed
    with pytest.raises(ValueError, match="not a trajectory-tracking task"):
        pe.plan_env_cfg("anymal_c_flat", 4)
    with pytest.raises(ValueError, match="B = 0"):
        pe.plan_env_cfg("anymal_c_flat_trajectory", 0)


# ------------------------------------------------------------------------------------------------ track_env's refusals
def _stub_env(B=3, Nw=10, kind=4, max_len=1000, vlim=0.35):
    return types.SimpleNamespace(num_envs=B, dt=0.02, max_episode_length=max_len,
                                 setup=types.SimpleNamespace(traj={"kind": kind, "N": Nw, "rom_dt": 0.1}),
                                 rom=types.SimpleNamespace(v_min=torch.tensor([-vlim, -vlim]), v_max=torch.tensor([vlim, vlim])))


def test_track_env_refusals():
    v, z0 = torch.zeros(3, 8, 2), torch.zeros(3, 2)
    assert pe.check_track(_stub_env(), v, z0, H_rev=10) == (3, 8, 10, 5, (10 + 8 + 1) * 5 + 5)
    for env, vv, zz, kw, word in (
            (_stub_env(kind=2), v, z0, {}, "PlanTrajectoryGenerator"),
            (types.SimpleNamespace(setup=types.SimpleNamespace(traj=None)), v, z0, {}, "PlanTrajectoryGenerator"),
            (_stub_env(), torch.zeros(3, 65, 2), z0, {}, "LG_PLAN_MAX_N"),
            (_stub_env(), torch.zeros(4, 8, 2), z0, {}, r"v must be \(3, Np >= 1, 2\)"),
            (_stub_env(), torch.zeros(3, 8, 3), z0, {}, "v must be"),
            (_stub_env(), torch.zeros(3, 0, 2), z0, {}, "v must be"),
            (_stub_env(), v, torch.zeros(2, 2), {}, r"z0 must be \(3, 2\)"),
            (_stub_env(), v, z0, {"H_rev": 11}, r"H_rev = 11 must lie in 0\.\.10"),
            (_stub_env(), v, z0, {"H_rev": -1}, "H_rev = -1"),
            (_stub_env(max_len=100), v, z0, {}, "100 env steps after the reset's own; max_episode_length is 100")):
        with pytest.raises(ValueError, match=word):
            pe.check_track(env, vv, zz, **kw)
    assert pe.check_track(_stub_env(max_len=101), v, z0)[4] == 100
    fast = torch.zeros(3, 8, 2)
    fast[1, 4, 1] = -1.0                                         # the `right` problem's vel_max against ANYmal's 0.35
    with pytest.raises(ValueError) as ei:
        pe.check_track(_stub_env(), fast, z0)
    assert "|v| = 1 m/s" in str(ei.value) and "[-0.35, -0.35] / [0.35, 0.35]" in str(ei.value) and "allow_fast" in str(ei.value)
    assert pe.check_track(_stub_env(), fast, z0, allow_fast=True)[1] == 8
    gap = torch.full((3, 8, 2), 0.2)
    gap[0] = -0.2
    assert pe.check_track(_stub_env(), gap, z0)[0] == 3           # the `gap` problem's 0.2 m/s fits
    with pytest.raises(ValueError, match="of x, rec"):
        pe.track_env(_stub_env(), None, v, z0, want=("u",))


# ------------------------------------------------------------------------------------------------ lg_traj_rec
def _rec(**kw):
    r = capi.lg_traj_rec()
    r.rows_max, r.x_n = 5, 0
    for name in ("z", "pz_x", "v", "rows", "dead", "k_mark"):
        setattr(r, name, 64)                                     # the check never dereferences
    for k, val in kw.items():
        setattr(r, k, val)
    return r


@pytest.mark.parametrize("change,N,word", [
    (dict(rows_max=1), 4, "rows_max"), (dict(rows_max=-3), 4, "rows_max"), (dict(z=None), 4, "z is null"), (dict(pz_x=None), 4, "pz_x"),
    (dict(v=None), 4, "v is null"), (dict(rows=None), 4, "rows is null"), (dict(dead=None), 4, "dead"), (dict(k_mark=None), 4, "k_mark"),
    (dict(x=64, x_n=36), 4, "x_n = 36 must be the env's 37"), (dict(x=64, x_n=0), 4, "x_n = 0"), (dict(x_n=37), 4, "must be 0 without x"),
    (dict(), 0, "N = 0")])
def test_recorder_check_names_the_field_on_both_sides(lib, change, N, word):
    r = _rec(**change)
    why = pe.rec_refusal(r, N, 37)
    assert why is not None and word in why
    assert lib.lg_traj_rec_check(C.byref(r), N, 37) == -1
    assert lib.lg_last_error().decode() == "lg_traj_rec: " + why                 # the same words


def test_recorder_check_passes_and_the_entries_refuse_before_a_device(lib):
    for r in (_rec(), _rec(rows_max=2), _rec(x=64, x_n=37)):
        assert pe.rec_refusal(r, 4, 37) is None and lib.lg_traj_rec_check(C.byref(r), 4, 37) == 0
    assert lib.lg_traj_rec_check(None, 4, 37) == -1 and "rec is null" in lib.lg_last_error().decode()
    for fn, args in (("lg_traj_rec_begin", (C.byref(_rec()),)), ("lg_traj_rec_step", (C.byref(_rec()),)), ("lg_traj_set_plans", (None, 0))):
        assert getattr(lib, fn)(None, *args) == -1 and "null argument" in lib.lg_last_error().decode()


def test_struct_and_constants_match_the_header():
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "legged_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %d %d\\n",' \
          'sizeof(lg_traj_rec),offsetof(lg_traj_rec,rows_max),offsetof(lg_traj_rec,x_n),offsetof(lg_traj_rec,z),offsetof(lg_traj_rec,pz_x),' \
          'offsetof(lg_traj_rec,v),offsetof(lg_traj_rec,rows),offsetof(lg_traj_rec,dead),offsetof(lg_traj_rec,k_mark),offsetof(lg_traj_rec,x),' \
          'LG_TG_KIND_PLAN,LG_PLAN_MAX_N);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    c = capi.lg_traj_rec
    assert out == [C.sizeof(c), c.rows_max.offset, c.x_n.offset, c.z.offset, c.pz_x.offset, c.v.offset, c.rows.offset, c.dead.offset,
                   c.k_mark.offset, c.x.offset, capi.TG_KINDS[PLAN], capi.PLAN_MAX_N]


# ------------------------------------------------------------------------------------------------ the restatement by hand
def test_law_by_hand():
    """Nw = 2, one env step per ROM step (dt = rom_dt = 0.5, exact in binary): the pre-roll leaves the window on the start, node k
    advances the head on the step that takes k to k + 1, past the plan the input is 0, and v_in is the input last applied."""
    law = ref.PlanLaw(np.float32([[[1, 0], [0, 2]], [[-1, -1], [4, 0]]]), Nw=2, rom_dt=0.5, dt=0.5)
    law.reset([0, 1], [[0, 0], [10, 10]])
    assert law.k.tolist() == [0, 0] and law.t.tolist() == [0, 0] and np.all(law.win[1] == 10) and np.all(law.v_in == 0)
    assert law.step().all()
    assert law.win[0].tolist() == [[0, 0], [0, 0], [0.5, 0]] and law.win[1, -1].tolist() == [9.5, 9.5] and law.v_in.tolist() == [[1, 0], [-1, -1]]
    law.step()
    assert law.win[0].tolist() == [[0, 0], [0.5, 0], [0.5, 1]] and law.win[1, -1].tolist() == [11.5, 9.5] and law.k.tolist() == [2, 2]
    law.step()                                                   # k = 2 = n_nodes: input 0, the head stays
    assert law.win[0].tolist() == [[0.5, 0], [0.5, 1], [0.5, 1]] and law.v_in.tolist() == [[0, 0], [0, 0]] and law.k.tolist() == [3, 3]
    law.reset([1], [[3, 4]])                                     # env 1 replays from node 0 at its new position; env 0 is not touched
    law.step()
    assert law.win[1, -1].tolist() == [2.5, 3.5] and law.k.tolist() == [4, 1] and law.win[0, -1].tolist() == [0.5, 1]
    # several env steps per ROM step: the input in force holds between ROM steps
    law = ref.PlanLaw(np.float32([[[1, 1], [2, 2]]]), Nw=1, rom_dt=0.5, dt=0.25)
    law.reset([0], [[0, 0]])
    seen = []
    for _ in range(5):
        stepped = law.step()
        seen.append((bool(stepped[0]), law.v_in[0].tolist(), law.win[0, -1].tolist()))
    assert seen == [(True, [1, 1], [0.5, 0.5]), (False, [1, 1], [0.5, 0.5]), (True, [2, 2], [1.5, 1.5]), (False, [2, 2], [1.5, 1.5]),
                    (True, [0, 0], [1.5, 1.5])]
    no_plan = ref.PlanLaw(np.zeros((1, 0, 2), np.float32), Nw=1, rom_dt=0.5, dt=0.5)     # before any plan was set
    no_plan.reset([0], [[1, 2]])
    no_plan.step()
    assert no_plan.win[0].tolist() == [[1, 2], [1, 2]] and no_plan.v_in.tolist() == [[0, 0]]
    np.testing.assert_array_equal(ref.chain(np.float32([[0, 0]]), np.float32([[[1, 0], [0, 2]]]), 0.5)[0], [[0, 0], [0.5, 0], [0.5, 1]])


def test_recorder_by_hand_on_a_six_step_script():
    """Three envs, rows_max = 4.  Env 0 steps its ROM on env steps 1, 3, 5; env 1 resets on step 3 (dead, rows kept, later ROM steps
    ignored); env 2's second ROM step comes an env step late (step 4 instead of 3) and is recorded when it comes."""
    rec = ref.Recorder(3, 4, x_n=1)
    z = lambda s: np.float32([[s, 0], [s, 1], [s, 2]])
    pz = lambda s: np.float32([[s, 10], [s, 11], [s, 12]])
    x = lambda s: np.float32([[s], [s + 0.25], [s + 0.5]])
    v = lambda s: np.float32([[s, -s]] * 3)
    rec.begin(z(0), pz(0), np.float32([5, 5, 5]), x(0))
    assert rec.rows.tolist() == [1, 1, 1] and rec.dead.tolist() == [0, 0, 0] and rec.k_mark.tolist() == [5, 5, 5]
    script = [  # (reset, k) after env steps 1..6
        ([0, 0, 0], [6, 6, 6]), ([0, 0, 0], [6, 6, 6]), ([0, 1, 0], [7, 0, 6]), ([0, 0, 0], [7, 1, 7]), ([0, 0, 0], [8, 1, 7]),
        ([0, 0, 0], [9, 2, 8])]
    for s, (reset, k) in enumerate(script, start=1):
        rec.step(np.array(reset, bool), z(s), pz(s), np.float32(k), v(s), x(s))
    assert rec.rows.tolist() == [4, 2, 4] and rec.dead.tolist() == [0, 1, 0]
    assert rec.z[0, :, 0].tolist() == [0, 1, 3, 5] and rec.pz_x[0, :, 1].tolist() == [10, 10, 10, 10]          # step 6: rows_max reached
    assert rec.z[1, :, 0].tolist() == [0, 1, 0, 0] and rec.v[1, :, 0].tolist() == [1, 0, 0]                    # dead from step 3 on
    assert rec.z[2, :, 0].tolist() == [0, 1, 4, 6] and rec.v[2].tolist() == [[1, -1], [4, -4], [6, -6]]        # the late step is row 2
    assert rec.x[2, :, 0].tolist() == [0.5, 1.5, 4.5, 6.5] and rec.k_mark.tolist() == [8, 6, 8]


# ------------------------------------------------------------------------------------------------ alignment
def test_alignment_on_a_stub():
    """Rows built from a known ROM path: plan node j is row Nw + j, the frame moves the window's start onto z0, the history is
    the lead-in rows' error, and completed needs every row and no reset."""
    Nw, Np, B, Hr = 3, 4, 3, 2
    rng = np.random.default_rng(0)
    R = Nw + Np + 1
    start = np.float32(rng.uniform(-30, 30, (B, 2)))
    v = np.float32(rng.uniform(-0.3, 0.3, (B, Np, 2)))
    Z = ref.chain(start, v, 0.1)                                                  # world nodes 0..Np
    rec_z = np.concatenate([np.repeat(start[:, None], Nw, 1), Z], 1)            # rows 0..Nw-1 on the start, then the nodes
    rec_pz = np.float32(rec_z + rng.normal(0, 0.01, rec_z.shape))
    rec_pz[:, 0] = rec_z[:, 0]
    rows, dead = np.int32([R, R - 1, R]), np.uint8([0, 0, 1])
    z0 = np.float32([[0.3, 0.3]] * B)
    want = ref.align(rec_z, rec_pz, rows, dead, z0, Nw, Np, Hr)
    got = pe.align(*(torch.as_tensor(a) for a in (rec_z, rec_pz, rows, dead, z0)), Nw, Np, Hr)
    assert got["completed"].tolist() == [True, False, False] == want["completed"].tolist() and got["dead"].tolist() == [False, False, True]
    for k in ("pz_x", "z_ref"):
        assert tuple(got[k].shape) == (B, Np + 1, 2)
        np.testing.assert_array_equal(got[k].numpy(), want[k])
    np.testing.assert_array_equal(got["z_ref"][:, 0].numpy(), z0)                  # node 0 is the plan's start
    plan_nodes = ref.chain(z0, v, 0.1)
    np.testing.assert_allclose(got["z_ref"].numpy(), plan_nodes, rtol=0, atol=4 * float(np.spacing(np.float32(30))))   # world rounding at |30|
    assert tuple(got["w_true"].shape) == (B, Np + 1) and tuple(got["e_past"].shape) == (B, Hr) and tuple(got["v_prev"].shape) == (B, Hr, 2)
    tol = dict(rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(got["w_true"].numpy(), want["w_true"], **tol)
    np.testing.assert_allclose(got["e_past"].numpy(), want["e_past"], **tol)
    np.testing.assert_allclose(got["e_past"].numpy(), np.linalg.norm(rec_z - rec_pz, axis=-1)[:, Nw - Hr:Nw], **tol)
    assert torch.equal(got["w0"], got["w_true"][:, 0]) and not got["v_prev"].any()
    assert pe.align(*(torch.as_tensor(a) for a in (rec_z, rec_pz, rows, dead, z0)), Nw, Np, 0)["e_past"].shape == (B, 0)


# ------------------------------------------------------------------------------------------------ audit_env
def _records():
    p = pl.PlanProblem(N=2, obs_c=[[5.0, 5.0]], obs_r=[1.0])
    score = {"w": torch.tensor([[0.0, 0.2, 0.2], [0.0, 0.1, 0.1], [0.0, 0.5, 0.5], [0.0, 0.5, 0.5]]),
             "min_clear": torch.tensor([0.5, -0.1, 0.3, 0.2])}
    trk = {"w_true": torch.tensor([[0.0, 0.1, 0.2], [0.0, 0.2, 0.05], [0.0, 0.0, 0.0], [0.0, 0.9, 0.0]]),
           "pz_x": torch.tensor([[[0, 0], [1, 1], [2, 2]], [[0, 0], [5, 5.5], [9, 9]], [[0, 0], [0, 0], [0, 0]], [[0, 0], [1, 0], [2, 0]]],
                                dtype=torch.float32),
           "completed": torch.tensor([True, True, False, True]), "dead": torch.tensor([False, False, True, False])}
    return p, score, trk


def test_audit_env_by_hand():
    p, score, trk = _records()
    r = pe.audit_env(score, trk, p)
    assert (r["plans"], r["completed"], r["terminated"], r["nodes"]) == (4, 3, 1, 3)
    # completed plans 0, 1, 3: plan 0 covered everywhere and safe; plan 1 uncovered at node 1, predicted unsafe, enters the obstacle;
    # plan 3 uncovered at node 1, predicted and actually safe; the fallen robot 2 counts only in covered_plans_of_all
    assert r["coverage_by_node"] == [1.0, 1 / 3, 1.0] and r["coverage"] == pytest.approx(7 / 9) and r["covered_plans"] == pytest.approx(1 / 3)
    assert r["covered_plans_of_all"] == 0.25 and r["predicted_safe"] == pytest.approx(2 / 3) and r["actually_safe"] == pytest.approx(2 / 3)
    assert r["table"] == {"safe_safe": pytest.approx(2 / 3), "safe_unsafe": 0.0, "unsafe_safe": 0.0, "unsafe_unsafe": pytest.approx(1 / 3)}
    assert r["w_true_max"] == pytest.approx(0.9)
    assert json.loads(json.dumps(r, allow_nan=False)) == r
    want = ref.audit_env(score["w"].numpy(), score["min_clear"].numpy(), trk["w_true"].numpy(), trk["pz_x"].numpy(), trk["completed"].numpy(),
                         trk["dead"].numpy(), p.obs_c, p.obs_r)
    assert set(want) == set(r)
    for k in want:
        assert r[k] == pytest.approx(want[k]), k
    # every robot completed: the library audit itself plus the counts
    trk_all = dict(trk, completed=torch.ones(4, dtype=torch.bool), dead=torch.zeros(4, dtype=torch.bool))
    full, base = pe.audit_env(score, trk_all, p), pl.audit(score, trk_all, p)
    assert all(full[k] == base[k] for k in base) and full["covered_plans_of_all"] == full["covered_plans"] == 0.5


def test_audit_env_with_every_robot_terminated():
    p, score, trk = _records()
    trk = dict(trk, completed=torch.zeros(4, dtype=torch.bool), dead=torch.ones(4, dtype=torch.bool))
    r = pe.audit_env(score, trk, p)
    assert (r["plans"], r["completed"], r["terminated"], r["nodes"], r["covered_plans_of_all"]) == (4, 0, 4, 3, 0.0)
    assert all(r[k] is None for k in ("coverage", "coverage_by_node", "covered_plans", "predicted_safe", "actually_safe", "table", "w_true_mean"))
    text = json.dumps(r, allow_nan=False)
    assert "null" in text and json.loads(text) == r
    assert r == ref.audit_env(score["w"].numpy(), score["min_clear"].numpy(), trk["w_true"].numpy(), trk["pz_x"].numpy(), np.zeros(4, bool),
                              np.ones(4, bool), p.obs_c, p.obs_r)


# ------------------------------------------------------------------------------------------------ the script's flags
def test_script_robot_flags(capsys):
    import audit_plans
    ok = ["--tube", "l2", "--problem", "gap", "--warm_start", "interpolate"]
    a = audit_plans.parse_args(ok)
    assert a.robot is False and a.task is None and a.push_robots is False
    a = audit_plans.parse_args(ok + ["--robot", "--task", "anymal_c_flat_trajectory", "--load_run", "r", "--policy_checkpoint", "40", "--push_robots"])
    assert a.robot and a.policy_checkpoint == 40 and a.load_run == "r" and a.push_robots and a.checkpoint == "best"
    for argv, word in ((ok + ["--task", "anymal_c_flat_trajectory"], "--task belongs to --robot"), (ok + ["--push_robots"], "--push_robots belongs"),
                       (ok + ["--load_run", "r"], "--load_run belongs"), (ok + ["--policy_checkpoint", "3"], "--policy_checkpoint belongs"),
                       (ok + ["--allow_fast"], "--allow_fast belongs"), (ok + ["--robot", "--sim_cfg", "controller.Kp=10"], "--sim_cfg configures")):
        with pytest.raises(SystemExit):
            audit_plans.parse_args(argv)
        assert word in capsys.readouterr().err
