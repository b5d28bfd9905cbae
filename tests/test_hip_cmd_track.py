"""The command tracker on the GPU (csrc/cmdtrack_kernels.hip, legged_gym_dev_amd/tube/cmd_track.py)
against tests/cmd_track_ref.py.  Tests 1, 2 and 5 are teacher-forced on anymal_c_flat through tests/harness.py: root_states and
the reset flags are installed before each tracker call, so no physics runs.

Tolerance: the project's e32 rule with the factor 4 of section 10.11 -- |device - float64| <= 4 max |float32 restatement - float64|
per quantity.  A row (env, call) is compared where the float64 restatement's raw command keeps 1e-4 from every clip bound and,
with track_yaw, the wrap's argument keeps 1e-4 from the cut; at least 90 % of the rows must qualify."""
import copy
import ctypes as C
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.tube import cmd_track as ct
from tests import cmd_track_ref as ref
from tests import harness

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
F = np.float32
KP = (1.5, 0.2, -0.1, -0.3, 1.2, 0.05, 0.1, -0.2, 0.8)
U_MIN, U_MAX = (-1.2, -0.9, -1.0), (1.1, 1.0, 0.9)
MARGIN = 1e-4


# ------------------------------------------------------------------------------------------------ teacher-forced env handles
_HANDLES = {}


def _handle(n):
    if n not in _HANDLES:
        from legged_gym_dev_amd.envs.base.env_setup import EnvSetup, sim_dt_float
        from legged_gym_dev_amd.model.robot_model import compile_model, resolve_model
        cfg = harness.make_cfg("anymal_c_flat")
        cfg.env.num_envs = n
        h = harness.HipHandle(EnvSetup(cfg, compile_model(resolve_model("", "anymal_c")), sim_dt_float(cfg.sim.dt), seed=1))
        h.set_step_counter(0)
        h.inject(0)
        h.call("reset_all")
        h.sync()
        h.view = types.SimpleNamespace(core=h.core, setup=h.setup, num_envs=n, num_actions=h.setup.num_dof, device=DEV, dt=h.setup.dt)
        _HANDLES[n] = h
    return _HANDLES[n]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


def _states(n_max, T, seed):
    """root_states (T + 1, n, 13) with arbitrary orientations and positions within +-1, dof_state, reset flags (T, n), an
    observation to write into.  Env j's values do not depend on how many envs are taken."""
    rng = np.random.default_rng(seed)
    roots = rng.uniform(-1, 1, (T + 1, n_max, 13)).astype(F)
    q = rng.normal(size=(T + 1, n_max, 4))
    roots[..., 3:7] = (q / np.linalg.norm(q, axis=-1, keepdims=True) * rng.uniform(0.8, 1.2, (T + 1, n_max, 1))).astype(F)
    dones = rng.random((T, n_max)) < 0.2
    dof = rng.uniform(-1, 1, (n_max, 12, 2)).astype(F)
    obs = rng.uniform(-1, 1, (n_max, 48)).astype(F)
    return roots, dones, dof, obs


def _cfg_dict(kind, track_yaw, scale, rom_dt, **gen):
    return {"kind": kind, "track_yaw": track_yaw, "Kp": KP, "u_min": U_MIN, "u_max": U_MAX, "cmd_scale": scale, "rom_dt": rom_dt, **gen}


def _qualify(cfg, parts):
    """(n,) bool: the float64 margins of one call."""
    raw, lo, hi = parts["raw"], np.asarray(cfg["u_min"], F).astype(np.float64), np.asarray(cfg["u_max"], F).astype(np.float64)
    ok = (np.minimum(np.abs(raw - lo), np.abs(raw - hi)) >= MARGIN).all(axis=1)
    if cfg["track_yaw"]:
        m = np.mod(parts["wrap_arg"] + np.pi, 2 * np.pi)
        ok &= np.minimum(m, 2 * np.pi - m) >= MARGIN
    return ok


def _e32(name, dev, r64, r32, mask):
    """The e32 rule on the rows of `mask`; returns the ratio."""
    e32 = float(np.abs(r32.astype(np.float64) - r64)[mask].max())
    err = float(np.abs(np.asarray(dev).astype(np.float64) - r64)[mask].max())
    print(f"{name}: e32 = {e32:.3e}, |device - float64| = {err:.3e}, device / e32 = {err / e32 if e32 else 0.0:.2f}")
    assert err <= 4 * e32 if e32 else err == 0.0, (name, err, e32)
    return err / e32 if e32 else 0.0


def _drive(h, tracker, T, roots, dones, dof, obs0, refs, other_cols=True, want_u=True, epoch=0, after=None):
    """begin + T steps on installed states; feeds the same states to the restatements `refs`.  Returns the records (numpy) and
    the command columns of the observation after every call."""
    n = h.setup.num_envs
    h.set("dof_state", dof[:n])
    h.set("obs", obs0[:n])
    cmds = []
    keep = np.r_[0:9, 12:48]

    def call(fn, root):
        h.set("root_states", root)
        before = h.get("obs")
        fn()
        got = h.get("obs")
        if other_cols:
            np.testing.assert_array_equal(got[:, keep].view(np.uint32), before[:, keep].view(np.uint32))
        cmds.append(got[:, 9:12].copy())
        if after is not None:
            after()
    call(lambda: tracker.begin(T, epoch=epoch, want_u=want_u), roots[0, :n])
    for r in refs:
        r.begin(roots[0, :n])
    for t in range(T):
        h.set("reset", dones[t, :n].astype(np.uint8))
        call(lambda: tracker.step(t), roots[t + 1, :n])
        for r in refs:
            r.step(t, roots[t + 1, :n], dones[t, :n])
    h.sync()
    return {k: v.cpu().numpy() for k, v in tracker.records().items()}, cmds


# ------------------------------------------------------------------------------------------------ 1. PLAN kind
T1, NODES = 6, 4
_PLAN_RUNS = {}


def _plan_inputs():
    roots, dones, dof, obs = _states(130, T1, seed=21)
    rng = np.random.default_rng(22)
    ang, mag = rng.uniform(-np.pi, np.pi, (130, NODES)), rng.uniform(0.2, 1.0, (130, NODES))
    plan = np.stack([mag * np.cos(ang), mag * np.sin(ang)], -1).astype(F)
    return roots, dones, dof, obs, plan


def _plan_run(n, track_yaw, raw):
    key = (n, track_yaw, raw)
    if key in _PLAN_RUNS:
        return _PLAN_RUNS[key]
    h = _handle(n)
    roots, dones, dof, obs, plan = _plan_inputs()
    cfg = ct.CmdTrackCfg.from_env(h.view, raw_commands=raw, want_x=True, kind=ct.PLAN, track_yaw=track_yaw, Kp=KP, u_min=U_MIN, u_max=U_MAX)
    assert cfg.cmd_scale == ((1.0, 1.0, 1.0) if raw else (2.0, 2.0, 0.25)) and cfg.rom_dt == h.setup.dt
    d = _cfg_dict(ref.PLAN, track_yaw, cfg.cmd_scale, cfg.rom_dt)
    r64, r32 = (ref.CmdTrackRef(d, n, T1, D, plan=plan[:n]) for D in (np.float64, np.float32))
    tr = ct.HipCommandTracker(h.view, cfg)
    try:
        tr.set_plans(plan[:n])
        rec, cmds = _drive(h, tr, T1, roots, dones, dof, obs, (r64, r32))
    finally:
        tr.close()
    _PLAN_RUNS[key] = dict(rec=rec, cmds=cmds, r64=r64, r32=r32, cfg=d, roots=roots[:, :n], dones=dones[:, :n], dof=dof[:n], plan=plan[:n])
    return _PLAN_RUNS[key]


@pytest.mark.parametrize("n", [1, 63, 65, 130])
def test_plan_kind_records_on_the_bits_and_commands_within_4_e32(n):
    """N below, across and past a wave; T = 6 on plans of 4 nodes, so the last two steps read past the plan."""
    for track_yaw in (False, True):
        for raw in (False, True):
            run = _plan_run(n, track_yaw, raw)
            rec, r32, r64, roots, dones = run["rec"], run["r32"], run["r64"], run["roots"], run["dones"]
            # ---- on the bits
            np.testing.assert_array_equal(rec["pz_x"], roots[:, :, :2].transpose(1, 0, 2))
            np.testing.assert_array_equal(rec["done"], dones.T)
            np.testing.assert_array_equal(rec["v"][:, :NODES].view(np.uint32), run["plan"].view(np.uint32))
            np.testing.assert_array_equal(rec["v"][:, NODES:].view(np.uint32), np.zeros((n, T1 - NODES, 2), np.uint32))   # +0.0
            dt = F(r32.c["rom_dt"])
            for t in range(T1):
                want = rec["z"][:, t] + dt * rec["v"][:, t]
                want[dones[t]] = roots[t + 1][dones[t], :2]
                np.testing.assert_array_equal(rec["z"][:, t + 1].view(np.uint32), want.view(np.uint32))
            np.testing.assert_array_equal(rec["z"].view(np.uint32), r32.rec["z"].view(np.uint32))
            dq, dqd = (np.broadcast_to(run["dof"][None, :, :, k], (T1 + 1, n, 12)) for k in (0, 1))
            x_want = np.concatenate([roots[..., :7], dq, roots[..., 7:], dqd], -1)        # get_state()'s layout
            np.testing.assert_array_equal(rec["x"], x_want.transpose(1, 0, 2))
            # ---- under the e32 bound, on the rows with margin
            ok = np.stack([_qualify(run["cfg"], p) for p in r64.parts], 1)                  # (n, T) : one command per call but the last
            assert ok.shape == (n, T1) and len(run["cmds"]) == T1 + 1
            assert ok.mean() >= 0.9, ok.mean()
            tag = f"N={n} yaw={int(track_yaw)} raw={int(raw)}"
            got = np.stack(run["cmds"][:T1], 1)
            if ok.any():
                _e32(tag + " obs[:, 9:12]", got, np.stack(r64.cmd, 1), np.stack(r32.cmd, 1), ok)
                _e32(tag + " u", rec["u"], r64.rec["u"], r32.rec["u"], ok)
            np.testing.assert_array_equal(run["cmds"][T1], run["cmds"][T1 - 1])             # the last step writes no command
            np.testing.assert_array_equal(got, rec["u"] * np.asarray(run["cfg"]["cmd_scale"], F))
            # the inputs exercise what the law has
            raw_u = np.stack([p["raw"] for p in r64.parts], 1)
            if n >= 63:
                axes = slice(0, 3 if track_yaw else 2)            # without yaw tracking the yaw command is only Kp's cross terms
                assert (raw_u < np.asarray(U_MIN)).any(axis=(0, 1))[axes].all() and (raw_u > np.asarray(U_MAX)).any(axis=(0, 1))[axes].all()
                assert dones.any() and not dones.all()
                if track_yaw:
                    arg = np.stack([p["wrap_arg"] for p in r64.parts], 1)
                    assert (arg > np.pi).any() and (arg < -np.pi).any()


def test_the_rows_with_margin_are_counted_on_the_float64_restatement_alone():
    """The 90 % cap is a property of the inputs: counted over all 130 envs without the device."""
    roots, dones, dof, obs, plan = _plan_inputs()
    for track_yaw in (False, True):
        d = _cfg_dict(ref.PLAN, track_yaw, (2, 2, 0.25), 0.02)
        r = ref.CmdTrackRef(d, 130, T1, np.float64, plan=plan)
        r.begin(roots[0])
        for t in range(T1):
            r.step(t, roots[t + 1], dones[t])
        ok = np.stack([_qualify(d, p) for p in r.parts], 1)
        print(f"track_yaw={track_yaw}: {int(ok.sum())} of {ok.size} rows qualify")
        assert ok.mean() >= 0.9


def test_an_envs_outputs_do_not_depend_on_the_number_of_envs():
    a, b = _plan_run(65, True, False), _plan_run(130, True, False)
    for k in ("z", "v", "pz_x", "done", "u", "x"):
        np.testing.assert_array_equal(b["rec"][k][:65].view(np.uint8), a["rec"][k].view(np.uint8), err_msg=k)
    for ca, cb in zip(a["cmds"], b["cmds"]):
        np.testing.assert_array_equal(cb[:65].view(np.uint32), ca.view(np.uint32))


# ------------------------------------------------------------------------------------------------ 2. RANDOM kind
N2, T2, R2 = 65, 40, 32
V_LIM = 0.75


def _random_cfg(h, seed=0):
    lo, hi = float(F(3 * 0.02)), float(F(8 * 0.02))             # hold times of 3..8 steps, float32 values
    gen = dict(rom_v_min=(-V_LIM, -V_LIM), rom_v_max=(V_LIM, V_LIM), t_low=lo, t_high=hi, freq_low=0.01, freq_high=2.0, prob_stationary=0.2,
               tg_N=10, weight_sampler=capi.TG_WEIGHT_SAMPLERS["UniformWeightSamplerNoRamp"])
    cfg = ct.CmdTrackCfg.from_env(h.view, kind=ct.RANDOM, track_yaw=True, Kp=KP, u_min=U_MIN, u_max=U_MAX, seed=seed, **gen)
    d = _cfg_dict(ref.RANDOM, True, cfg.cmd_scale, cfg.rom_dt, N=10, **{k: gen[k] for k in gen if k not in ("tg_N", "weight_sampler")},
                  weight_sampler="UniformWeightSamplerNoRamp")
    return cfg, d


def test_random_kind_on_injected_draws():
    h = _handle(N2)
    roots, dones, dof, obs = _states(N2, T2, seed=31)
    rng = np.random.default_rng(32)
    d_reset = rng.random((N2, capi.RS_NRESET)).astype(F)
    d_res = rng.random((N2, R2, capi.TG_NDRAW)).astype(F)
    d_res[:, :, 4:6] = rng.integers(0, 3, (N2, R2, 2))                               # torch.randint's value as itself
    cfg, d = _random_cfg(h)
    r64, r32 = (ref.CmdTrackRef(d, N2, T2, D, d_reset, d_res) for D in (np.float64, np.float32))
    tr = ct.HipCommandTracker(h.view, cfg)
    nres = []
    try:
        tr.inject(True, R2)
        assert tuple(tr.t["inject"].shape) == (N2, capi.RS_NRESET + R2 * capi.TG_NDRAW)
        tr.t["inject"].copy_(torch.as_tensor(np.concatenate([d_reset, d_res.reshape(N2, -1)], 1)))
        rec, cmds = _drive(h, tr, T2, roots, dones, dof, obs, (r64, r32), after=lambda: nres.append(tr.t["n_resample"].cpu().numpy().copy()))
        tr.inject_status()                                                           # overrun 0: raises otherwise
        assert not tr.t["inject_overrun"].cpu().numpy().any()
    finally:
        tr.close()
    # resample steps identical: the env's count after the begin's pre-roll and after every command
    want = np.stack(r32.nres, 0)                           # after the evaluation of command 0 (the begin), 1, ..., T - 1
    got = np.stack(nres[:T2], 0)
    np.testing.assert_array_equal(want, np.stack(r64.nres))
    assert want.shape == (T2, N2) and len(nres) == T2 + 1
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(nres[T2], nres[T2 - 1])  # the last step evaluates no input
    per_env = want[-1] - want[0]
    print(f"resamples per env over commands 1..{T2 - 1}: {per_env.min()}..{per_env.max()}; by command 0 (the begin's own, its pre-roll): "
          f"{want[0].min()}..{want[0].max()}")
    assert want[0].min() >= 2                                                        # the pre-roll resamples too
    assert per_env.min() >= 4                                                        # every env resamples several times
    all_rows = np.ones((N2, T2), bool)
    _e32("RANDOM v", rec["v"], r64.rec["v"], r32.rec["v"], all_rows)
    _e32("RANDOM z", rec["z"][:, 1:], r64.rec["z"][:, 1:], r32.rec["z"][:, 1:], all_rows)
    ok = np.stack([_qualify(d, p) for p in r64.parts], 1)
    print(f"RANDOM: {int(ok.sum())} of {ok.size} rows qualify")
    _e32("RANDOM u", rec["u"], r64.rec["u"], r32.rec["u"], ok)
    # bounds (a convex sum of inputs inside them: two float32 roundings of slack) and the stationary mask
    assert np.abs(rec["v"]).max() <= V_LIM * (1 + 4 * np.finfo(F).eps)
    still = (r64.rec["v"] == 0).all(axis=2)
    assert still.any() and not still.all()
    assert not rec["v"][still].any()
    np.testing.assert_array_equal(rec["done"], dones.T)


def test_random_kind_without_injection_is_keyed_by_the_seed():
    h = _handle(N2)
    T = 12
    roots, dones, dof, obs = _states(N2, T, seed=41)
    out = []
    for seed in (5, 5, 6):
        cfg, _ = _random_cfg(h, seed=seed)
        tr = ct.HipCommandTracker(h.view, cfg)
        try:
            rec, _ = _drive(h, tr, T, roots, dones, dof, obs, (), other_cols=False, epoch=3)
        finally:
            tr.close()
        out.append(rec)
    for k in ("z", "v", "u"):
        np.testing.assert_array_equal(out[0][k].view(np.uint32), out[1][k].view(np.uint32))
    assert not np.array_equal(out[0]["v"], out[2]["v"])
    assert np.abs(out[0]["v"]).max() <= V_LIM * (1 + 4 * np.finfo(F).eps) and out[0]["v"].any()


# ------------------------------------------------------------------------------------------------ 3. closed loop on the real env
class _Spy:
    """The env with every step's dones and roots kept (device clones: nothing is read back)."""

    def __init__(self, env):
        self.env, self.dones, self.roots = env, [], []

    def __getattr__(self, k):
        return getattr(self.env, k)

    def step(self, a):
        out = self.env.step(a)
        self.dones.append(out[3].clone())
        self.roots.append(self.env.root_states[:, :2].clone())
        return out


def test_closed_loop_on_the_real_env_and_the_pipeline_behind_it(tmp_path):
    """The script on 65 robots with 0.12 s episodes (time-outs inside T = 12); then collect() on its env with a zero-action
    policy: the record identities with the env's own dones; the device dataset equals the host's from the pickle; train_tube runs."""
    import collect_velocity_data as cvd
    import train_tube
    from legged_gym_dev_amd.tube import data as td
    from legged_gym_dev_amd.tube import device_data as dd
    out, T, keep = str(tmp_path / "vel"), 12, {}
    recs = cvd.main(["--task", "anymal_c_flat", "--num_envs", "65", "--headless", "--sim_device", DEV, "--rl_device", DEV, "--epochs", "1",
                     "--out", out, "--steps", str(T), "--episode_length_s", "0.12", "--untrained", "--Kp", "1.5", "--track_yaw"], keep=keep)
    env, tracker = keep["env"], keep["tracker"]
    try:
        with open(os.path.join(out, "epoch_0.pickle"), "rb") as f:
            pk = pickle.load(f)
        assert sorted(pk) == ["done", "pz_x", "v", "z"] and pk["z"].shape == (65, T + 1, 2) and pk["done"].dtype == bool
        for k in pk:
            np.testing.assert_array_equal(pk[k], recs[0][k])
        host = td.ScalarTubeDataset.from_folder(out)
        ds = dd.from_records(td.ScalarTubeDataset, keep["device_records"], device=DEV)
        assert len(host) > 0 and torch.equal(ds.data.cpu(), host.data) and torch.equal(ds.target.cpu(), host.target)
        # ---- collect with a zero-action policy: the identities, with the env's own dones
        spy = _Spy(env)
        zero = torch.zeros(65, env.num_actions, device=env.device)
        rec = ct.collect(spy, lambda o: zero, tracker, 1, T, first_epoch=1, want_u=True)[0]
        dones, roots = torch.stack(spy.dones, 1).cpu().numpy(), torch.stack(spy.roots, 1).cpu().numpy()
        assert dones.any() and not dones.all(axis=0).all()                            # a time-out falls inside T
        np.testing.assert_array_equal(rec["done"], dones)
        np.testing.assert_array_equal(rec["pz_x"][:, 1:], roots)
        np.testing.assert_array_equal(rec["z"][:, 0], rec["pz_x"][:, 0])
        dt = F(env.dt)
        want = rec["z"][:, :-1] + dt * rec["v"]
        want[dones] = roots[dones]                                                    # row t + 1 of a done env restarts at the robot
        np.testing.assert_array_equal(rec["z"][:, 1:].view(np.uint32), want.view(np.uint32))
        assert np.abs(rec["u"]).max() <= 1.0 and rec["v"].any()
        train_tube.main(["--data", out, "--dataset", "scalar", "--num_epochs", "1", "--batch_size", "300", "--out", str(tmp_path / "run"),
                         "--device", DEV, "--steps_per_model_checkpoint", "1000", "--steps_per_model_evaluation", "1000"])
    finally:
        tracker.close()
        env.close()


# ------------------------------------------------------------------------------------------------ 4. track_cmd
def test_track_cmd_returns_tracks_keys_and_audit_takes_them():
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.utils import get_args
    B, Np = 3, 10
    args = get_args(["--task", "anymal_c_flat", "--num_envs", str(B), "--headless"])
    args.sim_device = args.rl_device = DEV
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs("anymal_c_flat"))
    env, _ = task_registry.make_env(name="anymal_c_flat", args=args, env_cfg=env_cfg)
    try:
        train_cfg.runner.resume = False
        runner, _ = task_registry.make_alg_runner(env=env, name="anymal_c_flat", args=args, train_cfg=train_cfg, log_root=None)
        policy = runner.get_inference_policy(device=env.device)                       # freshly initialised: no convergence claim
        g = torch.Generator().manual_seed(1)
        v = torch.rand(B, Np, 2, generator=g) * 0.8 - 0.4
        z0 = torch.tensor([[0.0, 0.0], [1.0, -1.0], [2.0, 0.5]])
        trk = ct.track_cmd(env, policy, z0, v, want=("u", "x", "rec"))
        assert tuple(trk["pz_x"].shape) == (B, Np + 1, 2) and tuple(trk["w_true"].shape) == (B, Np + 1)
        assert tuple(trk["u"].shape) == (B, Np, 3) and tuple(trk["x"].shape) == (B, Np + 1, 37) and trk["pz_x"].is_cuda
        assert trk["completed"].dtype == torch.bool and tuple(trk["rows"].shape) == (B,) and bool((trk["completed"] == ~trk["dead"]).all())
        assert torch.equal(trk["z_ref"][:, 0].cpu(), z0) and torch.equal(trk["pz_x"][:, 0].cpu(), z0) and not trk["w_true"][:, 0].any()
        assert torch.equal(trk["rec"]["v"].cpu(), v) and bool(torch.isfinite(trk["w_true"]).all())
        p = pl.PlanProblem.named("gap", tube_kind="l2", N=Np, H_rev=0)
        res = pl.audit({"w": torch.full((B, Np + 1), 10.0), "min_clear": torch.ones(B)}, trk, p)
        assert res["plans"] == B and res["nodes"] == Np + 1 and res["coverage"] == 1.0
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------ 5. lifetime
def test_either_may_be_destroyed_first_and_a_foreign_env_is_refused():
    """The tracker holds no pointer into the env: each call is handed the env and refuses one of other dimensions; after the
    env is closed a call is refused on the host, and destroying the tracker then, or the env after the tracker, is clean."""
    from legged_gym_dev_amd.envs.base.env_setup import EnvSetup, sim_dt_float
    from legged_gym_dev_amd.lib import LeggedHipError
    from legged_gym_dev_amd.model.robot_model import compile_model, resolve_model

    def mk(n):
        cfg = harness.make_cfg("anymal_c_flat")
        cfg.env.num_envs = n
        h = harness.HipHandle(EnvSetup(cfg, compile_model(resolve_model("", "anymal_c")), sim_dt_float(cfg.sim.dt), seed=1))
        h.call("reset_all")
        h.view = types.SimpleNamespace(core=h.core, setup=h.setup, num_envs=n, num_actions=12, device=DEV, dt=h.setup.dt)
        return h
    a, b = mk(5), mk(7)
    try:
        tr = ct.HipCommandTracker(a.view, ct.CmdTrackCfg.from_env(a.view, kind=ct.PLAN))
        # n_nodes = 0: every input is 0, the ROM stands still at the robot's start
        tr.set_plans(torch.zeros(5, 0, 2))
        a.set("reset", np.zeros(5, np.uint8))                       # reset_all leaves the flags set
        tr.begin(3)
        for t in range(3):
            tr.step(t)
        rec = {k: v.cpu().numpy() for k, v in tr.records().items()}
        assert not rec["v"].any() and not rec["done"].any()
        np.testing.assert_array_equal(rec["z"], np.broadcast_to(rec["z"][:, :1], rec["z"].shape))
        np.testing.assert_array_equal(rec["z"][:, 0], a.get("root_states")[:, :2])
        with pytest.raises(LeggedHipError, match="t = 3 must lie in 0..2"):
            tr.step(3)
        with pytest.raises(LeggedHipError, match="n_nodes = 65"):
            tr.set_plans(torch.zeros(5, 65, 2))
        # an env of other dimensions, handed to the C side directly
        r = tr.struct
        assert tr.lib.lg_cmdtrack_step(tr.ctx, b.core.ctx, C.byref(r), 0) == -1
        assert "not the one the tracker was created for" in tr.lib.lg_last_error().decode()
        # the env goes first
        a.close()
        with pytest.raises(LeggedHipError, match="env is closed"):
            tr.step(0)
        tr.close()
        tr.close()
        # the tracker goes first
        tr2 = ct.HipCommandTracker(b.view, ct.CmdTrackCfg.from_env(b.view, kind=ct.PLAN))
        tr2.begin(2)
        tr2.close()
        b.step(np.zeros((7, 12), F))
        b.sync()
        assert np.isfinite(b.get("obs")).all()
        with pytest.raises(ValueError, match="trajectory env"):
            ct.HipCommandTracker(types.SimpleNamespace(core=b.core, setup=types.SimpleNamespace(traj={}), num_envs=7, num_actions=12,
                                                       device=DEV, dt=b.setup.dt))
    finally:
        for h in (a, b):
            if getattr(h.core, "ctx", None):
                h.close()
