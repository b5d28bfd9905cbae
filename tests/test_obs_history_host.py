"""Host side of the actor's observation history (envs/base/obs_history.py, lg_obs_hist_check, rl/checkpoint.py HistoryPolicy,
the runner's refusals and checkpoint key): the numpy restatement against an independent deque implementation, refusals that name
their field, widths, the TorchScript export and the consumers that refuse an env with a history.  No GPU."""
import collections
import ctypes
import os
import sys
import types

import numpy as np
import pytest
import torch

from legged_gym_dev_amd import capi
from legged_gym_dev_amd.envs.base import cfg_contract as cc
from legged_gym_dev_amd.envs.base import obs_history as oh
from legged_gym_dev_amd.envs.base.env_setup import EnvSetup, sim_dt_float
from legged_gym_dev_amd.model.robot_model import compile_model, resolve_model
from legged_gym_dev_amd.utils.helpers import class_to_dict, get_args, update_cfg_from_args
from tests import harness, obs_history_ref as ref


@pytest.fixture(scope="module")
def lib():
    import torch  # noqa: F401  (shares the HIP runtime instance)
    from legged_gym_dev_amd import lib as L
    if not os.path.isfile(L.SO_PATH):
        L.build()
    return capi.declare_obs_hist_api(ctypes.CDLL(L.SO_PATH))


def _struct(length, ranges=(), reset=0):
    c = capi.lg_obs_hist_cfg()
    c.length, c.num_ranges, c.reset_mode = length, len(ranges), reset
    for k, (lo, hi) in enumerate(list(ranges)[:capi.OBS_HIST_MAX_RANGES]):
        c.lo[k], c.hi[k] = lo, hi
    return c


def _check(lib, c, num_obs):
    """(rc, width, the library's sentence without its prefix)"""
    w = ctypes.c_int32(-7)
    rc = lib.lg_obs_hist_check(ctypes.byref(c), num_obs, ctypes.byref(w))
    msg = lib.lg_last_error().decode() if rc else ""
    assert rc in (0, -1) and (rc == 0 or msg.startswith("lg_obs_hist: "))
    return rc, w.value, msg[len("lg_obs_hist: "):]


def _setup(name):
    z, meta = harness.load_fixture(name)
    return harness.make_setup(name, z, meta)


# ---------------------------------------------------------------- the restatement against per-env deques
def _deque_rows(seq, num_obs, H, ranges, reset):
    """An independent statement of the rule: one deque of past selected frames per env, walked env by env."""
    cols = [c for lo, hi in ranges for c in range(lo, hi)] if ranges else list(range(num_obs))
    n = len(seq[0][0])
    past = [collections.deque(maxlen=H - 1) for _ in range(n)]
    last = [None] * n
    fresh = [True] * n
    out = []
    for obs, rst, marks in seq:
        rows = []
        for i in range(n):
            cur = [obs[i][c] for c in cols]
            if fresh[i] or rst[i] or (marks is not None and marks[i]):
                past[i].clear()
                for _ in range(H - 1):
                    past[i].append(list(cur) if reset == "repeat" else [np.float32(0.0)] * len(cols))
            else:
                past[i].appendleft(last[i])                     # newest first; the oldest falls off the right end
            fresh[i] = False
            last[i] = cur
            rows.append(list(obs[i]) + [v for frame in past[i] for v in frame])
        out.append(np.array(rows, np.float32))
    return out


def _sequence(n, num_obs, steps, seed, resets, marks):
    """Random float32 frames (with a few signed zeros and denormals: copying must keep their bits); resets / marks: {step: envs}."""
    rng = np.random.RandomState(seed)
    seq = []
    for t in range(steps):
        obs = rng.standard_normal((n, num_obs)).astype(np.float32)
        obs[rng.rand(n, num_obs) < 0.05] = np.float32(-0.0)
        obs[rng.rand(n, num_obs) < 0.02] = np.float32(1e-42)
        r = np.zeros(n, np.uint8)
        r[list(resets.get(t, ()))] = 1
        m = None
        if t in marks:
            m = np.zeros(n, np.uint8)
            m[list(marks[t])] = 1
        seq.append((obs, r, m))
    return seq


@pytest.mark.parametrize("reset", ["repeat", "zero"])
@pytest.mark.parametrize("H,ranges", [(2, None), (5, [(0, 7)]), (5, [(0, 3), (9, 12)]), (3, [(4, 5)]), (64, [(2, 4), (10, 11)]), (64, None)])
def test_the_restatement_equals_a_deque_per_env(H, ranges, reset):
    """Synthetic sequences with a reset at step 0, resets at two consecutive steps, a mark and a reset on the same step (on the same
    env and on different ones), a mark alone, and envs that never reset; H = 2 and H = 64; all columns, one range, two ranges and a
    single-column range.  More steps than frames, so that frames fall off the end."""
    n, O = 6, 13
    steps = H + 6 if H < 64 else 70
    resets = {0: [1], 3: [2], 4: [2, 3], 7: [0, 4]}
    marks = {5: [3], 7: [4, 1]}                                  # step 7: env 4 is marked and reset, env 1 marked, env 0 reset
    seq = _sequence(n, O, steps, 100 * H + len(ranges or ()), resets, marks)
    got = ref.restate(seq, O, H, ranges, reset)
    want = _deque_rows(seq, O, H, ranges, reset)
    S = len(ref.columns(O, ranges))
    for t in range(steps):
        assert got[t].shape == (n, O + (H - 1) * S)
        assert np.array_equal(ref.bits(got[t]), ref.bits(want[t])), (t, np.argwhere(ref.bits(got[t]) != ref.bits(want[t]))[:5])
    # env 5 never resets after the first step: once H - 1 steps have passed its oldest frame is the obs of H - 1 steps ago
    cols = ref.columns(O, ranges)
    t = steps - 1
    assert np.array_equal(ref.bits(got[t][5, -S:]), ref.bits(seq[t - (H - 1)][0][5, cols]))


# ---------------------------------------------------------------- lg_obs_hist_check
R9 = [(k, k + 1) for k in range(9)]


@pytest.mark.parametrize("c,num_obs,field", [
    (_struct(1), 48, "length = 1 must lie in 2..64"),
    (_struct(0), 48, "length = 0 must lie in 2..64"),
    (_struct(65), 48, "length = 65 must lie in 2..64"),
    (_struct(3, R9), 48, "num_ranges = 9 must lie in 0..8"),
    (_struct(3, [(5, 5)]), 48, "lo[0] = 5 is not below hi[0] = 5"),
    (_struct(3, [(0, 3), (9, 7)]), 48, "lo[1] = 9 is not below hi[1] = 7"),
    (_struct(3, [(0, 49)]), 48, "hi[0] = 49 exceeds num_obs = 48"),
    (_struct(3, [(0, 10), (9, 12)]), 48, "lo[1] = 9 lies below hi[0] = 10"),               # overlapping
    (_struct(3, [(9, 12), (0, 3)]), 48, "lo[1] = 0 lies below hi[0] = 12"),                # descending
    (_struct(5), 205, "width = num_obs + (length - 1) * selected = 205 + 4 * 205 = 1025 exceeds LG_OBS_HIST_MAX_WIDTH = 1024"),
    (_struct(2, [(0, 1)], reset=2), 48, "reset_mode = 2"),
    (_struct(3, [(-1, 3)]), 48, "lo[0] = -1 is negative"),
])
def test_every_refusal_names_its_field(lib, c, num_obs, field):
    rc, W, msg = _check(lib, c, num_obs)
    assert rc == -1 and W == -7 and field in msg, msg             # the width is left alone on a refusal
    assert oh.refusal(c, num_obs) == msg                          # the sentence ObsHistorySpec.from_cfg raises with


def test_accepted_at_the_limits_and_null_arguments(lib):
    assert _check(lib, _struct(4), 256)[:2] == (0, 1024)                                   # W = 1024
    assert _check(lib, _struct(64, [(47, 48)]), 48)[:2] == (0, 48 + 63)                    # H = 64 with one column
    assert _check(lib, _struct(2, [(k, k + 1) for k in range(0, 16, 2)]), 48)[:2] == (0, 56)      # 8 ranges
    assert _check(lib, _struct(5, [(0, 3), (3, 6)], reset=1), 48)[:2] == (0, 48 + 4 * 6)   # touching ranges do not overlap
    assert lib.lg_obs_hist_check(None, 48, None) == -1 and lib.lg_last_error().decode() == "lg_obs_hist: cfg is null"
    assert lib.lg_obs_hist_check(ctypes.byref(_struct(2)), 48, None) == 0                  # width may be NULL


def test_struct_size_matches_the_header(lib):
    import subprocess
    import tempfile
    src = '#include <stdio.h>\n#include "legged_hip.h"\nint main(){printf("%zu %d %d %d %d %d\\n",sizeof(lg_obs_hist_cfg),' \
          'LG_OBS_HIST_MAX_RANGES,LG_OBS_HIST_MAX_LENGTH,LG_OBS_HIST_MAX_WIDTH,LG_OBS_HIST_REPEAT,LG_OBS_HIST_ZERO);return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(harness.ROOT, "include"), os.path.join(d, "t.c"), "-o", os.path.join(d, "t")])
        out = [int(v) for v in subprocess.check_output([os.path.join(d, "t")]).decode().split()]
    assert out == [ctypes.sizeof(capi.lg_obs_hist_cfg), capi.OBS_HIST_MAX_RANGES, capi.OBS_HIST_MAX_LENGTH, capi.OBS_HIST_MAX_WIDTH,
                   capi.OBS_HIST_RESET.index("repeat"), capi.OBS_HIST_RESET.index("zero")]
    assert ctypes.sizeof(capi.lg_obs_hist_cfg) == 16 + 2 * 4 * capi.OBS_HIST_MAX_RANGES


# ---------------------------------------------------------------- ObsHistorySpec
def test_from_cfg_widths_offsets_and_struct():
    setup, cfg = _setup("anymal_c_flat")
    assert cfg.obs_history.length == 1 and cfg.obs_history.columns is None and cfg.obs_history.reset == "repeat"
    off = oh.ObsHistorySpec.from_cfg(cfg, setup)
    assert not off.enabled and off.width == 48 and off.num_obs == 48
    cfg.obs_history.length = 5
    spec = oh.ObsHistorySpec.from_cfg(cfg, setup)
    assert spec.enabled and spec.width == 240 and spec.num_selected == 48 and spec.frame_offsets() == [0, 48, 96, 144, 192]
    c = spec.to_struct()
    assert (c.length, c.num_ranges, c.reset_mode) == (5, 0, 0)
    setup, cfg = _setup("anymal_c_rough")
    cfg.obs_history.length, cfg.obs_history.columns, cfg.obs_history.reset = 5, [[0, 48]], "zero"
    spec = oh.ObsHistorySpec.from_cfg(cfg, setup)
    assert spec.width == 427 and spec.num_selected == 48 and spec.frame_offsets() == [0, 235, 283, 331, 379]
    c = spec.to_struct()
    assert (c.length, c.num_ranges, c.reset_mode, c.lo[0], c.hi[0]) == (5, 1, 1, 0, 48)
    cfg.obs_history.columns = [[0, 3], [9, 12], [36, 48]]
    spec = oh.ObsHistorySpec.from_cfg(cfg, setup)
    assert spec.columns() == [0, 1, 2, 9, 10, 11] + list(range(36, 48)) and spec.width == 235 + 4 * 18
    assert oh.ObsHistorySpec.from_dict(spec.as_dict()) == spec and spec.same_row(oh.ObsHistorySpec.from_dict(spec.as_dict()))
    assert oh.ObsHistorySpec.from_dict(None).enabled is False


def test_from_cfg_refuses_in_the_cfgs_words():
    setup, cfg = _setup("anymal_c_flat")
    for length, cols, reset, word in ((65, None, "repeat", "length = 65"), (0, None, "repeat", "length = 0"),
                                      (3, [[0, 49]], "repeat", "hi\\[0\\] = 49"), (3, [[3, 3]], "zero", "lo\\[0\\] = 3"),
                                      (3, [[k, k + 1] for k in range(9)], "repeat", "num_ranges = 9"),
                                      (22, None, "repeat", "width = .* 1056 exceeds"), (3, None, "last", "reset = 'last'"),
                                      (3, [5], "repeat", "columns")):
        cfg.obs_history.length, cfg.obs_history.columns, cfg.obs_history.reset = length, cols, reset
        with pytest.raises(ValueError, match="cfg.obs_history.*" + word):
            oh.ObsHistorySpec.from_cfg(cfg, setup)


def test_a_reference_style_cfg_without_the_section_is_off_and_the_flags_make_it():
    full = harness.make_cfg("anymal_c_flat")
    cfg = types.SimpleNamespace(**{k: getattr(full, k) for k in dir(full)
                                   if not k.startswith("_") and k != "obs_history" and not callable(getattr(full, k))})
    assert not hasattr(cfg, "obs_history")
    cm = compile_model(resolve_model("", "anymal_c"))
    setup = EnvSetup(cfg, cm, sim_dt_float(cfg.sim.dt))           # the contract walk accepts the tree without the section
    spec = oh.ObsHistorySpec.from_cfg(cfg, setup)
    assert not spec.enabled and spec.width == 48
    args = get_args(["--task", "anymal_c_flat", "--obs_history", "4", "--obs_history_columns", "0:3,9:12", "--obs_history_reset", "zero"])
    update_cfg_from_args(cfg, None, args)
    spec = oh.ObsHistorySpec.from_cfg(cfg, setup)
    assert (spec.length, spec.ranges, spec.reset, spec.width) == (4, ((0, 3), (9, 12)), "zero", 48 + 3 * 6)
    cc.enforce(cfg)


def test_arguments_reach_the_cfg_and_the_contract_knows_the_section():
    from legged_gym_dev_amd.envs.base.legged_robot_config import LeggedRobotCfg
    from legged_gym_dev_amd.envs.base.legged_robot_trajectory_config import LeggedRobotTrajectoryCfg
    cfg = harness.make_cfg("anymal_c_flat")
    update_cfg_from_args(cfg, None, get_args(["--task", "anymal_c_flat"]))
    assert cfg.obs_history.length == 1
    update_cfg_from_args(cfg, None, get_args(["--task", "anymal_c_flat", "--obs_history", "5"]))
    assert (cfg.obs_history.length, cfg.obs_history.columns, cfg.obs_history.reset) == (5, None, "repeat")
    update_cfg_from_args(cfg, None, get_args(["--task", "anymal_c_flat", "--obs_history_columns", "0:48"]))
    assert (cfg.obs_history.length, cfg.obs_history.columns) == (5, [[0, 48]])
    with pytest.raises(ValueError, match="lo:hi"):
        oh.parse_columns("0-48")
    for cls in (LeggedRobotCfg, LeggedRobotTrajectoryCfg):
        paths = [p for p, _ in cc.leaves(class_to_dict(cls())) if p.startswith("obs_history.")]
        assert sorted(paths) == ["obs_history.columns", "obs_history.length", "obs_history.reset"]
        for p in paths:
            row = cc.lookup(p)
            assert row is not None and row[1] == cc.CONSUMED and row[2].startswith("env:"), p


def test_base_task_widths():
    from legged_gym_dev_amd.envs.base.base_task import BaseTask
    _, cfg = _setup("anymal_c_flat")
    b = BaseTask(cfg, None, None, "cuda:0", True)
    assert b.num_actor_obs == b.num_obs == 48
    b.obs_buf = object()
    assert b.get_actor_observations() is b.obs_buf is b.get_observations()


# ---------------------------------------------------------------- export
def _actor_sd(W, seed=0):
    torch.manual_seed(seed)
    dims = [W, 32, 16, 12]
    sd = {"std": torch.ones(12)}
    for l in range(3):
        lin = torch.nn.Linear(dims[l], dims[l + 1])
        sd[f"actor.{2 * l}.weight"], sd[f"actor.{2 * l}.bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return sd


class _Facade:
    activation = "elu"

    def __init__(self, sd):
        self._sd = sd

    def state_dict(self):
        return self._sd


@pytest.mark.parametrize("H,ranges,reset", [(3, (), "repeat"), (4, ((0, 3), (9, 12)), "zero"), (2, ((5, 6),), "repeat")])
def test_exported_history_policy_equals_hand_stacked_rows(H, ranges, reset, tmp_path):
    """policy_hist_1.pt: 12 calls with a reset_memory() after call 5 equal the rows stacked by the restatement, through build_mlp."""
    from legged_gym_dev_amd.rl.checkpoint import build_mlp, export_policy_as_jit
    O = 20
    spec = oh.ObsHistorySpec(H, ranges, reset, O)
    sd = _actor_sd(spec.width)
    path = export_policy_as_jit(_Facade(sd), str(tmp_path), obs_history=spec)
    assert os.path.basename(path) == "policy_hist_1.pt"
    mod = torch.jit.load(path)
    assert tuple(mod.history.shape) == (1, spec.width)
    mlp = build_mlp(sd, "actor", "elu")
    hand = ref.HistoryRef(1, O, H, ranges or None, reset)
    g = torch.Generator().manual_seed(4)
    with torch.no_grad():
        for call in range(12):
            if call == 5:
                mod.reset_memory()
            obs = torch.randn(1, O, generator=g)
            row = hand.step(obs.numpy(), [0], [call == 5])
            got = mod(obs)
            assert torch.equal(mod.history, torch.from_numpy(row)), call
            assert torch.equal(got, mlp(torch.from_numpy(row))), call
    past, cur = hand.frames()
    assert not np.array_equal(past[0, 0], cur[0])               # the rows moved: the last call was no reinitialisation


def test_export_without_a_spec_is_unchanged(tmp_path):
    from legged_gym_dev_amd.rl.checkpoint import export_policy_as_jit
    sd = _actor_sd(48)
    assert os.path.basename(export_policy_as_jit(_Facade(sd), str(tmp_path))) == "policy_1.pt"
    assert os.path.basename(export_policy_as_jit(_Facade(sd), str(tmp_path), obs_history=oh.ObsHistorySpec(1, (), "repeat", 48))) == "policy_1.pt"
    with pytest.raises(ValueError, match="actor takes 48 columns"):
        export_policy_as_jit(_Facade(sd), str(tmp_path), obs_history=oh.ObsHistorySpec(3, (), "repeat", 48))


# ---------------------------------------------------------------- runner: refusals and the checkpoint key
class _FakePPO:
    def __init__(self):
        self.loaded = None

    def state_dict(self):
        return {"std": torch.ones(3)}

    def optimizer_state_dict(self):
        return {}

    def load_state_dict(self, sd):
        self.loaded = sd


def _bare_runner(spec):
    from legged_gym_dev_amd.rl.runner import OnPolicyRunner
    r = OnPolicyRunner.__new__(OnPolicyRunner)
    r.ppo, r.obs_history_spec, r.current_learning_iteration = _FakePPO(), spec, 7
    return r


def test_checkpoint_carries_the_spec_and_a_mismatch_is_named(tmp_path):
    a = oh.ObsHistorySpec(5, ((0, 48),), "zero", 235)
    b = oh.ObsHistorySpec(5, ((0, 48),), "repeat", 235)
    with_key, without = str(tmp_path / "a" / "model_7.pt"), str(tmp_path / "b" / "model_7.pt")
    _bare_runner(a).save(with_key)
    _bare_runner(None).save(without)
    d = torch.load(with_key, map_location="cpu", weights_only=True)
    assert d["obs_history"] == {"length": 5, "ranges": [[0, 48]], "reset": "zero", "num_obs": 235}
    assert set(d) == {"model_state_dict", "optimizer_state_dict", "iter", "infos", "obs_history"}
    assert set(torch.load(without, map_location="cpu", weights_only=True)) == {"model_state_dict", "optimizer_state_dict", "iter", "infos"}
    # same spec and no spec at all load
    r = _bare_runner(a)
    r.load(with_key)
    assert r.ppo.loaded is not None and r.current_learning_iteration == 7
    r = _bare_runner(None)
    r.load(without)
    assert r.ppo.loaded is not None
    # each mismatch names both specs and loads nothing
    for runner_spec, path, words in ((b, with_key, ("reset zero", "reset repeat")), (None, with_key, ("length 5, columns 0:48", "no history")),
                                     (a, without, ("no history", "length 5, columns 0:48, reset zero"))):
        r = _bare_runner(runner_spec)
        with pytest.raises(ValueError) as e:
            r.load(path)
        assert all(w in str(e.value) for w in words) and "cfg.obs_history" in str(e.value), str(e.value)
        assert r.ppo.loaded is None


def _fake_env(spec, num_priv=None):
    return types.SimpleNamespace(num_envs=8, num_obs=spec.num_obs, num_actor_obs=spec.width, num_privileged_obs=num_priv, num_actions=12,
                                 device="cuda:0", obs_history_spec=spec, setup=types.SimpleNamespace(traj=None),
                                 get_privileged_observations=lambda: (object() if num_priv else None))


def _train_cfg(policy_class):
    return {"runner": {"num_steps_per_env": 4, "save_interval": 50, "policy_class_name": policy_class}, "algorithm": {}, "policy": {}}


def test_runner_refuses_a_history_with_a_memory_and_a_critic_as_wide_as_the_actor():
    from legged_gym_dev_amd.rl.runner import OnPolicyRunner
    spec = oh.ObsHistorySpec(3, ((0, 6),), "repeat", 48)         # W = 60
    with pytest.raises(ValueError, match="cfg.obs_history.*ActorCriticRecurrent.*in front of a memory"):
        OnPolicyRunner(_fake_env(spec), _train_cfg("ActorCriticRecurrent"), None, device="cuda:0")
    with pytest.raises(ValueError, match="as wide as the policy's \\(60 columns\\)"):
        OnPolicyRunner(_fake_env(spec, num_priv=60), _train_cfg("ActorCritic"), None, device="cuda:0")


def test_the_learner_refuses_a_row_of_another_width_before_any_device_call():
    """obs_buf (48 columns) handed to a learner built on the history row (144): act, act_inference and compute_returns raise
    before they reach the library, which would read 144 floats per row from the pointer."""
    from legged_gym_dev_amd.rl.ppo import HipPPO, check_width

    class NoLibrary:
        def __getattr__(self, name):
            raise AssertionError(f"the library was reached: {name}")

    p = HipPPO.__new__(HipPPO)
    p.O, p.OC, p.A, p.privileged, p.lib, p.ctx, p.device = 144, 48, 12, True, NoLibrary(), None, "cpu"
    with pytest.raises(ValueError, match="act_inference: obs has shape \\(8, 48\\).*144 columns.*get_actor_observations"):
        p.act_inference(torch.zeros(8, 48))
    with pytest.raises(ValueError, match="act: obs has shape \\(8, 48\\).*144 columns"):
        p.act(torch.zeros(8, 48), torch.zeros(8, 48))
    with pytest.raises(ValueError, match="act: critic_obs has shape \\(8, 144\\).*48 columns"):
        p.act(torch.zeros(8, 144), torch.zeros(8, 144))
    with pytest.raises(ValueError, match="compute_returns: last_critic_obs has shape \\(8, 144\\).*48 columns"):
        p.compute_returns(torch.zeros(8, 144))
    check_width(torch.zeros(8, 144), 144, "obs")
    check_width(None, 144, "critic_obs")
    p.ctx = None                                                  # nothing for __del__ / close() to free


def test_the_tracker_and_the_plan_env_drivers_refuse_a_history():
    from legged_gym_dev_amd.tube import cmd_track, plan_env
    env = _fake_env(oh.ObsHistorySpec(3, (), "repeat", 48))
    with pytest.raises(ValueError, match="HipCommandTracker.*cfg.obs_history"):
        cmd_track.HipCommandTracker(env)
    with pytest.raises(ValueError, match="track_env.*cfg.obs_history"):
        plan_env.check_track(env, torch.zeros(8, 4, 2), torch.zeros(8, 2))
    with pytest.raises(ValueError, match="closed_loop_env.*cfg.obs_history"):
        plan_env.check_closed_loop(env, None, 3)
    sys.path.insert(0, os.path.join(harness.ROOT, "legged_gym_dev_amd", "scripts"))
    import collect_trajectory_data as ctd
    with pytest.raises(ValueError, match="collect_trajectory_data.collect.*cfg.obs_history"):
        ctd.collect(env, lambda o: o, 1)
    # an env without a history passes on to the drivers' own checks
    off = _fake_env(oh.ObsHistorySpec(1, (), "repeat", 48))
    with pytest.raises(ValueError, match="PlanTrajectoryGenerator"):
        plan_env.check_track(off, torch.zeros(8, 4, 2), torch.zeros(8, 2))
