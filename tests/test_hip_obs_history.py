"""GPU: the actor's observation history (csrc/obshist_kernels.hip through envs/base/obs_history.py, the env and the runner) against
its numpy restatement (tests/obs_history_ref.py) bit for bit, at env counts either side of the 16-env tile; the env it reads is
left exactly as it was; reset_idx on a subset; the view's lifetime; the product runner feeds the row to the actor and the single
frame to the critic; a wide actor beside a narrow critic against float64 (the yardstick of tests/ppo_act_ref.py); inference and
play on the row.

lg_ppo_debug_get_fused_act for the widths used here (printed by the tests): 1 -- the one-launch act takes O = 240 / OC = 48,
O = 144 / OC = 48 and O = 144 / OC = 49 with [512, 256, 128] (240 and 144 are whole 16-column k-steps below the 512-column image)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

from tests import harness, obs_history_ref as ref
from tests import ppo_act_ref as ar

pytestmark = pytest.mark.gpu

READ = ["root_states", "dof_state", "contact_forces", "torques", "actions", "commands", "trajectory", "base_lin_vel", "base_ang_vel",
        "projected_gravity", "measured_heights", "friction", "base_mass_delta", "material", "feet_air_time", "episode_length", "obs",
        "reset"]                                             # the READ list of tests/test_hip_priv_obs.py
TASKS = ["anymal_c_flat", "anymal_c_rough", "anymal_c_flat_trajectory"]
CONFIGS = [(2, None, "repeat"), (5, [[0, 48]], "zero"), (5, [[0, 3], [9, 12], [36, 48]], "repeat")]


def _args(task, n, extra=()):
    from legged_gym_dev_amd.utils import get_args
    a = get_args(["--task", task, "--num_envs", str(n), "--headless", *extra])
    a.sim_device = a.rl_device = "cuda:0"
    return a


def _cfgs(task, n):
    from legged_gym_dev_amd.envs import task_registry
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(task))
    env_cfg.env.num_envs = n
    if env_cfg.terrain.mesh_type in ("heightfield", "trimesh"):
        harness._small_terrain(env_cfg)
    return env_cfg, train_cfg


def _make(task, n, H=1, columns=None, reset="repeat", terms=(), env_cfg=None):
    from legged_gym_dev_amd.envs import task_registry
    if env_cfg is None:
        env_cfg, _ = _cfgs(task, n)
    env_cfg.obs_history.length, env_cfg.obs_history.columns, env_cfg.obs_history.reset = H, columns, reset
    env_cfg.privileged_obs.terms = list(terms)
    env, _ = task_registry.make_env(name=task, args=_args(task, n), env_cfg=env_cfg)
    return env


def _host(env, keys=READ):
    torch.cuda.synchronize()
    return {k: env.core.t[k].cpu().numpy() for k in keys}


def _actions(env, steps, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(steps, env.num_envs, env.num_actions, generator=g) * 2.0 - 1.0).to(env.device)


def _preset_clocks(env, n):
    ep = torch.arange(n, device=env.device) * 7 % 50
    ep[0::3] = int(env.max_episode_length) - 2                # ep > max at the third step from here
    ep[1::3] = int(env.max_episode_length) - 3                # ... at the fourth
    env.episode_length_buf = ep


def _ref_of(env):
    s = env.obs_history_spec
    return ref.HistoryRef(env.num_envs, s.num_obs, s.length, s.ranges or None, s.reset)


def _same(got, want, what):
    bad = ref.bits(got) != ref.bits(want)
    assert not bad.any(), (what, [(int(i), int(j), got[i, j], want[i, j]) for i, j in np.argwhere(bad)[:5]])


# ---------------------------------------------------------------- 1. the row equals the restatement
@pytest.mark.parametrize("cfg", CONFIGS, ids=["H2-all-repeat", "H5-0:48-zero", "H5-three-ranges-repeat"])
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
@pytest.mark.parametrize("task", TASKS)
def test_the_row_equals_the_restatement_after_every_step(task, n, cfg):
    """Seeded random actions, noise on, episode clocks preset so that envs time out at steps 3 and 4: after env.reset() and after
    each of 30 steps the row equals the restatement of the recorded obs and reset bit for bit.  The test's own conditions: a reset
    fell inside the compared steps; an env reset on a step where another did not (n > 1); every env has a step without a reset
    where past frame 1 differs in bits from the current selected block (a shift by the wrong count cannot pass); a reset env's
    past frames equal its current block under repeat and are all zero under zero."""
    H, columns, reset = cfg
    env = _make(task, n, H, columns, reset)
    try:
        spec = env.obs_history_spec
        O, S, W = spec.num_obs, spec.num_selected, spec.width
        assert env.num_actor_obs == W == O + (H - 1) * S and env.num_obs == O
        row = env.get_actor_observations()
        assert row is env.actor_obs_buf and tuple(row.shape) == (n, W) and env.get_observations() is env.obs_buf
        assert tuple(env.obs_buf.shape) == (n, O)
        env.reset()
        _preset_clocks(env, n)
        hist = _ref_of(env)
        t = _host(env, ("obs", "reset"))
        _same(row.cpu().numpy(), hist.step(t["obs"], t["reset"], np.ones(n, bool)), "after reset()")      # reset_idx marked every env
        acts = _actions(env, 30, 29 + n)
        cols = np.array(spec.columns())
        seen = {"reset": 0, "reset_steps": set(), "mixed": 0}
        moved = np.zeros(n, bool)
        for s in range(30):
            out = env.step(acts[s])
            assert out[0] is env.obs_buf and env.get_actor_observations() is row
            t = _host(env, ("obs", "reset"))
            got = row.cpu().numpy()
            _same(got, hist.step(t["obs"], t["reset"]), (task, n, s))
            rs = t["reset"].astype(bool)
            past = got[:, O:].reshape(n, H - 1, S)
            cur = got[:, :O][:, cols]
            assert np.array_equal(ref.bits(got[:, :O]), ref.bits(t["obs"]))
            if rs.any():
                seen["reset"] += int(rs.sum())
                seen["reset_steps"].add(s)
                seen["mixed"] += int(not rs.all())
                want = np.repeat(cur[rs][:, None, :], H - 1, 1) if reset == "repeat" else np.zeros((int(rs.sum()), H - 1, S), np.float32)
                assert np.array_equal(ref.bits(past[rs]), ref.bits(want)), (task, n, s)
            moved |= ~rs & (ref.bits(past[:, 0]) != ref.bits(cur)).any(1)
        print(f"{task} n={n} H={H}: W={W} {seen}")
        assert seen["reset"] > 0 and 2 in seen["reset_steps"] and (n < 2 or 3 in seen["reset_steps"]), seen
        assert n < 2 or seen["mixed"] > 0, seen
        assert moved.all(), np.flatnonzero(~moved)
    finally:
        env.close()


# ---------------------------------------------------------------- 2. the env is untouched
def test_compute_leaves_every_env_buffer_as_it_was():
    """compute() once more on a stepped env: every buffer of the privileged test's READ list is identical before and after, and
    so is the privileged row configured beside the history."""
    env = _make("anymal_c_rough", 33, 5, [[0, 48]], "repeat", terms=("obs", "friction", "heights"))
    try:
        env.reset()
        _preset_clocks(env, 33)
        acts = _actions(env, 4, 3)
        for s in range(4):
            env.step(acts[s])
        before, priv = _host(env), env.privileged_obs_buf.clone()
        row = env.actor_obs_buf.clone()
        env._hist.compute()
        after = _host(env)
        for k in READ:
            assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
        assert torch.equal(priv.view(torch.int32), env.privileged_obs_buf.view(torch.int32))
        assert not torch.equal(row, env.actor_obs_buf)         # and it did run: the rows moved on by one frame
    finally:
        env.close()


def test_the_privileged_row_and_the_env_are_the_same_with_and_without_the_history():
    outs = []
    for H in (1, 3):
        env = _make("anymal_c_flat", 33, H, None, "repeat", terms=("obs", "friction", "feet_contact"))
        try:
            assert (env._hist is not None) == (H > 1) and env.num_actor_obs == 48 * H
            env.reset()
            _preset_clocks(env, 33)
            acts = _actions(env, 8, 11)
            resets = 0
            for s in range(8):
                env.step(acts[s])
                resets += int(env.reset_buf.sum())
            torch.cuda.synchronize()
            assert resets > 0
            outs.append(({k: v.clone() for k, v in env.core.t.items()}, env.privileged_obs_buf.clone()))
        finally:
            env.close()
    (a, pa_), (b, pb) = outs
    assert set(a) == set(b) and len(a) > 40
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(pa_.view(torch.int32), pb.view(torch.int32))


# ---------------------------------------------------------------- 3. reset_idx on a subset
def test_reset_idx_on_a_subset_reinitialises_exactly_those_envs_at_the_next_step():
    n, ids = 33, [0, 15, 16, 32]
    env = _make("anymal_c_flat", n, 4, [[0, 12], [36, 48]], "repeat")
    try:
        spec = env.obs_history_spec
        O, S, H = spec.num_obs, spec.num_selected, spec.length
        cols = np.array(spec.columns())
        env.reset()
        hist = _ref_of(env)
        t = _host(env, ("obs", "reset"))
        hist.step(t["obs"], t["reset"], np.ones(n, bool))
        acts = _actions(env, 6, 8)
        for s in range(5):
            env.step(acts[s])
            t = _host(env, ("obs", "reset"))
            want = hist.step(t["obs"], t["reset"])
        before = env.actor_obs_buf.cpu().numpy()
        _same(before, want, "before reset_idx")
        env.reset_idx(torch.tensor(ids, device=env.device))
        torch.cuda.synchronize()
        _same(env.actor_obs_buf.cpu().numpy(), before, "reset_idx itself touches nothing")
        env.step(acts[5])
        t = _host(env, ("obs", "reset"))
        marks = np.zeros(n, bool)
        marks[ids] = True
        got = env.actor_obs_buf.cpu().numpy()
        _same(got, hist.step(t["obs"], t["reset"], marks), "the step after reset_idx")
        assert not t["reset"].any()                            # the step itself reset nobody: the marks alone did it
        past, cur = got[:, O:].reshape(n, H - 1, S), got[:, :O][:, cols]
        old_past, old_cur = before[:, O:].reshape(n, H - 1, S), before[:, :O][:, cols]
        rest = ~marks
        assert np.array_equal(ref.bits(past[marks]), ref.bits(np.repeat(cur[marks][:, None, :], H - 1, 1)))
        assert np.array_equal(ref.bits(past[rest, 0]), ref.bits(old_cur[rest])) and np.array_equal(ref.bits(past[rest, 1:]), ref.bits(old_past[rest, :-1]))
        assert (ref.bits(past[rest, 0]) != ref.bits(cur[rest])).any(1).all()
        # the marks lapsed with that compute: the next step shifts everyone
        env.step(acts[0])
        t = _host(env, ("obs", "reset"))
        _same(env.actor_obs_buf.cpu().numpy(), hist.step(t["obs"], t["reset"]), "the second step after reset_idx")
        env.reset()
        torch.cuda.synchronize()
        got = env.actor_obs_buf.cpu().numpy()
        past, cur = got[:, O:].reshape(n, H - 1, S), got[:, :O][:, cols]
        assert np.array_equal(ref.bits(past), ref.bits(np.repeat(cur[:, None, :], H - 1, 1)))
        assert np.array_equal(ref.bits(got[:, :O]), ref.bits(env.obs_buf.cpu().numpy())) and np.abs(cur).sum() > 0
    finally:
        env.close()


# ---------------------------------------------------------------- 4. lifetime
def test_buffer_lifetime():
    """Zeros before the first step; the same storage after every step; post_physics_step refreshes it too; closing the env and
    the handle in either order; a compute() after the core was closed is refused."""
    from legged_gym_dev_amd.lib import LeggedHipError
    for handle_first in (True, False):
        env = _make("anymal_c_flat", 17, 3, None, "zero")
        view = env.actor_obs_buf
        ptr = view.data_ptr()
        assert tuple(view.shape) == (17, 144) and view.dtype == torch.float32 and not bool(view.any())
        assert env.get_actor_observations() is view and env.num_actor_obs == 144 and env.num_obs == 48
        obs, priv = env.reset()
        assert obs is env.obs_buf and priv is None and bool(view[:, :48].any()) and not bool(view[:, 48:].any())
        for _ in range(3):
            env.step(torch.zeros(17, 12, device=env.device))
            assert env.get_actor_observations() is view and view.data_ptr() == ptr
        torch.cuda.synchronize()
        before = view.clone()
        env.post_physics_step()                               # the other entry that advances the row
        torch.cuda.synchronize()
        kept = ~env.reset_buf                                 # per env: those the call did not reset moved on by one frame
        assert bool(kept.any()) and torch.equal(view[kept, 48:96].view(torch.int32), before[kept, :48].view(torch.int32))
        assert torch.equal(view[:, :48].view(torch.int32), env.obs_buf.view(torch.int32)) and not bool(view[~kept, 48:].any())
        handle = env._hist
        if handle_first:
            handle.close()
            handle.close()
            env.close()
        else:
            env.close()
            with pytest.raises(LeggedHipError, match="closed"):
                handle.compute()
            with pytest.raises(LeggedHipError, match="closed"):
                handle.mark()
            handle.close()
        assert handle.ctx is None and handle.buf is None and env.get_actor_observations() is None


def test_a_refused_compute_leaves_row_and_marks_alone():
    """A mark holds until the next successful compute: a compute handed an env of other dimensions is refused, changes nothing,
    and the step after it still reinitialises the marked env and no other."""
    env, other = _make("anymal_c_flat", 17, 3, None, "repeat"), _make("anymal_c_flat", 4)
    try:
        env.reset()
        acts = _actions(env, 4, 6)
        for s in range(3):
            env.step(acts[s])
        env.reset_idx(torch.tensor([3], device=env.device))
        torch.cuda.synchronize()
        before = env.actor_obs_buf.clone()
        h = env._hist
        assert h.lib.lg_obs_hist_compute(h.ctx, other.core.ctx) == -1 and b"not the one the handle was created for" in h.lib.lg_last_error()
        assert h.lib.lg_obs_hist_mark(h.ctx, other.core.ctx, None, 0) == -1
        torch.cuda.synchronize()
        assert torch.equal(env.actor_obs_buf.view(torch.int32), before.view(torch.int32))
        env.step(acts[3])
        torch.cuda.synchronize()
        assert not bool(env.reset_buf.any())
        row = env.actor_obs_buf
        same = (row[:, 48:96].view(torch.int32) == row[:, :48].view(torch.int32)).all(1) & \
               (row[:, 96:].view(torch.int32) == row[:, :48].view(torch.int32)).all(1)
        assert same.tolist() == [i == 3 for i in range(17)]
        rest = [i for i in range(17) if i != 3]
        assert torch.equal(row[rest, 48:96].view(torch.int32), before[rest, :48].view(torch.int32))
    finally:
        env.close()
        other.close()


def test_a_bad_section_is_refused_before_any_device_work():
    env_cfg, _ = _cfgs("anymal_c_flat", 4)
    with pytest.raises(ValueError, match="cfg.obs_history: hi\\[0\\] = 49 exceeds num_obs = 48"):
        _make("anymal_c_flat", 4, 3, [[0, 49]], env_cfg=env_cfg)


# ---------------------------------------------------------------- 5. the product runner
def _runner(H, terms=(), steps=6, n=64):
    from legged_gym_dev_amd.rl.runner import OnPolicyRunner
    from legged_gym_dev_amd.utils.helpers import class_to_dict
    env_cfg, train_cfg = _cfgs("anymal_c_flat", n)
    env = _make("anymal_c_flat", n, H, None, "repeat", terms=terms, env_cfg=env_cfg)
    train_cfg.runner.num_steps_per_env = steps
    train_cfg.policy.actor_hidden_dims = train_cfg.policy.critic_hidden_dims = [512, 256, 128]
    torch.manual_seed(9)
    runner = OnPolicyRunner(env, class_to_dict(train_cfg), None, device="cuda:0")
    _preset_clocks(env, n)                                    # after the runner's own reset(): resets fall inside the rollout
    return env, runner


@pytest.mark.parametrize("terms", [(), ("obs", "friction")], ids=["critic-obs", "critic-privileged"])
def test_the_runner_feeds_the_row_to_the_actor_and_the_single_frame_to_the_critic(terms, monkeypatch):
    """anymal_c_flat, 64 envs, 6 steps per rollout, H = 3 (W = 144), with LG_FUSE_EPILOGUE at 1 and at 0.  Row t of the learner's obs
    storage is the row an identically seeded twin env shows at step t when stepped by hand with the stored actions, and row t of
    its critic_obs storage is the twin's obs_buf (or, with --privileged_obs obs,friction, its 49-column privileged row); the two
    settings agree; one update() gives finite losses and moves the (512, W) first layer of the actor."""
    W, OC = 144, 49 if terms else 48
    stores = []
    for fuse in ("1", "0"):
        monkeypatch.setenv("LG_FUSE_EPILOGUE", fuse)
        env, runner = _runner(3, terms)
        twin = _make("anymal_c_flat", 64, 3, None, "repeat", terms=terms)
        try:
            ppo = runner.ppo
            assert runner.fuse_epilogue == (fuse == "1")
            assert ppo.O == W == env.num_actor_obs and ppo.OC == OC and ppo.privileged and not ppo.is_recurrent
            print(f"O={ppo.O} OC={ppo.OC}: lg_ppo_debug_get_fused_act = {ppo.lib.lg_ppo_debug_get_fused_act(ppo.ctx)}")
            twin.reset()
            _preset_clocks(twin, 64)
            runner.rollout()
            torch.cuda.synchronize()
            obs, cobs, acts = ppo.t["obs"].clone(), ppo.t["critic_obs"].clone(), ppo.t["actions"].clone()
            assert tuple(obs.shape) == (6, 64, W) and tuple(cobs.shape) == (6, 64, OC)
            for t in range(6):
                assert torch.equal(obs[t].view(torch.int32), twin.actor_obs_buf.view(torch.int32)), t
                critic = twin.privileged_obs_buf if terms else twin.obs_buf
                assert torch.equal(cobs[t].view(torch.int32), critic.view(torch.int32)), t
                twin.step(acts[t])
            dones = ppo.t["dones"].clone()
            assert int(dones[:-1].sum()) > 0 and not bool(dones.all())          # resets fell inside, and their rows were compared
            assert not torch.equal(obs[1, :, 48:96], obs[1, :, :48])            # the rows are no copies of one frame
            stores.append({k: ppo.t[k].clone() for k in ("obs", "critic_obs", "values", "actions", "returns", "rewards", "dones")})
            w0 = ppo.param_views["actor.0.weight"].clone()
            assert tuple(w0.shape) == (512, W)
            vloss, sloss = ppo.update(None)
            torch.cuda.synchronize()
            assert bool(torch.isfinite(vloss)) and bool(torch.isfinite(sloss))
            w1 = ppo.param_views["actor.0.weight"]
            assert bool(torch.isfinite(w1).all()) and not torch.equal(w0, w1)
            assert bool((w0[:, 48:] != w1[:, 48:]).any())                       # the past frames' columns learn too
        finally:
            twin.close()
            env.close()
            runner.ppo.close()
    for k, v in stores[0].items():
        assert torch.equal(v, stores[1][k]), k


# ---------------------------------------------------------------- 6. wide actor, narrow critic
@pytest.mark.parametrize("rows", [17, 64])
def test_act_with_a_wide_actor_and_a_narrow_critic_matches_float64(rows):
    """lg_ppo_act at O = 240, OC = 48, [512, 256, 128]: mu and value against float64 with the checks and bounds of the rollout's
    own act tests (tests/ppo_act_ref.py through the helpers of tests/test_hip_ppo_act.py: structural bound, E_k <= M E_y + 2^-24),
    on the one-launch path and on the per-layer one."""
    from tests import test_hip_ppo_act as pa
    c = ar._case("512-256-128/o240-oc48", 240, 48, [512, 256, 128], [512, 256, 128], rows, 12, "elu")
    assert c["fused"] == ar.supported(ar.case_dims(c))
    inp = ar.build_inputs(c, "rand")
    refs = [pa._reference(c, inp, call) for call in inp["calls"]]
    hip = pa._learner(c)
    try:
        assert hip.O == 240 and hip.OC == 48 and hip.privileged
        print(f"O=240 OC=48: lg_ppo_debug_get_fused_act = {hip.lib.lg_ppo_debug_get_fused_act(hip.ctx)}")
        pa._write(hip, inp["params"])
        hip.inject_noise(1)
        for fused in (1, 0):
            path = pa._set_path(hip, c, fused)
            for t, call in enumerate(inp["calls"]):
                hip.t["noise"].copy_(call["noise"].to(pa.DEV))
                got = pa._act(hip, c, call)
                pa._check_heads(c, "rand", refs[t], got, f"o240-oc48 rows {rows} {path} call {t}")
                pa._idle_step(hip, rows)
            torch.cuda.synchronize()
            for t, call in enumerate(inp["calls"]):
                assert torch.equal(hip.t["obs"][t].cpu(), call["obs"]) and torch.equal(hip.t["critic_obs"][t].cpu(), call["cobs"])
            hip._call("end_update")
    finally:
        hip.close()


# ---------------------------------------------------------------- 7. inference and play
def test_inference_on_the_history_row_matches_the_actor_mlp():
    """lg_ppo_act_inference on the env's history row against the float64 forward of the actor's parameters -- the ones
    build_mlp(actor) holds -- within the bounds of test 6; build_mlp's own fp32 output lies within the structural bound too."""
    from legged_gym_dev_amd.rl.checkpoint import build_mlp
    env, runner = _runner(3)
    try:
        ppo = runner.ppo
        acts = _actions(env, 3, 2)
        for s in range(3):
            env.step(acts[s])
        row = env.get_actor_observations().clone()
        with pytest.raises(ValueError, match="shape \\(64, 48\\).*144 columns"):      # the reference idiom is refused, not read past its end
            runner.get_inference_policy()(env.get_observations())
        got = runner.get_inference_policy()(row).cpu().double()
        torch.cuda.synchronize()
        sd = {k: v.cpu() for k, v in ppo.state_dict().items()}
        c = ar._case("inference", 144, 48, [512, 256, 128], [512, 256, 128], 64, 12, ppo.activation)
        x = row.cpu()
        out, S, trace = ar.forward64(c, sd, x, "actor")
        bound = ar.structural_bound(trace)
        diff = (got - out).abs()
        worst = float((diff / bound).max())
        e_k = float((diff / S).max())
        e_y = float(((ar.yardstick(c, sd, x, "actor").double() - out).abs() / S).max())
        print(f"inference W=144: worst diff/bound {worst:.4f}, E_k {e_k:.3e}, E_y {e_y:.3e}")
        assert worst <= 1.0 and e_k <= ar.PRECISION_M[ar.on_expf(c)] * e_y + ar.U
        with torch.no_grad():
            mlp = build_mlp(sd, "actor", ppo.activation)(x).double()
        assert bool(((mlp - out).abs() <= bound).all())
    finally:
        env.close()
        runner.ppo.close()


def test_train_save_play_with_a_history(tmp_path, monkeypatch):
    """The way the scripts go: make_env / make_alg_runner with --obs_history 3, one learn iteration, a checkpoint with the
    "obs_history" key; play.py with the same flag loads it, runs 20 steps and writes policy_hist_1.pt; without the flag the load is
    refused in the cfg's words."""
    import legged_gym_dev_amd
    from legged_gym_dev_amd.envs import task_registry
    monkeypatch.setattr(legged_gym_dev_amd, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    monkeypatch.setattr(sys.modules["legged_gym_dev_amd.utils.task_registry"], "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    task = "anymal_c_flat"
    env_cfg, shared = task_registry.get_cfgs(task)              # registered cfg objects are shared and mutated in place: put them back
    monkeypatch.setattr(env_cfg.obs_history, "length", 1)
    monkeypatch.setattr(env_cfg.env, "num_envs", env_cfg.env.num_envs)
    monkeypatch.setattr(shared.runner, "resume", False)
    monkeypatch.setattr(shared.policy, "actor_hidden_dims", [64, 32])
    monkeypatch.setattr(shared.policy, "critic_hidden_dims", [64, 32])
    for k in ("num_rows", "num_cols", "curriculum"):
        monkeypatch.setattr(env_cfg.terrain, k, getattr(env_cfg.terrain, k))
    monkeypatch.setattr(env_cfg.noise, "add_noise", env_cfg.noise.add_noise)
    for k in ("randomize_friction", "push_robots"):
        monkeypatch.setattr(env_cfg.domain_rand, k, getattr(env_cfg.domain_rand, k))
    args = _args(task, 16, ("--obs_history", "3"))
    env, _ = task_registry.make_env(name=task, args=args)
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=task, args=args)
    assert runner.ppo.O == 144
    runner.learn(num_learning_iterations=1)
    d = torch.load(os.path.join(runner.log_dir, "model_1.pt"), map_location="cpu", weights_only=True)
    assert d["obs_history"] == {"length": 3, "ranges": [], "reset": "repeat", "num_obs": 48}
    assert tuple(d["model_state_dict"]["actor.0.weight"].shape) == (64, 144) and tuple(d["model_state_dict"]["critic.0.weight"].shape) == (64, 48)
    env.close(); runner.ppo.close()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged_gym_dev_amd", "scripts"))
    import importlib
    play = importlib.import_module("play")
    monkeypatch.setattr(play, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    rec = play.play(_args(task, 1, ("--obs_history", "3")), num_steps=20, out_mat=None)
    assert rec["action"].shape == (20, 12) and np.isfinite(rec["torque"]).all() and np.abs(rec["action"]).sum() > 0
    out = tmp_path / "logs" / train_cfg.runner.experiment_name / "exported" / "policies" / "policy_hist_1.pt"
    assert os.path.exists(out)
    mod = torch.jit.load(str(out))
    assert tuple(mod.history.shape) == (1, 144) and tuple(mod(torch.zeros(1, 48)).shape) == (1, 12)
    env_cfg.obs_history.length = 1
    with pytest.raises(ValueError, match="cfg.obs_history = \\(length 3, columns all, reset repeat, num_obs 48\\).*\\(no history\\)"):
        play.play(_args(task, 1), num_steps=2, out_mat=None)
