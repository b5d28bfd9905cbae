"""rsl_rl's ActorCriticRecurrent (runner.policy_class_name = 'ActorCritic' | 'ActorCriticRecurrent', policy.rnn_*) on the HIP
learner: config parsing (host only), then on the GPU parameters / initialisation, two rollouts, one minibatch's gradients, a full
update (also at a multi-tile shape with a privileged critic), deterministic mode, checkpoints, the LSTM policy export and the
refusals -- against tests/recurrent_ref.py (recalled rsl_rl semantics, see its docstring).

The numbers of the LSTM kernels themselves -- every row-tile shape, hidden size, dones pattern and the privileged critic, against
float64 and tensor by tensor -- are in tests/test_hip_recurrent.py (cases and references: tests/recurrent_loss_ref.py; the CPU
conditions on them: tests/test_recurrent_loss_host.py)."""
import ctypes
import os

import pytest
import torch

from legged_gym_dev_amd.rl.ppo import parse_policy_class

POLICY = {"actor_hidden_dims": [128, 64, 32], "critic_hidden_dims": [128, 64, 32], "activation": "elu", "init_noise_std": 1.0}
ALG = dict(value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01, num_learning_epochs=5,
           num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", gamma=0.99, lam=0.95, desired_kl=0.01, max_grad_norm=1.0)


# ---------------------------------------------------------------------------------------------------------------- host only
def test_actor_critic_keeps_the_feed_forward_learner():
    assert parse_policy_class("ActorCritic", dict(POLICY, rnn_type="gru", rnn_num_layers=3), 4096, 4) is None
    assert parse_policy_class(None, POLICY, 4096, 4) is None


def test_recurrent_defaults_and_accepted_settings():
    assert parse_policy_class("ActorCriticRecurrent", POLICY, 4096, 4) == {"type": 0, "hidden": 256, "layers": 1}
    for h in (32, 64, 128, 512):
        cfg = dict(POLICY, rnn_type="lstm", rnn_hidden_size=h, rnn_num_layers=1)
        assert parse_policy_class("ActorCriticRecurrent", cfg, 64, 4)["hidden"] == h

    class Cfg:                                              # the config classes of legged_robot_config.py hold attributes
        rnn_type, rnn_hidden_size, rnn_num_layers = "lstm", 64, 1
    assert parse_policy_class("ActorCriticRecurrent", Cfg, 8, 2)["hidden"] == 64


@pytest.mark.parametrize("name,cfg,n,nmb", [
    ("ActorCriticMLP", POLICY, 64, 4),
    ("actorcritic", POLICY, 64, 4),
    ("ActorCriticRecurrent", dict(POLICY, rnn_type="gru"), 64, 4),
    ("ActorCriticRecurrent", dict(POLICY, rnn_num_layers=2), 64, 4),
    ("ActorCriticRecurrent", dict(POLICY, rnn_hidden_size=100), 64, 4),
    ("ActorCriticRecurrent", dict(POLICY, rnn_hidden_size=544), 64, 4),
    ("ActorCriticRecurrent", dict(POLICY, rnn_hidden_size=0), 64, 4),
])
def test_unimplemented_settings_are_refused(name, cfg, n, nmb):
    with pytest.raises(NotImplementedError):
        parse_policy_class(name, cfg, n, nmb)


def test_recurrent_update_needs_whole_env_minibatches():
    """Inference on any env count (play.py runs one env with the task's num_mini_batches = 4); an update needs N % nmb == 0."""
    from legged_gym_dev_amd.rl.ppo import check_recurrent_update
    assert parse_policy_class("ActorCriticRecurrent", POLICY, 1, 4)["hidden"] == 256
    check_recurrent_update(64, 4)
    for n, nmb in ((66, 4), (1, 4), (10, 3)):
        with pytest.raises(NotImplementedError):
            check_recurrent_update(n, nmb)


def test_parameter_order_of_a_recurrent_state_dict():
    from legged_gym_dev_amd.rl.checkpoint import parameter_order
    from tests.recurrent_ref import ActorCriticRecurrent
    ac = ActorCriticRecurrent(48, 48, 12, [32, 32], [32, 32], rnn_hidden_size=32)
    sd = ac.state_dict()
    assert parameter_order({k: sd[k] for k in reversed(list(sd))}) == [n for n, _ in ac.named_parameters()]


def test_lstm_export_surface_matches_the_module(tmp_path):
    """policy_lstm_1.pt on CPU over a sequence == memory_a + actor stepped by hand, also after reset_memory()."""
    from legged_gym_dev_amd.rl.checkpoint import export_policy_as_jit
    from tests.recurrent_ref import ActorCriticRecurrent
    torch.manual_seed(0)
    ac = ActorCriticRecurrent(48, 48, 12, [64, 32], [64, 32], rnn_hidden_size=64)

    class Facade:
        activation = "elu"

        def state_dict(self):
            return ac.state_dict()
    path = export_policy_as_jit(Facade(), str(tmp_path))
    assert os.path.basename(path) == "policy_lstm_1.pt"
    pol = torch.jit.load(path)
    assert tuple(pol.hidden_state.shape) == (1, 1, 64) and tuple(pol.cell_state.shape) == (1, 1, 64)
    xs = torch.randn(6, 1, 48)
    with torch.no_grad():
        for rep in range(2):
            ac.memory_a.hidden_states = None
            for x in xs:
                torch.testing.assert_close(pol(x), ac.act_inference(x), rtol=1e-5, atol=1e-6)
            pol.reset_memory()
            assert float(pol.hidden_state.abs().sum()) == 0.0 and float(pol.cell_state.abs().sum()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- GPU
def _make(N, O, A, T, H=64, policy=POLICY, alg=ALG, seed=3, critic_obs=None):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    from tests.recurrent_ref import ActorCriticRecurrent
    torch.manual_seed(seed)
    hip = HipPPO(N, O, critic_obs, A, dict(policy, rnn_hidden_size=H), alg, T, device="cuda:0", seed=seed,
                 policy_class_name="ActorCriticRecurrent")
    torch.manual_seed(seed)
    ac = ActorCriticRecurrent(O, critic_obs or O, A, policy["actor_hidden_dims"], policy["critic_hidden_dims"], policy["activation"],
                              rnn_hidden_size=H, init_noise_std=policy["init_noise_std"]).cuda()
    return hip, ac


def _rollout(hip, ac, T, N, O, A, g, dones_at, critic_obs=None):
    """One rollout with injected noise on both sides; dones_at(t) -> uint8 (N,).  critic_obs: width of the privileged critic
    observations, drawn on their own (None: the critic sees obs).  Returns the reference's per-step records."""
    hip.inject_noise(1)
    rec = []
    for t in range(T):
        obs = torch.randn(N, O, device="cuda", generator=g)
        noise = torch.randn(N, A, device="cuda", generator=g)
        cobs = torch.randn(N, critic_obs, device="cuda", generator=g) if critic_obs else obs
        hip.t["noise"].copy_(noise)
        hip.act(obs, cobs)
        with torch.no_grad():
            hs = ac.get_hidden_states()                    # the transition keeps the state before the step (zero at the start)
            z = torch.zeros(N, hip.H, device="cuda")
            saved = [(z if pair is None else pair[k][0]).clone() for pair in hs for k in (0, 1)]
            ac.act(obs)
            mu = ac.action_mean
            act = mu + ac.std * noise
            lp = ac.get_actions_log_prob(act)
            v = ac.evaluate(cobs).squeeze(-1)
        rew = torch.randn(N, device="cuda", generator=g)
        dones = dones_at(t)
        hip.process_env_step(rew, dones, {})
        with torch.no_grad():
            ac.reset(dones.bool())
        rec.append(dict(obs=obs, act=act, mu=mu, lp=lp, v=v, saved=saved))
    last = torch.randn(N, critic_obs or O, device="cuda", generator=g)
    rec[-1]["h_c_before_returns"] = hip.t["h_c"].clone()   # the critic state after the last step, before compute_returns
    hip.compute_returns(last)
    with torch.no_grad():
        ac.evaluate(last)                                  # rsl_rl's compute_returns advances memory_c once more
    return rec


def _dones(N, T, g):
    d = (torch.rand(T, N, device="cuda", generator=g) < 0.15).to(torch.uint8)
    d[0, 0:3] = 1                                           # a done at t = 0 ...
    d[T - 1, 3:6] = 1                                       # ... at t = T - 1 ...
    d[:, 6:9] = 0                                           # ... and envs that never reset
    return lambda t: d[t].contiguous()


def _check_rollout(hip, rec):
    for t, r in enumerate(rec):
        torch.testing.assert_close(hip.t["mu"][t], r["mu"], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(hip.t["actions"][t], r["act"], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(hip.t["values"][t], r["v"], rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(hip.t["log_prob"][t], r["lp"], rtol=1e-4, atol=1e-4)
        for k, s in zip(("saved_h_a", "saved_c_a", "saved_h_c", "saved_c_c"), r["saved"]):
            torch.testing.assert_close(hip.t[k][t], s, rtol=2e-5, atol=2e-5)


def _storage(hip, critic_obs=None):
    st = {k: hip.t[k].clone() for k in ("obs", "dones", "actions", "values", "advantages", "returns", "log_prob", "mu",
                                        "saved_h_a", "saved_c_a", "saved_h_c", "saved_c_c", "sigma")}
    st["critic_obs"] = hip.t["critic_obs"].clone() if critic_obs else st["obs"]
    return st


@pytest.mark.gpu
def test_parameters_names_shapes_and_initialisation():
    hip, ac = _make(64, 48, 12, 4)
    ref = list(ac.named_parameters())
    assert list(hip.param_views.keys()) == [n for n, _ in ref]
    for n, p in ref:
        assert tuple(hip.param_views[n].shape) == tuple(p.shape), n
        assert torch.equal(hip.param_views[n], p.detach()), n
    assert hip.num_params == sum(p.numel() for _, p in ref)
    hip.close()


@pytest.mark.gpu
def test_two_rollouts_match_the_restatement():
    """Actions, values, log-probs and saved states over two rollouts (no update between: the parameters stay put); the second
    rollout's first critic step starts from the state compute_returns advanced."""
    N, O, A, T = 64, 48, 12, 8
    hip, ac = _make(N, O, A, T)
    g = torch.Generator(device="cuda").manual_seed(1)
    dn = _dones(N, T, g)
    rec1 = _rollout(hip, ac, T, N, O, A, g, dn)
    _check_rollout(hip, rec1)
    hc_before_returns = rec1[-1]["h_c_before_returns"]
    hip._call("end_update")
    rec = _rollout(hip, ac, T, N, O, A, g, dn)
    _check_rollout(hip, rec)
    # the critic's saved state at t = 0 of rollout 2 is the state after the extra evaluate(), not the one after the last step
    # (the envs done at t = T - 1 start from zero either way: compared on the others)
    live = dn(T - 1) == 0
    for got in (hip.t["saved_h_c"][0], rec[0]["saved"][2]):
        assert float((got[live] - hc_before_returns[live]).abs().max()) > 1e-2
    hip.close()


def _grad_check(hip, ac, mb, T, N):
    from tests import recurrent_ref as rr
    st = _storage(hip)
    hip._call("begin_update")
    hip._call("minibatch_backward", 0, mb)
    b = rr.recurrent_minibatch(st, mb, ALG["num_mini_batches"])
    ac.zero_grad()
    loss, kl, vl, sl = rr.minibatch_loss(ac, b)
    loss.backward()
    ref = torch.cat([p.grad.reshape(-1) for p in ac.parameters()])
    got = hip.t["grads"][: hip.num_params]
    scale = float(ref.abs().max())
    torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-4 * scale)
    rel = float((got - ref).norm() / ref.norm())
    assert rel < 2e-4, rel
    R = T * N // ALG["num_mini_batches"]
    torch.testing.assert_close(hip.t["grads"][hip.num_params] / R, kl, rtol=1e-3, atol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("O,H", [(48, 64), (235, 128)])
def test_minibatch_gradients_match_autograd_through_split_and_pad(O, H):
    """Second rollout (saved states at t = 0 nonzero): gradients of minibatch 1 == autograd through the literal
    split / pad / unpad generator."""
    N, A, T = 64, 12, 24
    hip, ac = _make(N, O, A, T, H=H)
    g = torch.Generator(device="cuda").manual_seed(5)
    dn = _dones(N, T, g)
    _rollout(hip, ac, T, N, O, A, g, dn)
    hip._call("end_update")
    _rollout(hip, ac, T, N, O, A, g, dn)
    assert float(hip.t["saved_h_a"][0].abs().max()) > 0
    _grad_check(hip, ac, 1, T, N)
    hip.close()


@pytest.mark.gpu
@pytest.mark.parametrize("N,nmb,H,OC", [(64, 4, 64, None), (130, 2, 96, 65)], ids=["one_tile", "multi_tile_privileged"])
def test_full_update_tracks_the_restatement(N, nmb, H, OC):
    """Five epochs over every minibatch.  The second shape has 65 envs per minibatch (a second row tile of one row), H = 96 and
    critic observations of their own, so the gather-ahead double buffer runs with mb_critic_obs != mb_obs on the recurrent path."""
    from tests import recurrent_ref as rr
    O, A, T = 48, 12, 8
    hip, ac = _make(N, O, A, T, H=H, alg=dict(ALG, num_mini_batches=nmb), critic_obs=OC)
    g = torch.Generator(device="cuda").manual_seed(4)
    _rollout(hip, ac, T, N, O, A, g, _dones(N, T, g), critic_obs=OC)
    st = _storage(hip, OC)
    p0 = hip.t["params"][: hip.num_params].clone()
    vl, sl = hip.update()
    torch.cuda.synchronize()
    opt = torch.optim.Adam(ac.parameters(), lr=ALG["learning_rate"])
    lr = ALG["learning_rate"]
    for ep in range(5):
        for mb in range(nmb):
            loss, kl, _, _ = rr.minibatch_loss(ac, rr.recurrent_minibatch(st, mb, nmb))
            if kl > 0.02:
                lr = max(1e-5, lr / 1.5)
            elif 0.0 < kl < 0.005:
                lr = min(1e-2, lr * 1.5)
            for grp in opt.param_groups:
                grp["lr"] = lr
            opt.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(ac.parameters(), 1.0)
            opt.step()
    got = hip.t["params"][: hip.num_params]
    ref = torch.cat([p.detach().reshape(-1) for p in ac.parameters()])
    moved = float((ref - p0).norm())
    assert moved > 0.05
    assert float((got - ref).norm()) / moved < 2e-2
    assert abs(hip.learning_rate - lr) < 1e-9
    assert torch.isfinite(vl) and torch.isfinite(sl)
    hip.close()


def _det_run():
    hip, ac = _make(64, 48, 12, 8)
    hip.set_deterministic(True)
    g = torch.Generator(device="cuda").manual_seed(7)
    dn = _dones(64, 8, g)
    for _ in range(2):
        _rollout(hip, ac, 8, 64, 48, 12, g, dn)
        hip.update()
    torch.cuda.synchronize()
    out = hip.t["params"][: hip.num_params].clone()
    hip.close()
    return out


@pytest.mark.gpu
def test_deterministic_mode_is_bit_exact():
    a, b = _det_run(), _det_run()
    assert torch.equal(a, b)


@pytest.mark.gpu
def test_checkpoint_round_trip_and_foreign_checkpoint(tmp_path):
    """A state dict written by the restatement loads and acts identically; save / load keeps parameters and Adam state."""
    N, O, A, T = 64, 48, 12, 4
    hip, _ = _make(N, O, A, T)
    from tests.recurrent_ref import ActorCriticRecurrent
    torch.manual_seed(11)
    foreign = ActorCriticRecurrent(O, O, A, POLICY["actor_hidden_dims"], POLICY["critic_hidden_dims"], rnn_hidden_size=64).cuda()
    torch.save({"model_state_dict": {k: v.cpu() for k, v in foreign.state_dict().items()}}, tmp_path / "m.pt")
    sd = torch.load(tmp_path / "m.pt", weights_only=True)["model_state_dict"]
    hip.load_state_dict(sd)
    x = torch.randn(N, O, device="cuda")
    with torch.no_grad():
        for _ in range(3):
            torch.testing.assert_close(hip.act_inference(x), foreign.act_inference(x), rtol=2e-5, atol=2e-5)
    # parameters + Adam state after an update survive a round trip into a fresh learner
    g = torch.Generator(device="cuda").manual_seed(2)
    _rollout(hip, foreign, T, N, O, A, g, lambda t: torch.zeros(N, dtype=torch.uint8, device="cuda"))
    hip.update()
    psd, osd = hip.state_dict(), hip.optimizer_state_dict()
    hip2, _ = _make(N, O, A, T, seed=9)
    hip2.load_state_dict(psd)
    hip2.load_optimizer_state_dict(osd)
    assert torch.equal(hip2.t["params"][: hip2.num_params], hip.t["params"][: hip.num_params])
    assert torch.equal(hip2.t["adam_m"][: hip2.num_params], hip.t["adam_m"][: hip.num_params])
    assert torch.equal(hip2.t["adam_v"][: hip2.num_params], hip.t["adam_v"][: hip.num_params])
    assert len(osd["state"]) == len(psd)
    hip.close()
    hip2.close()


@pytest.mark.gpu
def test_set_comm_and_wrong_inference_rows_are_refused():
    from legged_gym_dev_amd.lib import LeggedHipError
    hip, _ = _make(64, 48, 12, 4)
    lib = hip.lib
    lib.lg_ppo_set_comm.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    assert lib.lg_ppo_set_comm(hip.ctx, ctypes.c_void_p(1)) != 0
    assert b"LSTM" in lib.lg_last_error()
    with pytest.raises(LeggedHipError):
        hip.act_inference(torch.zeros(32, 48, device="cuda"))
    hip.close()


@pytest.mark.gpu
def test_runner_trains_saves_and_plays_a_recurrent_policy(tmp_path):
    """OnPolicyRunner with policy_class_name = 'ActorCriticRecurrent': two iterations, checkpoint with rsl_rl's keys, reload,
    inference through the facade, the exported policy_lstm_1.pt."""
    import bench
    from legged_gym_dev_amd.rl.checkpoint import export_policy_as_jit
    from legged_gym_dev_amd.rl.runner import OnPolicyRunner
    env, runner = bench.make_runner(64, [128, 64, 32], "cuda:0", 0, 1)
    cfg = {"runner": dict(runner.cfg, policy_class_name="ActorCriticRecurrent"),
           "algorithm": runner.alg_cfg, "policy": dict(runner.policy_cfg, rnn_hidden_size=64), "seed": 1}
    runner.ppo.close()
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    assert runner.alg.actor_critic.is_recurrent
    runner.learn(2, init_at_random_ep_len=True)
    assert bool(torch.isfinite(runner.ppo.t["params"][: runner.ppo.num_params]).all())
    path = str(tmp_path / "model_2.pt")
    runner.save(path)
    sd = torch.load(path, weights_only=True)["model_state_dict"]
    assert "memory_a.rnn.weight_hh_l0" in sd and "memory_c.rnn.bias_ih_l0" in sd
    runner.load(path)
    runner.alg.actor_critic.reset()
    policy = runner.get_inference_policy()
    obs = env.get_observations()
    a1 = policy(obs).clone()
    h = runner.alg.actor_critic.get_hidden_states()[0][0].clone()
    assert float(h.abs().max()) > 0
    runner.alg.actor_critic.reset(torch.ones(env.num_envs, dtype=torch.bool, device="cuda"))
    assert float(runner.alg.actor_critic.get_hidden_states()[0][0].abs().max()) == 0.0
    out = export_policy_as_jit(runner.alg.actor_critic, str(tmp_path / "exported"))
    pol = torch.jit.load(out)
    torch.testing.assert_close(pol(obs[:1].cpu()), a1[:1].cpu(), rtol=2e-5, atol=2e-5)


@pytest.mark.gpu
def test_play_script_on_a_recurrent_checkpoint(tmp_path, monkeypatch):
    """scripts/play.py resumes an ActorCriticRecurrent checkpoint on one env (num_mini_batches stays 4), exports
    policy_lstm_1.pt and plays."""
    import sys
    import numpy as np
    import legged_gym_dev_amd
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.utils import get_args
    task = "anymal_c_flat"

    def args(n):
        a = get_args(["--task", task, "--num_envs", str(n), "--headless"])
        a.sim_device = a.rl_device = "cuda:0"
        return a
    monkeypatch.setattr(legged_gym_dev_amd, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    monkeypatch.setattr(sys.modules["legged_gym_dev_amd.utils.task_registry"], "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    _, shared = task_registry.get_cfgs(task)             # registered cfg objects are shared: every change is undone by monkeypatch
    monkeypatch.setattr(shared.runner, "resume", False)
    monkeypatch.setattr(shared.runner, "policy_class_name", "ActorCriticRecurrent")
    monkeypatch.setattr(shared.policy, "actor_hidden_dims", [128, 64, 32])
    monkeypatch.setattr(shared.policy, "critic_hidden_dims", [128, 64, 32])
    monkeypatch.setattr(shared.policy, "rnn_hidden_size", 64, raising=False)
    env, _ = task_registry.make_env(name=task, args=args(16))
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=task, args=args(16))
    assert runner.alg.actor_critic.is_recurrent
    runner.learn(num_learning_iterations=1)
    env.close()
    runner.ppo.close()
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "legged_gym_dev_amd", "scripts"))
    import importlib
    play = importlib.import_module("play")
    monkeypatch.setattr(play, "LEGGED_GYM_ROOT_DIR", str(tmp_path))
    monkeypatch.chdir(tmp_path)
    rec = play.play(args(1), num_steps=60, out_mat=str(tmp_path / "play_data.mat"))
    assert rec["pos"].shape == (60, 3) and np.isfinite(rec["torque"]).all() and np.abs(rec["action"]).sum() > 0
    exported = tmp_path / "logs" / train_cfg.runner.experiment_name / "exported" / "policies" / "policy_lstm_1.pt"
    assert exported.exists()
    assert tuple(torch.jit.load(str(exported)).hidden_state.shape) == (1, 1, 64)
