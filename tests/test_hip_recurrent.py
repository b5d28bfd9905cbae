"""The LSTM learner (csrc/ppo_rnn.hip: k_lstm_fwd, k_lstm_bwd, k_lstm_bias_grad, k_lstm_reset; csrc/ppo_sched.hip: rnn_forward_seq,
rnn_backward_seq, rnn_live_step) against float64, across row tiles, hidden sizes, dones patterns and a privileged critic.

tests/test_recurrent_policy.py, written with the feature, runs every kernel at one row tile (16 or 64 rows), H = 64 | 128, critic
observations aliased to the actor's, storage from a real rollout (where the saved state of a step that carries equals the carried
state) and one tolerance over the joined gradient vector against fp32 autograd.  Here:

(a) one minibatch's gradients, KL and loss statistics on the cases of tests/recurrent_loss_ref.CASES -- storage, dones and saved
    states written directly (saved states unrelated to the recurrence, rows steered off every branch boundary of the loss) --
    against recurrent_loss_ref.reference() in float64, every tensor in the project's bands on its own.  What each case reaches:
      one_env_last_minibatch             M = 1 per step launch, env offset of the last of four minibatches, H = 32 (two j-blocks)
      three_rows_privileged_all_reload   M = 3 (one thread, three of its four rows), OC = 65 != O, every step reloads
      one_full_tile_h256_net128          M = 64 exactly, the default H = 256, the k_head_net<128> head path
      tile_plus_1_h96_privileged_tanh    a second row tile of one row, H = 96, O = 235 and OC = 187 (neither a multiple of the
                                         32-wide k-tile), generic head path, runs of consecutive dones
      three_tiles_last_2_rows_t24        M = 130: three tiles, the last with two rows; 24 steps of BPTT with cuts
      h512                               the largest H
      t1_70_rows                         T = 1 (no carry launch at all), 64 + 6 rows
      bias_split_r257                    k_lstm_bias_grad goes from one row split to two (per = 129, the last split one row
                                         short); five row tiles
      bias_split_r514                    three row splits (172, 172, 170 rows)
      bias_split_64way_r16448            R >= 16384: 64 splits of 257 rows
      bias_split_64way_r16445            64 splits with a remainder (63 of 257 rows, one of 254)
      full_depth_bptt                    no done anywhere: 24 steps carried, no cut
      t2_one_carry                       the shortest sequence with a carry
    Every size of the matrix is accepted by lg_ppo_create_recurrent; no case was removed.
(b) deterministic mode (the det64 accumulation of dW_ih, dW_hh and the bias gradients) in the same bands, and bit-equal when repeated;
(c) the live step (rollout act, compute_returns, act_inference), process_env_step / reset_hidden and the independence of the two
    memories against recurrent_loss_ref.step_reference, from states written by the test.
tests/test_recurrent_loss_host.py holds the CPU conditions on these inputs."""
import pytest
import torch

from tests import recurrent_loss_ref as rl

pytestmark = pytest.mark.gpu

RECURRENT = "ActorCriticRecurrent"
LIVE = ("h_a", "c_a", "h_c", "c_c")
# one row, three rows of one thread, a second tile of one row, three tiles (H = 32: two j-blocks); H = 96; the largest H
LIVE_SHAPES = [(1, 32), (3, 32), (65, 32), (130, 32), (65, 96), (3, 512)]


def _learner(N, O, OC, A, H, hidden, activation, nmb, T):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    policy = {"actor_hidden_dims": list(hidden), "critic_hidden_dims": list(hidden), "activation": activation,
              "init_noise_std": 1.0, "rnn_hidden_size": H}
    return HipPPO(N, O, OC, A, policy, dict(rl.ALG, num_mini_batches=nmb), T, device="cuda:0", seed=3, policy_class_name=RECURRENT)


def _load(hip, params):
    assert set(hip.param_views) == set(params)
    for k, v in params.items():
        hip.param_views[k].copy_(v)
    hip.params_changed()


def _run(case, deterministic=False):
    """begin_update + minibatch_backward(0, mb) (+ the same again in deterministic mode) + minibatch_step on the case's storage ->
    what the library computed, in the shape recurrent_loss_ref.reference() returns it."""
    m = case["meta"]
    T, N, mbs, R, mb = m["T"], m["N"], m["mbs"], m["R"], m["mb"]
    hip = _learner(N, m["O"], m["OC"], m["A"], m["H"], m["hidden"], m["activation"], m["nmb"], T)
    try:
        assert hip.privileged == (m["OC"] is not None)
        _load(hip, case["params"])
        for k in rl.STORAGE + rl.STATES + ("sigma", "dones") + (("critic_obs",) if hip.privileged else ()):
            assert hip.t[k].shape == case[k].shape and hip.t[k].dtype == case[k].dtype, k
            hip.t[k].copy_(case[k])
        if deterministic:
            hip.set_deterministic(True)

        def backward():
            hip._call("begin_update")
            hip._call("minibatch_backward", 0, mb)
            torch.cuda.synchronize()
            return {k: v.detach().cpu().clone() for k, v in hip.grad_views.items()}
        grads = backward()
        got = {"grads": grads, "kl": float(hip.t["grads"][hip.num_params]) / R}
        rows = hip.t["perm"][mb * R:(mb + 1) * R].long().cpu()          # t-major over the minibatch's envs
        want = (torch.arange(T).unsqueeze(1) * N + mb * mbs + torch.arange(mbs).unsqueeze(0)).reshape(-1)
        assert torch.equal(rows, want)
        if deterministic:
            again = backward()
            for k, g in grads.items():
                assert torch.equal(again[k], g), k
        hip._call("minibatch_step")
        torch.cuda.synchronize()
        st = hip.stats()
        assert st["n_updates"] == 1.0
        got["value_loss"] = st["value_loss_sum"] / st["n_updates"]
        got["surrogate_loss"] = st["surrogate_loss_sum"] / st["n_updates"]
        return got
    finally:
        hip.close()


def _compare(c, got, tag):
    case = rl.build_for(c)
    ref = rl.reference(case)
    assert list(got["grads"]) == list(ref["grads"])
    for k, g in got["grads"].items():
        assert bool(torch.isfinite(g).all()), k
    errs = rl.band_errors(got, ref, case)
    print(tag, rl.case_id(c), {k: "%.3g/%.3g" % v for k, v in errs.items()})
    print(tag + "_worst", rl.case_id(c), "%s %.3g" % rl.worst(errs))
    over = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not over, over


@pytest.mark.parametrize("c", rl.CASES, ids=rl.case_id)
def test_minibatch_gradients_kl_and_statistics_match_float64(c):
    _compare(c, _run(rl.build_for(c)), "recurrent_errors")


@pytest.mark.parametrize("label", rl.DETERMINISTIC)
def test_deterministic_mode_matches_float64_and_repeats_bit_exactly(label):
    c = rl.by_label(label)
    _compare(c, _run(rl.build_for(c), deterministic=True), "recurrent_det_errors")


# ------------------------------------------------------------------------------------------------ live step
def _close(got, want, tol=2e-5, what=""):
    torch.testing.assert_close(got.detach().double().cpu(), want, rtol=tol, atol=tol, msg=lambda s: f"{what}: {s}")


def _live_setup(N, H, seed):
    O, OC, A, T = 45, 65, 12, 3
    from tests.recurrent_ref import ActorCriticRecurrent
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        ac = ActorCriticRecurrent(O, OC, A, rl.M3, rl.M3, "elu", rnn_hidden_size=H)
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        ac.std.mul_(0.6 + 0.8 * torch.rand(A, generator=g))
    params = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    hip = _learner(N, O, OC, A, H, rl.M3, "elu", 1, T)
    _load(hip, params)
    draw = lambda *shape, scale=1.0: (scale * torch.randn(*shape, generator=g)).cuda()
    for k in LIVE:
        hip.t[k].copy_(draw(N, H, scale=0.5))
    return hip, params, draw, g, (O, OC, A, T)


def _states(hip):
    return {k: hip.t[k].clone() for k in LIVE}


def _check_reset(before, after, dones):
    done = dones.bool()
    for k in LIVE:
        assert float(after[k][done].abs().sum()) == 0.0, k
        assert torch.equal(after[k][~done], before[k][~done]), k


@pytest.mark.parametrize("N,H", LIVE_SHAPES)
def test_live_step_reset_and_independent_memories(N, H):
    hip, params, draw, g, (O, OC, A, T) = _live_setup(N, H, 100 + N + H)
    try:
        hip.inject_noise(1)
        for t in range(T):
            obs, cobs, noise = draw(N, O), draw(N, OC), draw(N, A)
            before = _states(hip)
            hip.t["noise"].copy_(noise)
            actions = hip.act(obs, cobs)
            for k in LIVE:                                   # the transition keeps the state before the step, bit for bit
                assert torch.equal(hip.t["saved_" + k][t], before[k]), (t, k)
            ref = rl.step_reference(params, "elu", obs, cobs, *(before[k] for k in LIVE), noise=noise)
            for k in LIVE:
                _close(hip.t[k], ref[k], what=f"t={t} {k}")
            _close(hip.t["mu"][t], ref["mu"], what=f"t={t} mu")
            _close(hip.t["values"][t], ref["value"], what=f"t={t} value")
            _close(hip.t["actions"][t], ref["actions"], what=f"t={t} actions")
            _close(actions, ref["actions"], what=f"t={t} returned actions")
            _close(hip.t["log_prob"][t], ref["log_prob"], tol=1e-4, what=f"t={t} log_prob")
            assert torch.equal(hip.t["obs"][t], obs) and torch.equal(hip.t["critic_obs"][t], cobs)
            dones = torch.zeros(N, dtype=torch.uint8, device="cuda")
            if t == 0:                                       # the first and the last env, and every third between
                dones[0] = dones[N - 1] = 1
                dones[4::3] = 1
            elif t == 1 and N > 1:
                dones[1::2] = 1
            after_act = _states(hip)
            hip.process_env_step(draw(N), dones, {})
            _check_reset(after_act, _states(hip), dones)
            assert torch.equal(hip.t["dones"][t], dones)
        last = draw(N, OC)
        before = _states(hip)
        hip.compute_returns(last)
        ref = rl.step_reference(params, "elu", torch.zeros(N, O), last, *(before[k] for k in LIVE))
        assert torch.equal(hip.t["h_a"], before["h_a"]) and torch.equal(hip.t["c_a"], before["c_a"])
        _close(hip.t["h_c"], ref["h_c"], what="compute_returns h_c")
        _close(hip.t["c_c"], ref["c_c"], what="compute_returns c_c")
        assert float((hip.t["h_c"] - before["h_c"]).abs().max()) > 1e-3
    finally:
        hip.close()


@pytest.mark.parametrize("N,H", LIVE_SHAPES)
def test_act_inference_advances_the_actor_memory_only_and_reset_hidden(N, H):
    hip, params, draw, g, (O, OC, A, T) = _live_setup(N, H, 200 + N + H)
    try:
        for rep in range(2):
            obs = draw(N, O)
            before = _states(hip)
            out = hip.act_inference(obs)
            ref = rl.step_reference(params, "elu", obs, torch.zeros(N, OC), *(before[k] for k in LIVE))
            _close(out, ref["mu"], what="act_inference")
            _close(hip.t["h_a"], ref["h_a"], what="h_a")
            _close(hip.t["c_a"], ref["c_a"], what="c_a")
            assert torch.equal(hip.t["h_c"], before["h_c"]) and torch.equal(hip.t["c_c"], before["c_c"])
        dones = torch.zeros(N, dtype=torch.uint8, device="cuda")
        dones[0] = dones[N - 1] = 1
        dones[2::5] = 1
        before = _states(hip)
        hip.reset_hidden(dones)
        _check_reset(before, _states(hip), dones)
        if N > 1:
            assert float(hip.t["h_a"].abs().sum()) > 0
        hip.reset_hidden(None)
        for k in LIVE:
            assert float(hip.t[k].abs().sum()) == 0.0, k
    finally:
        hip.close()
