"""GPU parity of the HIP PPO learner (through the lg_ppo_* C-ABI) against the fp32 torch restatement
of rsl_rl (oracle/ppo_torch.py): act/log-prob, GAE returns, minibatch gradients (MFMA GEMM
forward/backward vs autograd), KL-adaptive lr + grad clip + Adam, full update.

The gradient tests here update on the rollout's own parameters with 12 actions: importance ratio 1 and v_new = v_old, so every row is
inside the surrogate clip and on the tie branch of the clipped value loss.  The other branches of the loss, value_loss_coef != 1,
use_clipped_value_loss = False, 1 .. 16 actions and the second trip of the head kernels' tile loops are checked against float64, per
head kernel, in tests/test_hip_ppo_loss.py (inputs: tests/ppo_loss_ref.py, their conditions: tests/test_ppo_loss_host.py).
The whole feed-forward minibatch -- forward, head and backward chain as lg_ppo_minibatch_backward schedules them -- is checked against
float64 with a band on every parameter tensor and the launch of every GEMM named per case, at depths 1 .. 4, row counts off every tile
grid, a privileged critic, every activation, the side stream on and off and deterministic mode, in tests/test_hip_ppo_update.py
(tests/ppo_update_ref.py, tests/test_ppo_update_host.py).

The rollout half is checked against float64 elsewhere: act() on every dispatch path of the one-launch forward and on the per-layer path,
with per-action std, a numpy Philox and derived log-prob bounds, in tests/test_hip_ppo_act.py (tests/ppo_act_ref.py,
tests/test_ppo_act_host.py); process_env_step, GAE, the advantage moments and the episode bookkeeping in tests/test_hip_ppo_returns.py
(tests/ppo_rollout_ref.py, tests/test_ppo_rollout_host.py); the minibatch gathers and the gather-ahead in tests/test_hip_ppo_gather.py.
The optimiser step (lr rule and clamps, clip, Adam, world, late steps, weight planes, deterministic norm) against float64 is in
tests/test_hip_ppo_opt.py (tests/ppo_opt_ref.py, tests/test_ppo_opt_host.py)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def ctypes_ptr(t):
    import ctypes
    return ctypes.c_void_p(t.data_ptr())

POLICY = {"actor_hidden_dims": [512, 256, 128], "critic_hidden_dims": [512, 256, 128], "activation": "elu",
          "init_noise_std": 1.0}
ALG = dict(value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01,
           num_learning_epochs=5, num_mini_batches=4, learning_rate=1e-3, schedule="adaptive", gamma=0.99,
           lam=0.95, desired_kl=0.01, max_grad_norm=1.0)


def _make(N, O, A, T, policy=POLICY, alg=ALG, seed=3):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    from oracle import ppo_torch
    torch.manual_seed(seed)
    hip = HipPPO(N, O, None, A, policy, alg, T, device="cuda:0", seed=seed)
    ac = ppo_torch.ActorCritic(O, O, A, policy["actor_hidden_dims"], policy["critic_hidden_dims"], policy.get("activation", "elu"),
                               policy["init_noise_std"]).cuda()
    sd = {k: v.clone() for k, v in hip.state_dict().items()}
    ac.load_state_dict(sd)
    return hip, ac, ppo_torch


def _fill_rollout(hip, ac, T, N, O, A, g):
    """Drive act/process_env_step for T steps with synthetic env outputs; returns what the env 'said'."""
    hip.inject_noise(1)
    rec = []
    for t in range(T):
        obs = torch.randn(N, O, device="cuda", generator=g) * (1.0 + 0.2 * t)
        noise = torch.randn(N, A, device="cuda", generator=g)
        hip.t["noise"].copy_(noise)
        act = hip.act(obs).clone()
        rew = torch.randn(N, device="cuda", generator=g)
        dones = (torch.rand(N, device="cuda", generator=g) < 0.1).to(torch.uint8)
        tos = ((torch.rand(N, device="cuda", generator=g) < 0.5) & (dones > 0)).to(torch.uint8)
        hip.process_env_step(rew, dones, {"time_outs": tos})
        rec.append((obs, noise, act, rew, dones, tos))
    return rec


@pytest.mark.parametrize("O,hidden", [(48, [512, 256, 128]), (235, [512, 256, 128]), (48, [128, 64, 32]), (169, [96, 40, 24])])
def test_act_matches_torch(O, hidden):
    N, A, T = 300, 12, 4
    pol = dict(POLICY, actor_hidden_dims=hidden, critic_hidden_dims=hidden)
    hip, ac, _ = _make(N, O, A, T, pol)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn(N, O, device="cuda", generator=g) * 2
    noise = torch.randn(N, A, device="cuda", generator=g)
    hip.inject_noise(1)
    hip.t["noise"].copy_(noise)
    act = hip.act(obs)
    with torch.no_grad():
        mu = ac.actor(obs)
        v = ac.critic(obs).squeeze(-1)
        ref_act = mu + ac.std * noise
        ref_lp = torch.distributions.Normal(mu, ac.std.expand_as(mu)).log_prob(ref_act).sum(-1)
    torch.testing.assert_close(hip.t["act_mu"], mu, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(act, ref_act, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(hip.t["act_values"], v, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(hip.t["act_log_prob"], ref_lp, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(hip.act_inference(obs), mu, rtol=2e-5, atol=2e-5)
    hip.close()


@pytest.mark.parametrize("O", [48, 235, 169, 65])
def test_one_launch_act_equals_per_layer_act(O):
    """lg_ppo_act as ONE launch (fragment-order weights, sampling + transition store in the epilogue: ppo_mlp_fused.hip) against
    the per-layer GEMMs + k_act_sample on the same learner: sampled actions, log-probs, values and the stored transition.
    Philox noise (not injected): both paths draw the same stream.  Means / values go through differently tiled fp32 sums.
    Observation widths of the four tasks: 48 flat, 235 rough terrain, 169 Cassie, 65 trajectory task -- the last three are not
    whole k-steps of 16 (zero pad columns in the LDS image and in the weight image)."""
    N, A, T = 333, 12, 3
    hip, _, _ = _make(N, O, A, T)
    hip.lib.lg_ppo_debug_set_fused_act(hip.ctx, 1)
    assert hip.lib.lg_ppo_debug_get_fused_act(hip.ctx) == 1, "the one-launch forward must cover this shape"
    g = torch.Generator(device="cuda").manual_seed(5)
    obs = [torch.randn(N, O, device="cuda", generator=g) for _ in range(T)]
    got = []
    for fused in (1, 0):
        hip.lib.lg_ppo_debug_set_fused_act(hip.ctx, fused)
        hip.lib.lg_ppo_debug_set_act_count(hip.ctx, 0)
        rec = []
        for t in range(T):
            a = hip.act(obs[t]).clone()
            rec.append((a, hip.t["act_log_prob"].clone(), hip.t["act_values"].clone(), hip.t["act_mu"].clone()))
            hip.process_env_step(torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), {})
        st = {k: hip.t[k].clone() for k in ("obs", "actions", "mu", "values", "log_prob", "sigma")}
        got.append((rec, st))
        hip._call("end_update")                      # rewind the rollout cursor
    (ra, sa), (rb, sb) = got
    for t in range(T):
        for x, y in zip(ra[t], rb[t]):
            torch.testing.assert_close(x, y, rtol=2e-5, atol=2e-5)
    for k in sa:
        torch.testing.assert_close(sa[k], sb[k], rtol=2e-5, atol=2e-5, msg=k)
    assert torch.equal(sa["obs"], sb["obs"]) and torch.equal(sa["obs"][1], obs[1])
    hip.close()


def test_philox_sampling_is_standard_normal():
    hip, ac, _ = _make(4096, 48, 12, 2, dict(POLICY, actor_hidden_dims=[32, 32, 32], critic_hidden_dims=[32, 32, 32]))
    obs = torch.zeros(4096, 48, device="cuda")
    a = hip.act(obs)
    z = (a - hip.t["act_mu"]) / hip.param_views["std"]
    assert abs(float(z.mean())) < 0.02 and abs(float(z.std()) - 1.0) < 0.02
    assert abs(float((z ** 3).mean())) < 0.05 and abs(float((z ** 4).mean()) - 3.0) < 0.15
    hip.close()


@pytest.mark.parametrize("O,hidden", [(48, None), (235, None), (169, None), (65, None), (48, [128, 64, 32])])
def test_returns_and_gradients_match_torch(O, hidden):
    _returns_and_gradients(O, hidden, 512, 8)


@pytest.mark.parametrize("O", [48, 235])
def test_returns_and_gradients_match_torch_at_baseline_size(O):
    """The same comparison at BASELINE.json's size: 4096 envs x 24 steps, minibatches of 24 576 rows through [512,256,128] (flat and rough
    observation widths): returns / advantages against the restatement, the gradients of two minibatches against autograd."""
    # (gradients are means over 24 576 rows here: more first-layer weights sit within 10x of Adam's eps, where a step follows the
    # gradient's size -- the share of parameters outside the post-step band, 0.1 % measured, is asserted at 0.4 % instead of 0.05 %)
    _returns_and_gradients(O, None, 4096, 24, band_frac=4e-3)


def _returns_and_gradients(O, hidden, N, T, band_frac=5e-4):
    """O: the observation widths of the four tasks.  None of 48, 235, 169 and 65 is a multiple of 32: the minibatch gathers and the
    first layer's weight planes then carry zero pad columns (lg_ppo_create pads Op and OCp to whole k-tiles of 32: rows of
    64 / 256 / 192 / 96) and the first layer's weight gradient is
    computed on the padded width and stored on the true one.  hidden = [128, 64, 32]: the reference's own flat-task policy
    (anymal_c_flat_config.py:62-65), whose 32-wide last hidden layer takes the k_head_fused<32> path."""
    A = 12
    pol = POLICY if hidden is None else dict(POLICY, actor_hidden_dims=hidden, critic_hidden_dims=hidden)
    hip, ac, pt = _make(N, O, A, T, pol)
    g = torch.Generator(device="cuda").manual_seed(2)
    rec = _fill_rollout(hip, ac, T, N, O, A, g)
    last_obs = torch.randn(N, O, device="cuda", generator=g)
    hip.compute_returns(last_obs)
    # ---- torch side of the rollout bookkeeping
    with torch.no_grad():
        values = torch.stack([ac.critic(o).squeeze(-1) for o, *_ in rec])
        rewards = torch.stack([r + ALG["gamma"] * values[t] * to.float() for t, (_, _, _, r, _, to) in enumerate(rec)])
        dones = torch.stack([d for *_, d, _ in rec])
        lastv = ac.critic(last_obs).squeeze(-1)
        ret, adv = pt.compute_returns(rewards, dones, values, lastv, ALG["gamma"], ALG["lam"])
        advn = pt.normalize_advantages(adv)
    torch.testing.assert_close(hip.t["values"], values, rtol=2e-5, atol=2e-5)
    torch.testing.assert_close(hip.t["rewards"], rewards, rtol=2e-5, atol=2e-5)
    assert torch.equal(hip.t["dones"], dones)
    torch.testing.assert_close(hip.t["returns"], ret, rtol=1e-4, atol=1e-4)
    torch.testing.assert_close(hip.t["advantages"], advn, rtol=2e-4, atol=2e-4)

    # ---- one minibatch: gradients vs autograd
    hip._call("begin_update")
    torch.cuda.synchronize()
    perm = hip.t["perm"].long()
    R = T * N // ALG["num_mini_batches"]
    algo = pt.PPO(ac, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, max_grad_norm=1.0,
                  use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01)
    flat = lambda name: hip.t[name].reshape(T * N, *hip.t[name].shape[2:])
    old_sigma = hip.t["sigma"].clone()
    for mb in range(2):
        idx = perm[mb * R:(mb + 1) * R]
        hip._call("minibatch_backward", 0, mb)
        batch = (flat("obs")[idx], flat("obs")[idx], flat("actions")[idx], flat("values")[idx].unsqueeze(-1),
                 flat("advantages")[idx].unsqueeze(-1), flat("returns")[idx].unsqueeze(-1),
                 flat("log_prob")[idx].unsqueeze(-1), flat("mu")[idx], old_sigma.expand(R, A))
        batch = tuple(b.clone() for b in batch)
        ac.zero_grad()
        loss, kl, vl, sl = algo.minibatch_loss(*batch)
        loss.backward()
        ref = torch.cat([p.grad.reshape(-1) for p in ac.parameters()])
        got = hip.t["grads"][: hip.num_params]
        scale = float(ref.abs().max())
        torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-4 * scale)
        rel = float((got - ref).norm() / ref.norm())
        assert rel < 2e-4, rel
        torch.testing.assert_close(hip.t["grads"][hip.num_params] / R, kl, rtol=1e-3, atol=1e-6)
        g_got, g_ref = got.clone(), ref.clone()            # the step below clears the buffer `got` views
        # ---- optimizer step vs clip_grad_norm_ + Adam with the KL-adaptive learning rate
        hip._call("minibatch_step")
        kl_f = float(kl)
        if kl_f > 0.02:
            algo.learning_rate = max(1e-5, algo.learning_rate / 1.5)
        elif 0.0 < kl_f < 0.005:
            algo.learning_rate = min(1e-2, algo.learning_rate * 1.5)
        for grp in algo.optimizer.param_groups:
            grp["lr"] = algo.learning_rate
        torch.nn.utils.clip_grad_norm_(ac.parameters(), 1.0)
        algo.optimizer.step()
        assert abs(hip.learning_rate - algo.learning_rate) < 1e-9
        # Adam's first steps are lr * g / (|g| + eps) ~ lr * sign(g) per weight, whatever the gradient's size: a weight whose
        # gradient is comparable to the GEMMs' fp32 summation noise can step a different amount (up to the other way) in the
        # two implementations.  Asserted as stated: every parameter outside the band (2e-6 + 1e-4 |p|) has a gradient whose
        # HIP-vs-autograd difference is at least 2 % of the gradient itself (or a gradient below 1e-6 of the largest), there
        # are < 0.05 % of them, and none is off by more than the two sign steps taken so far.
        got_p, ref_p = hip.t["params"][: hip.num_params], pt.flat_params(ac)
        bad = (got_p - ref_p).abs() > (2e-6 + 1e-4 * ref_p.abs())
        assert float(bad.float().mean()) < band_frac, float(bad.float().mean())
        assert float((got_p - ref_p).abs().max()) <= 2.1 * algo.learning_rate * (mb + 1)
        if mb == 0 and bool(bad.any()):                    # (after the first step the Adam moments carry step 0's noise as well)
            gerr, gmag = (g_got - g_ref).abs()[bad], g_ref.abs()[bad]
            # ... or a gradient within 10x of Adam's eps (1e-8), where the step lr g / (|g| + eps) follows the gradient's SIZE
            explained = (gerr >= 0.02 * gmag) | (gmag <= 1e-6 * scale) | (gmag <= 1e-7)
            assert bool(explained.all()), (int((~explained).sum()), int(bad.sum()))
    hip.close()


@pytest.mark.parametrize("N,T,nmb,O,OC,hidden", [(256, 4, 4, 65, 169, [512, 256, 128]), (256, 8, 1, 48, 100, [64, 64, 32]),
                                                  (256, 8, 1, 65, 169, [64, 64, 32])])
def test_privileged_critic_observations(N, T, nmb, O, OC, hidden):
    """Asymmetric actor / critic inputs (rsl_rl's num_privileged_obs: the critic sees its own observation vector): 65-wide actor
    and 169-wide critic observations -- neither a multiple of 8, so both minibatch gathers and both first layers carry pad
    columns of different widths.  act() (one launch), the stored critic observations, returns, and the gradients of one
    minibatch against autograd.  The one-minibatch cases have 2048 rows: the first layers' weight-gradient launch then takes 8
    reduction slices over two problems of different tile counts (64 x 64 against 64 x 128, 64 x 96 against 64 x 192)."""
    _unequal_nets(N, T, nmb, O, OC, hidden, hidden)


@pytest.mark.parametrize("actor,critic", [([64, 32, 32], [128, 32, 32]), ([256, 256, 128], [128, 128, 64])])
def test_unequal_hidden_widths(actor, critic):
    """Equal observations, actor and critic of different hidden widths, one minibatch of 2048 rows: every GEMM launch of the
    update holds two problems of different shapes, and the weight-gradient launches split the rows into 8 slices or more."""
    _unequal_nets(256, 8, 1, 48, None, actor, critic)


def _unequal_nets(N, T, nmb, O, OC, actor, critic):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    from oracle import ppo_torch as pt
    A = 12
    policy = dict(POLICY, actor_hidden_dims=actor, critic_hidden_dims=critic)
    alg = dict(ALG, num_mini_batches=nmb)
    torch.manual_seed(3)
    hip = HipPPO(N, O, OC, A, policy, alg, T, device="cuda:0", seed=3)
    ac = pt.ActorCritic(O, OC or O, A, policy["actor_hidden_dims"], policy["critic_hidden_dims"], policy.get("activation", "elu"),
                        policy["init_noise_std"]).cuda()
    ac.load_state_dict({k: v.clone() for k, v in hip.state_dict().items()})
    g = torch.Generator(device="cuda").manual_seed(6)
    hip.inject_noise(1)
    for t in range(T):
        obs = torch.randn(N, O, device="cuda", generator=g)
        cobs = torch.randn(N, OC, device="cuda", generator=g) if OC else obs
        noise = torch.randn(N, A, device="cuda", generator=g)
        hip.t["noise"].copy_(noise)
        act = (hip.act(obs, cobs) if OC else hip.act(obs)).clone()
        with torch.no_grad():
            mu, v = ac.actor(obs), ac.critic(cobs).squeeze(-1)
        torch.testing.assert_close(hip.t["act_mu"], mu, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(hip.t["act_values"], v, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(act, mu + ac.std * noise, rtol=2e-5, atol=2e-5)
        if OC:
            assert torch.equal(hip.t["critic_obs"][t], cobs)
        assert torch.equal(hip.t["obs"][t], obs)
        rew = torch.randn(N, device="cuda", generator=g)
        dones = (torch.rand(N, device="cuda", generator=g) < 0.1).to(torch.uint8)
        hip.process_env_step(rew, dones, {"time_outs": torch.zeros(N, dtype=torch.uint8, device="cuda")})
    hip.compute_returns(torch.randn(N, OC or O, device="cuda", generator=g))
    hip._call("begin_update")
    torch.cuda.synchronize()
    perm = hip.t["perm"].long()
    R = T * N // nmb
    algo = pt.PPO(ac, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, max_grad_norm=1.0,
                  use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01)
    flat = lambda name: hip.t[name].reshape(T * N, *hip.t[name].shape[2:])
    idx = perm[:R]
    hip._call("minibatch_backward", 0, 0)
    batch = (flat("obs")[idx], flat("critic_obs" if OC else "obs")[idx], flat("actions")[idx], flat("values")[idx].unsqueeze(-1),
             flat("advantages")[idx].unsqueeze(-1), flat("returns")[idx].unsqueeze(-1), flat("log_prob")[idx].unsqueeze(-1),
             flat("mu")[idx], hip.t["sigma"].clone().expand(R, A))
    ac.zero_grad()
    loss, kl, vl, sl = algo.minibatch_loss(*(b.clone() for b in batch))
    loss.backward()
    ref = torch.cat([p.grad.reshape(-1) for p in ac.parameters()])
    got = hip.t["grads"][: hip.num_params]
    torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-4 * float(ref.abs().max()))
    assert float((got - ref).norm() / ref.norm()) < 2e-4
    hip.close()


def test_full_update_tracks_torch():
    """5 epochs x 4 minibatches on the same permutation: parameters stay within 2e-3 of torch's."""
    N, O, A, T = 256, 48, 12, 8
    pol = dict(POLICY, actor_hidden_dims=[128, 64, 32], critic_hidden_dims=[128, 64, 32])
    hip, ac, pt = _make(N, O, A, T, pol)
    g = torch.Generator(device="cuda").manual_seed(4)
    _fill_rollout(hip, ac, T, N, O, A, g)
    hip.compute_returns(torch.randn(N, O, device="cuda", generator=g))
    flat = lambda name: hip.t[name].reshape(T * N, *hip.t[name].shape[2:]).clone()
    data = {k: flat(k) for k in ("obs", "actions", "values", "advantages", "returns", "log_prob", "mu")}
    old_sigma = hip.t["sigma"].clone()
    p0 = hip.t["params"][: hip.num_params].clone()
    vl, sl = hip.update()
    torch.cuda.synchronize()
    perm = hip.t["perm"].long()
    algo = pt.PPO(ac)
    R = T * N // 4
    for ep in range(5):
        for mb in range(4):
            idx = perm[mb * R:(mb + 1) * R]
            algo.step_minibatch(data["obs"][idx], data["obs"][idx], data["actions"][idx], data["values"][idx].unsqueeze(-1),
                                data["advantages"][idx].unsqueeze(-1), data["returns"][idx].unsqueeze(-1),
                                data["log_prob"][idx].unsqueeze(-1), data["mu"][idx], old_sigma.expand(R, A))
    got, ref = hip.t["params"][: hip.num_params], pt.flat_params(ac)
    moved = float((ref - p0).norm())
    assert moved > 0.05
    assert float((got - ref).norm()) / moved < 2e-2
    assert abs(hip.learning_rate - algo.learning_rate) < 1e-9
    assert np.isfinite(float(vl)) and np.isfinite(float(sl))
    hip.close()


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("M,N,K", [(4096, 512, 48), (3001, 77, 45), (1024, 256, 512), (640, 12, 128), (777, 1, 129)])
def test_split_bf16_gemm_is_fp32_accurate(mode, M, N, K):
    """The split-bf16 (x6) mainloop against a float64 product, beside the exact fp32-input MFMA
    mainloop on the same operands: its error may not exceed the fp32 path's beyond fp32 rounding of
    the result (tolerance: max |err| <= 2 x fp32-MFMA error + 2^-22 x max |C|).  Modes: 0 = A.B^T (forward), 1 = A.B with the
    ELU' epilogue (input gradient; aux = 1), 2 = A^T.B accumulated with split-K atomics (weight
    gradient).  Ragged / tiny shapes take the masked staging path, the big ones the interior one."""
    import ctypes
    from legged_gym_dev_amd.lib import load
    lib = load()
    lib.ppok_debug_gemm.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(M + N + K + mode)
    # mixed magnitudes: the split has to be exact whatever the exponent
    scale = torch.exp2(torch.randint(-12, 12, (K,), device="cuda", generator=g).float())
    A = torch.randn(M, K, device="cuda", generator=g) * scale if mode < 2 else torch.randn(K, M, device="cuda", generator=g)
    B = torch.randn(N, K, device="cuda", generator=g) / scale if mode == 0 else torch.randn(K, N, device="cuda", generator=g)
    if mode == 1:
        B = B / scale[:, None]
    Ad = A.double() if mode < 2 else A.double().t()
    ref = Ad @ (B.double().t() if mode == 0 else B.double())
    splits = 1 if mode < 2 else 3
    err = {}
    try:
        for x6 in (0, 1):
            lib.ppok_debug_set_x6(ctypes.c_int(x6))
            C = torch.ones(M, N, device="cuda") if mode < 2 else torch.zeros(M, N, device="cuda")
            lib.ppok_debug_gemm(vp(A), vp(B), vp(C), M, N, K, mode, splits, st)
            torch.cuda.synchronize()
            assert torch.isfinite(C).all()
            err[x6] = float((C.double() - ref).abs().max())
    finally:
        lib.ppok_debug_set_x6(ctypes.c_int(1))
    bound = 2.0 * err[0] + 2.0 ** -22 * float(ref.abs().max())
    assert err[1] <= bound, err


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M,rows,cols", [(24576, 256, 512), (4096, 128, 256), (3001, 72, 48), (1000, 512, 48), (640, 16, 128), (515, 264, 40),
                                         (3001, 128, 64), (1000, 256, 96), (129, 384, 32)])
def test_weight_plane_gemms_are_fp32_accurate(mode, M, rows, cols):
    """The two GEMMs that take W [rows][cols] from its three bf16 planes -- forward A.W^T (planes as the reduction-contiguous
    operand) and input gradient A.W (the SAME planes read along their rows through ds_read_b64_tr_b16) -- against a float64
    product, beside the fp32-input MFMA kernel on the fp32 W: error <= 2 x that kernel's + 2^-22 max|C| (the planes are an
    exact split).  Shapes: the update's big interior tiles, the rollout's 64x64 tiles, ragged rows / columns / k-tails; the last three
    take the LDS-DMA forward (k_gemm_glds: K a multiple of 32, N of 128) with a ragged last row tile -- rows past M are clamped on the way in and
    never stored."""
    import ctypes
    from legged_gym_dev_amd.lib import load
    lib = load()
    lib.ppok_debug_gemm.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    lib.ppok_debug_gemm_planes.argtypes = [ctypes.c_void_p] * 4 + [ctypes.c_int64] + [ctypes.c_int] * 4 + [ctypes.c_void_p]
    vp = lambda t: ctypes.c_void_p(t.data_ptr())
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    g = torch.Generator(device="cuda").manual_seed(M + rows + cols + mode)
    K = cols if mode == 0 else rows
    scale = torch.exp2(torch.randint(-12, 12, (K,), device="cuda", generator=g).float())
    W = torch.randn(rows, cols, device="cuda", generator=g)
    W = W / scale if mode == 0 else W / scale[:, None]
    A = torch.randn(M, K, device="cuda", generator=g) * scale
    ref = A.double() @ (W.double().t() if mode == 0 else W.double())
    N = rows if mode == 0 else cols
    stride = (rows * cols + 7) // 8 * 8
    planes = torch.zeros(3 * stride + 8, dtype=torch.int16, device="cuda")
    C = torch.ones(M, N, device="cuda")
    rc = lib.ppok_debug_gemm_planes(vp(A), vp(W), vp(C), vp(planes), stride, M, rows, cols, mode, st)
    assert rc == 0
    torch.cuda.synchronize()
    err_pl = float((C.double() - ref).abs().max())
    try:
        lib.ppok_debug_set_x6(ctypes.c_int(0))
        C0 = torch.ones(M, N, device="cuda")
        lib.ppok_debug_gemm(vp(A), vp(W), vp(C0), M, N, K, mode, 1, st)
        torch.cuda.synchronize()
        err_f32 = float((C0.double() - ref).abs().max())
    finally:
        lib.ppok_debug_set_x6(ctypes.c_int(1))
    assert torch.isfinite(C).all()
    assert err_pl <= 2.0 * err_f32 + 2.0 ** -22 * float(ref.abs().max()), (err_pl, err_f32)


@pytest.mark.parametrize("activation", ["selu", "relu", "lrelu", "tanh", "sigmoid", "crelu"])
def test_other_activations_forward_and_gradients(activation):
    """ActorCritic `activation` values other than elu (legged_robot_config.py:244; rsl_rl's "crelu" is nn.ReLU): inference
    means and one minibatch's gradients (GEMM epilogues act / act' computed from the stored outputs) against
    autograd on the torch restatement.  Tolerances as for elu: 2e-4 on means, 2e-3 relative / 2e-4 of the
    gradient scale absolute on gradients."""
    N, O, A, T = 256, 48, 12, 8
    policy = dict(POLICY, actor_hidden_dims=[96, 64, 32], critic_hidden_dims=[96, 64, 32], activation=activation)
    alg = dict(ALG, num_mini_batches=1)
    hip, ac, pt = _make(N, O, A, T, policy, alg)
    try:
        g = torch.Generator(device="cuda").manual_seed(11)
        obs = torch.randn(N, O, device="cuda", generator=g)
        np.testing.assert_allclose(hip.act_inference(obs).cpu().numpy(), ac.actor(obs).detach().cpu().numpy(), rtol=2e-4, atol=2e-5)
        _fill_rollout(hip, ac, T, N, O, A, g)
        hip.compute_returns(torch.randn(N, O, device="cuda", generator=g))
        hip._call("begin_update")
        torch.cuda.synchronize()
        idx = hip.t["perm"].long()[: T * N]
        hip._call("minibatch_backward", 0, 0)
        algo = pt.PPO(ac, clip_param=0.2, value_loss_coef=1.0, entropy_coef=0.01, learning_rate=1e-3, max_grad_norm=1.0,
                      use_clipped_value_loss=True, schedule="adaptive", desired_kl=0.01)
        flat = lambda name: hip.t[name].reshape(T * N, *hip.t[name].shape[2:])
        R = T * N
        batch = (flat("obs")[idx], flat("obs")[idx], flat("actions")[idx], flat("values")[idx].unsqueeze(-1),
                 flat("advantages")[idx].unsqueeze(-1), flat("returns")[idx].unsqueeze(-1),
                 flat("log_prob")[idx].unsqueeze(-1), flat("mu")[idx], hip.t["sigma"].clone().expand(R, A))
        ac.zero_grad()
        loss, kl, vl, sl = algo.minibatch_loss(*(b.clone() for b in batch))
        loss.backward()
        ref = torch.cat([p.grad.reshape(-1) for p in ac.parameters()])
        got = hip.t["grads"][: hip.num_params]
        torch.testing.assert_close(got, ref, rtol=2e-3, atol=2e-4 * float(ref.abs().max()))
        assert float((got - ref).norm() / ref.norm()) < 3e-4
    finally:
        hip.close()


@pytest.mark.parametrize("W", [2, 8])
def test_two_rank_update_equals_single_process_update(W):
    """SURVEY.md §8(e) without a second GPU: W HipPPO shards (world_size 2 with 64 envs each; world_size 8 -- BASELINE
    configs[3]'s rank count -- with 16 each) whose `all_reduce` is
    emulated by summing their buffers in-process, against one HipPPO over the 128 envs.  One minibatch per epoch, so both
    sides average over the same samples: global advantage normalisation (3-float moment reduce), [gradient | KL] reduce,
    /world in the optimiser kernels, KL-adaptive lr and Adam must leave all three with the same parameters
    (rtol 2e-4 / atol 2e-6: fp32 sums in a different order)."""
    from legged_gym_dev_amd.rl.ppo import HipPPO
    N, O, A, T = 128, 48, 12, 8
    policy = dict(POLICY, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    alg = dict(ALG, num_mini_batches=1, num_learning_epochs=2)
    torch.manual_seed(5)
    one = HipPPO(N, O, None, A, policy, alg, T, device="cuda:0", seed=5)
    n = N // W
    sh = [HipPPO(n, O, None, A, policy, alg, T, device="cuda:0", seed=5, world_size=W, rank=r) for r in range(W)]
    try:
        sd = {k: v.clone() for k, v in one.state_dict().items()}
        for s in sh:
            s.load_state_dict(sd)
        g = torch.Generator(device="cuda").manual_seed(8)
        for p in [one] + sh:
            p.inject_noise(1)
        for t in range(T):
            obs = torch.randn(N, O, device="cuda", generator=g)
            noise = torch.randn(N, A, device="cuda", generator=g)
            rew = torch.randn(N, device="cuda", generator=g)
            dones = (torch.rand(N, device="cuda", generator=g) < 0.1).to(torch.uint8)
            tos = ((torch.rand(N, device="cuda", generator=g) < 0.5) & (dones > 0)).to(torch.uint8)
            for p, sl in [(one, slice(0, N))] + [(sh[r], slice(r * n, (r + 1) * n)) for r in range(W)]:
                p.t["noise"].copy_(noise[sl])
                p.act(obs[sl].contiguous())
                p.process_env_step(rew[sl].contiguous(), dones[sl].contiguous(), {"time_outs": tos[sl].contiguous()})
        last = torch.randn(N, O, device="cuda", generator=g)

        def reduce_over_shards(name, n=None):
            def f(_view):
                tot = sh[0].t[name][:n].clone()
                for s in sh[1:]:
                    tot += s.t[name][:n]
                for s in sh:
                    s.t[name][:n].copy_(tot)
            return f
        one.compute_returns(last)
        # shards: the collective is called once per rank on its own view; emulate by summing after both have produced theirs
        for r, s in enumerate(sh):
            s._call("compute_returns", __import__("ctypes").c_void_p(last[r * n:(r + 1) * n].contiguous().data_ptr()))
        torch.cuda.synchronize()
        reduce_over_shards("adv_partial")(None)
        for s in sh:
            s._call("normalize_advantages")
        torch.testing.assert_close(torch.cat([s.t["advantages"] for s in sh], dim=1), one.t["advantages"], rtol=1e-5, atol=1e-6)
        one.update()
        for s in sh:
            s._call("begin_update")
        for epoch in range(2):
            for s in sh:
                s._call("minibatch_backward", epoch, 0)
            torch.cuda.synchronize()
            reduce_over_shards("grads", sh[0].num_reduce)(None)
            for s in sh:
                s._call("minibatch_step")
        for s in sh:
            s._call("end_update")
        torch.cuda.synchronize()
        ref = one.t["params"][: one.num_params]
        for s in sh:
            torch.testing.assert_close(s.t["params"][: s.num_params], ref, rtol=2e-4, atol=2e-6)
            assert abs(s.learning_rate - one.learning_rate) < 1e-12
        for s in sh[1:]:
            assert torch.equal(sh[0].t["params"], s.t["params"])          # ranks stay in lock-step exactly
    finally:
        one.close()
        for s in sh:
            s.close()


def test_device_randperm_is_a_permutation():
    """mini_batch_generator's randperm, drawn by k_randperm (keyed Feistel bijection + cycle walking): every update's
    index list is a permutation of range(T*N), differs from the previous update's, is not the identity, and is reused
    unchanged by all epochs of that update."""
    for N, T in ((64, 24), (4096, 24), (100, 7)):
        hip, _, _ = _make(N, 48, 12, T, policy=dict(POLICY, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32]),
                          alg=dict(ALG, num_mini_batches=4 if (N * T) % 4 == 0 else 1))
        try:
            n = (N * T // hip.cfg.num_mini_batches) * hip.cfg.num_mini_batches
            seen = []
            for u in range(3):
                hip._call("begin_update")
                torch.cuda.synchronize()
                p = hip.t["perm"][:n].cpu().numpy().copy()
                assert np.array_equal(np.sort(p), np.arange(n)), (N, T, u)
                assert not np.array_equal(p, np.arange(n))
                assert (p[1:] - p[:-1] == 1).mean() < 0.01          # no long identity runs
                for q in seen:
                    assert (p == q).mean() < 0.01
                seen.append(p)
                hip._call("minibatch_backward", 0, 0)
                hip._call("minibatch_step")
                torch.cuda.synchronize()
                assert np.array_equal(hip.t["perm"][:n].cpu().numpy(), p)  # epochs reuse it
                hip._call("end_update")
        finally:
            hip.close()


def test_fewer_envs_than_action_dims():
    """play.py's single-env path: with N < A the sigma the rollout was sampled with must still be recorded for all A action
    dimensions (it feeds the KL term of the update), and the update stays finite."""
    N, O, A, T = 4, 48, 12, 6
    hip, _, _ = _make(N, O, A, T, policy=dict(POLICY, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32]), alg=dict(ALG, num_mini_batches=1))
    try:
        g = torch.Generator(device="cuda").manual_seed(2)
        for t in range(T):
            hip.act(torch.randn(N, O, device="cuda", generator=g))
            hip.process_env_step(torch.randn(N, device="cuda", generator=g), torch.zeros(N, dtype=torch.uint8, device="cuda"), {})
        torch.cuda.synchronize()
        np.testing.assert_array_equal(hip.t["sigma"].cpu().numpy(), hip.param_views["std"].cpu().numpy())
        hip.compute_returns(torch.randn(N, O, device="cuda", generator=g))
        hip.update()
        st = hip.stats()
        assert np.isfinite(st["kl"]) and st["lr"] > 1e-5 * 1.01 and bool(torch.isfinite(hip.t["params"]).all())
    finally:
        hip.close()


def test_native_rccl_comm_single_rank():
    """lg_comm_* (RCCL resolved from the process's librccl.so) with one rank -- what a one-GPU box can execute: unique id,
    communicator, in-place all-reduce and broadcast on the caller's stream, and the learner's overlapped gradient reduction
    (lg_ppo_set_comm: per-layer buckets all-reduced on the communicator's stream while the backward GEMMs run).  With one rank
    every collective is the identity, so an update with the communicator attached must match one without it (tolerance: the
    float atomics of the gradient kernels, as in test_two_rank_update_equals_single_process_update).  The same entries with 2 to 4
    ranks, over a stand-in transport whose ranks are threads: tests/test_hip_comm_standin.py."""
    from legged_gym_dev_amd.rl.comm import NativeComm
    comm = NativeComm(0, 1)
    try:
        x = torch.arange(1000, dtype=torch.float32, device="cuda")
        comm.all_reduce(x)
        comm.broadcast(x, 0)
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), torch.arange(1000, dtype=torch.float32))
        assert comm.lib.lg_comm_rank(comm.ctx) == 0 and comm.lib.lg_comm_size(comm.ctx) == 1
        N, O, A, T = 512, 48, 12, 8
        outs = []
        for attach in (False, True):
            hip, ac, _ = _make(N, O, A, T, alg=dict(ALG, num_learning_epochs=2))
            try:
                g = torch.Generator(device="cuda").manual_seed(4)
                _fill_rollout(hip, ac, T, N, O, A, g)
                hip.compute_returns(torch.randn(N, O, device="cuda", generator=g))
                if attach:
                    comm.attach(hip)
                    hip.comm_timing(True)              # lg_ppo_comm_timing: the learner stream's wait for the buckets, per minibatch
                hip.update()
                torch.cuda.synchronize()
                if attach:                             # 2 epochs x 4 minibatches recorded; a one-rank wait is short but not negative
                    ms, n = hip.comm_wait_ms()
                    assert n == 8 and 0.0 <= ms < 50.0, (ms, n)
                    assert hip.comm_wait_ms() == (0.0, 0)      # read clears
                    hip.comm_timing(False)
                outs.append(hip.t["params"][: hip.num_params].clone())
                assert bool(torch.isfinite(outs[-1]).all())
                if attach:
                    comm.lib.lg_ppo_set_comm(hip.ctx, None)
            finally:
                hip.close()
        rel = float((outs[0] - outs[1]).norm() / outs[0].norm())
        assert rel < 2e-4, rel
    finally:
        comm.close()


@pytest.mark.parametrize("hidden", [[512, 256, 128], [128, 64, 32], [96, 40]])
def test_gradient_buckets_tile_the_reduce_buffer(hidden):
    """The overlapped RCCL reduction (lg_ppo_set_comm) sends one bucket per layer: W, b of both nets, and with the head's
    bucket std and the [KL | pad] tail.  Host-side check of the extents it hands to RCCL: over all layers they cover
    grads[0 : num_reduce) exactly once -- no gap, no overlap -- for the per-layer head ([96, 40]) and both fused-head widths.
    (With one rank every collective is the identity, so a wrong extent would pass every numerical test in this file; with 2 and 4
    ranks over a stand-in transport the extents decide the numbers: tests/test_hip_comm_standin.py)"""
    import ctypes as C
    pol = dict(POLICY, actor_hidden_dims=hidden, critic_hidden_dims=hidden)
    hip, _, _ = _make(64, 235, 12, 4, pol)
    try:
        cover = np.zeros(hip.num_reduce, np.int32)
        offs, cnts = (C.c_int64 * 4)(), (C.c_int64 * 4)()
        nl = len(hidden) + 1
        for l in range(nl):
            n = hip.lib.lg_ppo_debug_bucket_extents(hip.ctx, l, offs, cnts)
            assert n == (4 if l == nl - 1 else 2)
            for k in range(n):
                assert 0 <= offs[k] and offs[k] + cnts[k] <= hip.num_reduce
                cover[offs[k]:offs[k] + cnts[k]] += 1
        assert hip.lib.lg_ppo_debug_bucket_extents(hip.ctx, nl, offs, cnts) == -1
        assert (cover == 1).all(), (int((cover == 0).sum()), int((cover > 1).sum()))
    finally:
        hip.close()


def test_parameter_write_in_the_middle_of_a_rollout_reaches_act():
    """The one-launch act reads a fragment-order image of the weights: after load_state_dict() between two act() calls of one
    rollout (runner.load, a broadcast) the next act must sample from the NEW actor -- the image is rebuilt whenever the
    parameters were announced changed, not only at the first step of a rollout."""
    N, O, A, T = 256, 48, 12, 6
    hip, ac, pt = _make(N, O, A, T)
    try:
        g = torch.Generator(device="cuda").manual_seed(9)
        obs = torch.randn(N, O, device="cuda", generator=g)
        hip.act(obs)
        mu0 = hip.t["act_mu"].clone()
        hip.process_env_step(torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), {})
        sd = {k: v * 0.5 for k, v in hip.state_dict().items()}
        hip.load_state_dict(sd)
        ac.load_state_dict(sd)
        hip.act(obs)                                            # step 1 of the same rollout
        with torch.no_grad():
            want = ac.actor(obs)
        assert float((want - mu0).abs().max()) > 1e-3
        torch.testing.assert_close(hip.t["act_mu"], want, rtol=2e-5, atol=2e-5)
        torch.testing.assert_close(hip.act_inference(obs), want, rtol=2e-5, atol=2e-5)
    finally:
        hip.close()


def test_optimiser_step_equals_torch_adam_with_clip_and_adaptive_lr():
    """Known-answer test of lg_ppo_minibatch_step ("Adam step vs torch.optim.Adam"): the SAME gradients are written into
    the library's gradient buffer and into torch parameters' .grad; `clip_grad_norm_(max_grad_norm)` + `torch.optim.Adam.step()` with
    rsl_rl's KL-adaptive learning rate applied by hand must land on the library's parameters and Adam moments to float rounding, over
    six steps that exercise: clipping on / off, lr up (KL < desired / 2), lr down (KL > 2 desired), lr unchanged."""
    N, O, A, T = 64, 48, 12, 8
    pol = dict(POLICY, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    hip, ac, pt = _make(N, O, A, T, pol)
    n = hip.num_params
    params = list(ac.parameters())                      # std, actor..., critic...: the flat buffer's order
    assert sum(p.numel() for p in params) == n
    lr = 1e-3
    opt = torch.optim.Adam(params, lr=lr)
    hip._call("begin_update")
    g = torch.Generator(device="cuda").manual_seed(9)
    rows = T * N // ALG["num_mini_batches"]
    cases = [(5.0, 0.010), (0.01, 0.010), (0.3, 0.001), (0.3, 0.050), (2.0, 0.004), (0.02, 0.030)]   # (gradient scale, mean KL)
    for scale, kl in cases:
        grad = torch.randn(n, device="cuda", generator=g) * scale / n ** 0.5
        hip.t["grads"][:n].copy_(grad)
        hip.t["grads"][n] = kl * rows                   # the KL SUM of the minibatch rides behind the gradients
        if kl > 0.01 * 2.0:
            lr = max(1e-5, lr / 1.5)
        elif 0.0 < kl < 0.01 / 2.0:
            lr = min(1e-2, lr * 1.5)
        for pg in opt.param_groups:
            pg["lr"] = lr
        off = 0
        for p in params:
            p.grad = grad[off:off + p.numel()].view_as(p).clone()
            off += p.numel()
        total = torch.nn.utils.clip_grad_norm_(params, ALG["max_grad_norm"])
        opt.step()
        hip._call("minibatch_step")
        torch.cuda.synchronize()
        assert (float(total) > 1.0) == (scale >= 2.0)   # the cases on either side of the clip threshold are what they claim
        ref = pt.flat_params(ac)
        torch.testing.assert_close(hip.t["params"][:n], ref, rtol=3e-6, atol=1e-7)   # a step is lr ~ 1e-3: 1e-4 of a step
        assert abs(hip.learning_rate - lr) <= 3e-7 * lr                     # the library keeps lr as fp32 in HBM
        assert float(hip.t["grads"][: n + 2].abs().max()) == 0.0            # the step leaves the gradient buffer cleared
    st = opt.state_dict()["state"]
    m = torch.cat([st[i]["exp_avg"].reshape(-1) for i in range(len(params))])
    v = torch.cat([st[i]["exp_avg_sq"].reshape(-1) for i in range(len(params))])
    # (the norm is reduced in another order, so the clip coefficient may differ by an ulp: absolute band = rounding at the moments' scale)
    torch.testing.assert_close(hip.t["adam_m"][:n], m, rtol=3e-6, atol=1e-6 * float(m.abs().max()))
    torch.testing.assert_close(hip.t["adam_v"][:n], v, rtol=3e-6, atol=1e-6 * float(v.abs().max()))
    hip.close()


def test_gae_kernel_on_the_hand_computed_example():
    """The hand-computed GAE example that pins the torch restatement (tests/test_ppo_oracle.py: 3 steps x 2 envs, a done in the middle of
    env 0, gamma 0.9, lambda 0.5) through the LIBRARY: rewards / values / dones written into the rollout storage, the bootstrap values
    (1, -1) produced by a critic wired to return obs[0] - 3, then lg_ppo_compute_returns + lg_ppo_normalize_advantages."""
    N, O, A, T = 2, 48, 12, 3
    alg = dict(ALG, gamma=0.9, lam=0.5, num_mini_batches=2)
    pol = dict(POLICY, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    hip, ac, pt = _make(N, O, A, T, pol, alg)
    for k, v in hip.param_views.items():
        if k.startswith("critic."):
            v.zero_()
    for name in ("critic.0.weight", "critic.2.weight", "critic.4.weight"):
        hip.param_views[name][0, 0] = 1.0                                 # obs[0] > 0 passes the ELU layers unchanged
    hip.param_views["critic.4.bias"][0] = -3.0
    hip.params_changed()
    hip.t["rewards"].copy_(torch.tensor([[1.0, 2.0], [0.5, -1.0], [2.0, 0.0]]))
    hip.t["values"].copy_(torch.tensor([[0.5, 1.0], [1.5, 0.0], [-0.5, 2.0]]))
    hip.t["dones"].copy_(torch.tensor([[0, 0], [1, 0], [0, 0]], dtype=torch.uint8))
    last_obs = torch.zeros(N, O, device="cuda")
    last_obs[:, 0] = torch.tensor([4.0, 2.0])                             # V(s_T) = 1, -1
    hip._call("compute_returns", ctypes_ptr(last_obs))
    torch.cuda.synchronize()
    g, l = 0.9, 0.5
    a2 = 2.0 + g * 1.0 - (-0.5)
    a1 = 0.5 + 0.0 - 1.5                                                  # done at t = 1 cuts the bootstrap and the trace
    a0 = 1.0 + g * 1.5 - 0.5 + g * l * a1
    b2 = 0.0 + g * (-1.0) - 2.0
    b1 = -1.0 + g * 2.0 - 0.0 + g * l * b2
    b0 = 2.0 + g * 0.0 - 1.0 + g * l * b1
    adv = torch.tensor([[a0, b0], [a1, b1], [a2, b2]], device="cuda")
    torch.testing.assert_close(hip.t["returns"], adv + hip.t["values"], rtol=1e-6, atol=1e-6)
    torch.testing.assert_close(hip.t["advantages"], adv, rtol=1e-6, atol=1e-6)        # raw until normalize_advantages
    hip._call("normalize_advantages")
    torch.cuda.synchronize()
    torch.testing.assert_close(hip.t["advantages"], (adv - adv.mean()) / (adv.std() + 1e-8), rtol=1e-5, atol=1e-6)
    hip.close()


@pytest.mark.parametrize("sign,expected", [(1.0, (-0.7 - 1.0 - 1.2) / 3), (-1.0, (0.8 + 1.0 + 1.3) / 3)])
def test_clipped_surrogate_and_kl_known_answers_through_the_library(sign, expected):
    """The known-answer cases that pin the torch restatement (tests/test_ppo_oracle.py) through the LIBRARY's loss path: three rows whose
    importance ratios are 0.7, 1.0, 1.3 (the stored log-prob shifted by -ln r), advantages +1 (then -1), clip 0.2:
    mean surrogate = mean max(-A r, -A clip(r, 0.8, 1.2)); the KL of a policy with itself = sum_a ln(1 + 1e-5) (rsl_rl's epsilon inside the
    log); value loss 0 when returns = values.  Three loss statistics on the k_head_fused<32> path; the gradients of these branches, on
    every head kernel, are in tests/test_hip_ppo_loss.py."""
    N, O, A, T = 3, 48, 12, 1
    alg = dict(ALG, num_mini_batches=1, num_learning_epochs=1)
    pol = dict(POLICY, actor_hidden_dims=[64, 32], critic_hidden_dims=[64, 32])
    hip, ac, pt = _make(N, O, A, T, pol, alg)
    g = torch.Generator(device="cuda").manual_seed(1)
    obs = torch.randn(N, O, device="cuda", generator=g)
    hip.inject_noise(1)
    hip.t["noise"].zero_()                                                 # a = mu
    hip.act(obs)
    hip.process_env_step(torch.zeros(N, device="cuda"), torch.zeros(N, dtype=torch.uint8, device="cuda"), {})
    torch.cuda.synchronize()
    ratios = torch.tensor([0.7, 1.0, 1.3], device="cuda")
    hip.t["log_prob"].view(-1).sub_(torch.log(ratios))                      # exp(lp_new - lp_old) = r
    hip.t["advantages"].fill_(sign)
    hip.t["returns"].copy_(hip.t["values"])
    hip._call("begin_update")
    hip._call("minibatch_backward", 0, 0)
    hip._call("minibatch_step")
    torch.cuda.synchronize()
    st = hip.stats()
    assert abs(st["surrogate_loss_sum"] / st["n_updates"] - expected) < 2e-6, st
    assert abs(st["value_loss_sum"]) < 1e-10, st
    assert abs(st["kl"] - A * np.log1p(1e-5)) < 2e-7, st
    hip.close()
