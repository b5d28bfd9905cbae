"""process_env_step, compute_returns and normalize_advantages of the HIP learner against the float64 loops of tests/ppo_rollout_ref.py, at
env counts around the 256-lane block (1, 255, 256, 257, 300), 1 / 2 / 24 steps, dones at the first and the last step and on a whole
step, time-outs on / off / absent, rewards of mean 0 and of mean 3 std (where the one-pass variance cancels).  Bounds: derived in
tests/ppo_rollout_ref.py, shown to hold for an fp32 emulation of the kernels' order in tests/test_ppo_rollout_host.py.

Values are written into the storage after each act() (the critic's own output is the business of tests/test_hip_ppo_act.py); the
bootstrap values come from a critic wired to return obs[0] - 3 exactly.  The raw advantages are compared with the float64 scan; the
moments and the normalised advantages with float64 on the learner's OWN stored raw advantages, which isolates the summation order.
Episode bookkeeping is read back after every step: running sums bit-equal, totals within the atomics' rounding, the ring of the last 100
as multisets of the slots each step writes."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ppo_rollout_ref as rr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = rr.U
O, A = 8, 4
POLICY = {"actor_hidden_dims": [32, 32], "critic_hidden_dims": [32, 32], "activation": "elu", "init_noise_std": 1.0}
ALG = dict(value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01, num_learning_epochs=1, num_mini_batches=1,
           learning_rate=1e-3, schedule="adaptive", gamma=rr.GAMMA, lam=rr.LAM, desired_kl=0.01, max_grad_norm=1.0)


def _learner(N, T):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    hip = HipPPO(N, O, None, A, POLICY, ALG, T, device=DEV, seed=2)
    for k, v in hip.param_views.items():                      # V(obs) = obs[0] - 3 for obs[0] > 0 (ELU passes it unchanged)
        if k.startswith("critic."):
            v.zero_()
    for name in ("critic.0.weight", "critic.2.weight", "critic.4.weight"):
        hip.param_views[name][0, 0] = 1.0
    hip.param_views["critic.4.bias"][0] = -3.0
    hip.params_changed()
    return hip


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _rollout(hip, s, N, T, check_episodes=True):
    """Drives act / process_env_step with the scenario's env outputs; checks the episode bookkeeping after every step."""
    ep = rr.Episodes(N)
    ring = {}                                               # slot -> (return, length) wherever one episode alone can have landed
    g = torch.Generator(device=DEV).manual_seed(1)
    for t in range(T):
        hip.act(torch.randn(N, O, device=DEV, generator=g))
        hip.t["values"][t].copy_(_dev(s["values"][t]))
        infos = {} if s["tos"] is None else {"time_outs": _dev(s["tos"][t])}
        hip.process_env_step(_dev(s["rew"][t]), _dev(s["dones"][t]), infos)
        if not check_episodes:
            continue
        torch.cuda.synchronize()
        slots, pairs = ep.step(s["rew"][t], s["dones"][t])
        assert np.array_equal(hip.t["cur_reward_sum"].cpu().numpy(), ep.cr), f"step {t}: cur_reward_sum"
        assert np.array_equal(hip.t["cur_episode_len"].cpu().numpy(), ep.cl), f"step {t}: cur_episode_len"
        st = hip.t["ep_stats"].cpu().double().numpy()
        assert abs(st[0] - ep.sum_r) <= (ep.count + 1) * U * ep.sum_abs, f"step {t}: ep_stats[0] {st[0]} against {ep.sum_r}"
        assert st[1] == ep.sum_l and st[2] == ep.count and int(hip.t["ep_ring_count"][0]) == ep.count, f"step {t}: episode totals"
        got = hip.t["ep_ring"].cpu().numpy()
        if len(pairs) <= 100:                               # each slot written once this step: the slots hold the step's pairs in some order
            assert sorted(zip(got[0, slots].tolist(), got[1, slots].tolist())) == pairs, f"step {t}: ring slots {slots[:4]}.."
            for k in slots:
                ring[k] = (float(got[0, k]), float(got[1, k]))
        else:                                               # the ring wrapped within one step: every slot holds some episode of this step
            rets, lens = {p[0] for p in pairs}, {p[1] for p in pairs}
            assert all(x in rets for x in got[0].tolist()) and all(x in lens for x in got[1].tolist()), f"step {t}: wrapped ring"
            ring = {k: (float(got[0, k]), float(got[1, k])) for k in range(100)}
        for k, pair in ring.items():                        # what earlier steps left and this one did not overwrite is unchanged
            assert (float(got[0, k]), float(got[1, k])) == pair, f"step {t}: ring slot {k} changed"
        assert not got[:, [k for k in range(100) if k not in ring]].any(), f"step {t}: a ring slot nobody owns was written"
    return ep


def _returns(hip, s, N, T):
    last_obs = torch.zeros(N, O, device=DEV)
    last_obs[:, 0] = _dev(s["last_x"])
    hip._call("compute_returns", ctypes.c_void_p(last_obs.data_ptr()))
    torch.cuda.synchronize()
    raw = {k: hip.t[k].cpu().numpy().copy() for k in ("rewards", "returns", "advantages", "dones")}
    hip._call("normalize_advantages")
    torch.cuda.synchronize()
    raw["norm"] = hip.t["advantages"].cpu().numpy().copy()
    raw["stats"] = hip.t["stats"].cpu().numpy().copy()
    return raw


def _check_returns(case, s, got):
    N, T = case[0], case[1]
    ref = rr.returns64(s["rew"], s["dones"], s["tos"], s["values"], s["last_v"], rr.GAMMA, rr.LAM)
    assert np.array_equal(got["dones"], s["dones"])
    for key, want, bound in (("rewards", ref["rewards"], ref["E_r"]), ("returns", ref["returns"], ref["E_ret"]), ("advantages", ref["adv"], ref["E_a"])):
        diff = np.abs(got[key].astype(np.float64) - want)
        used = float((diff / np.maximum(bound, 1e-300)).max())
        print(f"RETURNS {rr.case_id(case)} {key} worst diff/bound {used:.4f}")
        assert (diff <= bound).all(), f"{key}: {used:.3f}x the bound"
    mo = rr.moments64(got["advantages"], N, T)
    print(f"MOMENTS {rr.case_id(case)} mean {mo['mean']:.4f} std {mo['std']:.4f} 1+mean^2/var {mo['factor']:.2f} "
          f"|mean err|/bound {abs(float(got['stats'][6]) - mo['mean']) / mo['e_mean']:.4f} |std err|/bound {abs(float(got['stats'][7]) - mo['std']) / max(mo['e_std'], 1e-300):.4f}")
    assert abs(float(got["stats"][6]) - mo["mean"]) <= mo["e_mean"] and abs(float(got["stats"][7]) - mo["std"]) <= mo["e_std"]
    want, bound = rr.normalised64(got["advantages"], mo)
    diff = np.abs(got["norm"].astype(np.float64) - want)
    assert np.isfinite(got["norm"]).all() and (diff <= bound).all(), f"normalised advantages: {float((diff / np.maximum(bound, 1e-300)).max()):.3f}x the bound"


@pytest.mark.parametrize("case", rr.CASES, ids=rr.case_id)
def test_returns_and_bookkeeping_match_float64(case):
    N, T = case[0], case[1]
    s = rr.scenario(*case)
    hip = _learner(N, T)
    try:
        ep = _rollout(hip, s, N, T)
        if N == 300 and T == 24:
            assert ep.count > 400                           # the ring of 100 wrapped more than once
        _check_returns(case, s, _returns(hip, s, N, T))
    finally:
        hip.close()


def test_deterministic_mode_is_bit_identical_and_inside_the_same_bounds():
    """mean / std = 3 rewards at 300 envs x 24 steps under set_deterministic(True): two runs agree bit for bit (the moments are summed in
    fixed point, any order), and each sits inside the bounds of the float atomics' path."""
    case = (300, 24, "on", "three")
    N, T = case[0], case[1]
    s = rr.scenario(*case)
    runs = []
    for _ in range(2):
        hip = _learner(N, T)
        try:
            hip.set_deterministic(True)
            _rollout(hip, s, N, T, check_episodes=False)
            got = _returns(hip, s, N, T)
            _check_returns(case, s, got)
            runs.append(got)
        finally:
            hip.close()
    for k in ("rewards", "returns", "advantages", "norm"):
        assert np.array_equal(runs[0][k], runs[1][k]), k
    assert np.array_equal(runs[0]["stats"][6:8], runs[1]["stats"][6:8])
