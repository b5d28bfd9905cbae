"""The minibatch gathers of the PPO update, looked at directly (lg_ppo_debug_mb_sets): k_gather (action counts off the 4-grid), k_gather4
(float4 rows; row_copy for observation widths off the 4-grid, whose second trip needs more than 256 columns; the float4 loop's second
trip needs more than 32 pieces per row) and the gather-ahead blocks of k_opt_prepare, which fill the OTHER buffer set with the following
minibatch while the optimiser step runs.

After begin_update and minibatch_backward(0, mb) the current set must hold the storage rows perm[mb R + r], bit for bit, with every pad
column zero.  After minibatch_step the other set must hold minibatch mb + 1 (action counts on the 4-grid; otherwise nothing is gathered
ahead), and the next minibatch_backward must read that set: the storage is changed in between, so a second gather would show."""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
POLICY = {"activation": "elu", "init_noise_std": 1.0}
ALG = dict(value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01, num_learning_epochs=1, num_mini_batches=3,
           learning_rate=1e-3, schedule="adaptive", gamma=0.99, lam=0.95, desired_kl=0.01, max_grad_norm=1.0)
T = 3                                      # three minibatches of R = N rows

# (A, O, OC, R): A in {3, 12, 16}; O in {48, 65, 235, 301, 320}; a privileged critic with 169 or 400 columns; R in {1, 7, 8, 9, 300}
CASES = [(12, 48, None, 300), (12, 65, 169, 9), (12, 235, None, 8), (12, 301, None, 7), (12, 320, 400, 300), (12, 48, 400, 1),
         (16, 301, 400, 7), (16, 320, 169, 1), (16, 235, None, 300), (16, 65, None, 9), (16, 48, 169, 8),
         (3, 48, None, 9), (3, 301, 400, 8), (3, 65, 169, 300), (3, 320, None, 1), (3, 235, 169, 7)]


def test_cases_cover_the_sizes():
    assert {c[0] for c in CASES} == {3, 12, 16} and {c[1] for c in CASES} == {48, 65, 235, 301, 320}
    assert {c[2] for c in CASES} == {None, 169, 400} and {c[3] for c in CASES} == {1, 7, 8, 9, 300}
    g4 = [c for c in CASES if c[0] % 4 == 0]
    assert any(c[1] > 256 and c[1] & 3 for c in g4)                                            # row_copy's second trip
    pieces = lambda c: (0 if c[1] & 3 else c[1] // 4) + (c[2] // 4 if c[2] and not c[2] & 3 else 0) + 2 * (c[0] // 4) + 1
    assert any(pieces(c) > 64 for c in g4) and any(pieces(c) <= 32 for c in g4)                 # one, and more than two, trips of the float4 loop


def _expect(store, idx, Op, OCp, priv):
    """What a buffer set must hold for the storage rows idx: payload columns from the storage, pad columns zero."""
    R = idx.numel()
    obs = torch.zeros(R, Op, device=DEV)
    obs[:, :store["obs"].shape[1]] = store["obs"][idx]
    want = dict(obs=obs, actions=store["actions"][idx], mu=store["mu"][idx],
                scalars=torch.stack([store[k][idx] for k in ("values", "returns", "advantages", "log_prob")], 1))
    if priv:
        want["critic_obs"] = torch.zeros(R, OCp, device=DEV)
        want["critic_obs"][:, :store["critic_obs"].shape[1]] = store["critic_obs"][idx]
    return want


def _same(got, want, what):
    for k, w in want.items():
        assert got[k].shape == w.shape and torch.equal(got[k], w), f"{what}: {k} differs in {int((got[k] != w).sum())} of {w.numel()} elements"


@pytest.mark.parametrize("A,O,OC,R", CASES, ids=[f"A{c[0]}-O{c[1]}-OC{c[2]}-R{c[3]}" for c in CASES])
def test_minibatch_sets_hold_the_permuted_storage_rows(A, O, OC, R):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    N = R
    hip = HipPPO(N, O, OC, A, dict(POLICY, actor_hidden_dims=[32, 32], critic_hidden_dims=[32, 32]), ALG, T, device=DEV, seed=4)
    try:
        g = torch.Generator(device=DEV).manual_seed(O + A + R)
        names = ("obs", "actions", "mu", "values", "returns", "advantages", "log_prob") + (("critic_obs",) if OC else ())
        for k in names:
            hip.t[k].copy_(torch.randn(hip.t[k].shape, device=DEV, generator=g))
        hip.t["sigma"].fill_(1.0)
        flat = lambda k: hip.t[k].reshape(T * N, *hip.t[k].shape[2:])
        store = {k: flat(k).clone() for k in names}
        hip._call("begin_update")
        torch.cuda.synchronize()
        perm = hip.t["perm"].long().clone()
        assert sorted(perm.tolist()) == list(range(T * N))
        ahead = A % 4 == 0
        for mb in range(T):
            hip._call("minibatch_backward", 0, mb)
            torch.cuda.synchronize()
            cur, other = hip.debug_mb_sets()
            Op, OCp = cur["obs"].shape[1], cur["critic_obs"].shape[1]
            assert Op == (O + 31) // 32 * 32 and OCp == ((OC or O) + 31) // 32 * 32 and cur["obs"].shape[0] == R
            if mb and ahead:                               # it read the set gathered ahead: from the storage as it was BEFORE the change below
                assert cur["obs"].data_ptr() == ahead_ptr, "minibatch_backward did not switch to the set gathered ahead"
                _same(cur, _expect(before, perm[mb * R:(mb + 1) * R], Op, OCp, OC), f"minibatch {mb} (gathered ahead)")
            else:
                _same(cur, _expect(store, perm[mb * R:(mb + 1) * R], Op, OCp, OC), f"minibatch {mb} (gathered by the backward)")
            hip._call("minibatch_step")
            torch.cuda.synchronize()
            cur, other = hip.debug_mb_sets()
            nxt = (mb + 1) % T
            if ahead:
                _same(other, _expect(store, perm[nxt * R:(nxt + 1) * R], Op, OCp, OC), f"minibatch {nxt} gathered ahead by the step of {mb}")
                ahead_ptr = other["obs"].data_ptr()
            # change the storage: a gather after this point is told from one before it
            before = store
            store = {k: v + 1.0 for k, v in store.items()}
            for k in names:
                flat(k).copy_(store[k])
            assert torch.equal(hip.t["perm"].long(), perm)
    finally:
        hip.close()
