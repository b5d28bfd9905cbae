"""CPU conditions on the inputs and references of tests/test_hip_recurrent.py (tests/recurrent_loss_ref.py builds them), on every
case of the GPU matrix:

* the literal split / pad / unpad generator (recurrent_ref) and the step loop that reloads at t = 0 and after every done agree per
  tensor to 1e-10 in float64, with saved states unrelated to the recurrence -- the equivalence the GPU schedule relies on.  At one
  env per minibatch this is the check that a bare squeeze() in recurrent_ref.minibatch_loss fails (log-probabilities (T, 1) against
  (T,) broadcast to (T, T): relative gradient difference 0.5 .. 6);
* every row of the minibatch is off every branch boundary of the loss and the rows cover all six regime pairs;
* every tensor's float64 gradient carries signal (at least 1e-4 of the whole gradient's norm), so a per-tensor relative bound means
  something;
* the fp32 torch restatement alone stays below a quarter of every band the GPU test asserts (a band may only ever be raised to four
  times the restatement's own error: below a quarter that never applies), so a kernel that misses a band is wrong, not unlucky;
* every dones pattern does what its name says."""
import pytest
import torch

from tests import ppo_loss_ref as plr
from tests import recurrent_loss_ref as rl

CLIP = rl.CLIP


@pytest.mark.parametrize("c", rl.CASES, ids=rl.case_id)
def test_literal_generator_and_step_loop_agree_in_float64(c):
    case = rl.build_for(c)
    ref, loop = rl.reference(case), rl.reference_loop(case)
    assert list(ref["grads"]) == list(loop["grads"])
    for k, r in ref["grads"].items():
        assert bool(torch.isfinite(r).all()), k
        assert rl._rel(loop["grads"][k], r) < 1e-10, (k, rl._rel(loop["grads"][k], r))
    for k in ("kl", "value_loss", "surrogate_loss"):
        assert abs(loop[k] - ref[k]) <= 1e-10 * max(1.0, abs(ref[k])), k


def test_one_env_minibatch_keeps_its_env_axis():
    """Why the squeezes of recurrent_ref.minibatch_loss name their axis: at mbs = 1 a bare squeeze leaves (T,) old
    log-probabilities, which broadcast against the (T, 1) new ones into (T, T)."""
    case = rl.build_for(rl.by_label("one_env_last_minibatch"))
    m = case["meta"]
    assert m["mbs"] == 1
    from tests import recurrent_ref as rr
    b = rr.recurrent_minibatch(rl.storage_of(case, torch.float64), m["mb"], m["nmb"])
    assert tuple(b["log_prob"].shape) == (m["T"], 1, 1)
    assert tuple(torch.squeeze(b["log_prob"]).shape) == (m["T"],) and tuple(torch.squeeze(b["log_prob"], -1).shape) == (m["T"], 1)


def _check_margins_and_labels(case):
    """The assertions of tests/test_ppo_loss_host.py on the minibatch's rows."""
    q = rl.row_quantities(case)
    ratio, d, l1, l2, adv = q["ratio"], q["d"], q["l1"], q["l2"], q["adv"]
    assert float(torch.minimum((ratio - (1 + CLIP)).abs(), (ratio - (1 - CLIP)).abs()).min()) > 1e-3
    assert float((d.abs() - CLIP).abs().min()) > 1e-3
    outside = d.abs() > CLIP
    if bool(outside.any()):
        assert float((l1 - l2).abs()[outside].min()) > 1e-3
    assert float(adv.abs().min()) >= 0.1
    sur = ((adv > 0) & (ratio > 1 + CLIP)) | ((adv < 0) & (ratio < 1 - CLIP))
    assert torch.equal(sur.long(), case["surrogate_regime"])
    val = torch.where(~outside, plr.TIE, torch.where(l1 > l2, plr.UNCLIPPED_WINS, plr.CLIPPED_WINS))
    assert torch.equal(val, case["value_regime"])
    t = case["targets"]
    assert float((ratio - t[:, 0]).abs().max()) < 1e-5 and float((d - t[:, 2]).abs().max()) < 1e-5
    return sur.long(), val


@pytest.mark.parametrize("c", rl.CASES, ids=rl.case_id)
def test_rows_keep_off_branch_boundaries_and_cover_regimes(c):
    case = rl.build_for(c)
    sur, val = _check_margins_and_labels(case)
    R = case["meta"]["R"]
    assert sur.numel() == R
    if R >= len(plr.TABLE):                             # at least one full pass through the table
        for s in (plr.FLOWS, plr.CLIPPED):
            for v in (plr.TIE, plr.UNCLIPPED_WINS, plr.CLIPPED_WINS):
                share = int(((sur == s) & (val == v)).sum()) / R
                assert share >= 0.03, (plr.SURROGATE_NAMES[s], plr.VALUE_NAMES[v], share)


def test_some_case_covers_all_regimes():
    """The coverage check above is not vacuous: the 3120-row and the 16 448-row case pass through the whole table."""
    assert sum(c[1] * (c[2] // c[3]) >= len(plr.TABLE) for c in rl.CASES) >= 2


@pytest.mark.parametrize("c", rl.CASES, ids=rl.case_id)
def test_every_tensor_has_signal(c):
    ref = rl.reference(rl.build_for(c))
    total = float(torch.cat([g.reshape(-1) for g in ref["grads"].values()]).norm())
    assert total > 0
    share = {k: float(g.norm()) / total for k, g in ref["grads"].items()}
    print("signal", rl.case_id(c), {k: "%.3g" % v for k, v in share.items()})
    low = {k: v for k, v in share.items() if v < 1e-4}
    assert not low, low


@pytest.mark.parametrize("c", rl.CASES, ids=rl.case_id)
def test_fp32_restatement_uses_at_most_a_quarter_of_every_band(c):
    case = rl.build_for(c)
    ref = rl.reference(case)
    got = rl.reference(case, torch.float32)
    errs = rl.band_errors(got, ref, case)
    print("restatement_errors", rl.case_id(c), {k: "%.3g/%.3g" % v for k, v in errs.items()})
    print("restatement_worst", rl.case_id(c), "%s %.3g" % rl.worst(errs),
          "worst norm %.3g" % max(v[0] for k, v in errs.items() if k.startswith("norm.")))
    over = {k: v for k, v in errs.items() if v[0] > 0.25 * v[1]}
    assert not over, over


@pytest.mark.parametrize("c", rl.CASES, ids=rl.case_id)
def test_dones_pattern_does_what_its_name_says(c):
    case = rl.build_for(c)
    m = case["meta"]
    T, N, mbs, pattern = m["T"], m["N"], m["mbs"], m["pattern"]
    d = case["dones"]
    assert d.dtype == torch.uint8 and tuple(d.shape) == (T, N) and int(d.max()) <= 1
    sl = slice(m["mb"] * mbs, (m["mb"] + 1) * mbs)
    mine = d[:, sl]
    reloads = int(rl.reload_mask(mine).sum())           # steps of the minibatch that start from their saved state
    chain = rl.longest_carry_chain(mine)
    if pattern == "none":
        assert int(d.sum()) == 0 and reloads == mbs and chain == T
    elif pattern == "all":
        assert int(d.sum()) == T * N and reloads == T * mbs and chain == 1
    elif pattern == "last":
        assert int(d[:-1].sum()) == 0 and int(d[-1].sum()) == N and reloads == mbs and chain == T
    elif pattern == "runs":
        for e in range(N):
            on = d[:, e].nonzero().reshape(-1)
            assert on.numel() in (2, 3) and int(on[-1] - on[0]) == on.numel() - 1, e     # one run of two or three steps
        assert mbs < reloads < T * mbs
    else:
        assert pattern == "rand"
        assert int(d[:, 0].sum()) == T                                       # env 0 done at every step
        if N > 1:
            assert int(d[:, 1].sum()) == 0                                   # env 1 never
        if N > 3:
            assert int(d[0, 2]) == 1 and int(d[T - 1, 3]) == 1
        assert bool(d[0].any()) and bool(d[T - 1].any())
        if mbs >= 4:                                                         # ... and all four kinds inside the checked minibatch
            assert int(mine[:, 0].sum()) == T and int(mine[:, 1].sum()) == 0 and int(mine[0, 2]) == 1 and int(mine[T - 1, 3]) == 1
            assert chain == T
        if T > 1 and mbs > 1:
            assert mbs < reloads < T * mbs                                   # some steps reload, some carry
        frac = float(d.float().mean())
        assert 0.1 < frac < 0.75 or N * T < 40


def test_step_reference_matches_nn_lstm():
    """lstm_cell / step_reference against nn.LSTM and the restatement's modules in float64."""
    from tests import recurrent_ref as rr
    torch.manual_seed(0)
    ac = rr.ActorCriticRecurrent(7, 9, 3, [16, 8], [16, 8], "elu", rnn_hidden_size=32).double()
    x, xc = torch.randn(5, 7, dtype=torch.float64), torch.randn(5, 9, dtype=torch.float64)
    st = [0.5 * torch.randn(5, 32, dtype=torch.float64) for _ in range(4)]
    noise = torch.randn(5, 3, dtype=torch.float64)
    out = rl.step_reference(ac.state_dict(), "elu", x, xc, *st, noise=noise)
    with torch.no_grad():
        ac.memory_a.hidden_states = (st[0].unsqueeze(0), st[1].unsqueeze(0))
        ac.memory_c.hidden_states = (st[2].unsqueeze(0), st[3].unsqueeze(0))
        ac.act(x)
        v = ac.evaluate(xc).squeeze(-1)
        lp = ac.get_actions_log_prob(out["actions"])
    (ha, ca), (hc, cc) = ac.get_hidden_states()
    for got, want in ((out["h_a"], ha[0]), (out["c_a"], ca[0]), (out["h_c"], hc[0]), (out["c_c"], cc[0]), (out["mu"], ac.action_mean),
                      (out["value"], v), (out["log_prob"], lp)):
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12)
