"""CPU conditions on the inputs of tests/test_hip_ppo_loss.py (tests/ppo_loss_ref.py builds them): every row of every case of
the GPU matrix sits away from every branch boundary of the PPO loss, the rows cover every (surrogate, value) regime pair, the
single-regime cases are what they claim, and the fp32 torch restatement alone, against the float64 one on the same case, stays
at or below 5 % of every band the GPU test asserts -- so a kernel that misses a band is wrong, not unlucky."""
import pytest
import torch

from tests import ppo_loss_ref as plr

CLIP = plr.CLIP


def _check_margins_and_labels(case):
    q = plr.row_quantities(case)
    ratio, d, l1, l2, adv = q["ratio"], q["d"], q["l1"], q["l2"], q["adv"]
    # margins, no row excluded (the table gives 0.1, 0.1 and at least 0.02; 1e-3 is two orders above the nets' fp32 forward error)
    assert float(torch.minimum((ratio - (1 + CLIP)).abs(), (ratio - (1 - CLIP)).abs()).min()) > 1e-3
    assert float((d.abs() - CLIP).abs().min()) > 1e-3
    outside = d.abs() > CLIP
    if bool(outside.any()):
        assert float((l1 - l2).abs()[outside].min()) > 1e-3
    assert float(adv.abs().min()) >= 0.1
    # the float64 computation lands every row in the regime the table assigned to it
    sur = ((adv > 0) & (ratio > 1 + CLIP)) | ((adv < 0) & (ratio < 1 - CLIP))
    assert torch.equal(sur.long(), case["surrogate_regime"])
    val = torch.where(~outside, plr.TIE, torch.where(l1 > l2, plr.UNCLIPPED_WINS, plr.CLIPPED_WINS))
    assert torch.equal(val, case["value_regime"])
    t = case["targets"]
    assert float((ratio - t[:, 0]).abs().max()) < 1e-5 and float((d - t[:, 2]).abs().max()) < 1e-5
    return sur.long(), val


def test_table_and_regime_rule():
    assert len(plr.TABLE) == 784 and len(plr.SINGLE_REGIME_TABLE) == 64
    pairs = {}
    for t in plr.TABLE:
        pairs[plr.regime_of(*t)] = pairs.get(plr.regime_of(*t), 0) + 1
    assert len(pairs) == 6 and min(pairs.values()) >= 0.08 * len(plr.TABLE), pairs
    for r, adv, d, e in plr.SINGLE_REGIME_TABLE:
        assert abs(d) > CLIP and ((adv > 0 and r > 1 + CLIP) or (adv < 0 and r < 1 - CLIP))


@pytest.mark.parametrize("c", plr.CASES, ids=plr.case_id)
def test_rows_keep_off_branch_boundaries_and_cover_regimes(c):
    case = plr.build_for(c)
    R, nmb = c[6], c[7]
    sur, val = _check_margins_and_labels(case)
    if R >= 193:                                        # with more than one minibatch any R rows may be picked: coverage of the pool
        n = R * nmb
        for s in (plr.FLOWS, plr.CLIPPED):
            for v in (plr.TIE, plr.UNCLIPPED_WINS, plr.CLIPPED_WINS):
                share = int(((sur == s) & (val == v)).sum()) / n
                assert share >= 0.03, (plr.SURROGATE_NAMES[s], plr.VALUE_NAMES[v], share)


@pytest.mark.parametrize("c", plr.CASES, ids=plr.case_id)
def test_fp32_restatement_uses_at_most_5_percent_of_every_band(c):
    case, alg = plr.build_for(c), plr.alg_for(c)
    R, nmb, mb = c[6], c[7], c[8]
    rows = None if nmb == 1 else torch.arange(mb * R, (mb + 1) * R)     # the GPU test takes the rows of the device permutation
    ref = plr.reference(case, alg, rows)
    got = plr.reference(case, alg, rows, dtype=torch.float32)
    errs = plr.band_errors(got, ref, case)
    print({k: "%.3g of %.3g" % v for k, v in errs.items()})
    over = {k: v for k, v in errs.items() if v[0] > 0.05 * v[1]}
    assert not over, over
    assert all(bool(torch.isfinite(g).all()) for g in ref["grads"].values())


@pytest.mark.parametrize("label", plr.LABELS)
def test_single_regime_case_has_only_the_entropy_gradient(label):
    hidden, critic, act = plr.PATHS[label]
    A = 16 if label == "net128_16" else 12
    case = plr.single_regime_case(8, A, hidden, act, 193, 11, critic)
    sur, val = _check_margins_and_labels(case)
    assert bool((sur == plr.CLIPPED).all()) and bool((val == plr.CLIPPED_WINS).all())
    ref = plr.reference(case, plr.ALG)
    for k, g in ref["grads"].items():
        if k == "std":
            want = -plr.ALG["entropy_coef"] / case["params"]["std"].double()
            torch.testing.assert_close(g, want, rtol=1e-12, atol=0)
        else:
            assert torch.equal(g, torch.zeros_like(g)), k
