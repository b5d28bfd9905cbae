"""CPU conditions on the inputs of tests/test_hip_ppo_update.py (tests/ppo_update_ref.py builds them): every row of every case sits
away from every branch boundary of the PPO loss by the margins of tests/test_ppo_loss_host.py, every (surrogate, value) regime pair
occurs in every case of 193 rows or more, every case has sizes HipPPO accepts and names a launch for every GEMM of its pass, and the
fp32 torch restatement alone, against the float64 one on the same inputs, uses at most 25 % of every band the GPU test asserts --
every parameter tensor's own relative-norm band included -- so a tensor that misses its band on the GPU is wrong, not unlucky."""
import pytest
import torch

from tests import ppo_loss_ref as plr
from tests import ppo_update_ref as pur
from tests.test_ppo_loss_host import _check_margins_and_labels


def test_matrix_is_what_the_gpu_test_expects():
    assert set(pur.TRACES) == set(pur.BY_ID)
    assert set(pur.DETERMINISTIC) <= set(pur.BY_ID)
    reached = set()
    for c in pur.CASES:
        assert pur.accepted_by_hip_ppo(c) is None, (pur.case_id(c), pur.accepted_by_hip_ppo(c))
        rows = pur.parse_trace(pur.TRACES[pur.case_id(c)])
        nl = len(c["hidden"]) + 1
        kinds = [r[0] for r in rows]
        nf = kinds.count(0)
        assert nf in (nl - 1, nl) and kinds[:nf] == [0] * nf, "forward: every hidden layer, the head layer when it is not fused"
        assert kinds[nf:] == [2, 1] * (nf - 1) + [2], "backward: dW, dX per layer from the top down, the first layer's dW last"
        reached |= pur.paths_of(c)
    want = {"k_gemm_glds", "k_gemm planes-1 64x64", "k_gemm planes-2 64x64", "k_gemm planes-2 128x128", "k_gemm fp32-operand 64x64",
            "k_gemm_dw_t 64x64 1 slice", "k_gemm_dw_t 64x64 8+ slices", "k_gemm_dw_t 128x128"}
    assert want <= reached, want - reached


@pytest.mark.parametrize("c", pur.CASES, ids=pur.case_id)
def test_rows_keep_off_branch_boundaries_and_cover_regimes(c):
    case = pur.build_for(c)
    assert case["obs"].shape == (c["R"] * c["nmb"], c["O"])
    assert ("critic_obs" in case) == (c["OC"] is not None) and (c["OC"] is None or case["critic_obs"].shape[1] == c["OC"] != c["O"])
    sur, val = _check_margins_and_labels(case)
    if c["R"] >= 193:
        n = c["R"] * c["nmb"]
        for s in (plr.FLOWS, plr.CLIPPED):
            for v in (plr.TIE, plr.UNCLIPPED_WINS, plr.CLIPPED_WINS):
                share = int(((sur == s) & (val == v)).sum()) / n
                assert share >= 0.03, (plr.SURROGATE_NAMES[s], plr.VALUE_NAMES[v], share)


@pytest.mark.parametrize("c", pur.CASES, ids=pur.case_id)
def test_fp32_restatement_uses_at_most_25_percent_of_every_band(c):
    case, alg = pur.build_for(c), pur.alg_for(c)
    R, nmb, mb = c["R"], c["nmb"], c["mb"]
    if nmb == 1:
        rows, ref = None, pur.reference_cached(pur.case_id(c))
    else:                                               # the GPU test takes the rows of the device permutation
        rows = torch.arange(mb * R, (mb + 1) * R)
        ref = pur.reference(case, alg, rows)
    got = pur.reference(case, alg, rows, dtype=torch.float32)
    errs = pur.band_errors(got, ref, case)
    assert {"grad.norm." + k for k in case["params"]} <= set(errs)       # no tensor without a band of its own
    print({k: "%.3g of %.3g" % v for k, v in errs.items()})
    over = {k: v for k, v in errs.items() if v[0] > pur.FP32_SHARE * v[1]}
    assert not over, over
    assert all(bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0 for g in ref["grads"].values())
