"""One whole feed-forward PPO minibatch of the HIP learner against float64, tensor by tensor: lg_ppo_minibatch_backward = sched::forward,
the head, sched::backward (legged_gym_dev_amd/csrc/ppo_sched.hip, ppo_api.hip), then lg_ppo_minibatch_step.  The loss heads, every GEMM
launch, the gathers and the optimiser step have float64 tests of their own (tests/test_hip_ppo_loss.py, test_hip_ppo_gemm.py,
test_hip_recurrent.py); this file pins what joins them: which operand, leading dimension, pad width, plane image, aux, colsum and nstore
every launch of the chain gets, at depths 1 .. 4, with the product's widths at row counts off every tile grid, a privileged critic,
unequal actor / critic widths, widths the plane and LDS-DMA paths refuse, every activation, the minibatch gathered ahead by the
optimiser step, the side stream on and off, and deterministic mode.

Cases, reference and bands: tests/ppo_update_ref.py; what the bands rest on: tests/test_ppo_update_host.py.  Per case the parameters and
the storage are written verbatim; compared against oracle.ppo_torch.PPO.minibatch_loss on a float64 model: EVERY parameter tensor of
both nets and std in a relative-norm band of its own (2e-4; 3e-4 for an activation other than elu), the element-wise band over the
whole vector, the KL sum and the two loss means.  The launch trace of the pass (ppok_debug_gemm_trace: kernel and reduction slices of
every GEMM launch as the launchers report them) must equal what the case names (ppo_update_ref.TRACES).

One run on the MI355X (profiles/ppo_update_f64_errors.txt has every error / bound pair): all 29 cases and the 3 deterministic ones
pass, every trace as named.  Worst share of a tensor's own band used, over the cases whose trace holds the path (a case reaches
several paths, so the figure bounds the path from above):
    path                                      worst error / bound   tensor, case
    k_gemm fp32-operand 64x64                 0.0056                actor.2.weight, 96x44x20 R300
    k_gemm_dw_t 64x64, 1 slice                0.0090                actor.6.bias, 512x256x128 O235 R65
    k_gemm_dw_t 64x64, 2-7 slices             0.0073                actor.0.bias, 512x256x128 O235 R1000
    k_gemm_glds, planes-1 64x64, planes-2
    64x64 and 128x128, k_gemm_dw_t 64x64 with
    8+ slices, k_gemm_dw_t 128x128            0.059                 critic.4.bias, 512x256x128 tanh R6145 (next: 0.020
                                                                    critic.0.bias, 512x256x128 elu O48 R6145)
Everywhere else a tensor uses 0.3 % to 1 % of its band (relative norm about 1e-6); the largest share of any band is that 0.059, the
mean surrogate uses up to 0.024 of its own.  The element-wise band is used to 0.4 % at worst.

The case [96, 40, 24] keeps the weight planes on every launch: 40 and 24 are multiples of 8, which is all planes_ok asks of a width.
The fp32-operand k_gemm launches are reached by [96, 44, 20] (forward of layer 3 and the head, input gradients of the head and
layer 3), which is in the matrix beside it.
"""
import ctypes

import pytest
import torch

from tests import ppo_update_ref as pur

pytestmark = pytest.mark.gpu

_STORAGE = ("obs", "actions", "values", "advantages", "returns", "log_prob", "mu")


def _read_trace(lib):
    lib.ppok_debug_gemm_trace.argtypes = [ctypes.POINTER(ctypes.c_int), ctypes.c_int]
    lib.ppok_debug_gemm_trace.restype = ctypes.c_int
    buf = (ctypes.c_int * (4 * 64))()
    n = lib.ppok_debug_gemm_trace(buf, 64)
    assert 0 <= n <= 64
    return [tuple(buf[4 * k:4 * k + 4]) for k in range(n)]


class _Learner:
    """A HipPPO with the case's parameters and storage written verbatim (as tests/test_hip_ppo_loss.py does), after begin_update."""

    def __init__(self, c, deterministic=False):
        from legged_gym_dev_amd.rl.ppo import HipPPO
        self.c, self.case, self.alg = c, pur.build_for(c), pur.alg_for(c)
        case = self.case
        self.hip = hip = HipPPO(c["R"] * c["nmb"], c["O"], c["OC"], c["A"], pur.policy_for(c), self.alg, 1, device="cuda:0", seed=3)
        try:
            assert hip.privileged == (c["OC"] is not None)
            assert set(hip.param_views) == set(case["params"])
            for k, v in case["params"].items():
                hip.param_views[k].copy_(v)
            hip.params_changed()
            for k in _STORAGE + (("critic_obs",) if hip.privileged else ()):
                hip.t[k].copy_(case[k].reshape(hip.t[k].shape))
            hip.t["sigma"].copy_(case["sigma"])
            if deterministic:
                hip.set_deterministic(True)
            hip._call("begin_update")
        except Exception:
            hip.close()
            raise

    def backward(self, mb=0, overlap=None):
        """One lg_ppo_minibatch_backward -> gradients by name, KL mean, the launch trace of the pass, the storage rows it took."""
        hip, R = self.hip, self.c["R"]
        if overlap is not None:
            hip.lib.lg_ppo_debug_set_overlap(hip.ctx, overlap)
        _read_trace(hip.lib)                            # clears whatever earlier launches left
        hip._call("minibatch_backward", 0, mb)
        torch.cuda.synchronize()
        trace = _read_trace(hip.lib)
        rows = hip.t["perm"][mb * R:(mb + 1) * R].long().cpu()
        got = {"grads": {k: v.detach().cpu().clone() for k, v in hip.grad_views.items()}, "kl": float(hip.t["grads"][hip.num_params]) / R,
               "kl_sum_bits": hip.t["grads"][hip.num_params:hip.num_params + 1].cpu().clone()}
        return got, trace, rows

    def step(self, got, n_updates=1.0):
        """lg_ppo_minibatch_step; adds the loss means of the update so far to `got`."""
        hip = self.hip
        hip._call("minibatch_step")
        torch.cuda.synchronize()
        st = hip.stats()
        assert st["n_updates"] == n_updates
        got["value_loss"] = st["value_loss_sum"] / st["n_updates"]
        got["surrogate_loss"] = st["surrogate_loss_sum"] / st["n_updates"]

    def close(self):
        self.hip.close()


def _check_trace(c, trace):
    want = pur.parse_trace(pur.TRACES[pur.case_id(c)])
    assert trace == want, ("the case names the wrong path for this shape: it names  " + pur.format_trace(want) + "  and the library launched  " +
                           pur.format_trace(trace) + "  (nz " + str(sorted({t[1] for t in trace})) + ")")


def _check_bands(c, case, got, ref, tag=""):
    assert list(got["grads"]) == list(ref["grads"])
    for k, g in got["grads"].items():
        assert bool(torch.isfinite(g).all()), k
    errs = pur.band_errors(got, ref, case)
    print("ppo_update_errors", pur.case_id(c) + tag, {k: "%.3g/%.3g" % v for k, v in errs.items()})
    over = {k: v for k, v in errs.items() if not v[0] <= v[1]}
    assert not over, over


@pytest.mark.parametrize("c", pur.CASES, ids=pur.case_id)
def test_update_gradients_per_tensor_kl_statistics_and_launches_match_float64(c):
    R, nmb, mb = c["R"], c["nmb"], c["mb"]
    L = _Learner(c)
    try:
        case, hip = L.case, L.hip
        params = None
        if nmb > 1:                                     # backward(0), step: the step gathers minibatch 1 into the other buffer set
            assert (nmb, mb) == (2, 1)
            first, _, _ = L.backward(0)
            L.step(first)
            params = {k: v.detach().cpu().clone() for k, v in hip.param_views.items()}
            moved = max(float((params[k].double() - case["params"][k].double()).abs().max()) for k in params)
            assert 0 < moved <= 1.1e-6, moved           # Adam at a learning rate of 1e-6: the rows keep their regimes (ppo_update_ref.alg_for)
            cur = hip.debug_mb_sets()[0]["obs"].data_ptr()
        got, trace, rows = L.backward(mb)
        if nmb > 1:
            assert hip.debug_mb_sets()[0]["obs"].data_ptr() != cur, "minibatch 1 was not taken from the set gathered ahead"
            ref = pur.reference(case, L.alg, rows, params=params)
        else:
            assert sorted(rows.tolist()) == list(range(R))
            ref = pur.reference_cached(pur.case_id(c))
        _check_trace(c, trace)
        L.step(got, n_updates=float(mb + 1))
        if nmb > 1:                                     # the statistics are sums over both steps
            for k in ("value_loss", "surrogate_loss"):
                got[k] = got[k] * 2 - first[k]
        _check_bands(c, case, got, ref)
    finally:
        L.close()


@pytest.mark.parametrize("cid", pur.DETERMINISTIC)
def test_deterministic_mode_is_bit_equal_with_and_without_the_side_stream(cid):
    """set_deterministic(True): the gradients and the KL sum with the weight gradients on the main stream (overlap 0), on the side
    stream (1) and on the side stream again are bit-equal -- an operand read before the other stream wrote it shows up here without
    depending on luck -- and a pass of a fresh update, stepped, sits in the bands of the test above."""
    c = pur.BY_ID[cid]
    L = _Learner(c, deterministic=True)
    try:
        runs = []
        for overlap in (0, 1, 1):
            got, trace, rows = L.backward(0, overlap=overlap)
            _check_trace(c, trace)
            runs.append(got)
        for k, other in enumerate(runs[1:]):
            for name, g in runs[0]["grads"].items():
                assert torch.equal(g, other["grads"][name]), (name, "overlap 0 against overlap 1" if k == 0 else "overlap 0 against overlap 1 repeated")
            assert torch.equal(runs[0]["kl_sum_bits"], other["kl_sum_bits"])
        L.hip._call("begin_update")                     # a fresh update: the loss sums start at zero again
        got, trace, rows = L.backward(0)
        assert sorted(rows.tolist()) == list(range(c["R"]))
        _check_trace(c, trace)
        L.step(got)
        _check_bands(c, L.case, got, pur.reference_cached(cid), tag="-deterministic")
    finally:
        L.close()
