"""The rollout's policy step (HipPPO.act) against float64: every case of tests/ppo_act_ref.py on the one-launch forward (k_mlp_fwd) and on
the per-layer GEMMs + k_act_sample it falls back to (lg_ppo_debug_set_fused_act), through the same assertions.  Reference, dispatch
arithmetic, input families and bounds: tests/ppo_act_ref.py; what those bounds rest on: tests/test_ppo_act_host.py.

Per case one learner with two rollout steps; parameters written through param_views.  With injected noise the means, values, actions
and log-probs of both act() calls and the stored transition are compared element by element (integer families: means and values EQUAL
the float64 reference); storage rows of the step after the one being written hold a sentinel that must survive (a row past N would land
there).  Without injection the draws are compared with the numpy Philox + float64 Box-Muller per env, action and call.

Measured on the MI355X (rand family; E = max |. - ref| / S over both heads and both calls; the one-launch forward and the per-layer GEMMs
gave the SAME figures in every case -- both walk k in steps of 16 through one accumulator per output, so means and values are equal bit
for bit):
    case (actor | critic widths / observation widths)      activation   E_k / E_y
    288-160-96 / 3, 65                                     elu          0.94
    288-160-96 / 48, 169                                   relu         1.12
    256-384-64 | 160-416-32 / 16, 235                      relu         1.55
    160-416-32 | 256-384-64 / 235, 16                      elu          0.84
    32-160-32 | 192-32-32 / 48                             elu          0.84
    416-32-32 | 512-32-32 / 3, 512                         relu         1.15
    512-32-32 | 416-32-32 / 500, 3                         elu          1.00
    512-256-128 / 48, 235, 169, 65                         elu          0.89, 0.90, 1.19, 1.02
    160-96-32 / 48                                         selu 0.78, relu 0.95, lrelu 1.15, tanh 1.78, sigmoid 0.60, crelu 0.97
    96-40-24 / 169 and 64-32 / 520 (per-layer only)        elu, relu    0.78, 0.85
Asserted: E_k <= 4 E_y + 2^-24 (ppo_act_ref.PRECISION_M: twice 1.55 for the activations exact in fp32, twice 1.78 for those on __expf,
each rounded up to one digit).  The structural bound is used to 0.01 % at worst: its (6 K + 8) roundings per output and the
__expf allowance of gemm_ref are far from what a k-sequential fp32 accumulator loses.
Sampling: device normals against the float64 Box-Muller, in units of the numpy-float32 formula's own worst error: 1.16 at worst (asserted
3 = twice that, rounded up); the log-prob bound with LOGF_MARGIN = 1 is used to 0.51 at worst.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import ppo_act_ref as ar

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = ar.U
SENTINEL = -12345.0
ALG = dict(value_loss_coef=1.0, use_clipped_value_loss=True, clip_param=0.2, entropy_coef=0.01, num_learning_epochs=1, num_mini_batches=1,
           learning_rate=1e-3, schedule="adaptive", gamma=0.99, lam=0.95, desired_kl=0.01, max_grad_norm=1.0)
STORED = ("obs", "critic_obs", "actions", "mu", "values", "log_prob")


def _learner(c, T=2, seed=3, **kw):
    from legged_gym_dev_amd.rl.ppo import HipPPO
    return HipPPO(c["N"], c["O"], c["OC"], c["A"], ar.policy_cfg(c), ALG, T, device=DEV, seed=seed, **kw)


def _write(hip, params):
    for k, v in params.items():
        hip.param_views[k].copy_(v.to(DEV))
    hip.params_changed()


def _set_path(hip, c, fused):
    hip.lib.lg_ppo_debug_set_fused_act(hip.ctx, fused)
    assert hip.lib.lg_ppo_debug_get_fused_act(hip.ctx) == (1 if fused and c["fused"] else 0), "the case names the wrong path for this shape"
    return "one-launch" if fused and c["fused"] else "per-layer"


def _act(hip, c, call):
    obs = call["obs"].to(DEV)
    if c["OC"]:
        hip.act(obs, call["cobs"].to(DEV))
    else:
        hip.act(obs)
    torch.cuda.synchronize()
    return {k: hip.t["act_" + k].cpu().double() for k in ("mu", "values", "actions", "log_prob")}


def _idle_step(hip, N):
    hip.process_env_step(torch.zeros(N, device=DEV), torch.zeros(N, dtype=torch.uint8, device=DEV), {})


def _reference(c, inp, call):
    """Float64 means / values of one call with their structural bounds, S of both heads and the yardstick's E_y."""
    cobs = call["cobs"] if c["OC"] else call["obs"]
    r = {}
    e_y = 0.0
    for net, x in (("actor", call["obs"]), ("critic", cobs)):
        out, S, trace = ar.forward64(c, inp["params"], x, net)
        r[net] = dict(out=out, S=S, bound=ar.structural_bound(trace))
        Y = ar.yardstick(c, inp["params"], x, net).double()
        e_y = max(e_y, float(((Y - out).abs() / S).max()))
    r["e_y"] = e_y
    return r


def _check_heads(c, fam, ref, got, tag):
    """Means and values against the float64 reference: equality for the integer families, both bounds for rand."""
    e_k = 0.0
    for net, key in (("actor", "mu"), ("critic", "values")):
        want, g = ref[net]["out"], got[key].reshape(ref[net]["out"].shape)
        assert bool(torch.isfinite(g).all()), f"{tag} {key}: non-finite"
        diff = (g - want).abs()
        if fam != "rand":
            bad = int((diff != 0).sum())
            assert bad == 0, f"{tag} {key}: {bad} of {diff.numel()} elements differ from the exact result, max |diff| {float(diff.max())}"
            continue
        worst = float((diff / ref[net]["bound"]).max())
        print(f"STRUCT {tag} {key} worst diff/bound {worst:.4f}")
        assert worst <= 1.0, f"{tag} {key}: structural bound exceeded {worst:.3f}x"
        e_k = max(e_k, float((diff / ref[net]["S"]).max()))
    if fam == "rand":
        ratio = e_k / ref["e_y"]
        M = ar.PRECISION_M[ar.on_expf(c)]
        print(f"RATIO {tag} E_k {e_k:.3e} E_y {ref['e_y']:.3e} ratio {ratio:.3f}")
        assert e_k <= M * ref["e_y"] + U, (tag, e_k, ref["e_y"], ratio)


def _check_sampling(c, fam, ref, got, z, std, tag):
    """Actions from the kernel's own mean and from the reference mean; log-prob from the noise alone (it does not depend on the mean)."""
    mu_k, act_k = got["mu"], got["actions"]
    own = mu_k + std * z
    lim = U * ((std * z).abs() + act_k.abs())
    assert bool(((act_k - own).abs() <= lim).all()), f"{tag}: actions are not mu + std z of the kernel's own mu ({float(((act_k - own).abs() / lim.clamp_min(1e-300)).max()):.2f}x)"
    mu_err = ref["actor"]["bound"] if fam == "rand" else torch.zeros_like(mu_k)
    assert bool(((act_k - (ref["actor"]["out"] + std * z)).abs() <= ar.action_bound(mu_err, act_k, z, std)).all()), f"{tag}: actions off the reference"
    lp64 = ar.log_prob64(z, std)
    bound = ar.lp_bound(mu_k, act_k, z, std)
    used = float(((got["log_prob"] - lp64).abs() / bound).max())
    print(f"LOGPROB {tag} worst diff/bound {used:.4f}")
    assert used <= 1.0, f"{tag}: log-prob off by {used:.3f}x its bound"


@pytest.mark.parametrize("run", ar.runs(), ids=ar.run_id)
def test_act_matches_float64_on_both_paths(run):
    c, fam = run
    N, A = c["N"], c["A"]
    inp = ar.build_inputs(c, fam)
    std = inp["std"].double()
    refs = [_reference(c, inp, call) for call in inp["calls"]]
    hip = _learner(c)
    try:
        _write(hip, inp["params"])
        hip.inject_noise(1)
        for fused in (1, 0):
            path = _set_path(hip, c, fused)
            for k in STORED + ("sigma",):
                hip.t[k].fill_(SENTINEL)
            shots = []
            for t, call in enumerate(inp["calls"]):
                tag = f"{ar.run_id(run)} {path} call {t}"
                hip.t["noise"].copy_(call["noise"].to(DEV))
                got = _act(hip, c, call)
                _check_heads(c, fam, refs[t], got, tag)
                _check_sampling(c, fam, refs[t], got, call["noise"].double(), std, tag)
                if t == 0:                         # nothing past row N of step 0: step 1's rows still hold the sentinel
                    for k in STORED:
                        assert bool((hip.t[k][1] == SENTINEL).all()), f"{tag}: {k} written past row {N}"
                shots.append(got)
                _idle_step(hip, N)
            torch.cuda.synchronize()
            for t, call in enumerate(inp["calls"]):
                assert torch.equal(hip.t["obs"][t].cpu(), call["obs"])
                assert torch.equal(hip.t["critic_obs"][t].cpu(), call["cobs"] if c["OC"] else call["obs"])
                for k in ("actions", "mu", "values", "log_prob"):
                    assert torch.equal(hip.t[k][t].cpu().double(), shots[t][k]), f"{path}: stored {k} of step {t} differs from what act returned"
            assert torch.equal(hip.t["sigma"].cpu(), inp["std"]), f"{path}: sigma is not std for all {A} actions (N = {N})"
            hip._call("end_update")
    finally:
        hip.close()


PHILOX = [("160-96-32/o48/relu", 1, 0), ("512-256-128/o48", 1, 0), ("256-384-64|160-416-32/o16-oc235", 1, 0),
          ("288-160-96/o48-oc169", 1, 0), ("160-416-32|256-384-64/o235-oc16", 1, 0), ("160-96-32/o48/tanh", 2, 1)]


@pytest.mark.parametrize("label,world,rank", PHILOX, ids=[f"{p[0]}/rank{p[2]}of{p[1]}" for p in PHILOX])
def test_philox_draws_match_the_numpy_reference(label, world, rank):
    """Not injected: with the actor's head zeroed and std a distinct power of two per action, actions = std z exactly, so
    (actions - mu) / std IS the device's normal.  Compared with the float64 Box-Muller of the numpy Philox per env, action and call, at
    act_count 0 and above 2^32 (the counter word takes the low 32 bits), on both act paths.  A learner of rank 1 in a world of 2 draws the
    stream of its own seed; the learner's env_offset is 0 in every rank (the library never sets another), so that is what the rank-1 case
    pins.  Bound: NORMAL_MARGIN times the worst error of the same formula in numpy float32."""
    c = next(x for x in ar.CASES if x["label"] == label)
    N, A, seed = c["N"], c["A"], 7
    inp = ar.build_inputs(c, c["families"][-1])
    hip = _learner(c, seed=seed, world_size=world, rank=rank)
    try:
        nl = len(c["actor"])
        inp["params"][f"actor.{2 * nl}.weight"].zero_()
        inp["params"][f"actor.{2 * nl}.bias"].zero_()
        std = torch.exp2(torch.arange(A).float() - 6)
        inp["params"]["std"] = std
        _write(hip, inp["params"])
        seed64 = ar.learner_seed(seed, rank)
        for fused in (1, 0):
            path = _set_path(hip, c, fused)
            for count in (0, (1 << 32) + 11):
                hip.lib.lg_ppo_debug_set_act_count(hip.ctx, ctypes.c_longlong(count))
                for t, call in enumerate(inp["calls"]):
                    got = _act(hip, c, call)
                    assert not bool(got["mu"].any())
                    zk = (got["actions"] - got["mu"]) / std.double()
                    u1, u2 = ar.uniforms(seed64, N, A, count + t)
                    z64 = torch.from_numpy(ar.box_muller64(u1, u2))
                    e_y = float(np.abs(ar.box_muller32(u1, u2).astype(np.float64) - z64.numpy()).max())
                    e_k = float((zk - z64).abs().max())
                    print(f"NORMAL {label} {path} count {count + t} E_k {e_k:.3e} E_y {e_y:.3e} ratio {e_k / e_y:.3f}")
                    assert e_k <= ar.NORMAL_MARGIN * e_y, f"{path} count {count + t}: draws differ from the Philox reference by {e_k:.3e} (yardstick {e_y:.3e})"
                    lp_used = float(((got["log_prob"] - ar.log_prob64(zk, std.double())).abs() / ar.lp_bound(got["mu"], got["actions"], zk, std.double())).max())
                    assert lp_used <= 1.0, f"{path}: log-prob of the drawn actions off by {lp_used:.3f}x its bound"
                    _idle_step(hip, N)
                hip._call("end_update")
    finally:
        hip.close()


@pytest.mark.parametrize("label", ["160-96-32/o48/tanh", "256-384-64|160-416-32/o16-oc235"])
def test_parameter_write_between_two_acts_reaches_the_second_act(label):
    """load_state_dict of a second parameter set between the two act() calls of one rollout, on nets that are not ELU: the second act
    equals the float64 reference on the NEW set, on both paths."""
    c = next(x for x in ar.CASES if x["label"] == label)
    first, second = ar.build_inputs(c, "rand"), ar.build_inputs(c, "rand", tag="second")
    hip = _learner(c)
    try:
        hip.inject_noise(1)
        for fused in (1, 0):
            path = _set_path(hip, c, fused)
            _write(hip, first["params"])
            for t, inp in enumerate((first, second)):
                if t:
                    hip.load_state_dict({k: v.to(DEV) for k, v in inp["params"].items()})
                call = first["calls"][t]
                hip.t["noise"].copy_(call["noise"].to(DEV))
                got = _act(hip, c, call)
                ref = _reference(c, inp, call)
                tag = f"{label} {path} after set {t}"
                _check_heads(c, "rand", ref, got, tag)
                _check_sampling(c, "rand", ref, got, call["noise"].double(), inp["std"].double(), tag)
                _idle_step(hip, c["N"])
            old = _reference(c, first, first["calls"][1])
            assert float((old["actor"]["out"] - ref["actor"]["out"]).abs().max()) > 1e-3      # the two sets differ where it is looked at
            hip._call("end_update")
    finally:
        hip.close()
