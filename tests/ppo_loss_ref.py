"""Test-only case builder and float64 reference for the PPO minibatch loss of the HIP learner (csrc/ppo_loss.h, as the four kernels of
legged_gym_dev_amd/csrc/ppo_kernels.hip run it: k_loss, k_head_fused<32|64>, k_head_net<128, 12|16> + k_head_finish).  Plain torch, no
GPU needed: tests/test_ppo_loss_host.py checks the inputs built here on the CPU, tests/test_hip_ppo_loss.py runs them through the
library.

A case is a set of fp32 tensors.  They are written verbatim into the learner's storage and upcast to float64 for the reference,
so both sides see bit-identical inputs.  Every row is steered to a target (ratio, advantage, v_new - v_old, v_new - return) from a
fixed table, so that it sits well inside one branch of the clipped surrogate and one branch of the clipped value loss: a row that
takes another branch in fp32 than in float64 would differ by order one, not by rounding.
"""
import functools
import itertools

import torch

from oracle import ppo_torch

CLIP = 0.2
RATIOS = (0.5, 0.7, 0.9, 1.0, 1.1, 1.3, 1.6)
ADVS = (-1.5, -0.4, 0.4, 1.5)
DVS = (-0.5, -0.3, -0.1, 0.0, 0.1, 0.3, 0.5)           # v_new - v_old
ERRS = (-1.0, -0.25, 0.25, 1.0)                        # v_new - return
TABLE = tuple(itertools.product(RATIOS, ADVS, DVS, ERRS))

FLOWS, CLIPPED = 0, 1                                  # surrogate regimes
TIE, UNCLIPPED_WINS, CLIPPED_WINS = 0, 1, 2            # value regimes
SURROGATE_NAMES = ("flows", "clipped")
VALUE_NAMES = ("tie", "unclipped_wins", "clipped_wins")

# what the update is run with (the driver of tests/test_hip_ppo_loss.py); value_loss_coef is not 1, so a dropped coefficient shows
ALG = dict(value_loss_coef=0.5, use_clipped_value_loss=True, clip_param=CLIP, entropy_coef=0.01, num_learning_epochs=1,
           num_mini_batches=1, learning_rate=1e-3, schedule="adaptive", gamma=0.99, lam=0.95, desired_kl=0.01, max_grad_norm=1.0)


def regime_of(r, adv, d, e, clip=CLIP):
    """(surrogate, value) regime of a target tuple, from the tuple alone."""
    sur = CLIPPED if (adv > 0 and r > 1 + clip) or (adv < 0 and r < 1 - clip) else FLOWS
    if abs(d) <= clip:
        val = TIE
    else:
        vc_err = e - d + (clip if d > 0 else -clip)     # v_clipped - return
        val = UNCLIPPED_WINS if e * e > vc_err * vc_err else CLIPPED_WINS
    return sur, val


SINGLE_REGIME_TABLE = tuple(t for t in TABLE if regime_of(*t) == (CLIPPED, CLIPPED_WINS) and abs(t[2]) > CLIP)


def _model(case, dtype):
    m = case["meta"]
    ac = ppo_torch.ActorCritic(m["O"], m.get("OC", m["O"]), m["A"], m["hidden"], m["critic_hidden"], m["activation"], 1.0)
    ac.load_state_dict(case["params"])
    return ac.to(dtype)


def _build(O, A, hidden, activation, R, seed, critic_hidden, table, OC=None):
    """OC (tests/ppo_update_ref.py): a privileged critic with OC != O inputs and observations of its own, drawn from a generator of
    their own, so that every draw of a case without them is what it was."""
    hidden = list(hidden)
    critic_hidden = list(critic_hidden) if critic_hidden is not None else hidden
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        ac = ppo_torch.ActorCritic(O, O if OC is None else OC, A, hidden, critic_hidden, activation, 1.0)
    with torch.no_grad():
        std = (ac.std.double() * (0.6 + 0.8 * torch.rand(A, generator=g, dtype=f64))).float()
        ac.std.copy_(std)
    params = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    case = {"params": params, "meta": dict(O=O, A=A, hidden=hidden, critic_hidden=critic_hidden, activation=activation, R=R)}
    if OC is not None:
        case["meta"]["OC"] = OC
    ac64 = _model(case, f64)
    std64 = std.double()
    obs = torch.randn(R, O, generator=g, dtype=f64).float()
    cobs = obs if OC is None else torch.randn(R, OC, generator=torch.Generator().manual_seed(seed + 1000003), dtype=f64).float()
    with torch.no_grad():
        mu_new = ac64.actor(obs.double())
        v_new = ac64.critic(cobs.double()).squeeze(-1)
    sigma = (std64 * (0.8 + 0.45 * torch.rand(A, generator=g, dtype=f64))).float()
    mu = (mu_new + 0.3 * torch.randn(R, A, generator=g, dtype=f64)).float()
    actions = (mu_new + std64 * torch.randn(R, A, generator=g, dtype=f64)).float()
    lp_new = torch.distributions.Normal(mu_new, std64.expand_as(mu_new)).log_prob(actions.double()).sum(-1)
    tab = torch.tensor(table, dtype=f64)
    order = torch.randperm(len(table), generator=g)
    targets = tab[order[torch.arange(R) % len(table)]]
    r, adv, d, e = targets.unbind(-1)
    labels = torch.tensor([regime_of(*t) for t in targets.tolist()], dtype=torch.int64).reshape(R, 2)
    case.update(obs=obs, actions=actions, mu=mu, sigma=sigma, log_prob=(lp_new - torch.log(r)).float(), values=(v_new - d).float(),
                returns=(v_new - e).float(), advantages=adv.float(), targets=targets, surrogate_regime=labels[:, 0],
                value_regime=labels[:, 1])
    if OC is not None:
        case["critic_obs"] = cobs
    return case


@functools.lru_cache(maxsize=None)
def _build_cached(O, A, hidden, activation, R, seed, critic_hidden, single):
    return _build(O, A, hidden, activation, R, seed, critic_hidden, SINGLE_REGIME_TABLE if single else TABLE)


def build_case(O, A, hidden, activation, R, seed, critic_hidden=None):
    """Parameters (an ActorCritic initialisation, std scaled per action by U(0.6, 1.4)) and R rows of rollout storage: obs ~ N(0, 1),
    old sigma = std U(0.8, 1.25), old mu = mu_new + 0.3 N(0, 1), actions = mu_new + std N(0, 1), and per row a target
    (r, adv, d, e) from a seeded permutation of TABLE (repeated as needed): lp_old = lp_new - ln r, v_old = v_new - d,
    return = v_new - e, advantage = adv.  Everything is computed in float64 and stored as fp32.  Cached: callers must not write
    into the tensors."""
    return _build_cached(O, A, tuple(hidden), activation, R, seed, None if critic_hidden is None else tuple(critic_hidden), False)


def single_regime_case(O, A, hidden, activation, R, seed, critic_hidden=None):
    """The same with every row's target drawn from SINGLE_REGIME_TABLE only: surrogate clipped, and a value loss whose clipped
    branch is outside the clip range and the larger.  Neither loss then has a gradient: what is left is the entropy bonus."""
    return _build_cached(O, A, tuple(hidden), activation, R, seed, None if critic_hidden is None else tuple(critic_hidden), True)


def batch_of(case, rows=None, dtype=torch.float64):
    """The argument tuple of oracle.ppo_torch.PPO.minibatch_loss for the given rows (all of them by default)."""
    idx = slice(None) if rows is None else rows
    pick = lambda k: case[k][idx].to(dtype)
    obs = pick("obs")
    return (obs, pick("critic_obs") if "critic_obs" in case else obs, pick("actions"), pick("values").unsqueeze(-1), pick("advantages").unsqueeze(-1), pick("returns").unsqueeze(-1),
            pick("log_prob").unsqueeze(-1), pick("mu"), case["sigma"].to(dtype).expand(obs.shape[0], -1))


def reference(case, alg, rows=None, dtype=torch.float64):
    """Parameter gradients (by name, ActorCritic.parameters() order), mean KL, mean value loss and mean surrogate of one minibatch
    through oracle.ppo_torch.PPO.minibatch_loss on a model of `dtype` (float64: the reference; float32: the restatement whose own
    error the host test measures)."""
    ac = _model(case, dtype)
    algo = ppo_torch.PPO(ac, clip_param=alg["clip_param"], value_loss_coef=alg["value_loss_coef"], entropy_coef=alg["entropy_coef"],
                         use_clipped_value_loss=alg["use_clipped_value_loss"])
    with torch.random.fork_rng():                       # minibatch_loss samples actions it does not use
        loss, kl, vl, sl = algo.minibatch_loss(*batch_of(case, rows, dtype))
    loss.backward()
    return {"grads": {k: p.grad.detach().double() for k, p in ac.named_parameters()}, "kl": float(kl), "value_loss": float(vl.detach()),
            "surrogate_loss": float(sl.detach())}


def row_quantities(case, clip=CLIP):
    """What the branches of the loss look at, per row in float64: ratio, v_new - v_old, the two value losses, the advantage."""
    ac = _model(case, torch.float64)
    obs, cobs, actions, v_old, adv, ret, lp_old, _, _ = batch_of(case)
    with torch.no_grad():
        mu = ac.actor(obs)
        v = ac.critic(cobs)
        lp = torch.distributions.Normal(mu, ac.std.expand_as(mu)).log_prob(actions).sum(-1)
    d = (v - v_old).squeeze(-1)
    vc = v_old + (v - v_old).clamp(-clip, clip)
    return {"ratio": torch.exp(lp - lp_old.squeeze(-1)), "d": d, "l1": (v - ret).pow(2).squeeze(-1), "l2": (vc - ret).pow(2).squeeze(-1),
            "adv": adv.squeeze(-1)}


def blocks(case):
    """The parameter blocks that get a relative-norm bound of their own: std and, per network, head weight, head bias,
    last-hidden bias and first-layer weight -- a head-only error is not diluted by the first layer's block."""
    m = case["meta"]
    names = ["std"]
    for net, hid in (("actor", m["hidden"]), ("critic", m["critic_hidden"])):
        L = len(hid)
        for n in (f"{net}.{2 * L}.weight", f"{net}.{2 * L}.bias", f"{net}.{2 * (L - 1)}.bias", f"{net}.0.weight"):
            if n not in names:
                names.append(n)
    return names


def _rel(got, ref):
    n = float(ref.norm())
    e = float((got - ref).norm())
    if n == 0.0:                                        # a block whose reference gradient is exactly zero must come out exactly zero
        return 0.0 if e == 0.0 else float("inf")
    return e / n


def band_errors(got, ref, case):
    """Every band of the comparison as name -> (error, bound); `got` / `ref` as reference() returns them.  Gradients: the
    project's bands from tests/test_hip_ppo.py -- element-wise rtol 2e-3 + atol 2e-4 max|ref| (reported as the worst fraction of
    that band used, bound 1), relative norm of the whole vector 2e-4 (3e-4 for an activation other than elu), and the same
    relative-norm bound on each of blocks().  KL: rtol 1e-3, atol 1e-6.  Mean value loss and mean surrogate: rtol 1e-4, atol 1e-6."""
    names = list(ref["grads"])
    g = torch.cat([got["grads"][k].double().reshape(-1) for k in names])
    r = torch.cat([ref["grads"][k].reshape(-1) for k in names])
    nb = 2e-4 if case["meta"]["activation"] == "elu" else 3e-4
    diff, band = (g - r).abs(), 2e-3 * r.abs() + 2e-4 * float(r.abs().max())
    used = torch.where(diff == 0, torch.zeros_like(diff), diff / band)
    out = {"grad.elementwise": (float(used.max()), 1.0), "grad.norm": (_rel(g, r), nb)}
    for k in blocks(case):
        out["grad.norm." + k] = (_rel(got["grads"][k].double(), ref["grads"][k]), nb)
    out["kl"] = (abs(got["kl"] - ref["kl"]), 1e-3 * abs(ref["kl"]) + 1e-6)
    for k in ("value_loss", "surrogate_loss"):
        out[k] = (abs(got[k] - ref[k]), 1e-4 * abs(ref[k]) + 1e-6)
    return out


# ---- the case matrix: (path label, hidden, critic hidden or None, activation, O, A, R, num_mini_batches, minibatch checked,
# use_clipped_value_loss).  R = rows per minibatch.  The label is the kernel lg_ppo_minibatch_backward dispatches to:
#   generic    k_loss after the head GEMMs: activation not elu, or actor / critic last widths differ or are not 32 / 64 / 128
#   fused32/64 k_head_fused<32|64>: elu, both last widths 32 | 64 -- with ONE hidden layer too: the `nl >= 2` of the dispatch counts
#              the head layer, so it always holds (arithmetic mutants of k_head_fused fail the [64] case, mutants of k_loss do not)
#   net128_12  k_head_net<128, 12> + k_head_finish<128>: both last widths 128, num_actions <= 12
#   net128_16  k_head_net<128, 16> + k_head_finish<128>: both last widths 128, num_actions 13..16
PATHS = {"fused32": ([64, 32], None, "elu"), "fused64": ([64, 64], None, "elu"), "net128_12": ([32, 128], None, "elu"),
         "net128_16": ([32, 128], None, "elu"), "generic": ([96, 40], None, "elu")}
LABELS = tuple(PATHS)


def _cases():
    out = []

    def add(label, A, R, hidden=None, critic=None, activation=None, O=8, nmb=1, mb=0, clipped=True):
        h, c, act = PATHS[label]
        out.append((label, hidden or h, critic or c, activation or act, O, A, R, nmb, mb, clipped))
    for R in (1, 63, 64, 65, 193, 12353):               # 12 353 = 192 * 64 + 65: a second trip of the tile loop, then a one-row tile
        add("fused32", 12, R)
    for A in (1, 3, 5, 13, 16):
        add("fused32", A, 193)
    for R in (65, 193, 12353):
        add("fused64", 12, R)
    for A in (3, 16):
        add("fused64", A, 193)
    for R in (1, 65, 193, 24641):                       # 24 641 = 384 * 64 + 65
        add("net128_12", 12, R)
    for A in (1, 3, 11):
        add("net128_12", A, 193)
    for A in (13, 16):
        for R in (65, 193):
            add("net128_16", A, R)
    add("net128_16", 16, 24641)
    for A in (12, 13):
        for R in (1, 255, 256, 300):
            add("generic", A, R)
    add("generic", 12, 300, hidden=[64, 64], activation="tanh")           # a fused width, but not elu
    add("generic", 12, 300, hidden=[64, 64], critic=[64, 32])             # last widths differ
    add("fused64", 5, 300, hidden=[64])                                   # one hidden layer: still the fused head (see above)
    for label in LABELS:
        add(label, 16 if label == "net128_16" else 12, 300, clipped=False)
    for label in ("fused32", "net128_12"):
        add(label, 12, 193, O=65, nmb=2, mb=1)                            # a padded first layer; the second minibatch
    return out


CASES = _cases()


def case_id(c):
    label, hidden, critic, act, O, A, R, nmb, mb, clipped = c
    s = f"{label}-{'x'.join(map(str, hidden))}"
    if critic:
        s += "-c" + "x".join(map(str, critic))
    s += f"-{act}-O{O}-A{A}-R{R}"
    if nmb > 1:
        s += f"-mb{mb}of{nmb}"
    return s if clipped else s + "-unclipped"


# Two of the compared numbers are sums that cancel: the mean surrogate (advantages of both signs) and the critic head's bias
# gradient (a single number: the mean of d loss / d value over rows whose v_new - return has both signs).  Where a sample's sum
# falls near zero the band around it shrinks to fp32 rounding of the terms, for any implementation.  The seed is one for which no
# case of the matrix does: tests/test_ppo_loss_host.py asserts it (the fp32 restatement stays below 5 % of every band).
SEED = 15


def build_for(c, seed=SEED):
    """The case of one CASES entry: R * num_mini_batches rows of storage."""
    label, hidden, critic, act, O, A, R, nmb, mb, clipped = c
    return build_case(O, A, hidden, act, R * nmb, seed, critic)


def alg_for(c):
    return dict(ALG, num_mini_batches=c[7], use_clipped_value_loss=c[9])
