"""Test-only case builder and float64 references for the recurrent (LSTM) minibatch of the HIP learner: k_lstm_fwd, k_lstm_bwd,
k_lstm_bias_grad (legged_gym_dev_amd/csrc/ppo_rnn.hip) and rnn_forward_seq / rnn_backward_seq / rnn_live_step
(csrc/ppo_sched.hip).  Plain torch, no GPU needed: tests/test_recurrent_loss_host.py checks what is built here on the CPU,
tests/test_hip_recurrent.py runs it through the library.  The pattern (and the TABLE / regime_of steering) is that of
tests/ppo_loss_ref.py.

A case is a set of fp32 tensors.  They are written verbatim into the learner and upcast to float64 for the reference, so both
sides see bit-identical inputs.  The saved states are drawn at every (t, env), unrelated to the recurrence: a step that must carry
sees a saved state it must ignore, a step that must reload sees a nonzero one -- a forward that reloads where it should carry (or
the reverse) is then wrong by order one, not only in where the gradient is cut.

Three float64 computations of the same minibatch, none sharing code with another beyond torch itself:
  reference()       recurrent_ref.recurrent_minibatch + minibatch_loss: nn.LSTM over the literal split / pad / unpad generator
  reference_loop()  a step loop over t on the minibatch's envs that reloads (h, c) at t = 0 and after every done; the cell, the
                    MLPs and the loss spelled out -- the form the GPU schedule runs
  step_reference()  one live step (rollout / compute_returns / act_inference)
"""
import functools
import math

import torch
import torch.nn.functional as F

from tests import ppo_loss_ref as plr
from tests import recurrent_ref as rr

CLIP = plr.CLIP
ALG = dict(plr.ALG)                                    # value_loss_coef 0.5: a dropped coefficient shows
PATTERNS = ("none", "all", "last", "rand", "runs")
STATES = ("saved_h_a", "saved_c_a", "saved_h_c", "saved_c_c")
STORAGE = ("obs", "actions", "values", "advantages", "returns", "log_prob", "mu")

_ACT = {"elu": F.elu, "selu": F.selu, "relu": F.relu, "lrelu": F.leaky_relu, "tanh": torch.tanh, "sigmoid": torch.sigmoid}


# ------------------------------------------------------------------------------------------------ spelled-out forward
def lstm_cell(x, h, c, w_ih, w_hh, b_ih, b_hh):
    """One nn.LSTM step, gate order i, f, g, o."""
    z = x @ w_ih.T + b_ih + h @ w_hh.T + b_hh
    i, f, g, o = z.chunk(4, dim=-1)
    c_new = torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g)
    return torch.sigmoid(o) * torch.tanh(c_new), c_new


def _mem(p, m):
    return tuple(p[f"memory_{m}.rnn.{k}_l0"] for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))


def mlp(p, net, x, activation):
    nl = sum(1 for k in p if k.startswith(net + ".") and k.endswith(".weight"))
    for l in range(nl):
        x = x @ p[f"{net}.{2 * l}.weight"].T + p[f"{net}.{2 * l}.bias"]
        if l < nl - 1:
            x = _ACT[activation](x)
    return x


def _log_prob(actions, mu, std):
    return (-0.5 * ((actions - mu) / std) ** 2 - torch.log(std) - 0.5 * math.log(2.0 * math.pi)).sum(-1)


def _loop_forward(case, p):
    """mu (T, mbs, A) and value (T, mbs) of the case's minibatch: every env's T-step sequence, (h, c) reloaded from the saved state
    at t = 0 and after every done (the saved states are constants: no gradient into them or across a reload)."""
    m = case["meta"]
    sl = slice(m["mb"] * m["mbs"], (m["mb"] + 1) * m["mbs"])
    f64 = torch.float64
    xs = {"a": case["obs"][:, sl].to(f64), "c": case["critic_obs"][:, sl].to(f64)}
    dones = case["dones"][:, sl].bool()
    outs = {}
    for k in ("a", "c"):
        w = _mem(p, k)
        sh, sc = case[f"saved_h_{k}"][:, sl].to(f64), case[f"saved_c_{k}"][:, sl].to(f64)
        h = c = None
        hs = []
        for t in range(m["T"]):
            if t == 0:
                h, c = sh[0], sc[0]
            else:
                reload = dones[t - 1].unsqueeze(-1)
                h, c = torch.where(reload, sh[t], h), torch.where(reload, sc[t], c)
            h, c = lstm_cell(xs[k][t], h, c, *w)
            hs.append(h)
        outs[k] = torch.stack(hs)
    return mlp(p, "actor", outs["a"], m["activation"]), mlp(p, "critic", outs["c"], m["activation"]).squeeze(-1)


# ------------------------------------------------------------------------------------------------ dones patterns
def make_dones(pattern, T, N, g, mb=0, mbs=None):
    """(T, N) uint8.  'rand': Bernoulli 0.3, then env 0 done at every step, env 1 never, env 2 done at t = 0, env 3 at t = T - 1
    (where N allows), and the same four at the start of the checked minibatch where it has four envs.  'runs': every env has one
    run of two or three consecutive dones."""
    d = torch.zeros(T, N, dtype=torch.uint8)
    if pattern == "all":
        d[:] = 1
    elif pattern == "last":
        d[T - 1] = 1
    elif pattern == "rand":
        d = (torch.rand(T, N, generator=g, dtype=torch.float64) < 0.3).to(torch.uint8)
        starts = [0] + ([mb * mbs] if mbs is not None and mbs >= 4 and mb > 0 else [])
        for e0 in starts:
            d[:, e0] = 1
            if e0 + 1 < N:
                d[:, e0 + 1] = 0
            if e0 + 3 < N:
                d[0, e0 + 2] = 1
                d[T - 1, e0 + 3] = 1
    elif pattern == "runs":
        assert T >= 3
        for e in range(N):
            n = 2 + int(torch.randint(0, 2, (1,), generator=g))
            s = int(torch.randint(0, T - n + 1, (1,), generator=g))
            d[s:s + n, e] = 1
    elif pattern != "none":
        raise ValueError(pattern)
    return d


def reload_mask(dones):
    """(T, N) bool: step t starts from its saved state (t = 0, or a done at t - 1)."""
    r = torch.zeros_like(dones, dtype=torch.bool)
    r[0] = True
    r[1:] = dones[:-1].bool()
    return r


def longest_carry_chain(dones):
    """The largest number of consecutive steps of one env that run from one reload (BPTT depth)."""
    r = reload_mask(dones)
    best = 0
    run = torch.zeros(dones.shape[1], dtype=torch.int64)
    for t in range(dones.shape[0]):
        run = torch.where(r[t], torch.ones_like(run), run + 1)
        best = max(best, int(run.max()))
    return best


# ------------------------------------------------------------------------------------------------ cases
def _model(case, dtype):
    m = case["meta"]
    ac = rr.ActorCriticRecurrent(m["O"], m["OC"] or m["O"], m["A"], m["hidden"], m["hidden"], m["activation"], rnn_hidden_size=m["H"])
    ac.load_state_dict(case["params"])
    return ac.to(dtype)


def _build(T, N, nmb, mb, O, OC, A, H, hidden, activation, pattern, seed):
    hidden = list(hidden)
    assert N % nmb == 0 and 0 <= mb < nmb
    mbs = N // nmb
    R = T * mbs
    g = torch.Generator().manual_seed(seed)
    f64 = torch.float64
    with torch.random.fork_rng():
        torch.manual_seed(seed)
        ac = rr.ActorCriticRecurrent(O, OC or O, A, hidden, hidden, activation, rnn_hidden_size=H)
    with torch.no_grad():
        std = (ac.std.double() * (0.6 + 0.8 * torch.rand(A, generator=g, dtype=f64))).float()
        ac.std.copy_(std)
    params = {k: v.detach().clone() for k, v in ac.state_dict().items()}
    case = {"params": params, "meta": dict(T=T, N=N, nmb=nmb, mb=mb, mbs=mbs, R=R, O=O, OC=OC, A=A, H=H, hidden=hidden,
                                           activation=activation, pattern=pattern, seed=seed)}
    case["obs"] = torch.randn(T, N, O, generator=g, dtype=f64).float()
    case["critic_obs"] = torch.randn(T, N, OC, generator=g, dtype=f64).float() if OC else case["obs"]
    case["dones"] = make_dones(pattern, T, N, g, mb, mbs)
    for k in STATES:
        case[k] = (0.5 * torch.randn(T, N, H, generator=g, dtype=f64)).float()
    std64 = std.double()
    with torch.no_grad():
        mu_new, v_new = _loop_forward(case, {k: v.double() for k, v in params.items()})
    # the other envs of the storage: any finite values
    case["actions"] = torch.randn(T, N, A, generator=g, dtype=f64).float()
    case["mu"] = torch.randn(T, N, A, generator=g, dtype=f64).float()
    for k in ("values", "returns", "advantages"):
        case[k] = torch.randn(T, N, generator=g, dtype=f64).float()
    case["log_prob"] = (-A + torch.randn(T, N, generator=g, dtype=f64)).float()
    # the minibatch's rows, steered as ppo_loss_ref._build does (row = t * mbs + env, the order of the update's workspace)
    case["sigma"] = (std64 * (0.8 + 0.45 * torch.rand(A, generator=g, dtype=f64))).float()
    mu = (mu_new + 0.3 * torch.randn(T, mbs, A, generator=g, dtype=f64)).float()
    actions = (mu_new + std64 * torch.randn(T, mbs, A, generator=g, dtype=f64)).float()
    lp_new = _log_prob(actions.double(), mu_new, std64)
    tab = torch.tensor(plr.TABLE, dtype=f64)
    order = torch.randperm(len(plr.TABLE), generator=g)
    targets = tab[order[torch.arange(R) % len(plr.TABLE)]]
    r, adv, d, e = (x.reshape(T, mbs) for x in targets.unbind(-1))
    labels = torch.tensor([plr.regime_of(*t) for t in targets.tolist()], dtype=torch.int64).reshape(R, 2)
    sl = slice(mb * mbs, (mb + 1) * mbs)
    case["actions"][:, sl] = actions
    case["mu"][:, sl] = mu
    case["log_prob"][:, sl] = (lp_new - torch.log(r)).float()
    case["values"][:, sl] = (v_new - d).float()
    case["returns"][:, sl] = (v_new - e).float()
    case["advantages"][:, sl] = adv.float()
    case.update(targets=targets, surrogate_regime=labels[:, 0], value_regime=labels[:, 1])
    return case


@functools.lru_cache(maxsize=None)
def _build_cached(*key):
    return _build(*key)


def build_case(T, N, nmb, mb, O, OC, A, H, hidden, activation, pattern, seed):
    """Parameters (an ActorCriticRecurrent initialisation, std scaled per action by U(0.6, 1.4)), obs and critic_obs ~ N(0, 1) (drawn
    independently when OC is given, else one tensor), dones from the named pattern, the four saved states 0.5 N(0, 1) at every
    (t, env), and storage whose minibatch-mb rows are steered to a seeded permutation of ppo_loss_ref.TABLE from the float64 forward of
    that minibatch.  Everything is computed in float64 and stored as fp32.  Cached: callers must not write into the tensors."""
    return _build_cached(T, N, nmb, mb, O, OC, A, H, tuple(hidden), activation, pattern, seed)


def storage_of(case, dtype):
    st = {k: case[k].to(dtype) for k in STORAGE + STATES + ("sigma",)}
    st["critic_obs"] = case["critic_obs"].to(dtype)
    st["dones"] = case["dones"]
    return st


def reference(case, dtype=torch.float64):
    """Parameter gradients (by name, parameters() order), mean KL, mean value loss and mean surrogate of the case's minibatch through
    the literal generator: recurrent_ref.recurrent_minibatch + minibatch_loss on a model of `dtype`."""
    if dtype != torch.float64:
        return _reference(case, dtype)
    key = tuple(sorted((k, tuple(v) if isinstance(v, list) else v) for k, v in case["meta"].items()))
    if key not in _REF64:                               # computed once, shared by the tests that need it: callers must not write into it
        _REF64[key] = _reference(case, dtype)
    return _REF64[key]


_REF64 = {}


def _reference(case, dtype):
    m = case["meta"]
    ac = _model(case, dtype)
    b = rr.recurrent_minibatch(storage_of(case, dtype), m["mb"], m["nmb"])
    loss, kl, vl, sl = rr.minibatch_loss(ac, b, clip_param=ALG["clip_param"], value_loss_coef=ALG["value_loss_coef"],
                                         entropy_coef=ALG["entropy_coef"], use_clipped_value_loss=ALG["use_clipped_value_loss"])
    loss.backward()
    return {"grads": {k: p.grad.detach().double() for k, p in ac.named_parameters()}, "kl": float(kl), "value_loss": float(vl.detach()),
            "surrogate_loss": float(sl.detach())}


def _minibatch_rows(case):
    m = case["meta"]
    sl = slice(m["mb"] * m["mbs"], (m["mb"] + 1) * m["mbs"])
    pick = lambda k: case[k][:, sl].double()
    return pick("actions"), pick("values"), pick("advantages"), pick("returns"), pick("log_prob"), pick("mu"), case["sigma"].double()


def reference_loop(case):
    """The same quantities in float64 from the step loop, with the cell, the MLPs, the Gaussian and the loss spelled out."""
    names = [n for n, _ in _model(case, torch.float32).named_parameters()]
    p = {k: case["params"][k].double().clone().requires_grad_(True) for k in names}
    actions, v_old, adv, ret, lp_old, mu_old, sig_old = _minibatch_rows(case)
    mu, v = _loop_forward(case, p)
    std = p["std"]
    lp = _log_prob(actions, mu, std)
    ratio = torch.exp(lp - lp_old)
    surrogate = torch.maximum(-adv * ratio, -adv * ratio.clamp(1.0 - CLIP, 1.0 + CLIP)).mean()
    v_clipped = v_old + (v - v_old).clamp(-CLIP, CLIP)
    value_loss = torch.maximum((v - ret) ** 2, (v_clipped - ret) ** 2).mean()
    entropy = (0.5 + 0.5 * math.log(2.0 * math.pi) + torch.log(std)).sum()      # the same for every row
    loss = surrogate + ALG["value_loss_coef"] * value_loss - ALG["entropy_coef"] * entropy
    loss.backward()
    with torch.no_grad():
        kl = (torch.log(std / sig_old + 1e-5) + (sig_old ** 2 + (mu_old - mu) ** 2) / (2.0 * std ** 2) - 0.5).sum(-1).mean()
    return {"grads": {k: p[k].grad.detach() for k in names}, "kl": float(kl), "value_loss": float(value_loss.detach()),
            "surrogate_loss": float(surrogate.detach())}


def row_quantities(case, clip=CLIP):
    """What the branches of the loss look at, per row (t * mbs + env) in float64: ratio, v_new - v_old, the two value losses, the
    advantage."""
    actions, v_old, adv, ret, lp_old, _, _ = _minibatch_rows(case)
    p = {k: v.double() for k, v in case["params"].items()}
    with torch.no_grad():
        mu, v = _loop_forward(case, p)
        lp = _log_prob(actions, mu, p["std"])
    vc = v_old + (v - v_old).clamp(-clip, clip)
    flat = lambda x: x.reshape(-1)
    return {"ratio": flat(torch.exp(lp - lp_old)), "d": flat(v - v_old), "l1": flat((v - ret) ** 2), "l2": flat((vc - ret) ** 2),
            "adv": flat(adv)}


def step_reference(params, activation, obs, critic_obs, h_a, c_a, h_c, c_c, noise=None):
    """One live step in float64 from the given states: new (h, c) of both memories, actor mean, value and -- with `noise` -- the
    action mu + std noise and its log-probability."""
    p = {k: v.detach().double().cpu() for k, v in params.items()}
    d = lambda x: x.detach().double().cpu()
    out = {}
    out["h_a"], out["c_a"] = lstm_cell(d(obs), d(h_a), d(c_a), *_mem(p, "a"))
    out["h_c"], out["c_c"] = lstm_cell(d(critic_obs), d(h_c), d(c_c), *_mem(p, "c"))
    out["mu"] = mlp(p, "actor", out["h_a"], activation)
    out["value"] = mlp(p, "critic", out["h_c"], activation).squeeze(-1)
    if noise is not None:
        out["actions"] = out["mu"] + p["std"] * d(noise)
        out["log_prob"] = _log_prob(out["actions"], out["mu"], p["std"])
    return out


# ------------------------------------------------------------------------------------------------ bands
def _rel(got, ref):
    n = float(ref.norm())
    e = float((got - ref).norm())
    if n == 0.0:
        return 0.0 if e == 0.0 else float("inf")
    return e / n


def band_errors(got, ref, case):
    """Every band of the comparison as name -> (error, bound); `got` / `ref` as reference() returns them.  The project's bands
    (ppo_loss_ref.band_errors, tests/test_hip_ppo.py), applied tensor by tensor: element-wise rtol 2e-3 + atol 2e-4 max|ref of that
    tensor| (reported as the worst fraction of the band used, bound 1) and relative norm 2e-4 (3e-4 for an activation other than
    elu).  KL: rtol 1e-3, atol 1e-6.  Mean value loss and mean surrogate: rtol 1e-4, atol 1e-6."""
    nb = 2e-4 if case["meta"]["activation"] == "elu" else 3e-4
    out = {}
    for k, r in ref["grads"].items():
        g = got["grads"][k].double()
        diff, band = (g - r).abs(), 2e-3 * r.abs() + 2e-4 * float(r.abs().max())
        used = torch.where(diff == 0, torch.zeros_like(diff), diff / band)
        out["elem." + k] = (float(used.max()), 1.0)
        out["norm." + k] = (_rel(g, r), nb)
    out["kl"] = (abs(got["kl"] - ref["kl"]), 1e-3 * abs(ref["kl"]) + 1e-6)
    for k in ("value_loss", "surrogate_loss"):
        out[k] = (abs(got[k] - ref[k]), 1e-4 * abs(ref[k]) + 1e-6)
    return out


def worst(errs):
    """(name, error / bound) of the band used most."""
    k = max(errs, key=lambda n: errs[n][0] / errs[n][1])
    return k, errs[k][0] / errs[k][1]


# ---- the case matrix: (label, T, N, nmb, mb, O, OC, A, H, hidden, activation, dones).  mbs = N / nmb rows per step launch (64 rows
# per workgroup, 4 per thread), R = T mbs rows for the GEMMs and k_lstm_bias_grad (ceil(R / 256) row splits, 64 from R = 16384).
M3, M2 = (128, 64, 32), (64, 32)
CASES = (
    ("one_env_last_minibatch", 5, 4, 4, 3, 48, None, 12, 32, M3, "elu", "rand"),
    ("three_rows_privileged_all_reload", 6, 6, 2, 1, 48, 65, 3, 64, M3, "elu", "all"),
    ("one_full_tile_h256_net128", 8, 128, 2, 0, 48, None, 12, 256, (512, 256, 128), "elu", "rand"),
    ("tile_plus_1_h96_privileged_tanh", 8, 130, 2, 1, 235, 187, 12, 96, (96, 40), "tanh", "runs"),
    ("three_tiles_last_2_rows_t24", 24, 260, 2, 1, 48, None, 12, 128, M3, "elu", "rand"),
    ("h512", 3, 16, 1, 0, 48, None, 12, 512, M3, "elu", "last"),
    ("t1_70_rows", 1, 140, 2, 1, 48, None, 12, 64, M3, "elu", "none"),
    ("bias_split_r257", 1, 257, 1, 0, 45, None, 12, 32, M2, "elu", "none"),
    ("bias_split_64way_r16448", 64, 257, 1, 0, 45, None, 12, 32, M2, "elu", "rand"),
    ("full_depth_bptt", 24, 8, 2, 0, 48, None, 12, 64, M3, "elu", "none"),
    # added: the smallest sequence with a carry (one k_lstm_bwd launch with dG_next, cut_next read at its only position)
    ("t2_one_carry", 2, 10, 2, 1, 48, None, 12, 64, M3, "elu", "rand"),
    # added: R = 514, past the next change of k_lstm_bias_grad's split count (513) and no multiple of it: three splits of
    # ceil(514 / 3) = 172, 172 and 170 rows -- a floor there would drop a row (513 = 3 * 171 divides exactly and could not tell)
    ("bias_split_r514", 2, 257, 1, 0, 45, None, 12, 32, M2, "elu", "rand"),
    # added: the 64-way split with a remainder (the issue's 16 448 = 64 * 257 divides exactly): 65 * 253 = 16 445 rows, 63 splits of
    # 257 and one of 254
    ("bias_split_64way_r16445", 65, 253, 1, 0, 45, None, 12, 32, M2, "elu", "rand"),
    # added: a privileged critic on 2048 rows -- the dW_ih launch (4H = 128 rows of W_ih against Op = 64 and OCp = 128 columns: 2 and 4
    # tiles of 64 x 64) takes 8 reduction slices, the count from which the weight-gradient kernel regroups its workgroups per XCD
    ("privileged_r2048_unequal_wih_tiles", 8, 256, 1, 0, 48, 100, 12, 32, M2, "elu", "rand"),
)
DETERMINISTIC = ("tile_plus_1_h96_privileged_tanh", "three_tiles_last_2_rows_t24")

# Two of the compared numbers are sums that cancel (the mean surrogate, the critic head's bias gradient): see ppo_loss_ref.SEED.
# tests/test_recurrent_loss_host.py asserts that with these seeds the fp32 restatement stays below a quarter of every band and that
# every tensor's gradient carries signal.
SEED = 15
# with seed 15 the five rows of the one-env case leave a critic head bias gradient of 1e-9 of the whole (d loss / d value cancels
# exactly over them), and the 21 passes through the symmetric table of the 16 448-row case leave one of 7e-4 on which the fp32
# restatement alone uses a quarter of the band
SEEDS = {"one_env_last_minibatch": 10, "bias_split_64way_r16448": 21}


def case_id(c):
    return c[0]


def by_label(label):
    return next(c for c in CASES if c[0] == label)


def build_for(c):
    label, T, N, nmb, mb, O, OC, A, H, hidden, act, pattern = c
    return build_case(T, N, nmb, mb, O, OC, A, H, hidden, act, pattern, SEEDS.get(label, SEED))
