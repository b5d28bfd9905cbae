"""Float64 reference, dispatch arithmetic, case list and bounds for the rollout's policy step (HipPPO.act): the one-launch forward of
both MLPs with its sampling epilogue (k_mlp_fwd, csrc/ppo_mlp_fused.hip) and the per-layer GEMMs + k_act_sample it falls back to.
tests/test_ppo_act_host.py proves on the CPU what the bounds below rest on; tests/test_hip_ppo_act.py runs the cases on the GPU, each
on both paths through the same assertions.

Input families -- none of their bounds comes from the library under test (helpers of tests/gemm_ref.py):
  int_relu  activation relu; observations and first-layer weights integers in [-15, 15] (h term only), deeper layers ternary with four
            nonzero entries per output (gemm_ref._ternary, cap 4), biases integers in [-100, 100].  For every layer |W| . |x| + |b| <
            2^24: every retained term product and every partial sum is an integer below 2^24, exact in fp32 in any order, so means and
            values must EQUAL the float64 reference.  A wrong tile, a dropped or doubled k-step, a stale pad column: a difference.
  int_elu   the same with every entry non-negative: each pre-activation is >= 0, where the ELU compiled into the ACT = 1 instantiation
            is the identity (exp(0) - 1 = 0).  Equality again.
  rand      randn observations scaled per column by 2^randint(-6, 6), the inverse scale on the first layer's columns, nn.Linear-scale
            weights and biases elsewhere.  Two bounds, both from the float64 reference alone:
              structural  B_pre,l = (6 K_l + 8) 2^-24 (|W_l| . |x_(l-1)| + |b_l|) + |W_l| . B_out,(l-1);  B_out,l from B_pre,l by the
                          slope and kink rule of gemm_ref (bound_through_activation, __expf terms included);  B_out,0 = 0
              precision   E_k <= M E_y + 2^-24,  E = max |. - ref| / S over both heads (S = |W| . |x| + |b| of the head layer), the
                          yardstick Y the textbook fp32 evaluation in torch on the CPU (yardstick(): rank-one updates along k)
Every family draws a per-action std in [0.05, 3], all distinct.

Sampling: Philox4x32-10 in numpy with philox_normal's layout (counter {env_offset + env, low word of act_count, action, 0x5eed}, key =
seed lo / hi), Box-Muller on it in float64, and the log-prob in float64 with the bound lp_bound() derives from the kernel's arithmetic.
"""
import zlib

import numpy as np
import torch

from tests import gemm_ref as gr

F64 = torch.float64
U = gr.U

MLP_NW, MLP_KMAX = 4, 512                       # waves per workgroup, widest LDS image (csrc/ppo_mlp_fused.hip)
ACT_CODE = {"elu": 1, "selu": 2, "relu": 3, "lrelu": 4, "tanh": 5, "sigmoid": 6, "crelu": 3}      # the kernels' activation codes

# E_k <= M E_y + 2^-24: twice the largest E_k / E_y measured over the rand runs on the MI355X, rounded up to one digit, separately for
# the activations evaluated exactly in fp32 (relu, lrelu, crelu: 1.55) and for those on __expf / __frcp_rn (elu, selu, tanh, sigmoid:
# 1.78, on tanh), whose error the yardstick (torch's expm1 / tanh / sigmoid) does not share.  Both round to 4.  The table is in the
# docstring of tests/test_hip_ppo_act.py.
PRECISION_M = {False: 4.0, True: 4.0}
# the device's sqrtf, logf and cosf of Box-Muller against the same formula in numpy float32: twice the largest ratio measured (1.16)
NORMAL_MARGIN = 3.0
# the device's logf(std) inside the log-prob, in units of the worst |float32 log - float64 log| over the case's std.  Its share cannot
# be read off the log-prob alone; with margin 1 the whole bound lp_bound() is used to 0.51 at worst on the MI355X, so 1 stays.
LOGF_MARGIN = 1.0


# ------------------------------------------------------------------------------------------------ the dispatch arithmetic, restated
def kpad(K):
    return (K + 15) & ~15


def layer_dispatch(K, N):
    """What k_mlp_fwd does for a layer of K inputs and N outputs: per wave, `mine` column tiles and the mlp_layer<CT, S> calls that
    cover them as (CT, S, t0, nkb, tail) -- nkb blocks of S k-steps, tail: the last block is cut short by the k-tail `break`."""
    nks, ntiles = kpad(K) // 16, (N + 31) // 32
    waves = []
    for wave in range(MLP_NW):
        mine = -(-(ntiles - wave) // MLP_NW) if ntiles > wave else 0
        calls, t0 = [], 0
        while t0 < mine:
            c = mine - t0
            CT, S = (4, 1) if c >= 4 else (2, 2) if c >= 2 else (1, 4)
            calls.append((CT, S, t0, -(-nks // S), nks % S != 0))
            t0 += CT
        waves.append((mine, calls))
    return dict(kpad=kpad(K), nks=nks, ntiles=ntiles, waves=waves)


def supported(dims):
    """ppok_mlp_supported on dims = (actor widths, critic widths), input first, head last; HipPPO builds both nets equally deep."""
    for d in dims:
        for l in range(len(d) - 1):
            K, N = d[l], d[l + 1]
            if (l > 0 and K % 16) or kpad(K) > MLP_KMAX or K < 1:
                return False
            if l < len(d) - 2 and (N % 32 or N > MLP_KMAX):
                return False
    return len(dims[0]) == len(dims[1])


def nkb_class(nkb):
    return "1" if nkb == 1 else "even" if nkb % 2 == 0 else "odd>1"


# every entry the case list must reach: (CT, S, class of nkb, k-tail) -- S = 1 has no tail -- every `mine`, and a workgroup whose waves differ
MATRIX = [(4, 1, c, False) for c in ("1", "even", "odd>1")] + \
         [(CT, S, c, tail) for CT, S in ((2, 2), (1, 4)) for c in ("1", "even", "odd>1") for tail in (False, True)] + \
         [("mine", m) for m in range(5)] + [("mixed",)]


def case_dims(c):
    return ([c["O"]] + list(c["actor"]) + [c["A"]], [c["OC"] or c["O"]] + list(c["critic"]) + [1])


def entries(c):
    """The MATRIX entries a case reaches (empty when the one-launch kernel refuses its shape)."""
    out = set()
    dims = case_dims(c)
    if not supported(dims):
        return out
    for d in dims:
        for l in range(len(d) - 1):
            waves = layer_dispatch(d[l], d[l + 1])["waves"]
            if len({m for m, _ in waves if m}) > 1:
                out.add(("mixed",))
            for mine, calls in waves:
                out.add(("mine", mine))
                for CT, S, t0, nkb, tail in calls:
                    out.add((CT, S, nkb_class(nkb), tail))
    return out


# ------------------------------------------------------------------------------------------------ cases
def _case(label, O, OC, actor, critic, N, A, act="elu", fused=True):
    fams = {"relu": ("int_relu", "rand"), "elu": ("int_elu", "rand")}.get(act, ("rand",))
    return dict(label=label, O=O, OC=OC, actor=actor, critic=critic, N=N, A=A, act=act, fused=fused, families=fams)


def _cases():
    c = []
    w3 = [288, 160, 96]
    # the three small nets whose layers reach most of the matrix (mixed `mine` in one workgroup: 288 -> 3, 2, 2, 2; 160 -> 2, 1, 1, 1;
    # 416 -> 4, 3, 3, 3), against observation widths of 1, 3, 5, 11 and 15 k-steps
    c.append(_case("288-160-96/o3-oc65", 3, 65, w3, w3, 33, 12, "elu"))
    c.append(_case("288-160-96/o48-oc169", 48, 169, w3, w3, 31, 1, "relu"))
    c.append(_case("256-384-64|160-416-32/o16-oc235", 16, 235, [256, 384, 64], [160, 416, 32], 32, 16, "relu"))
    c.append(_case("160-416-32|256-384-64/o235-oc16", 235, 16, [160, 416, 32], [256, 384, 64], 1, 12, "elu"))
    # <2,2> on two k-steps (one whole block) and <1,4> on twelve (three whole blocks)
    c.append(_case("32-160-32|192-32-32/o48", 48, None, [32, 160, 32], [192, 32, 32], 300, 12, "elu"))
    # <4,1> on one k-step and on an even count; the widest LDS image (512 = MLP_KMAX) and pad columns just under it (500)
    c.append(_case("416-32-32|512-32-32/o3-oc512", 3, 512, [416, 32, 32], [512, 32, 32], 33, 12, "relu"))
    c.append(_case("512-32-32|416-32-32/o500-oc3", 500, 3, [512, 32, 32], [416, 32, 32], 31, 12, "elu"))
    # the product shapes
    for O, N in ((48, 300), (235, 300), (169, 33), (65, 32)):
        c.append(_case(f"512-256-128/o{O}", O, None, [512, 256, 128], [512, 256, 128], N, 12, "elu"))
    # the six other activation names on one small net (ACT = -1 instantiation)
    for act in ("selu", "relu", "lrelu", "tanh", "sigmoid", "crelu"):
        c.append(_case(f"160-96-32/o48/{act}", 48, None, [160, 96, 32], [160, 96, 32], 33, 12, act))
    # shapes the one-launch kernel refuses: hidden widths off the 32-grid, an observation wider than the LDS image
    c.append(_case("96-40-24/o169-refused", 169, None, [96, 40, 24], [96, 40, 24], 33, 12, "elu", fused=False))
    c.append(_case("64-32/o520-refused", 520, None, [64, 32], [64, 32], 33, 12, "relu", fused=False))
    return tuple(c)


CASES = _cases()


def runs():
    return [(c, f) for c in CASES for f in c["families"]]


def run_id(r):
    return f"{r[0]['label']}/{r[1]}"


def policy_cfg(c):
    return {"actor_hidden_dims": list(c["actor"]), "critic_hidden_dims": list(c["critic"]), "activation": c["act"], "init_noise_std": 1.0}


# ------------------------------------------------------------------------------------------------ inputs
INT_X, INT_B, INT_CAP = 15, 100, 4


def build_inputs(c, fam, tag=""):
    """Parameters under HipPPO's names (fp32, CPU), std [A], and per act() call observations / critic observations / injected noise.
    Seeded by (label, family, tag): `tag` draws a second, independent set (the parameter-write test)."""
    g = torch.Generator().manual_seed(zlib.crc32(f"{c['label']}/{fam}/{tag}".encode()))
    dims = case_dims(c)
    N, A = c["N"], c["A"]
    params = {}
    if fam == "rand":
        scale = [torch.exp2(torch.randint(-6, 7, (d[0],), generator=g).float()) for d in dims]
    for z, (net, d) in enumerate(zip(("actor", "critic"), dims)):
        for l in range(len(d) - 1):
            K, Nn = d[l], d[l + 1]
            if fam == "rand":
                W = (torch.rand(Nn, K, generator=g) * 2 - 1) / K ** 0.5
                b = (torch.rand(Nn, generator=g) * 2 - 1) / K ** 0.5
                if l == 0:
                    W = torch.randn(Nn, K, generator=g) / K ** 0.5 / scale[z]
            else:
                W = torch.randint(-INT_X, INT_X + 1, (Nn, K), generator=g).float() if l == 0 else gr._ternary(Nn, K, g, INT_CAP)
                b = torch.randint(-INT_B, INT_B + 1, (Nn,), generator=g).float()
                if fam == "int_elu":
                    W, b = W.abs(), b.abs()
            params[f"{net}.{2 * l}.weight"], params[f"{net}.{2 * l}.bias"] = W, b
    std = (0.05 + 2.95 * (torch.randperm(A, generator=g).double() + torch.rand(A, generator=g).double() * 0.5) / A).float()
    params["std"] = std

    def observations(z):
        O = dims[z][0]
        if fam == "rand":
            return torch.randn(N, O, generator=g) * scale[z]
        x = torch.randint(-INT_X, INT_X + 1, (N, O), generator=g).float()
        return x.abs() if fam == "int_elu" else x
    calls = []
    for _ in range(2):
        obs = observations(0)
        cobs = observations(1) if c["OC"] else None
        calls.append(dict(obs=obs, cobs=cobs, noise=torch.randn(N, A, generator=g)))
    return dict(params=params, std=std, calls=calls)


# ------------------------------------------------------------------------------------------------ reference, yardstick, bounds
def _layers(params, net):
    l = 0
    while f"{net}.{2 * l}.weight" in params:
        yield params[f"{net}.{2 * l}.weight"], params[f"{net}.{2 * l}.bias"]
        l += 1


def forward64(c, params, x, net):
    """Float64 forward of one net on fp32 inputs.  Returns out [N][head], S of the head layer, the per-layer (K, S, pre) for the bounds."""
    act = ACT_CODE[c["act"]]
    x = x.to(F64)
    layers = list(_layers(params, net))
    trace = []
    for l, (W, b) in enumerate(layers):
        W, b = W.to(F64), b.to(F64)
        pre = x @ W.t() + b
        S = x.abs() @ W.abs().t() + b.abs()
        head = l == len(layers) - 1
        out = pre if head else gr.act_fwd64(act, pre)
        trace.append(dict(K=W.shape[1], W=W, S=S, pre=pre, out=out, act=0 if head else act))
        x = out
    return x, trace[-1]["S"], trace


def structural_bound(trace):
    """B_out of the head layer, propagated layer by layer as the module docstring states."""
    B_out = None
    for t in trace:
        B = (6 * t["K"] + 8) * U * t["S"]
        if B_out is not None:
            B = B + B_out @ t["W"].abs().t()
        B_out = gr.bound_through_activation(t["act"], t["pre"], t["out"], B)
    return B_out


def pre_bounds(trace):
    """B_pre of every layer (the host test looks at the intervals pre +- B_pre)."""
    out, B_out = [], None
    for t in trace:
        B = (6 * t["K"] + 8) * U * t["S"]
        if B_out is not None:
            B = B + B_out @ t["W"].abs().t()
        out.append(B)
        B_out = gr.bound_through_activation(t["act"], t["pre"], t["out"], B)
    return out


def yardstick(c, params, x, net):
    """The textbook fp32 evaluation on the CPU: per layer a loop over k of rank-one updates in torch.float32, bias, activation."""
    act = ACT_CODE[c["act"]]
    layers = list(_layers(params, net))
    x = x.float()
    for l, (W, b) in enumerate(layers):
        acc = torch.zeros(x.shape[0], W.shape[0])
        for k in range(W.shape[1]):
            acc += x[:, k, None] * W[None, :, k]
        acc = acc + b
        x = acc if l == len(layers) - 1 else gr.act_fwd64(act, acc)
    return x


def on_expf(c):
    return ACT_CODE[c["act"]] in (1, 2, 5, 6)


# ------------------------------------------------------------------------------------------------ Philox4x32-10, Box-Muller
_M0, _M1, _W0, _W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays of one shape (or scalars), key: (k0, k1).  Returns the four output words as uint32 arrays."""
    c = [np.asarray(x, dtype=np.uint64) & 0xFFFFFFFF for x in ctr]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0, p1 = c[0] * np.uint64(_M0), c[2] * np.uint64(_M1)
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & np.uint64(0xFFFFFFFF), p1 >> np.uint64(32), p1 & np.uint64(0xFFFFFFFF)
        c = [hi1 ^ c[1] ^ np.uint64(k0), lo1, hi0 ^ c[3] ^ np.uint64(k1), lo0]
        k0, k1 = (k0 + _W0) & 0xFFFFFFFF, (k1 + _W1) & 0xFFFFFFFF
    return [x.astype(np.uint32) for x in c]


def learner_seed(seed, rank=0):
    """The 64-bit seed HipPPO hands to the library."""
    return (int(seed) * 1000003 + rank) & 0xFFFFFFFFFFFFFFFF


def uniforms(seed64, N, A, act_count, env_offset=0):
    """u1 in (0, 1], u2 in [0, 1) of philox_normal for every (env, action) of one act() call, as float64 [N][A] (both are multiples of
    2^-24: exact in fp32 as in float64)."""
    env = (np.arange(N, dtype=np.uint64)[:, None] + np.uint64(env_offset))
    a = np.arange(A, dtype=np.uint64)[None, :]
    r = philox4x32_10([env, np.uint64(act_count & 0xFFFFFFFF), a, np.uint64(0x5EED)], (seed64 & 0xFFFFFFFF, seed64 >> 32))
    u1 = ((r[0] >> np.uint32(8)).astype(np.float64) + 1.0) / 16777216.0
    u2 = (r[1] >> np.uint32(8)).astype(np.float64) / 16777216.0
    return u1, u2


def box_muller64(u1, u2):
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


def box_muller32(u1, u2):
    """philox_normal's formula in numpy float32, operation by operation: the yardstick for the device's logf, sqrtf and cosf."""
    u1, u2 = u1.astype(np.float32), u2.astype(np.float32)
    return np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(np.float32(6.283185307179586) * u2)


# ------------------------------------------------------------------------------------------------ log-prob
LOG_SQRT_2PI = 0.9189385332046727


def log_prob64(z, std):
    """sum_a -(z^2 / 2) - log std_a - log sqrt(2 pi): the log-prob of a = mu + std z, whatever mu is.  z [N][A], std [A] float64."""
    return (-(z * z) / 2 - torch.log(std) - LOG_SQRT_2PI).sum(-1)


def lp_bound(mu, act, z, std):
    """Bound on |lp_kernel - log_prob64(z, std)| per env, from the kernel's arithmetic on ITS mean mu and action act (float64 [N][A]):
      act = fl(mu + std z) carries one rounding of |act| (the compiler contracts it into an fma);  d = act - mu is exact or carries one
      more rounding;  the quadratic's sensitivity to act is |d| / std^2.
      term error <= |d| |act| 2^-23 / std^2 + 4 2^-24 (|term| + |log std|) + the device's logf error (LOGF_MARGIN times the worst
      |float32 log - float64 log| over the case's std);  the sequential fp32 sum over A terms adds (A - 1) 2^-24 sum |term|."""
    d = act - mu
    term = -(z * z) / 2 - torch.log(std) - LOG_SQRT_2PI
    logf_err = float((torch.log(std.float()).double() - torch.log(std)).abs().max())
    per = d.abs() * act.abs() * 2 * U / (std * std) + 4 * U * (term.abs() + torch.log(std).abs()) + LOGF_MARGIN * logf_err
    A = z.shape[-1]
    return per.sum(-1) + (A - 1) * U * term.abs().sum(-1)


def action_bound(mu_err, act, z, std):
    """|act_kernel - (mu_ref + std z)| <= the mean's own bound + one rounding each of |std z| and |act|."""
    return mu_err + U * ((std * z).abs() + act.abs())
