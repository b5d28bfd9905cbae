"""Float64 reference, fp32 yardstick, input families and case lists for the single tube trainer (k_tube_rows, k_tube_adam,
k_tube_eval_finish of csrc/tube_kernels.hip, through HipTubeTrainer).  Nothing here comes from the library but the pure-Python window
item of tube/data.py: the model and losses are tests/tube_ref.py and tests/tube_level_ref.py under torch autograd, Adam is restated in
numpy float64.  tests/test_tube_train_host.py asserts the conditions of every case on the CPU; tests/test_hip_tube_train.py runs the
cases on the GPU.

Yardstick of a step.  The kernel sums a gradient entry over the LG_TUBE_ROWS = 32 rows of a tile in one workgroup and then over the
tiles in tile order.  The yardstick restates that in float32 (grad_chains): every dot product one fmaf chain in the kernel's index
order, the rows inside a tile in sequence with one fmaf each, the tile partials added in tile order; the loss sum follows the same
order.  A coarser restatement -- per tile float32 AUTOGRAD of (the tile's loss sum) / (the step's norm), partials added in tile order
(grad_tiles) -- was the first yardstick; it stays as the cross-check of the host test and as the gradient of the trajectories'
yardstick.  It is not the step's yardstick because torch's matrix products sum in blocks, which at 130 inputs is several times more
accurate than a sequential chain: on vector-softplus (33 rows, 130 -> 32 x 3 -> 2) its error is 6.9e-8 of max |g| where the chain
restatement's is 3.0e-7 -- and the device's, to the digit (Accuracy).
e32 = max |yardstick - float64| over the whole gradient and again over every block of the parameter layout; the device must
lie within MARGIN = 4 e32, the project's margin for two valid fp32 evaluations of one arithmetic.  A block's
e32 is floored at the whole vector's e32 scaled by (the block's max |g64| / the vector's max |g64|): a block of one element is a
single draw that can land on the float64 value by luck (the argument of tests/ppo_opt_ref.py).

Families.  "rand": randn inputs, default initialisation.  "saturated": the hidden layers' weights and biases scaled so that the smooth
activations sit in the branches tube_act_grad forms from the activation's OUTPUT (softplus past its threshold, tanh with 1 - h^2
cancelling, deep-negative ELU).  "exact": every intermediate exactly representable in fp32, so gradient and loss equal the float64
reference on the bits in any summation order and the tie rules (r = 0, |l| = delta, ReLU'(0) = 0, ELU'(0) = 1) can be hit on purpose.

Kinks.  The pinball residual r = w - fw and a ReLU pre-activation switch the gradient discontinuously at 0: a row on the other side
of a kink in fp32 is no rounding error.  Rows come from a pool; a row is used only where its float64 margin (the smallest |ReLU
pre-activation| and, for the tube losses, the smallest |w - fw|) is at least KINK = 32 x the largest |float32 - float64| difference
of those same quantities over the pool, computed per case.

Adam.  One step's reference is float64 Adam applied to the DEVICE's own gradient (that isolates the optimiser from the step); the
yardstick is torch.optim.Adam in float32.  Floors: c sqrt(k) 2^-24 mag with c = 1, 2, 3 for params, m, v -- the count of roundings of
a valid fp32 evaluation derived in tests/ppo_opt_ref.py's module docstring (its clip coefficient is absent here, which only lowers
the count).  There is no allowance for the bias corrections: k_tube_adam forms them in double, as torch does.
"""
import functools
import math
from collections import OrderedDict
from types import SimpleNamespace

import numpy as np
import torch

from tests import tube_level_ref, tube_ref

R = 32                              # LG_TUBE_ROWS
MARGIN = 4.0
U24 = 2.0 ** -24
ALPHA, DELTA = 0.6875, 0.5          # both exact in fp32: the float64 reference and the device hold the same constants
LEVEL_LO, LEVEL_HI = 0.0625, 0.9375
POOL = 4096
KINK_FACTOR, SENTINEL_FACTOR = 32.0, 16.0
LEVEL_LOSSES = ("scalar_level", "vector_level")
FLOOR_ROUNDINGS = {"params": 1.0, "m": 2.0, "v": 3.0}       # tests/ppo_opt_ref.py


# ------------------------------------------------------------------------------------------------ model, layout, losses
def param_shapes(I, O, U, L):
    dims = [I] + [U] * L + [O]
    out = []
    for i in range(L + 1):
        out += [(f"layers.{2 * i}.weight", (dims[i + 1], dims[i])), (f"layers.{2 * i}.bias", (dims[i + 1],))]
    return out


def block_starts(dims):
    """Offsets of the blocks of lg_tube_param_layout: weight then bias per Linear layer, in state-dict order."""
    off, out = 0, []
    for _, s in param_shapes(*dims):
        out.append(off)
        off += int(np.prod(s))
    return np.array(out, dtype=np.int64), off


def default_params(dims, seed):
    """nn.Linear's default initialisation in the reference MLP's construction order after torch.manual_seed(seed)."""
    I, O, U, L = dims
    torch.manual_seed(seed)
    d = [I] + [U] * L + [O]
    sd = OrderedDict()
    for i in range(L + 1):
        lin = torch.nn.Linear(d[i], d[i + 1])
        sd[f"layers.{2 * i}.weight"], sd[f"layers.{2 * i}.bias"] = lin.weight.detach().clone(), lin.bias.detach().clone()
    return sd


def model(sd, dims, act, beta, dtype):
    I, O, U, L = dims
    m = tube_ref.MLP(I, O, U, L, act, beta).to(dtype)
    m.load_state_dict({k: v.to(dtype) for k, v in sd.items()})
    return m


def flat(sd_or_model, grad=False):
    if isinstance(sd_or_model, torch.nn.Module):
        return torch.cat([(p.grad if grad else p.detach()).reshape(-1) for p in sd_or_model.parameters()])
    return torch.cat([v.reshape(-1) for v in sd_or_model.values()])


def unflat(vec, dims):
    sd, off = OrderedDict(), 0
    for k, s in param_shapes(*dims):
        n = int(np.prod(s))
        sd[k] = torch.as_tensor(vec[off:off + n]).reshape(s).clone()
        off += n
    return sd


def kernel_loss(loss):
    return {"scalar": "scalar", "scalar_horizon": "scalar", "scalar_level": "scalar", "vector": "vector", "vector_level": "vector",
            "error": "error"}[loss]


def loss_norm(loss, count, O):
    return count if kernel_loss(loss) == "vector" else count * O


def terms(loss, fw, y, a, delta):
    """The summands of the loss before the mean: per element (scalar, error) or per row (vector).  a: alpha, or levels (B, 1)."""
    k = kernel_loss(loss)
    if k == "error":
        return (fw - y) ** 2
    l = tube_level_ref.pinball(fw, y, a) if torch.is_tensor(a) else tube_ref.pinball(fw, y, a)
    if k == "vector":
        l = l.sum(dim=-1)
    return torch.nn.functional.huber_loss(l, torch.zeros_like(l), delta=delta, reduction="none")


def ref_loss(loss, fw, y, a, delta):
    """The loss as tests/tube_ref.py and tests/tube_level_ref.py state it (the mean): what `terms` must add up to."""
    if torch.is_tensor(a):
        return tube_level_ref.loss(loss, fw, y, a, delta)
    return tube_ref.loss(loss, fw, y, a, delta)


def grad_whole(m, loss, x, y, a, delta, norm):
    """(gradient, loss) of terms.sum() / norm by autograd in the model's dtype, the whole batch at once."""
    m.zero_grad()
    val = terms(loss, m(x), y, a, delta).sum() / norm
    val.backward()
    return flat(m, grad=True).clone(), val.detach().clone()


def grad_tiles(m32, loss, x, y, a, delta, norm):
    """The yardstick: float32, per tile of R rows autograd of (tile loss sum) / norm, partials and loss sums added in tile order."""
    nrm = torch.tensor(float(norm), dtype=torch.float32)
    acc, ls = None, torch.zeros((), dtype=torch.float32)
    for b in range(0, x.shape[0], R):
        m32.zero_grad()
        s = terms(loss, m32(x[b:b + R]), y[b:b + R], a[b:b + R] if torch.is_tensor(a) else a, delta).sum()
        (s / nrm).backward()
        g = flat(m32, grad=True)
        acc = g.clone() if acc is None else acc + g
        ls = ls + s.detach()
    return acc, ls / nrm


def e32_blocks(yard, ref, dims):
    """(whole-vector e32, per-block e32) of a float32 vector against the float64 one, blocks floored (module docstring)."""
    starts, _ = block_starts(dims)
    err, mag = np.abs(np.asarray(yard, dtype=np.float64) - ref), np.abs(ref)
    whole = float(err.max())
    floor = whole * np.maximum.reduceat(mag, starts) / max(float(mag.max()), 1e-300)
    return whole, np.maximum(np.maximum.reduceat(err, starts), floor)


def ratio(err, bound):
    return 0.0 if err == 0.0 else float("inf") if bound == 0.0 else err / bound


def grad_ratios(got, ref, e32, dims):
    """Worst |got - ref| / (MARGIN e32): (over the whole vector, over the blocks)."""
    starts, _ = block_starts(dims)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    whole, blocks = e32
    return ratio(float(err.max()), MARGIN * whole), max(ratio(float(e), MARGIN * float(b)) for e, b in zip(np.maximum.reduceat(err, starts), blocks))


def scalar_e32(vals32, val64):
    """e32 of a scalar: the largest error of the fp32 evaluations given, floored at 2^-23 |value| (the final division and the store)."""
    return max(max(abs(float(v) - val64) for v in vals32), 2.0 ** -23 * abs(val64))


def norm_rtol(P):
    """k_tube_adam's gradient norm against the float64 norm of its own grads: n^2 is a sum of positive terms with at most one add per
    thread, eight in the tree and `blocks` in the last block, each 2^-24 relative; the square root halves the relative error."""
    return (math.ceil(P / 256) + 10) * 2.0 ** -25


# ------------------------------------------------------------------------------------------------ step cases
# (id, family, loss, activation, batch rows, I, O, U, L, horizon (H_fwd, H_rev, nz, m) or None).  I counts the level column of a level
# loss; a horizon case's I and O follow from the window.  Between them: every loss x activation, both level losses, the horizon
# dataset plain and level-conditioned, batch counts 1, 31, 32, 33, 63, 65, 2047, 2048, the envelope corner 256 -> 128 x 4 -> 64 (the
# 144 KiB LDS layout) and 3 -> 16 x 1 -> 1.
STEP_CASES = [
    ("scalar-relu", "rand", "scalar", "relu", 2048, 3, 1, 16, 1, None),
    ("scalar-softplus", "rand", "scalar", "softplus", 2047, 30, 2, 128, 1, None),
    ("scalar-tanh", "rand", "scalar", "tanh", 1, 130, 50, 48, 3, None),
    ("scalar-elu", "rand", "scalar", "elu", 31, 130, 1, 16, 4, None),
    ("vector-relu", "rand", "vector", "relu", 32, 30, 50, 128, 4, None),
    ("vector-softplus", "rand", "vector", "softplus", 33, 130, 2, 32, 3, None),
    ("vector-tanh", "rand", "vector", "tanh", 63, 3, 1, 128, 2, None),
    ("vector-elu", "rand", "vector", "elu", 65, 30, 50, 48, 1, None),
    ("error-relu", "rand", "error", "relu", 33, 3, 2, 48, 4, None),
    ("error-softplus-corner", "rand", "error", "softplus", 2047, 256, 64, 128, 4, None),
    ("error-tanh-full", "rand", "error", "tanh", 2048, 30, 1, 32, 1, None),
    ("error-elu", "rand", "error", "elu", 65, 3, 50, 128, 3, None),
    ("scalar_level-relu", "rand", "scalar_level", "relu", 63, 10, 3, 32, 2, None),
    ("vector_level-tanh", "rand", "vector_level", "tanh", 2047, 6, 4, 16, 2, None),
    ("horizon-softplus", "rand", "scalar_horizon", "softplus", 65, None, None, 32, 2, (4, 3, 2, 2)),
    ("horizon_level-elu", "rand", "scalar_level", "elu", 33, None, None, 16, 2, (4, 3, 2, 2)),
    ("sat-softplus", "saturated", "scalar", "softplus", 65, 30, 2, 128, 1, None),
    ("sat-tanh", "saturated", "error", "tanh", 33, 30, 1, 64, 2, None),
    ("sat-elu", "saturated", "vector", "elu", 2047, 30, 3, 48, 2, None),
]
STEP_IDS = [c[0] for c in STEP_CASES]
SAT_SCALE = 6.0
HORIZON_ENVS, HORIZON_T = 128, 24


class Horizon:
    """A synthetic (w, z, v) namespace; the window item and target are tube/data.py's."""

    def __init__(self, w, z, v, H_fwd, H_rev):
        self.w, self.z, self.v, self.H_fwd, self.H_rev = w, z, v, H_fwd, H_rev

    def item(self, env, start):
        from legged_gym_dev_amd.tube.data import ScalarHorizonTubeDataset
        return ScalarHorizonTubeDataset._get_item_helper(self, env, start)


class Flat:
    def __init__(self, x, y):
        self.data, self.target = x, y


def _seed_of(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % (2 ** 31)


@functools.lru_cache(maxsize=None)
def case(name):
    """The fixed part of a step case: model, parameters, data pool, the stand-in draws of the host test, KINK and the survivors."""
    _, family, loss, act, B, I, O, U, L, hz = STEP_CASES[STEP_IDS.index(name)]
    g = torch.Generator().manual_seed(_seed_of(name))
    level = loss in LEVEL_LOSSES
    c = SimpleNamespace(name=name, family=family, loss=loss, act=act, B=B, level=level, horizon=hz, seed=_seed_of(name),
                        beta=5.0 if act == "softplus" else 1.0, alpha=None if level else ALPHA, delta=DELTA)
    if hz:
        Hf, Hr, nz, m = hz
        I, O = Hr + nz + (Hr + Hf) * m + int(level), Hf
        c.ds = Horizon(torch.rand(HORIZON_ENVS, HORIZON_T, generator=g), torch.randn(HORIZON_ENVS, HORIZON_T, nz, generator=g),
                        torch.randn(HORIZON_ENVS, HORIZON_T, m, generator=g), Hf, Hr)
        c.pool = HORIZON_ENVS
    else:
        c.x = torch.randn(POOL, I - int(level), generator=g)
        c.y = (torch.rand(POOL, O, generator=g) - 0.4) * 2.0
        c.pool = POOL
    c.dims = (I, O, U, L)
    sd = default_params(c.dims, c.seed)
    if family == "saturated":
        for i in range(L):
            sd[f"layers.{2 * i}.weight"] *= SAT_SCALE
            sd[f"layers.{2 * i}.bias"] *= SAT_SCALE
    c.sd = sd
    c.m64, c.m32 = model(sd, c.dims, act, c.beta, torch.float64), model(sd, c.dims, act, c.beta, torch.float32)
    # stand-in draws, one per pool position: the device's own are read back after a first step
    c.standin_starts = torch.randint(hz[1], HORIZON_T - hz[0] - 1, (c.pool,), generator=g, dtype=torch.int32) if hz else None
    c.standin_levels = (LEVEL_LO + (LEVEL_HI - LEVEL_LO) * torch.rand(c.pool, generator=g)) if level else None
    c.order = torch.randperm(c.pool, generator=g)
    ids = torch.arange(c.pool)
    x64, y64, _ = items(c, ids, c.standin_starts, c.standin_levels, torch.float64)
    x32, y32, _ = items(c, ids, c.standin_starts, c.standin_levels, torch.float32)
    q64, q32 = kink_quantities(c, c.m64, x64, y64), kink_quantities(c, c.m32, x32, y32)
    c.kink = KINK_FACTOR * float((q32.double() - q64).abs().max()) if q64.shape[1] else 0.0
    c.pool_survives = margin(c, x64, y64) >= c.kink
    return c


def items(c, rows, starts=None, levels=None, dtype=torch.float64):
    """(x (B, I), y (B, O), a) of the batch: row ids, and per POSITION the window start and the level where the case has them."""
    rows = torch.as_tensor(rows).long()
    if c.horizon:
        pairs = [c.ds.item(int(r), int(s)) for r, s in zip(rows, starts)]
        x, y = torch.stack([p[0] for p in pairs]), torch.stack([p[1] for p in pairs])
    else:
        x, y = c.x[rows], c.y[rows]
    a = c.alpha
    if c.level:
        lv = torch.as_tensor(levels, dtype=torch.float32).reshape(-1, 1)
        x, a = torch.cat([x, lv], dim=1), lv.to(dtype)
    return x.to(dtype), y.to(dtype), a


def kink_quantities(c, m, x, y):
    """Per row, everything whose sign switches the gradient: the ReLU pre-activations and, for the tube losses, w - fw."""
    q, h = [], x
    with torch.no_grad():
        for layer in m.layers:
            h = layer(h)
            if isinstance(layer, torch.nn.Linear) and c.act == "relu" and layer is not m.layers[-1]:
                q.append(h)
        if kernel_loss(c.loss) != "error":
            q.append(y - h)
    return torch.cat(q, dim=1) if q else torch.zeros(x.shape[0], 0, dtype=x.dtype)


def margin(c, x64, y64):
    q = kink_quantities(c, c.m64, x64, y64)
    return q.abs().min(dim=1).values if q.shape[1] else torch.full((x64.shape[0],), float("inf"), dtype=torch.float64)


def select_rows(c, starts=None, levels=None):
    """The batch's row ids: the case's pool order, every position's row checked against KINK at that position's draw and swapped
    for the next unused pool row where it fails.  starts / levels: the draws per position (None: the host's stand-ins)."""
    B = c.B
    if starts is None and c.horizon:
        starts = c.standin_starts[:B]
    if levels is None and c.level:
        levels = c.standin_levels[:B]
    rows, spare = c.order[:B].clone(), iter(c.order[B:].tolist())
    x64, y64, _ = items(c, rows, starts, levels)
    bad = (margin(c, x64, y64) < c.kink).nonzero().reshape(-1).tolist()
    for pos in bad:
        while True:
            r = next(spare)             # StopIteration: the pool is used up, the case is not viable
            x1, y1, _ = items(c, [r], None if starts is None else starts[pos:pos + 1], None if levels is None else levels[pos:pos + 1])
            if float(margin(c, x1, y1)) >= c.kink:
                rows[pos] = r
                break
    return rows.to(torch.int32)


def sentinel_positions(B):
    return sorted({p for p in (0, 31, 32, (B - 1) // R * R, B - 1) if 0 <= p < B})


def step_reference(c, rows, starts=None, levels=None):
    """Everything a step of the case is compared with: float64 gradient and loss, the yardstick's, e32 (whole, blocks), the loss's
    e32, the margins of the batch rows, and per sentinel position how far removing that row's term moves the float64 gradient."""
    if starts is None and c.horizon:
        starts = c.standin_starts[:c.B]
    if levels is None and c.level:
        levels = c.standin_levels[:c.B]
    O, B = c.dims[1], len(rows)
    norm = loss_norm(c.loss, B, O)
    x64, y64, a64 = items(c, rows, starts, levels, torch.float64)
    x32, y32, a32 = items(c, rows, starts, levels, torch.float32)
    g64, l64 = grad_whole(c.m64, c.loss, x64, y64, a64, c.delta, norm)
    auto, yl = grad_tiles(c.m32, c.loss, x32, y32, a32, c.delta, norm)
    _, wl = grad_whole(c.m32, c.loss, x32, y32, a32, c.delta, norm)
    yard, cl = grad_chains(c, x32.numpy(), y32.numpy(), a32.numpy() if torch.is_tensor(a32) else a32, norm)
    g64 = g64.numpy()
    out = SimpleNamespace(g64=g64, l64=float(l64), yard=yard, auto=auto.numpy(), e32=e32_blocks(yard, g64, c.dims),
                          e32_auto=e32_blocks(auto.numpy(), g64, c.dims),
                          loss_e32=scalar_e32([yl, wl, cl], float(l64)), margins=margin(c, x64, y64), norm=norm,
                          mean64=float(ref_loss(c.loss, c.m64(x64), y64, a64, c.delta).detach()), x64=x64, y64=y64, a64=a64)
    out.sentinels = {}
    for p in sentinel_positions(B):
        gp, _ = grad_whole(c.m64, c.loss, x64[p:p + 1], y64[p:p + 1], a64[p:p + 1] if torch.is_tensor(a64) else a64, c.delta, norm)
        out.sentinels[p] = float(gp.abs().max())        # g64 without the row is g64 - gp, at the unchanged norm
    return out


# ------------------------------------------------------------------------------------------------ the exact family
# (id, loss, activation, rows, I, O, U, L).  alpha 0.75, delta 0.5, integer inputs in [-3, 3], ternary weights, zero biases, targets
# fw64 + r with r from EXACT_R; the norm (rows x O, or rows for vector) is a power of two.
EXACT_ALPHA, EXACT_DELTA = 0.75, 0.5
EXACT_R = (-4.0, -2.0, -1.0, -0.5, 0.0, 0.0, 0.25, 0.5, 1.0, 2.0)
EXACT_CASES = [("scalar-relu-64", "scalar", "relu", 64, 5, 2, 16, 2), ("vector-relu-2048", "vector", "relu", 2048, 5, 2, 16, 2),
               ("scalar-relu-32", "scalar", "relu", 32, 7, 4, 32, 1), ("error-relu-64", "error", "relu", 64, 3, 1, 16, 3),
               ("scalar-elu-64", "scalar", "elu", 64, 3, 1, 16, 1)]
EXACT_IDS = [c[0] for c in EXACT_CASES]
TIES = dict(relu0=0.0, elu0=1.0, pin0=0.0)          # torch's: ReLU'(0), ELU'(0), the pinball's dl/dfw at r = 0


@functools.lru_cache(maxsize=None)
def exact_case(name):
    _, loss, act, B, I, O, U, L = EXACT_CASES[EXACT_IDS.index(name)]
    g = torch.Generator().manual_seed(_seed_of("exact" + name))
    dims = (I, O, U, L)
    elu = act == "elu"
    x = torch.randint(0 if elu else -3, 4, (B, I), generator=g).float()
    sd = OrderedDict()
    for i, (k, s) in enumerate(param_shapes(*dims)):
        if k.endswith("bias"):
            sd[k] = torch.zeros(s)
        elif elu and i == 0:
            sd[k] = (torch.rand(s, generator=g) < 0.4).float()                              # non-negative first layer: pre-activations >= 0
        else:
            u = torch.rand(s, generator=g)
            sd[k] = (u < 0.25).float() - (u > 0.75).float()
    m64, m32 = model(sd, dims, act, 1.0, torch.float64), model(sd, dims, act, 1.0, torch.float32)
    with torch.no_grad():
        fw = m64(x.double())
    r = torch.tensor(EXACT_R, dtype=torch.float64)[torch.randint(0, len(EXACT_R), (B, O), generator=g)]
    y = (fw + r).float()
    return SimpleNamespace(name=name, loss=loss, act=act, B=B, dims=dims, sd=sd, x=x, y=y, m64=m64, m32=m32, alpha=EXACT_ALPHA,
                           delta=EXACT_DELTA, beta=1.0, norm=loss_norm(loss, B, O))


def manual_grad(c, x, y, ties=TIES, per_row=False):
    """The step's gradient and loss terms by hand in numpy float64, every tie rule explicit: ties["relu0"] = ReLU'(0),
    ties["elu0"] = ELU'(0), ties["pin0"] = the pinball's dl/dfw at r = 0.  Returns (gradient [P] or per-row gradients [B, P], the
    loss summands / norm, the pre-activations, r or None, the Huber argument l or None)."""
    I, O, U, L = c.dims
    W = [c.sd[f"layers.{2 * i}.weight"].double().numpy() for i in range(L + 1)]
    b = [c.sd[f"layers.{2 * i}.bias"].double().numpy() for i in range(L + 1)]
    a, z = [np.asarray(x, dtype=np.float64)], []
    for i in range(L):
        zi = a[-1] @ W[i].T + b[i]
        z.append(zi)
        a.append(np.maximum(zi, 0.0) if c.act == "relu" else np.where(zi > 0, zi, np.expm1(np.minimum(zi, 0.0))))
    fw = a[-1] @ W[L].T + b[L]
    y = np.asarray(y, dtype=np.float64)
    k, r, l = kernel_loss(c.loss), None, None
    if k == "error":
        d, t = 2.0 * (fw - y) / c.norm, (fw - y) ** 2 / c.norm
    else:
        r = y - fw
        l = np.where(r > 0, c.alpha * r, (1 - c.alpha) * np.abs(r))
        dl = np.where(r > 0, -c.alpha, np.where(r < 0, 1 - c.alpha, ties["pin0"]))
        if k == "vector":
            l = l.sum(axis=1, keepdims=True)
        al = np.abs(l)
        t = np.where(al < c.delta, 0.5 * l * l, c.delta * (al - 0.5 * c.delta)) / c.norm        # |l| = delta: the linear branch
        d = np.clip(l, -c.delta, c.delta) * dl / c.norm
    parts = []
    for i in range(L, -1, -1):
        parts = [np.einsum("rj,rk->rjk", d, a[i]).reshape(d.shape[0], -1), d] + parts
        if i:
            zi = z[i - 1]
            if c.act == "relu":
                dact = np.where(zi > 0, 1.0, np.where(zi == 0, ties["relu0"], 0.0))
            else:
                dact = np.where(zi > 0, 1.0, np.where(zi == 0, ties["elu0"], np.exp(np.minimum(zi, 0.0))))
            d = (d @ W[i]) * dact
    rows = np.concatenate(parts, axis=1)
    return (rows if per_row else rows.sum(axis=0)), t, z, r, l


def pow2_divisor(v):
    """The largest power of two dividing every nonzero element of the float64 array v (1.0 for an all-zero array)."""
    v = np.abs(np.asarray(v, dtype=np.float64).reshape(-1))
    v = v[v != 0]
    if v.size == 0:
        return 1.0
    mant, ex = np.frexp(v)
    mi = (mant * 2.0 ** 53).astype(np.int64)
    low = ex - 53 + np.round(np.log2((mi & -mi).astype(np.float64))).astype(np.int64)
    return 2.0 ** int(low.min())


def exact_reference(c, x=None, y=None):
    x, y = (c.x if x is None else x), (c.y if y is None else y)
    g64, l64 = grad_whole(c.m64, c.loss, x.double(), y.double(), c.alpha, c.delta, c.norm)
    return g64.numpy(), float(l64)


# ------------------------------------------------------------------------------------------------ Adam
def lr_of_step(lr0, gamma, step_size, t):
    """The rate that sizes Adam step t (StepLR stepped after every batch: t - 1 scheduler steps lie before it)."""
    return lr0 * gamma ** ((t - 1) // step_size)


def lr_logged(lr0, gamma, step_size, t):
    """get_last_lr() after the scheduler step that follows Adam step t: what the log holds."""
    return lr0 * gamma ** (t // step_size)


def adam64(p, m, v, g, t, lr):
    """torch.optim.Adam (defaults) in numpy float64; t: the step count after this step."""
    p, m, v, g = (np.asarray(a, dtype=np.float64) for a in (p, m, v, g))
    m = 0.9 * m + 0.1 * g
    v = 0.999 * v + 0.001 * g * g
    p = p - lr / (1.0 - 0.9 ** t) * m / (np.sqrt(v) / math.sqrt(1.0 - 0.999 ** t) + 1e-8)
    return dict(params=p, m=m, v=v)


def adam32(p, m, v, g, t, lr):
    """The same step through torch.optim.Adam on float32 CPU tensors: the yardstick, in torch's own operation order."""
    f = lambda a: torch.from_numpy(np.array(a, dtype=np.float32))
    q = torch.nn.Parameter(f(p))
    opt = torch.optim.Adam([q], lr=lr, foreach=False)
    opt.state[q] = {"step": torch.tensor(float(t - 1)), "exp_avg": f(m), "exp_avg_sq": f(v)}
    q.grad = f(g)
    opt.step()
    st = opt.state[q]
    return dict(params=q.detach().numpy(), m=st["exp_avg"].numpy(), v=st["exp_avg_sq"].numpy())


def adam_mag(mag, before, ref, g):
    """Largest magnitude every element has held, per array (tests/ppo_opt_ref.py's grow_mag): for m also the 0.1 g it absorbed."""
    new = {a: np.maximum(np.abs(before[a]), np.abs(ref[a])) for a in ("params", "m", "v")}
    new["m"] = np.maximum(new["m"], 0.1 * np.abs(np.asarray(g, dtype=np.float64)))
    return new if mag is None else {a: np.maximum(mag[a], new[a]) for a in new}


def adam_e32(yard, ref, mag, dims, k=1):
    """{array: (whole e32, block e32)} after k steps, floored at c sqrt(k) 2^-24 mag (tests/ppo_opt_ref.py; for m at most 2.3)."""
    starts, _ = block_starts(dims)
    out = {}
    for a in ("params", "m", "v"):
        fl = U24 * FLOOR_ROUNDINGS[a] * (min(math.sqrt(k), 2.3) if a == "m" else math.sqrt(k))
        err = np.abs(np.asarray(yard[a], dtype=np.float64) - ref[a])
        out[a] = (max(float(err.max()), fl * float(mag[a].max())),
                  np.maximum(np.maximum.reduceat(err, starts), fl * np.maximum.reduceat(mag[a], starts)))
    return out


def adam_ratios(got, ref, e32, dims):
    """Worst |got - ref| / (MARGIN e32) per array: {array: whole, array + "/block": worst block}."""
    starts, _ = block_starts(dims)
    out = {}
    for a in ("params", "m", "v"):
        err = np.abs(np.asarray(got[a], dtype=np.float64) - ref[a])
        whole, blocks = e32[a]
        out[a] = ratio(float(err.max()), MARGIN * whole)
        out[a + "/block"] = max(ratio(float(e), MARGIN * float(b)) for e, b in zip(np.maximum.reduceat(err, starts), blocks))
    return out


def adam_one_step(before, g, t, lr, dims):
    """Reference, yardstick and e32 of one Adam step from `before` (params, m, v as fp32 arrays) on the fp32 gradient g."""
    ref = adam64(before["params"], before["m"], before["v"], g, t, lr)
    yard = adam32(before["params"], before["m"], before["v"], g, t, lr)
    b64 = {a: np.asarray(before[a], dtype=np.float64) for a in before}
    return ref, yard, adam_e32(yard, ref, adam_mag(None, b64, ref, g), dims, 1)


# One Adam step in isolation: (id, t, warmed moments, tiny gradient).  5 -> 16 x 2 -> 2 relu, units 3 and 11 of the first layer dead
# (zero weights, bias -1): their rows of W1, their biases and their columns of W2 see g = 0 and, with m = v = 0, must come back unchanged.
ADAM_DIMS, ADAM_ROWS, ADAM_LR, ADAM_DEAD = (5, 2, 16, 2), 33, 2.0 ** -10, (3, 11)
ADAM_CASES = [("t1-fresh", 1, False, False), ("t2-warm", 2, True, False), ("t1000-warm", 1000, True, False),
              ("t1000000-warm", 10 ** 6, True, False), ("t1000-fresh", 1000, False, False), ("t1-tiny", 1, False, True)]
ADAM_IDS = [c[0] for c in ADAM_CASES]


def adam_dead_mask():
    I, O, U, L = ADAM_DIMS
    mask = np.zeros(block_starts(ADAM_DIMS)[1], dtype=bool)
    w1 = np.zeros((U, I), dtype=bool); w1[list(ADAM_DEAD)] = True
    b1 = np.zeros(U, dtype=bool); b1[list(ADAM_DEAD)] = True
    w2 = np.zeros((U, U), dtype=bool); w2[:, list(ADAM_DEAD)] = True
    mask[:U * I], mask[U * I:U * I + U], mask[U * I + U:U * I + U + U * U] = w1.reshape(-1), b1, w2.reshape(-1)
    return mask


@functools.lru_cache(maxsize=None)
def adam_case(name):
    """Parameters, data and starting moments of a one-step case: `error` loss, relu.  tiny: targets = the model's float64 output +
    1e-9 noise (rounded to fp32), so that sqrt(v-hat) lies below eps for most elements and eps decides the step."""
    _, t, warm, tiny = ADAM_CASES[ADAM_IDS.index(name)]
    g = torch.Generator().manual_seed(_seed_of("adam" + name))
    sd = default_params(ADAM_DIMS, 7)
    sd["layers.0.weight"][list(ADAM_DEAD)] = 0.0
    sd["layers.0.bias"][list(ADAM_DEAD)] = -1.0
    x = torch.randn(ADAM_ROWS, ADAM_DIMS[0], generator=g)
    m64 = model(sd, ADAM_DIMS, "relu", 1.0, torch.float64)
    with torch.no_grad():
        fw = m64(x.double())
    y = (fw + 1e-9 * torch.randn(fw.shape, generator=g, dtype=torch.float64)).float() if tiny else torch.rand(ADAM_ROWS, ADAM_DIMS[1], generator=g)
    P, dead = block_starts(ADAM_DIMS)[1], adam_dead_mask()
    m0, v0 = np.zeros(P, dtype=np.float32), np.zeros(P, dtype=np.float32)
    if warm:
        m0 = (3e-4 * torch.randn(P, generator=g)).numpy()
        v0 = (1e-6 * (0.5 + torch.rand(P, generator=g))).numpy()
        m0[dead], v0[dead] = 0.0, 0.0
    g64, _ = grad_whole(m64, "error", x.double(), y.double(), None, 1.0, ADAM_ROWS * ADAM_DIMS[1])
    return SimpleNamespace(name=name, t=t, warm=warm, tiny=tiny, sd=sd, x=x, y=y, m0=m0, v0=v0, dead=dead, g64=g64.numpy(),
                           p0=flat(sd).numpy(), dims=ADAM_DIMS, lr=ADAM_LR)


# StepLR: step_size 3, gamma 0.5, steps 1..10 from fresh moments at lr0 = 2^-10, on the one-step model and data
STEPLR = dict(step_size=3, gamma=0.5, lr0=2.0 ** -10, steps=10)

# Trajectories of 20 steps: (id, loss, activation, I, O, U, L, counts cycled, lr).  The pinball one keeps batch <= 65 and O = 1.
TRAJ_STEPS = 20
TRAJ_CASES = [("error-tanh", "error", "tanh", 12, 3, 32, 2, (2048, 33, 1, 64, 2047), 1e-3),
              ("scalar-softplus", "scalar", "softplus", 12, 1, 32, 2, (65, 33, 1, 64, 31), 1e-3)]
TRAJ_IDS = [c[0] for c in TRAJ_CASES]


@functools.lru_cache(maxsize=None)
def trajectory(name):
    """The float64 trajectory (float64 gradients + adam64) and the yardstick's own fp32 trajectory (tile-ordered gradients + fp32
    Adam) from the same start on the same rows: per step the rows, ref and yard states after it and e32 with the sqrt(k) floors;
    plus min_r (the float64 trajectory's smallest |w - fw| over all batches, inf for `error`) and out_diff (the largest output
    difference between the two trajectories on the batches).  Computed once; read-only."""
    _, loss, act, I, O, U, L, counts, lr = TRAJ_CASES[TRAJ_IDS.index(name)]
    dims, beta = (I, O, U, L), 5.0 if act == "softplus" else 1.0
    g = torch.Generator().manual_seed(_seed_of("traj" + name))
    x, y = torch.randn(POOL, I, generator=g), (torch.rand(POOL, O, generator=g) - 0.4) * 2.0
    sd = default_params(dims, 11)
    P = block_starts(dims)[1]
    ref = dict(params=flat(sd).double().numpy(), m=np.zeros(P), v=np.zeros(P))
    yard = dict(params=flat(sd).numpy(), m=np.zeros(P, dtype=np.float32), v=np.zeros(P, dtype=np.float32))
    steps, mag, min_r, out_diff = [], None, float("inf"), 0.0
    for s in range(TRAJ_STEPS):
        B = counts[s % len(counts)]
        rows = torch.randperm(POOL, generator=g)[:B]
        norm = loss_norm(loss, B, O)
        m64, m32 = model(unflat(ref["params"], dims), dims, act, beta, torch.float64), model(unflat(yard["params"], dims), dims, act, beta, torch.float32)
        with torch.no_grad():
            f64, f32 = m64(x[rows].double()), m32(x[rows])
        out_diff = max(out_diff, float((f32.double() - f64).abs().max()))
        if loss != "error":
            min_r = min(min_r, float((y[rows].double() - f64).abs().min()))
        g64, _ = grad_whole(m64, loss, x[rows].double(), y[rows].double(), ALPHA, DELTA, norm)
        g32, _ = grad_tiles(m32, loss, x[rows], y[rows], ALPHA, DELTA, norm)
        before = ref
        ref = adam64(ref["params"], ref["m"], ref["v"], g64.numpy(), s + 1, lr)
        yard = adam32(yard["params"], yard["m"], yard["v"], g32.numpy(), s + 1, lr)
        mag = adam_mag(mag, before, ref, g64.numpy())
        steps.append(dict(rows=rows.to(torch.int32), ref=ref, yard=yard, e32=adam_e32(yard, ref, mag, dims, s + 1)))
    return SimpleNamespace(name=name, loss=loss, act=act, beta=beta, dims=dims, sd=sd, x=x, y=y, lr=lr, steps=steps, min_r=min_r,
                           out_diff=out_diff)


# ------------------------------------------------------------------------------------------------ eval metrics
# (id, loss, activation, test rows, I, O, U, L, fixed level or None).  8225 rows are 258 tiles: threads 0 and 1 of k_tube_eval_finish
# take a second trip through its strided loop.
EVAL_CASES = [("n1", "scalar", "tanh", 1, 9, 5, 48, 3, None), ("n31", "vector", "relu", 31, 9, 5, 48, 3, None),
              ("n33", "scalar", "elu", 33, 9, 5, 48, 3, None), ("n8225", "scalar", "relu", 8225, 3, 1, 16, 1, None),
              ("level-n65", "scalar_level", "softplus", 65, 6, 2, 32, 2, 0.8125)]
EVAL_IDS = [c[0] for c in EVAL_CASES]
EVAL_POOL = 9216


@functools.lru_cache(maxsize=None)
def eval_case(name):
    """A test split of n rows from a kink-filtered pool and everything its metrics are compared with: loss (float64, e32 as in a
    step), count64 = the float64 count of fw > w, and mean |w - fw| over those with its e32."""
    _, loss, act, n, I, O, U, L, level = EVAL_CASES[EVAL_IDS.index(name)]
    dims, beta = (I, O, U, L), 5.0 if act == "softplus" else 1.0
    g = torch.Generator().manual_seed(_seed_of("eval" + name))
    c = SimpleNamespace(name=name, loss=loss, act=act, beta=beta, dims=dims, level=level is not None, horizon=None, alpha=ALPHA, delta=DELTA)
    x, y = torch.randn(EVAL_POOL, I - int(c.level), generator=g), (torch.rand(EVAL_POOL, O, generator=g) - 0.4) * 0.5
    c.sd = default_params(dims, 13)
    c.m64, c.m32 = model(c.sd, dims, act, beta, torch.float64), model(c.sd, dims, act, beta, torch.float32)
    c.x, c.y = x, y
    lv = torch.full((EVAL_POOL,), level) if c.level else None
    x64, y64, a64 = items(c, torch.arange(EVAL_POOL), None, lv, torch.float64)
    x32, y32, a32 = items(c, torch.arange(EVAL_POOL), None, lv, torch.float32)
    c.kink = KINK_FACTOR * float((kink_quantities(c, c.m32, x32, y32).double() - kink_quantities(c, c.m64, x64, y64)).abs().max())
    keep = (margin(c, x64, y64) >= c.kink).nonzero().reshape(-1)
    c.pool_survivors, c.n, c.fixed_level = int(keep.numel()), n, level
    keep = keep[:n]
    c.tx, c.ty = x[keep].contiguous(), y[keep].contiguous()
    x64, y64, x32, y32 = x64[keep], y64[keep], x32[keep], y32[keep]
    a64, a32 = (a64[keep], a32[keep]) if c.level else (a64, a32)
    norm = loss_norm(loss, n, O)
    with torch.no_grad():
        f64, f32 = c.m64(x64), c.m32(x32)
        c.l64 = float(terms(loss, f64, y64, a64, DELTA).sum() / norm)
        nrm, ls = torch.tensor(float(norm), dtype=torch.float32), torch.zeros((), dtype=torch.float32)
        for b in range(0, n, R):
            ls = ls + terms(loss, f32[b:b + R], y32[b:b + R], a32[b:b + R] if c.level else a32, DELTA).sum()
        c.loss_e32 = scalar_e32([ls / nrm, terms(loss, f32, y32, a32, DELTA).sum() / nrm], c.l64)
        c.mean64 = float(ref_loss(loss, f64, y64, a64, DELTA))
        sel = f64 > y64
        c.count64, c.elems = int(sel.sum()), n * O
        c.same_side = bool(((f32 > y32) == sel).all())
        c.err64 = float((y64[sel] - f64[sel]).abs().mean()) if c.count64 else float("nan")
        if c.count64:
            e32 = (y32 - f32).abs() * (f32 > y32)
            tl = torch.zeros((), dtype=torch.float32)
            for b in range(0, n, R):
                tl = tl + e32[b:b + R].sum()
            cnt = torch.tensor(float(c.count64), dtype=torch.float32)
            c.err_e32 = scalar_e32([tl / cnt, (y32[f32 > y32] - f32[f32 > y32]).abs().mean()], c.err64)
    return c


# the permutation sizes of section 3
PERM_SIZES = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)


# ------------------------------------------------------------------------------------------------ the kernel's order, in numpy float32
def _fma(a, b, c):
    """fmaf on float32 arrays: the product of two floats is exact in float64, the sum is rounded there and once more to float32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _act32(act, z, beta):
    f = np.float32
    if act == "relu":
        return np.maximum(z, f(0))
    if act == "softplus":
        zb = z * f(beta)
        with np.errstate(over="ignore"):
            return np.where(zb > f(20), z, np.log1p(np.exp(np.minimum(zb, f(30)))) / f(beta)).astype(f)
    if act == "tanh":
        return np.tanh(z)
    return np.where(z > 0, z, np.expm1(np.minimum(z, f(0)))).astype(f)


def _act_grad32(act, h, beta):
    """The derivative from the activation's OUTPUT, as tube_act_grad forms it."""
    f = np.float32
    if act == "relu":
        return (h > 0).astype(f)
    if act == "softplus":
        hb = h * f(beta)
        return np.where(hb > f(20), f(1), -np.expm1(-hb)).astype(f)
    if act == "tanh":
        return f(1) - h * h
    return np.where(h > 0, f(1), h + f(1)).astype(f)


def grad_chains(c, x, y, a, norm):
    """The step in float32 in k_tube_rows' own order of sums: every dot product one fmaf chain from 0 over k (forward) or j (input
    gradient) ascending, a row's loss summed over its outputs in sequence, a weight gradient one fmaf chain over the rows of its
    tile in sequence (the bias gradient a chain of adds), tiles and tile loss sums added in tile order.  x (B, I), y (B, O)
    float32 arrays; a: alpha or the levels (B, 1).  Returns (gradient [P], loss) as float32."""
    f = np.float32
    I, O, U, L = c.dims
    W = [c.sd[f"layers.{2 * i}.weight"].numpy().astype(f) for i in range(L + 1)]
    b = [c.sd[f"layers.{2 * i}.bias"].numpy().astype(f) for i in range(L + 1)]
    x, y = np.asarray(x, dtype=f), np.asarray(y, dtype=f)
    B = x.shape[0]
    alpha = np.asarray(a, dtype=f).reshape(-1, 1) if np.ndim(a) else f(a if a is not None else 0.0)
    nrm, delta = f(norm), f(c.delta)
    acts = [x]
    for i in range(L + 1):
        acc = np.zeros((B, W[i].shape[0]), dtype=f)
        for k in range(W[i].shape[1]):
            acc = _fma(acts[-1][:, k:k + 1], W[i][:, k][None, :], acc)
        z = acc + b[i]
        acts.append(z if i == L else _act32(c.act, z, c.beta))
    fw = acts.pop()
    kind = kernel_loss(c.loss)
    rowloss = np.zeros(B, dtype=f)
    if kind == "error":
        d = fw - y
        for j in range(O):
            rowloss = rowloss + d[:, j] * d[:, j]
        d = f(2) * d / nrm
    else:
        r = y - fw
        l = np.where(r > 0, alpha * r, (f(1) - alpha) * np.abs(r)).astype(f)
        dl = np.where(r > 0, -alpha, np.where(r < 0, f(1) - alpha, f(0))).astype(f)
        hub = lambda v: np.where(np.abs(v) < delta, f(0.5) * np.abs(v) * np.abs(v), delta * (np.abs(v) - f(0.5) * delta)).astype(f)
        if kind == "vector":
            lsum = np.zeros(B, dtype=f)
            for j in range(O):
                lsum = lsum + l[:, j]
            rowloss = hub(lsum)
            d = np.clip(lsum, -delta, delta)[:, None] * dl / nrm
        else:
            for j in range(O):
                rowloss = rowloss + hub(l[:, j])
            d = np.clip(l, -delta, delta) * dl / nrm
    tiles = -(-B // R)
    pad = lambda v: np.concatenate([v, np.zeros((tiles * R - B,) + v.shape[1:], dtype=f)]).reshape((tiles, R) + v.shape[1:])
    ls = f(0)
    for tl in pad(rowloss):
        s = f(0)
        for v in tl:
            s = f(s + v)
        ls = f(ls + s)
    parts = []
    d = d.astype(f)
    for i in range(L, -1, -1):
        dt, at = pad(d), pad(acts[i])
        gw, gb = np.zeros((tiles, W[i].shape[0], W[i].shape[1]), dtype=f), np.zeros((tiles, W[i].shape[0]), dtype=f)
        for r_ in range(R):
            gw = _fma(dt[:, r_, :, None], at[:, r_, None, :], gw)
            gb = gb + dt[:, r_, :]
        sw, sb = np.zeros_like(gw[0]), np.zeros_like(gb[0])
        for t_ in range(tiles):
            sw, sb = sw + gw[t_], sb + gb[t_]
        parts = [sw.reshape(-1), sb] + parts
        if i:
            acc = np.zeros((B, W[i].shape[1]), dtype=f)
            for j in range(W[i].shape[0]):
                acc = _fma(d[:, j:j + 1], W[i][j][None, :], acc)
            d = (acc * _act_grad32(c.act, acts[i], c.beta)).astype(f)
    return np.concatenate(parts).astype(f), f(ls / nrm)
