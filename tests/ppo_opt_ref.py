"""Float64 reference, fp32 yardstick and case lists for the optimiser step between two PPO minibatches (k_opt_prepare, k_det_fold,
k_opt_adam, k_sync_planes / write_planes of csrc/ppo_kernels.hip, launched by lg_ppo_minibatch_step and lg_ppo_begin_update).
Nothing here comes from the library: numpy float64 for the reference, torch.optim.Adam + clip_grad_norm_ on the CPU for the yardstick.
tests/test_ppo_opt_host.py checks the conditions of the cases on the CPU; tests/test_hip_ppo_opt.py runs them on the GPU.

One step, state = (params, m, v, t, lr), inputs = the SUMS over the ranks of the gradient and of the minibatch's KL:
    g = grad_sum / world;  kl = kl_sum / world / mb_rows
    adaptive schedule (rsl_rl PPO.update):  kl > 2 desired: lr = max(1e-5, lr / 1.5);  0 < kl < desired / 2: lr = min(1e-2, lr * 1.5)
    g *= min(max_grad_norm / (|g| + 1e-6), 1)                                     (clip_grad_norm_)
    t += 1;  m = 0.9 m + 0.1 g;  v = 0.999 v + 0.001 g^2
    params -= lr / (1 - 0.9^t) * m / (sqrt(v) / sqrt(1 - 0.999^t) + 1e-8)         (torch.optim.Adam)

Bounds.  Per array (params, m, v), over the whole vector and again over every block of the parameter layout, e32 = max |yardstick -
reference| on the same inputs, the yardstick running its own fp32 trajectory; the library must lie within 4 e32 (the margin
tests/test_hip_tube_eval.py uses for two valid fp32 evaluations of one arithmetic).  A maximum over a block of one element (the critic
head's bias) is one draw: the yardstick can land on the float64 value by luck.  So e32 is floored at what the roundings of any valid
fp32 evaluation add up to after k steps, as a root mean square, counted from the arithmetic (u = 2^-24 bounds one rounding, whose
standard deviation is u / sqrt(3); `mag` is the largest magnitude the element has held, for m also the 0.1 g it absorbed, since
0.9 m + 0.1 g cancels and rounds at the size of its operands):
  g = grad inv_world coef carries the clip coefficient's roundings (sum of squares, square root, + 1e-6, division) and two products;
  v = 0.999f v + 0.001f g g sees those twice, three roundings of its own and the representation of 0.001f (0.8 u): about eleven
      roundings and one fixed offset per step, 3 u mag;
  m = 0.9f m + 0.1f g sees them once and three of its own: seven roundings per step, 2 u mag;
  the parameter is stored once per step, u mag (the error of the step itself is a few u of lr, far below).
The errors carry over with factor 0.999 (v), 0.9 (m) and 1 (parameters): after k steps sqrt(k) times the above, for m no more than
1 / sqrt(1 - 0.81) = 2.3 times.  Floor: c sqrt(k) 2^-24 max mag over the same elements, c = 1 (parameters), 2 (m), 3 (v).
The bias corrections.  torch.optim.Adam forms 1 - 0.9^t and 1 - 0.999^t in double; k_opt_adam forms 1 - powf(0.9f, t) and
1 - powf(0.999f, t).  0.999f is 1.3e-8 above 0.999, powf is good to one ulp, and 1 - 0.999^t is about 1e-3 t while t << 1000: the
difference cancels, and what is one rounding of 0.999^t is (1.3e-8 t + 2^-23) / (1e-3 t) of the correction -- not a rounding of the
result, so e32 does not stand for it, and it has one sign over many steps.  The project holds a step to 1e-4 of itself
(tests/test_hip_ppo.py); the corrections stay inside that (bc_allowance: 6.7e-5 of a step at t = 1, 3.7e-5 at t = 2, 3.8e-6 at
t = 1000, nothing later), so the kernel keeps its arithmetic, and the parameters are asked to lie within 4 e32 of the float64 step
GIVEN that allowance: err - sum over the steps of bc_allowance(t) |step_t|, per element, against 4 e32.  The ratio against 4 e32 alone is
printed beside it ("raw") and recorded in DESIGN.md; m and v do not see the corrections and have no allowance.
lr: the library keeps it in fp32 and
every change is one rounding -- the trajectories change it at most four times before a clamp resets it, with the rounding of the
starting value five roundings of 2^-24: 3e-7 relative.  KL: one fp32 division, 2^-23 relative.
"""
import functools

import numpy as np
import torch

from tests.gemm_ref import split_planes  # noqa: F401  (the split itself: re-exported for the tests)

U = 2.0 ** -24
DESIRED_KL, MAX_GRAD_NORM = 0.01, 1.0
LR_MIN, LR_MAX = 1e-5, 1e-2
LR_RTOL, KL_RTOL = 3e-7, 2.0 ** -23
MARGIN = 4.0
STEP_SHARE = 1e-4                   # the project's figure for an acceptable error of one step, as a share of lr (tests/test_hip_ppo.py)

# ------------------------------------------------------------------------------------------------ sizes
# tiny: the smallest net lg_ppo_create accepts (one hidden layer of one unit; 9 parameters: part of one block, 127 idle blocks in the
# prepare launch).  small: the net of test_optimiser_step_equals_torch_adam_with_clip_and_adaptive_lr.  large: more than 2 x 262 144
# parameters (second and third trip of k_opt_adam's loop) and 235-wide first-layer rows padded to 256.  priv: pad widths 65 -> 96 and
# 169 -> 192.  rnn: the LSTM weights have no plane image, the MLPs read the 32-wide hidden state.
SIZES = {
    "tiny": dict(N=4, T=2, nmb=1, O=1, OC=None, A=1, actor=[1], critic=[1], rnn=0),
    "small": dict(N=64, T=8, nmb=4, O=48, OC=None, A=12, actor=[64, 32], critic=[64, 32], rnn=0),
    "large": dict(N=64, T=8, nmb=4, O=235, OC=None, A=12, actor=[512, 256, 128], critic=[512, 256, 128], rnn=0),
    "priv": dict(N=64, T=8, nmb=4, O=65, OC=169, A=12, actor=[64, 64, 32], critic=[64, 64, 32], rnn=0),
    "rnn": dict(N=64, T=8, nmb=4, O=48, OC=None, A=12, actor=[64, 32], critic=[64, 32], rnn=32),
}
PLANE_SIZES = ("large", "priv", "rnn")


def mb_rows(size):
    s = SIZES[size]
    return s["N"] * s["T"] // s["nmb"]


@functools.lru_cache(maxsize=None)
def layout(size):
    """Restatement of lg_ppo_param_layout and of the plane map of lg_ppo_create: blocks = [(name, offset, rows, cols)] (cols 0: a
    vector) in ActorCritic.parameters() order, n = number of parameters, dest = int64 [n] element of each parameter inside a plane or
    -1, pl_stride = elements per plane.  One segment per weight matrix, actor layers then critic layers; rows of a first layer padded to
    a multiple of 32; segment lengths rounded up to 8; biases, std and LSTM weights have no image."""
    s = SIZES[size]
    H = s["rnn"]
    OC = s["OC"] or s["O"]
    blocks, off = [("std", 0, s["A"], 0)], s["A"]
    segs = []
    for net, hidden, i, o in (("actor", s["actor"], H or s["O"], s["A"]), ("critic", s["critic"], H or OC, 1)):
        dims = [i] + list(hidden) + [o]
        for l in range(len(dims) - 1):
            blocks.append((f"{net}.{2 * l}.weight", off, dims[l + 1], dims[l]))
            segs.append((off, dims[l + 1], dims[l], -(-dims[l] // 32) * 32 if l == 0 else dims[l]))
            off += dims[l + 1] * dims[l]
            blocks.append((f"{net}.{2 * l}.bias", off, dims[l + 1], 0))
            off += dims[l + 1]
    if H:
        for mem, width in (("memory_a", s["O"]), ("memory_c", OC)):
            for name, r, c in (("weight_ih_l0", 4 * H, width), ("weight_hh_l0", 4 * H, H), ("bias_ih_l0", 4 * H, 0), ("bias_hh_l0", 4 * H, 0)):
                blocks.append((f"{mem}.rnn.{name}", off, r, c))
                off += r * (c or 1)
    dest = np.full(off, -1, dtype=np.int64)
    po = 0
    for w_off, rows, cols, ld in segs:
        e = np.arange(rows * cols)
        dest[w_off + e] = po + (e // cols) * ld + e % cols
        po += -(-(rows * ld) // 8) * 8
    return dict(blocks=blocks, n=off, dest=dest, pl_stride=po, segs=segs)


def block_starts(size):
    return np.array([b[1] for b in layout(size)["blocks"]], dtype=np.int64)


# ------------------------------------------------------------------------------------------------ trajectories
# (gradient family, pre-clip norm of grad_sum / world, mean KL of the minibatch, the regime the step is in).  Regimes: "clip" / "free"
# for the norm against max_grad_norm = 1; "down" (KL > 2 desired), "up" (0 < KL < desired / 2), "band", "zero" (KL = 0) for the rule,
# followed by "@min" / "@max" where the clamp decides the new lr.  Every KL is 10 % or more away from 0.02 and 0.005, every norm 1 % or
# more away from 1.  A begin_update falls after step BEGIN_AFTER (odd: the norm slot's parity continues across it).
BEGIN_AFTER = 5
_R, _S, _Z = "randn", "spread", "zero"
TRAJECTORIES = {
    # every regime in turn, both families, the all-zero gradient
    "mixed": dict(adaptive=True, lr0=1e-3, steps=[
        (_R, 5.0, 0.010, "clip band"), (_R, 0.01, 0.010, "free band"), (_R, 0.3, 0.001, "free up"), (_R, 0.3, 0.050, "free down"),
        (_S, 2.0, 0.004, "clip up"), (_R, 0.02, 0.030, "free down"), (_Z, 0.0, 0.0, "free zero"), (_R, 2.0, 0.0, "clip zero"),
        (_S, 0.5, 0.012, "free band"), (_R, 1.5, 0.0225, "clip down"), (_R, 0.9, 0.0044, "free up"), (_R, 1.05, 0.0175, "clip band"),
        (_R, 0.98, 0.0056, "free band")]),
    # 2e-3 x 1.5^4 = 1.0125e-2: the fourth raise meets the clamp, four more are held by it
    "raise": dict(adaptive=True, lr0=2e-3, steps=[
        (_R, 0.5, 0.001, "free up"), (_R, 3.0, 0.002, "clip up"), (_R, 0.5, 0.001, "free up"), (_R, 3.0, 0.004, "clip up@max"),
        (_R, 0.5, 0.001, "free up@max"), (_R, 3.0, 0.002, "clip up@max"), (_R, 0.5, 0.003, "free up@max"), (_R, 0.5, 0.001, "free up@max"),
        (_R, 3.0, 0.010, "clip band"), (_R, 0.5, 0.0, "free zero"), (_R, 3.0, 0.015, "clip band"), (_R, 0.5, 0.007, "free band")]),
    # 5e-5 / 1.5^4 = 9.9e-6: the fourth cut meets the clamp, four more are held by it
    "lower": dict(adaptive=True, lr0=5e-5, steps=[
        (_R, 0.5, 0.050, "free down"), (_R, 3.0, 0.030, "clip down"), (_R, 0.5, 0.100, "free down"), (_R, 3.0, 0.025, "clip down@min"),
        (_R, 0.5, 0.050, "free down@min"), (_R, 3.0, 0.030, "clip down@min"), (_R, 0.5, 1.000, "free down@min"), (_R, 0.5, 0.050, "free down@min"),
        (_R, 3.0, 0.0, "clip zero"), (_R, 0.5, 0.0, "free zero"), (_R, 3.0, 0.010, "clip band"), (_R, 0.5, 0.0, "free zero")]),
    # schedule = "fixed": the same KLs leave lr alone
    "fixed": dict(adaptive=False, lr0=1e-3, steps=[
        (_R, 0.5, 0.050, "free down"), (_R, 3.0, 0.001, "clip up"), (_R, 0.5, 0.0, "free zero"), (_R, 3.0, 0.010, "clip band"),
        (_R, 0.5, 0.100, "free down"), (_R, 3.0, 0.002, "clip up"), (_S, 0.5, 0.030, "free down"), (_R, 0.5, 0.004, "free up"),
        (_R, 3.0, 0.050, "clip down"), (_R, 0.5, 0.001, "free up"), (_R, 3.0, 0.0, "clip zero"), (_R, 0.5, 0.025, "free down")]),
    # sign x 10^U(-12, 0) on every step: eps decides the step on part of the vector; one entry in twenty is never touched
    "spread": dict(adaptive=True, lr0=1e-3, steps=[
        (_S, 0.5, 0.010, "free band"), (_S, 3.0, 0.001, "clip up"), (_S, 0.5, 0.010, "free band"), (_S, 3.0, 0.050, "clip down"),
        (_S, 0.5, 0.010, "free band"), (_S, 3.0, 0.010, "clip band"), (_Z, 0.0, 0.010, "free band"), (_S, 0.5, 0.0, "free zero"),
        (_S, 3.0, 0.010, "clip band"), (_S, 0.5, 0.003, "free up"), (_S, 3.0, 0.010, "clip band"), (_S, 0.5, 0.030, "free down")]),
}
ZERO_EVERY = 20                      # spread: entries k with k % 20 == 7 are exactly zero on every step


def zero_mask(n):
    return np.arange(n) % ZERO_EVERY == 7


def _seed(*key):
    return np.random.default_rng([sum(ord(c) * (i + 1) for i, c in enumerate(str(k))) for k in key])


def gradient(size, traj, step, family, norm, world=1):
    """grad_sum of one step: fp32 [n], built in float64 so that grad_sum / world has the pre-clip norm asked for, rounded once."""
    n = layout(size)["n"]
    g = _seed(size, traj, step, family, world)
    if family == _Z:
        return np.zeros(n, dtype=np.float32)
    if family == _R:
        x = g.standard_normal(n)
    else:
        x = np.where(g.random(n) < 0.5, -1.0, 1.0) * 10.0 ** g.uniform(-12.0, 0.0, n)
        x[zero_mask(n)] = 0.0
    if world > 1:                                   # the sum of `world` ranks' gradients around a common mean
        x = sum(x + 0.3 * g.standard_normal(n) * np.abs(x) for _ in range(world))
    x *= norm * world / np.sqrt((x * x).sum())
    return x.astype(np.float32)


def kl_sum(size, kl, world=1):
    """The KL tail of the gradient buffer: fp32(kl x mb_rows x world).  The mean KL of the case is DEFINED as this value / (mb_rows
    world), so the product is exactly representable and both precisions divide the same number."""
    return np.float32(kl * mb_rows(size) * world)


def initial_state(size, lr0):
    """params: std = 1, everything else 0.1 x N(0, 1), rounded to fp32 once; zero moments; t = 0; lr = fp32(lr0)."""
    n, A = layout(size)["n"], SIZES[size]["A"]
    p = (0.1 * _seed(size, "params").standard_normal(n)).astype(np.float32)
    p[:A] = 1.0
    return dict(params=p.astype(np.float64), m=np.zeros(n), v=np.zeros(n), t=0, lr=float(np.float32(lr0)))


# ------------------------------------------------------------------------------------------------ one step
def lr_rule(lr, kl, adaptive):
    if adaptive:
        if kl > DESIRED_KL * 2.0:
            return max(LR_MIN, lr / 1.5)
        if DESIRED_KL / 2.0 > kl > 0.0:
            return min(LR_MAX, lr * 1.5)
    return lr


def step(state, grad_sum, kl_sum_, cfg):
    """The float64 reference.  cfg = dict(world, mb_rows, adaptive); grad_sum fp32 or float64 [n]; returns the new state, with the
    step's KL, pre-clip norm and clip coefficient beside it."""
    g = np.asarray(grad_sum, dtype=np.float64) / cfg["world"]
    kl = float(kl_sum_) / cfg["world"] / cfg["mb_rows"]
    lr = lr_rule(state["lr"], kl, cfg["adaptive"])
    norm = float(np.sqrt((g * g).sum()))
    coef = min(MAX_GRAD_NORM / (norm + 1e-6), 1.0)
    g = g * coef
    t = state["t"] + 1
    m = 0.9 * state["m"] + 0.1 * g
    v = 0.999 * state["v"] + 0.001 * g * g
    p = state["params"] - lr / (1.0 - 0.9 ** t) * m / (np.sqrt(v) / np.sqrt(1.0 - 0.999 ** t) + 1e-8)
    return dict(params=p, m=m, v=v, t=t, lr=lr, kl=kl, norm=norm, coef=coef)


def _tt(x, dtype):
    return torch.from_numpy(np.array(x)).to(dtype)


def torch_step(state, grad_sum, kl_sum_, cfg, dtype):
    """The same step through torch.optim.Adam + clip_grad_norm_ on the CPU in `dtype`, the lr rule applied by hand on a Python float:
    float32 is the yardstick (state arrays in, fp32 arrays out), float64 the cross-check of step()."""
    p = torch.nn.Parameter(_tt(state["params"], dtype))
    kl = float(kl_sum_) / cfg["world"] / cfg["mb_rows"]
    lr = lr_rule(state["lr"], kl, cfg["adaptive"])
    opt = torch.optim.Adam([p], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    opt.state[p] = {"step": torch.tensor(float(state["t"])), "exp_avg": _tt(state["m"], dtype),
                    "exp_avg_sq": _tt(state["v"], dtype)}
    p.grad = _tt(grad_sum, dtype) / cfg["world"]
    norm = torch.nn.utils.clip_grad_norm_([p], MAX_GRAD_NORM)
    opt.step()
    st = opt.state[p]
    return dict(params=p.detach().numpy(), m=st["exp_avg"].numpy(), v=st["exp_avg_sq"].numpy(), t=state["t"] + 1, lr=lr, kl=kl,
                norm=float(norm))


def emulate32(state, grad_sum, kl_sum_, cfg, pow64=False):
    """The order of operations of k_opt_prepare / k_opt_adam in numpy float32 (the norm summed pairwise instead of by 128 blocks): a
    second fp32 evaluation, for the CPU test that places it inside the bounds.  The two bias corrections are 1 - powf(0.9f, t) and
    1 - powf(0.999f, t) as in the kernel; pow64 = True forms them in double and rounds once, to show what the fp32 form costs."""
    f = np.float32
    inv_world = f(1.0) / f(cfg["world"])
    kl = f(kl_sum_) / (f(cfg["mb_rows"]) * f(cfg["world"]))
    lr = f(state["lr"])
    if cfg["adaptive"]:
        if kl > f(DESIRED_KL) * f(2.0):
            lr = max(f(1e-5), lr / f(1.5))
        elif kl < f(DESIRED_KL) / f(2.0) and kl > f(0.0):
            lr = min(f(1e-2), lr * f(1.5))
    gs = np.asarray(grad_sum, dtype=f)
    g = gs * inv_world
    total = np.sqrt((g * g).sum(dtype=f))
    coef = min(f(MAX_GRAD_NORM) / (total + f(1e-6)), f(1.0))
    t = f(state["t"] + 1)
    if pow64:
        bc1, bc2 = f(1.0 - 0.9 ** float(t)), f(1.0 - 0.999 ** float(t))
    else:
        bc1, bc2 = f(1.0) - np.power(f(0.9), t), f(1.0) - np.power(f(0.999), t)
    g = gs * inv_world * coef
    m = f(0.9) * state["m"].astype(f) + f(0.1) * g
    v = f(0.999) * state["v"].astype(f) + f(0.001) * g * g
    p = state["params"].astype(f) - (lr / bc1) * m / (np.sqrt(v) / np.sqrt(bc2) + f(1e-8))
    return dict(params=p, m=m, v=v, t=state["t"] + 1, lr=float(lr), kl=float(kl), norm=float(total))


# ------------------------------------------------------------------------------------------------ errors and bounds
ARRAYS = ("params", "m", "v")
FLOOR_ROUNDINGS = {"params": 1.0, "m": 2.0, "v": 3.0}           # rms roundings per step of a valid fp32 evaluation (module docstring)


def grow_mag(mag, ref, grad_sum, cfg):
    """Largest magnitude every element has held so far, per array: what one rounding is measured against.  For m also the 0.1 g it
    absorbed (0.9 m + 0.1 g cancels: the rounding is that of the operands, not of the small result)."""
    g = np.abs(np.asarray(grad_sum, dtype=np.float64)) / cfg["world"] * ref["coef"]
    new = {a: np.abs(ref[a]) for a in ARRAYS}
    new["m"] = np.maximum(new["m"], 0.1 * g)
    return new if mag is None else {a: np.maximum(mag[a], new[a]) for a in ARRAYS}


def e32_of(yard, ref, size, mag, steps):
    """{array: (whole-vector e32, per-block e32 [blocks])} after `steps` steps, floored at sqrt(steps) roundings of the largest value
    held (module docstring)."""
    starts = block_starts(size)
    out = {}
    for a in ARRAYS:
        fl = U * FLOOR_ROUNDINGS[a] * (min(np.sqrt(steps), 2.3) if a == "m" else np.sqrt(steps))
        err = np.abs(yard[a].astype(np.float64) - ref[a])
        out[a] = (max(float(err.max()), fl * float(mag[a].max())),
                  np.maximum(np.maximum.reduceat(err, starts), fl * np.maximum.reduceat(mag[a], starts)))
    return out


def bc_allowance(t):
    """Largest relative difference between the step with the kernel's fp32 bias corrections at step count t and the step with the exact
    ones, to first order: the step is proportional to 1 / bc1 and at most to sqrt(bc2); c^t is off by |fl32(c)^t - c^t| for the
    constant and by one ulp (2^-23 c^t) for powf, and the subtraction from 1 is exact (c^t >= 1 / 2) or one more ordinary rounding."""
    out = 0.0
    for c, weight in ((0.9, 1.0), (0.999, 0.5)):
        a = abs(float(np.float32(c)) ** t - c ** t) + 2.0 * U * c ** t
        out += weight * a / (1.0 - c ** t)
    return out


def ratios(got, ref, e32, size, allow=None):
    """Worst err / (4 e32) of fp32 arrays `got` against the reference: {array: ratio over the whole vector, array + "/block": worst
    ratio over the layout's blocks}.  0 / 0 counts as 0 (an array that must be, and is, exactly the reference).  allow [n]: the
    accumulated bias-correction allowance of the parameters (module docstring), taken off their error per element; the ratios
    without it are returned as "params (raw)" and "params/block (raw)", which nothing asserts."""
    starts = block_starts(size)
    out = {}
    for a in ARRAYS:
        err = np.abs(np.asarray(got[a], dtype=np.float64) - ref[a])
        whole, blocks = e32[a]
        if a == "params" and allow is not None:
            out["params (raw)"] = _ratio(float(err.max()), MARGIN * whole)
            out["params/block (raw)"] = float(max(_ratio(e, MARGIN * b) for e, b in zip(np.maximum.reduceat(err, starts), blocks)))
            err = np.maximum(err - allow, 0.0)
        out[a] = _ratio(float(err.max()), MARGIN * whole)
        out[a + "/block"] = float(max(_ratio(e, MARGIN * b) for e, b in zip(np.maximum.reduceat(err, starts), blocks)))
    return out


def asserted(worst):
    return {k: v for k, v in worst.items() if "(raw)" not in k}


def _ratio(err, bound):
    return 0.0 if err == 0.0 else float("inf") if bound == 0.0 else err / bound


@functools.lru_cache(maxsize=None)
def run(size, traj, world=1):
    """The trajectory in float64, with the yardstick's fp32 trajectory beside it: a list with, per step, grad_sum (fp32), kl_sum
    (fp32), ref (the state after the step), yard (the yardstick's state after it), e32 and allow (the accumulated bias-correction
    allowance of the parameters).  Computed once; read-only."""
    spec = TRAJECTORIES[traj]
    cfg = dict(world=world, mb_rows=mb_rows(size), adaptive=spec["adaptive"])
    ref = initial_state(size, spec["lr0"])
    yard = {k: (v.astype(np.float32) if isinstance(v, np.ndarray) else v) for k, v in ref.items()}
    out, mag, allow = [], None, np.zeros(layout(size)["n"])
    for i, (family, norm, kl, regime) in enumerate(spec["steps"]):
        gs, ks = gradient(size, traj, i, family, norm, world), kl_sum(size, kl, world)
        before = ref["params"]
        ref = step(ref, gs, ks, cfg)
        allow = allow + bc_allowance(ref["t"]) * np.abs(ref["params"] - before)
        allow.setflags(write=False)
        yard = torch_step(yard, gs, ks, cfg, torch.float32)
        mag = grow_mag(mag, ref, gs, cfg)
        for d in (ref, yard):
            for a in ARRAYS:
                d[a].setflags(write=False)
        gs.setflags(write=False)
        out.append(dict(grad_sum=gs, kl_sum=ks, ref=ref, yard=yard, e32=e32_of(yard, ref, size, mag, i + 1), allow=allow, regime=regime, cfg=cfg))
    return out


# ------------------------------------------------------------------------------------------------ late steps and large norms
LATE_T = (999, 9999, 99999)


def late_case(size, t):
    """A state at Adam step t with moments of the size a run leaves behind (|g| about 1e-3: m about 3e-4, v about 1e-6), parameters
    ZERO so that the parameters after one step are the step itself, to fp32 relative precision; and that step's gradient."""
    n = layout(size)["n"]
    g = _seed(size, "late", t)
    m = (3e-4 * g.standard_normal(n)).astype(np.float32).astype(np.float64)
    v = (1e-6 * (0.5 + g.random(n))).astype(np.float32).astype(np.float64)
    state = dict(params=np.zeros(n), m=m, v=v, t=t, lr=float(np.float32(1e-3)))
    grad = (1e-3 * g.standard_normal(n)).astype(np.float32)
    return state, grad, kl_sum(size, 0.010)


NORMS = (1e-7, 1e3, 1e4)            # pre-clip norms of the one-step cases: 1e4 squares to 1e8, beyond 2^23 = 8.4e6


@functools.lru_cache(maxsize=None)
def norm_case(size, norm):
    """One step from the initial state on a randn gradient of the given pre-clip norm: (state, grad_sum, kl_sum, cfg, ref, e32, allow)."""
    cfg = dict(world=1, mb_rows=mb_rows(size), adaptive=True)
    state = initial_state(size, 1e-3)
    gs, ks = gradient(size, "norm", repr(norm), _R, norm), kl_sum(size, 0.010)
    ref = step(state, gs, ks, cfg)
    yard = torch_step({k: (v.astype(np.float32) if isinstance(v, np.ndarray) else v) for k, v in state.items()}, gs, ks, cfg, torch.float32)
    allow = bc_allowance(1) * np.abs(ref["params"] - state["params"])
    return state, gs, ks, cfg, ref, e32_of(yard, ref, size, grow_mag(None, ref, gs, cfg), 1), allow
