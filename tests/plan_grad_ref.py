"""Our own restatement of the gradient planner (legged_gym_dev_amd/tube/plan.py) on top of
tests/plan_ref.py's definitions: J = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z on torch CPU tensors -- the tube from the
model's ``state_dict()`` or analytic -- differentiated by torch autograd, in float64 (the yardstick) and in float32 (which gives e32);
projected Adam and the elite in NumPy.

Constants enter as their float32 values in both modes, as the device holds them (plan_ref.c32).  The problem is plan_ref's dict.
torch's own tie rules are the kernel's: a hinge (clamp(min=0)) and ReLU have derivative 0 at 0, |v| has derivative 0 at 0, Softplus
is linear above beta x = 20.  `margin` is the smallest distance of a plan from any such kink.
"""
import numpy as np
import torch

from tests.plan_ref import c32

F = np.float32
ACTS = {"relu": torch.relu, "tanh": torch.tanh, "elu": torch.nn.functional.elu}


def _t(x, dtype):
    """A constant or an input: its float32 value as a torch tensor of the working dtype."""
    if isinstance(x, torch.Tensor):
        return x.detach().cpu().to(torch.float32).to(dtype)
    return torch.from_numpy(np.asarray(x, F)).to(dtype)


def mlp(sd, x, act, beta, dtype):
    """The reference MLP from a state dict (layers.{0,2,..}.weight (out, in) / .bias): (output, [hidden pre-activations])."""
    keys = list(sd)
    h, pre = x, []
    for i in range(0, len(keys), 2):
        W, b = _t(sd[keys[i]], dtype), _t(sd[keys[i + 1]], dtype)
        h = h @ W.T + b
        if i + 2 < len(keys):
            pre.append(h)
            h = torch.nn.functional.softplus(h, beta=float(beta), threshold=20.0) if act == "softplus" else ACTS[act](h)
    return h, pre


def tube(p, v, dtype, model=None, e=None, v_prev=None, level=None):
    """fw (B, N) of the plans v (B, N, 2) and the kink margins of the tube itself.  model: None for an analytic kind, else a dict
    sd, act, beta.  The item is [e, v_prev.flatten(), v.flatten(), (level)], as plan_ref.item builds it."""
    B, N = v.shape[:2]
    inf = torch.full((B,), float("inf"), dtype=torch.float64)
    kind = p["tube_kind"]
    if kind == "nn":
        cols = [_t(e, dtype).reshape(B, -1), _t(v_prev, dtype).reshape(B, -1), v.reshape(B, -1)]
        if level is not None:
            cols.append(torch.full((B, 1), float(np.float32(level)), dtype=dtype))
        fw, pre = mlp(model["sd"], torch.cat(cols, dim=1), model["act"], model["beta"], dtype)
        m = inf
        if model["act"] in ("relu", "elu"):
            for h in pre:
                m = torch.minimum(m, h.detach().abs().double().min(dim=1).values)
        return fw, m
    s = _t(p["scaling"], dtype)
    l1 = kind.startswith("l1")
    base = s * (v[..., 0].abs() + v[..., 1].abs() if l1 else v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1])
    a = v.detach().abs().double().reshape(B, -1)                         # an input that is exactly 0 is a stated tie, not a kink: see objective()
    m = torch.where(a > 0, a, inf[:, None]).min(dim=1).values if l1 else inf
    if not kind.endswith("rolling"):
        return base, m
    out = []
    for k in range(N):
        k0 = max(k - int(p["window_size"]) + 1, 0)
        out.append(base[:, k0:k + 1].sum(dim=1) / (k - k0 + 1))
    return torch.stack(out, dim=1), m


def objective(p, rho, z0, v, dtype, model=None, e=None, v_prev=None, level=None, w0=None, offset=None):
    """J (B) of the plans v (B, N, 2) (a torch tensor of `dtype`, possibly requiring grad) and a dict of its parts: cost, pen (B, 3),
    min_clear, n_viol0 (nodes inside an obstacle) and margin (B) float64, the smallest |argument| of any hinge, of |v| (l1 kinds) and
    of a ReLU / ELU pre-activation.  An element of v that is exactly 0 does not count: it is an input, 0 in every precision, and
    the tie rule there (sign(0) = 0) is torch's and the kernel's alike, so no rounding can put the two on different sides."""
    B, N = v.shape[:2]
    fw, margin = tube(p, v, dtype, model, e, v_prev, level)
    dt, goal, Qw, w_max = (_t(p[k], dtype) for k in ("dt", "goal", "Qw", "w_max"))
    Q, Qf, R = _t(p["Q"], dtype), _t(p["Qf"] if p.get("Qf") is not None else p["Q"], dtype), _t(p["R"], dtype)
    oc, orad = _t(p["obs_c"], dtype).reshape(-1, 2), _t(p["obs_r"], dtype).reshape(-1)
    zmin, zmax = _t(p["rom_z_min"], dtype), _t(p["rom_z_max"], dtype)
    rg, rw, rz = (_t(x, dtype) for x in rho)
    quad = lambda M, d: (d[:, 0] * M[0] + d[:, 1] * M[2]) * d[:, 0] + (d[:, 0] * M[1] + d[:, 1] * M[3]) * d[:, 1]
    zk = _t(z0, dtype)
    wk = torch.zeros(B, dtype=dtype) if w0 is None else _t(w0, dtype)
    zero = torch.zeros(B, dtype=dtype)
    cost, pg, pw, pz = zero, zero, zero, zero
    minc = torch.full((B,), float("inf"), dtype=dtype)
    nv0 = torch.zeros(B, dtype=torch.int64)

    def note(a):
        nonlocal margin
        margin = torch.minimum(margin, a.detach().abs().double())
    for k in range(N + 1):
        hit = torch.zeros(B, dtype=torch.bool)
        for i in range(len(orad)):
            d, rr = zk - oc[i], orad[i] + wk
            g = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) - rr * rr
            note(g)
            minc = torch.minimum(minc, g.detach())
            hit |= g.detach() < 0
            pg = pg + (-g).clamp(min=0)
        nv0 += hit
        note(wk - w_max)
        pw = pw + (wk - w_max).clamp(min=0)
        for d in range(2):
            note(zk[:, d] - zmax[d]), note(zmin[d] - zk[:, d])
            pz = pz + ((zk[:, d] - zmax[d]).clamp(min=0) + (zmin[d] - zk[:, d]).clamp(min=0))
        cost = cost + quad(Q if k < N else Qf, zk - goal)
        if k < N:
            cost = cost + quad(R, v[:, k])
        cost = cost + (wk * Qw) * wk
        if k < N:
            zk = zk + dt * v[:, k]
            wk = fw[:, k] + _t(offset, dtype)[k] if offset is not None else fw[:, k]
    J = ((cost + rg * pg) + rw * pw) + rz * pz
    return J, {"cost": cost.detach(), "pen": torch.stack([pg, pw, pz], dim=1).detach(), "min_clear": minc, "n_viol0": nv0, "margin": margin}


def value_and_grad(p, rho, z0, v, dtype=torch.float64, **kw):
    """(J (B), dJ/dv (B, N, 2), parts) as NumPy arrays of the working precision, by torch autograd."""
    x = (v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dtype).clone().requires_grad_(True)
    J, parts = objective(p, rho, z0, x, dtype, **kw)
    (g,) = torch.autograd.grad(J.sum(), x)
    return J.detach().numpy(), g.numpy(), {k: t.numpy() for k, t in parts.items()}


def bias_corrections(beta1, beta2, t):
    """1 - beta^t of step index t >= 1 as the library takes them: float32 betas, the power in double, rounded once."""
    return F(1.0 - float(F(beta1)) ** t), F(1.0 - float(F(beta2)) ** t)


def adam_step(v, g, m, s, t, lr, beta1, beta2, eps, v_min, v_max, dtype=F):
    """One projected Adam step on plans v (.., N, 2) with the gradient g and the moments m, s: (v, m, s, the step before the clip).
    With dtype = float32 every operation is one float32 op in the kernel's order."""
    D = np.dtype(dtype).type
    v, g, m, s = (np.asarray(a).astype(D) for a in (v, g, m, s))
    lr, b1, b2, eps = c32(lr, D), c32(beta1, D), c32(beta2, D), c32(eps, D)
    bc1, bc2 = (D(x) for x in bias_corrections(beta1, beta2, t))
    m = b1 * m + (D(1) - b1) * g
    s = b2 * s + ((D(1) - b2) * g) * g
    x = v - (lr * (m / bc1)) / (np.sqrt(s / bc2) + eps)
    return np.minimum(np.maximum(x, c32(v_min, D)), c32(v_max, D)), m, s, x


def elite(best_J, best_v, J, v, reset):
    """The elite after the evaluation of plans v (B, N, 2) with scores J (B): a finite J wins at a reset or where J < best_J; a
    reset without a finite J leaves (inf, the plan)."""
    J, v = np.asarray(J), np.asarray(v)
    fin = np.isfinite(J)
    win = fin & (np.ones_like(fin) if reset else J < np.asarray(best_J))
    if reset:
        return np.where(win, J, J.dtype.type(np.inf)), v.copy()
    return np.where(win, J, best_J), np.where(win[:, None, None], v, best_v)


def descend(p, rho, z0, v0, iters, lr, beta1=0.9, beta2=0.999, eps=1e-8, dtype=np.float64, **kw):
    """Projected Adam from v0 (B, N, 2): iters steps, then the evaluation of the last iterate.  Returns (v, best_J, best_v, hist
    (iters + 1, B, 2) = (J, max |dJ/dv|))."""
    D = np.dtype(dtype).type
    td = torch.float64 if D is np.float64 else torch.float32
    v = np.asarray(v0).astype(D)
    m, s = np.zeros_like(v), np.zeros_like(v)
    best_J = best_v = None
    hist = []
    for it in range(iters + 1):
        J, g, _ = value_and_grad(p, rho, z0, v, td, **kw)
        hist.append(np.stack([J, np.abs(g).reshape(len(J), -1).max(axis=1)], axis=1))
        best_J, best_v = elite(best_J, best_v, J, v, it == 0)
        if it < iters:
            ok = np.isfinite(J) & np.isfinite(g).reshape(len(J), -1).all(axis=1)
            nv, nm, ns, _ = adam_step(v, g, m, s, it + 1, lr, beta1, beta2, eps, p["rom_v_min"], p["rom_v_max"], D)
            k = ok[:, None, None]
            v, m, s = np.where(k, nv, v), np.where(k, nm, m), np.where(k, ns, s)
    return v, best_J, best_v, np.stack(hist)
