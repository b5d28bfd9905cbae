"""Our own NumPy restatement of the sampling planner (legged_gym_dev_amd/tube/plan.py) on top of
tests/plan_ref.py: the hinge sums, J, the softmin update in the device's summation order, the elite, the closed-loop shifts, and a
plain MPPI loop on plan_ref.score.

With dtype = float32 every operation is one numpy float32 op in the order the kernels evaluate it; with float64 it is the yardstick.
The candidates are an argument: the tests pass the device's own (lg_plan_mppi_candidates), so the noise is checked on its own and
the arithmetic on identical inputs."""
import numpy as np

from tests import plan_ref
from tests.plan_ref import c32

F = np.float32
CH = 64                                 # MPPI_CH: chunks of a sum over the candidates


def sigma_it(sigma, decay, it):
    s, d = F(sigma), F(decay)
    for _ in range(it):
        s = F(s * d)
    return s


def penalties(p, res, dtype=F):
    """(B, 3): pen_g, pen_w, pen_z from plan_ref.score's z, w, g of the same dtype, each one chain over the nodes ascending."""
    D = np.dtype(dtype).type
    z, w, g = res["z"].astype(D), res["w"].astype(D), res["g"].astype(D)
    w_max, zmin, zmax = c32(p["w_max"], D), c32(p["rom_z_min"], D), c32(p["rom_z_max"], D)
    B, N1 = w.shape
    zero = D(0)
    pg, pw, pz = np.zeros(B, D), np.zeros(B, D), np.zeros(B, D)
    for k in range(N1):
        for i in range(g.shape[2]):
            pg = pg + np.maximum(zero, -g[:, k, i])
        pw = pw + np.maximum(zero, w[:, k] - w_max)
        for d in range(2):
            pz = pz + (np.maximum(zero, z[:, k, d] - zmax[d]) + np.maximum(zero, zmin[d] - z[:, k, d]))
    return np.stack([pg, pw, pz], axis=1)


def total(cost, pen, rho, dtype=F):
    """J = ((cost + rho_g pen_g) + rho_w pen_w) + rho_z pen_z."""
    D = np.dtype(dtype).type
    cost, pen = np.asarray(cost).astype(D), np.asarray(pen).astype(D)
    r = c32(rho, D)
    return ((cost + r[0] * pen[..., 0]) + r[1] * pen[..., 1]) + r[2] * pen[..., 2]


def chunk_sum(x, dtype=F):
    """Sum over axis 0 (the K candidates) in the update kernel's order: chunk c adds j = c, c + 64, .. ascending from 0, then a
    halving tree over the 64 chunks."""
    D = np.dtype(dtype).type
    x = np.asarray(x).astype(D)
    K = x.shape[0]
    pad = (-K) % CH
    if pad:
        x = np.concatenate([x, np.zeros((pad,) + x.shape[1:], D)])
    x = x.reshape((-1, CH) + x.shape[1:])
    acc = np.zeros(x.shape[1:], D)
    for r in range(x.shape[0]):
        acc = acc + x[r]
    h = CH // 2
    while h:
        acc = acc[:h] + acc[h:2 * h]
        h //= 2
    return acc[0]


def weights(J, lam, dtype=F):
    """(weights (K), Jmin, first arg-min or -1): exp(-(J - Jmin) / lambda) over the finite J, 0 elsewhere."""
    D = np.dtype(dtype).type
    J = np.asarray(J).astype(D)
    fin = np.isfinite(J)
    if not fin.any():
        return np.zeros(J.shape, D), D(np.inf), -1
    Jm = np.where(fin, J, D(np.inf))
    idx = int(np.argmin(Jm))
    with np.errstate(invalid="ignore", over="ignore"):
        w = np.exp((-(J - Jm[idx]) / c32(lam, D)).astype(D)).astype(D)
    return np.where(fin, w, D(0)), Jm[idx], idx


def update(cand, J, lam, dtype=F):
    """One instance: cand (K, N, 2), J (K).  The new mean plan (N, 2), or None where no J is finite (the mean stays)."""
    D = np.dtype(dtype).type
    w, _, idx = weights(J, lam, D)
    if idx < 0:
        return None
    S = chunk_sum(w, D)
    return chunk_sum(w[:, None, None] * np.asarray(cand).astype(D), D) / S


def elite(best_J, best_v, J, cand, mean, reset):
    """The elite after one iteration of one instance: (best_J, best_v)."""
    _, Jmin, idx = weights(J, 1.0, np.asarray(J).dtype)
    if idx >= 0 and (reset or Jmin < best_J):
        return Jmin, np.array(cand[idx])
    return (np.asarray(J).dtype.type(np.inf), np.array(mean)) if reset else (best_J, best_v)


def shift_plan(v):
    return np.concatenate([v[:, 1:], v[:, -1:]], axis=1)


def shift_past(e, v_prev, err, v_k):
    if e.shape[1] == 0:
        return e, v_prev
    return np.concatenate([e[:, 1:], err[:, None]], axis=1), np.concatenate([v_prev[:, 1:], v_k[:, None]], axis=1)


def score_J(p, z0, v, rho, dtype=F):
    """cost, min_clear, pen and J of plans v (B, N, 2) from z0 (2) under an analytic tube."""
    fw = plan_ref.analytic(p["tube_kind"], v, p["scaling"], p["window_size"], dtype)
    res = plan_ref.score(p, np.repeat(np.asarray(z0, F)[None], v.shape[0], 0), v, fw, None, None, dtype)
    pen = penalties(p, res, dtype)
    return res, pen, total(res["cost"], pen, rho, dtype)


def mppi(p, z0, v0, K, iters, sigma, decay, lam, rho, seed, dtype=F):
    """A plain MPPI loop with NumPy's generator (not Philox): the final mean plan (N, 2)."""
    D = np.dtype(dtype).type
    rng = np.random.default_rng(seed)
    vbar = np.asarray(v0).astype(D)
    lo, hi = c32(p["rom_v_min"], D), c32(p["rom_v_max"], D)
    for it in range(iters):
        eps = rng.standard_normal((K,) + vbar.shape).astype(D)
        eps[0] = 0
        cand = np.clip(vbar[None] + D(sigma_it(sigma, decay, it)) * eps, lo, hi).astype(D)
        _, _, J = score_J(p, z0, cand, rho, D)
        new = update(cand, J, lam, D)
        vbar = vbar if new is None else new.astype(D)
    return vbar
