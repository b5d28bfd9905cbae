"""Our own restatement of planning against obstacles that move: tests/plan_ref.py's `score` and
tests/plan_grad_ref.py's `objective` with the centre of obstacle i at node k at c_i + u_i * (k * dt) -- three operations, each rounded
on its own in the working dtype: k * dt, u * t_k, c + (..) -- and the fleet rule of lg_plan_fleet_scenes in NumPy float32.

As in those two files, constants enter as their float32 values in both precisions.  The problem is plan_ref's dict with one more
key, "obs_v" (n_obs, 2): the velocities of its obstacles.
"""
import numpy as np
import torch

from tests.plan_grad_ref import _t, tube
from tests.plan_ref import _quad, c32

F = np.float32


def centres(p, k, D):
    """(n_obs, 2): where the obstacles are at node k."""
    oc, u = c32(p["obs_c"], D).reshape(-1, 2), c32(p["obs_v"], D).reshape(-1, 2)
    t = D(k) * c32(p["dt"], D)
    return oc + u * t


def score(p, z0, v, fw, w0=None, offset=None, dtype=F):
    """plan_ref.score against moving obstacles: the same dict."""
    D = np.dtype(dtype).type
    B, N = v.shape[:2]
    v, fw, z0 = v.astype(D), fw.astype(D), z0.astype(D)
    dt, goal, Qw, w_max = c32(p["dt"], D), c32(p["goal"], D), c32(p["Qw"], D), c32(p["w_max"], D)
    Q, Qf, R = c32(p["Q"], D), c32(p["Qf"] if p.get("Qf") is not None else p["Q"], D), c32(p["R"], D)
    orad = c32(p["obs_r"], D).reshape(-1)
    zmin, zmax, vmin, vmax = (c32(p[k], D) for k in ("rom_z_min", "rom_z_max", "rom_v_min", "rom_v_max"))
    z, w = np.zeros((B, N + 1, 2), D), np.zeros((B, N + 1), D)
    g = np.zeros((B, N + 1, len(orad)), D)
    zk = z0.copy()
    wk = np.zeros(B, D) if w0 is None else w0.astype(D)
    cost = np.zeros(B, D)
    minc, worst = np.full(B, np.inf, D), np.full(B, -1, np.int32)
    nv = np.zeros((B, 4), np.int32)
    bound = np.full(B, np.inf)
    for k in range(N + 1):
        z[:, k], w[:, k] = zk, wk
        hit = np.zeros(B, bool)
        oc = centres(p, k, D)
        for i in range(len(orad)):
            dx, dy, rr = zk[:, 0] - oc[i, 0], zk[:, 1] - oc[i, 1], orad[i] + wk
            gi = (dx * dx + dy * dy) - rr * rr
            g[:, k, i] = gi
            better = gi < minc
            minc, worst = np.where(better, gi, minc), np.where(better, k, worst).astype(np.int32)
            hit |= gi < 0
        nv[:, 0] += hit
        nv[:, 2] += ((zk < zmin) | (zk > zmax)).any(axis=1)
        nv[:, 3] += wk > w_max
        bound = np.minimum(bound, np.minimum(np.abs(zk - zmin), np.abs(zk - zmax)).min(axis=1))
        bound = np.minimum(bound, np.abs(wk - w_max))
        d0, d1 = zk[:, 0] - goal[0], zk[:, 1] - goal[1]
        cost = cost + _quad(Q if k < N else Qf, d0, d1)
        if k < N:
            vk = v[:, k]
            nv[:, 1] += ((vk < vmin) | (vk > vmax)).any(axis=1)
            bound = np.minimum(bound, np.minimum(np.abs(vk - vmin), np.abs(vk - vmax)).min(axis=1))
            cost = cost + _quad(R, vk[:, 0], vk[:, 1])
        cost = cost + (wk * Qw) * wk
        if k < N:
            zk = zk + dt * vk
            wk = fw[:, k] + c32(offset[k], D) if offset is not None else fw[:, k]
    gmargin = np.abs(g).reshape(B, -1).min(axis=1) if len(orad) else np.full(B, np.inf)
    return {"z": z, "w": w, "g": g, "cost": cost, "min_clear": minc, "worst_node": worst, "n_viol": nv, "margin": (gmargin, bound)}


def objective(p, rho, z0, v, dtype, model=None, e=None, v_prev=None, level=None, w0=None, offset=None):
    """plan_grad_ref.objective against moving obstacles: (J (B), its parts); `pen_g_nodes` (B, N+1) is the obstacle hinge per node."""
    B, N = v.shape[:2]
    fw, margin = tube(p, v, dtype, model, e, v_prev, level)
    dt, goal, Qw, w_max = (_t(p[k], dtype) for k in ("dt", "goal", "Qw", "w_max"))
    Q, Qf, R = _t(p["Q"], dtype), _t(p["Qf"] if p.get("Qf") is not None else p["Q"], dtype), _t(p["R"], dtype)
    oc0, ou, orad = _t(p["obs_c"], dtype).reshape(-1, 2), _t(p["obs_v"], dtype).reshape(-1, 2), _t(p["obs_r"], dtype).reshape(-1)
    zmin, zmax = _t(p["rom_z_min"], dtype), _t(p["rom_z_max"], dtype)
    rg, rw, rz = (_t(x, dtype) for x in rho)
    quad = lambda M, d: (d[:, 0] * M[0] + d[:, 1] * M[2]) * d[:, 0] + (d[:, 0] * M[1] + d[:, 1] * M[3]) * d[:, 1]
    zk = _t(z0, dtype)
    wk = torch.zeros(B, dtype=dtype) if w0 is None else _t(w0, dtype)
    zero = torch.zeros(B, dtype=dtype)
    cost, pg, pw, pz = zero, zero, zero, zero
    minc = torch.full((B,), float("inf"), dtype=dtype)
    nv0 = torch.zeros(B, dtype=torch.int64)
    nodes = []

    def note(a):
        nonlocal margin
        margin = torch.minimum(margin, a.detach().abs().double())
    for k in range(N + 1):
        hit = torch.zeros(B, dtype=torch.bool)
        t = torch.tensor(float(k), dtype=dtype) * dt
        oc = oc0 + ou * t
        here = zero
        for i in range(len(orad)):
            d, rr = zk - oc[i], orad[i] + wk
            g = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) - rr * rr
            note(g)
            minc = torch.minimum(minc, g.detach())
            hit |= g.detach() < 0
            pg = pg + (-g).clamp(min=0)
            here = here + (-g).detach().clamp(min=0)
        nodes.append(here)
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
    return J, {"cost": cost.detach(), "pen": torch.stack([pg, pw, pz], dim=1).detach(), "min_clear": minc, "n_viol0": nv0, "margin": margin,
               "pen_g_nodes": torch.stack(nodes, dim=1)}


def value_and_grad(p, rho, z0, v, dtype=torch.float64, **kw):
    """(J (B), dJ/dv (B, N, 2), parts) as NumPy arrays of the working precision, by torch autograd."""
    x = (v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(v))).to(dtype).clone().requires_grad_(True)
    J, parts = objective(p, rho, z0, x, dtype, **kw)
    (g,) = torch.autograd.grad(J.sum(), x)
    return J.detach().numpy(), g.numpy(), {k: t.numpy() for k, t in parts.items()}


def fleet_rule(separation, sense_radius, max_neighbours, pos, vel, static_obs=None, static_vel=None, n_static=None, t=0.0):
    """lg_plan_fleet_scenes restated: (obs (P, 8, 3), obs_vel (P, 8, 2), n_obs (P) int32) from pos, vel (P, 2) float32.
    1. robot p's n_s = clamp(n_static[p], 0, 8) static obstacles first, each centre advanced to time t: c + u * t, two roundings;
    2. then at most min(max_neighbours, 8 - n_s) robots q != p with d2 = dx*dx + dy*dy <= sense_radius^2 in float32, a d2 that is
       not finite never passing; 3. ordered by (d2, q) ascending; 4. a neighbour's slot is (pos_q, separation) with velocity vel_q;
    5. slots past n_obs[p] are zeros."""
    pos, vel = np.asarray(pos, F), np.asarray(vel, F)
    P = pos.shape[0]
    obs, ov, n = np.zeros((P, 8, 3), F), np.zeros((P, 8, 2), F), np.zeros(P, np.int32)
    s2 = F(sense_radius) * F(sense_radius)
    tt = F(t)
    with np.errstate(invalid="ignore", over="ignore"):
        for p in range(P):
            ns = 0 if static_obs is None else int(min(max(int(n_static[p]), 0), 8))
            for i in range(ns):
                u = np.zeros(2, F) if static_vel is None else np.asarray(static_vel[p, i], F)
                c = np.asarray(static_obs[p, i, :2], F)
                obs[p, i, :2] = c + u * tt if static_vel is not None else c
                obs[p, i, 2] = static_obs[p, i, 2]
                ov[p, i] = u
            dx, dy = pos[:, 0] - pos[p, 0], pos[:, 1] - pos[p, 1]
            d2 = dx * dx + dy * dy
            ok = np.isfinite(d2) & (d2 <= s2)
            ok[p] = False
            q = np.flatnonzero(ok)
            q = q[np.lexsort((q, d2[q]))][:max(0, min(int(max_neighbours), 8 - ns))]
            for j, qq in enumerate(q):
                obs[p, ns + j] = (pos[qq, 0], pos[qq, 1], F(separation))
                ov[p, ns + j] = vel[qq]
            n[p] = ns + len(q)
    return obs, ov, n
