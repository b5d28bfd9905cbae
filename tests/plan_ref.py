"""Our own NumPy restatement of scoring and tracking plans (legged_gym_dev_amd/tube/plan.py): the tube item,
the analytic tubes, the nodes, clearance, cost and counts of lg_plan_score, the tracking loop of lg_plan_track and the audit.

With dtype = float32 every operation is one numpy float32 op in the order the kernels evaluate it; with float64 it is the yardstick
the fp32 evaluations are measured against.  Constants enter as their float32 values in both modes, as the device holds them.
The problem is a dict: N, H_rev, dt, goal, obs_c, obs_r, Q, Qf, R (4 numbers, row-major), Qw, w_max, scaling, window_size, tube_kind,
rom_z_min/max, rom_v_min/max.
"""
import numpy as np

F = np.float32


def c32(x, D):
    """A constant: its float32 value, in the working dtype."""
    return np.asarray(x, F).astype(D)


def item(e, v_prev, v, level=None):
    """[e, v_prev.flatten(), v.flatten(), (level)] per plan: the ScalarHorizonTubeDataset item at start = H_rev."""
    B = v.shape[0]
    cols = [e.reshape(B, -1), v_prev.reshape(B, -1), v.reshape(B, -1)]
    if level is not None:
        cols.append(np.full((B, 1), level, v.dtype))
    return np.concatenate(cols, axis=1)


def window_arrays(e, v_prev, v):
    """The host-built arrays of the window query that the item equals: w (B, H_rev + N) with e in front, v (B, H_rev + N, 2)."""
    B, N = v.shape[:2]
    return np.concatenate([e, np.zeros((B, N), e.dtype)], 1), np.concatenate([v_prev, v], 1)


def analytic(kind, v, scaling, window_size, dtype=F):
    """fw (B, N) of l1, l2, l1_rolling, l2_rolling; the rolling mean sums the last min(window_size, k + 1) values oldest first."""
    D = np.dtype(dtype).type
    v = v.astype(D)
    s = c32(scaling, D)
    base = np.abs(v[..., 0]) + np.abs(v[..., 1]) if kind.startswith("l1") else v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]
    l = (s * base).astype(D)
    if not kind.endswith("rolling"):
        return l
    out = np.zeros_like(l)
    for k in range(l.shape[1]):
        k0 = max(k - window_size + 1, 0)
        acc = np.zeros(l.shape[0], D)
        for i in range(k0, k + 1):
            acc = acc + l[:, i]
        out[:, k] = acc / D(k - k0 + 1)
    return out


def _quad(M, d0, d1):
    return (d0 * M[0] + d1 * M[2]) * d0 + (d0 * M[1] + d1 * M[3]) * d1


def score(p, z0, v, fw, w0=None, offset=None, dtype=F):
    """Nodes, clearance, cost and counts from the tube values fw (B, N) (the MLP's, taken from the device, or analytic()).
    Returns a dict: z (B, N+1, 2), w (B, N+1), g (B, N+1, n_obs), cost, min_clear, worst_node, n_viol (B, 4) and `margin`, the
    smallest distance of any compared quantity from its threshold per plan: (|g| over nodes and obstacles, bound distance)."""
    D = np.dtype(dtype).type
    B, N = v.shape[:2]
    v, fw, z0 = v.astype(D), fw.astype(D), z0.astype(D)
    dt, goal, Qw, w_max = c32(p["dt"], D), c32(p["goal"], D), c32(p["Qw"], D), c32(p["w_max"], D)
    Q, Qf, R = c32(p["Q"], D), c32(p["Qf"] if p.get("Qf") is not None else p["Q"], D), c32(p["R"], D)
    oc, orad = c32(p["obs_c"], D).reshape(-1, 2), c32(p["obs_r"], D).reshape(-1)
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


def controller(c, x, ref, ff, D):
    """DoubleSingleTracking with DoubleInt2D.clip_v_z: min with the upper bound first, then max with the lower.
    c: Kp, Kd, model_dt, model_z_min/max (4), model_v_min/max (2).  Returns (action, the bounds hi, lo)."""
    Kp, Kd, dt = c32(c["Kp"], D), c32(c["Kd"], D), c32(c["model_dt"], D)
    u = Kp * (ref - x[:, :2]) + Kd * (ff - x[:, 2:])
    hi = np.minimum(c32(c["model_v_max"], D), (c32(c["model_z_max"], D)[2:] - x[:, 2:]) / dt)
    lo = np.maximum(c32(c["model_v_min"], D), (c32(c["model_z_min"], D)[2:] - x[:, 2:]) / dt)
    return np.maximum(np.minimum(u, hi), lo).astype(D), hi, lo


def track(c, z, v, x0=None, S=1, rom_dt=None, dtype=F):
    """The tracking loop: per node t and substep s the reference z[t] + (z[t+1] - z[t]) ((s model_dt) / rom_dt), the feed-forward
    v[min(t+1, N-1)], the controller, x = f(x, a).  Returns x (B, N+1, 4), u (B, N S, 2), pz_x, w_true and `bind`
    (B, N S, 2) int8: +1 / -1 where the action sits on the upper / lower bound, +-2 where that bound is the velocity one."""
    D = np.dtype(dtype).type
    B, N = v.shape[:2]
    z, v = z.astype(D), v.astype(D)
    dt = c32(c["model_dt"], D)
    rdt = c32(c["model_dt"] * S if rom_dt is None else rom_dt, D)
    xk = np.concatenate([z[:, 0], np.zeros((B, 2), D)], 1) if x0 is None else x0.astype(D)
    x, u = np.zeros((B, N + 1, 4), D), np.zeros((B, N * S, 2), D)
    bind = np.zeros((B, N * S, 2), np.int8)
    x[:, 0] = xk
    for t in range(N):
        ff = v[:, min(t + 1, N - 1)]
        for s in range(S):
            frac = (D(s) * dt) / rdt
            ref = z[:, t] + (z[:, t + 1] - z[:, t]) * frac
            a, hi, lo = controller(c, xk, ref, ff, D)
            amax, amin = c32(c["model_v_max"], D), c32(c["model_v_min"], D)
            bind[:, t * S + s] = np.where(a == hi, np.where(hi < amax, 2, 1), np.where(a == lo, np.where(lo > amin, -2, -1), 0))
            pos = xk[:, :2] + dt * xk[:, 2:]
            vel = xk[:, 2:] + dt * a
            xk = np.concatenate([pos, vel], 1)
            u[:, t * S + s] = a
        x[:, t + 1] = xk
    pz = x[:, :, :2]
    e = pz - z
    s2 = np.zeros((B, N + 1), D)
    s2 = s2 + e[..., 0] * e[..., 0]
    s2 = s2 + e[..., 1] * e[..., 1]
    return {"x": x, "u": u, "pz_x": pz.copy(), "w_true": np.sqrt(s2), "bind": bind}


def audit(w, w_true, pz_x, min_clear, obs_c, obs_r):
    w, wt, pz = np.asarray(w, np.float64), np.asarray(w_true, np.float64), np.asarray(pz_x, np.float64)
    cov = w >= wt
    pred = np.asarray(min_clear, np.float64) >= 0
    act = np.ones(w.shape[0], bool)
    for c, r in zip(obs_c, obs_r):
        act &= ~(np.linalg.norm(pz - np.asarray(c, np.float64), axis=-1) < r).any(axis=1)
    m = lambda a: float(np.mean(a))
    return {"plans": int(w.shape[0]), "nodes": int(w.shape[1]), "coverage_by_node": [float(x) for x in cov.mean(axis=0)],
            "coverage": m(cov), "covered_plans": m(cov.all(axis=1)), "predicted_safe": m(pred), "actually_safe": m(act),
            "table": {"safe_safe": m(pred & act), "safe_unsafe": m(pred & ~act), "unsafe_safe": m(~pred & act),
                      "unsafe_unsafe": m(~pred & ~act)},
            "w_true_mean": float(wt.mean()), "w_true_max": float(wt.max())}
