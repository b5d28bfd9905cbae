"""NumPy restatement of plans tracked on the legged env (legged_gym_dev_amd/tube/plan_env.py, csrc/lg_traj.h LG_TG_KIND_PLAN,
k_traj_record): the plan-following generator's law one float32 rounding at a time, the recorder's three
rules, the row alignment and audit_env.  Nothing here imports the library."""
import numpy as np

f32 = np.float32


class PlanLaw:
    """PlanTrajectoryGenerator for n envs: ROM step counter k, clock t, window (n, Nw + 1, 2) and the in-force input v_in, as
    tg_reset / tg_callback_step keep them.  plans: (n, n_nodes, 2) float32, n_nodes may be 0."""

    def __init__(self, plans, Nw, rom_dt, dt):
        self.plans = np.asarray(plans, f32)
        self.n, self.n_nodes = self.plans.shape[0], self.plans.shape[1]
        self.Nw, self.rom_dt, self.dt = int(Nw), f32(rom_dt), f32(dt)
        self.k = np.zeros(self.n, f32)
        self.t = np.zeros(self.n, f32)
        self.win = np.zeros((self.n, self.Nw + 1, 2), f32)
        self.v_in = np.zeros((self.n, 2), f32)

    def reset(self, ids, z):
        """tg_reset: the window restarts at z, the clocks at -Nw rom_dt; Nw pre-roll ROM steps at k < 0, so with input 0."""
        ids = np.atleast_1d(ids)
        z = np.asarray(z, f32).reshape(len(ids), 2)
        t = f32(f32(-self.Nw) * self.rom_dt)
        for _ in range(self.Nw):
            t = f32(t + self.rom_dt)
        self.k[ids], self.t[ids] = f32(0), t
        self.win[ids] = z[:, None, :]                              # z + rom_dt * 0 = z, every point
        self.v_in[ids] = 0

    def input(self, i):
        k = int(self.k[i])
        return self.plans[i, k] if 0 <= k < self.n_nodes else np.zeros(2, f32)

    def step(self):
        """One env step of every env (tg_callback_step); returns the mask of envs whose ROM stepped."""
        stepped = np.zeros(self.n, bool)
        for i in range(self.n):
            if self.t[i] >= f32(f32(self.k[i] * self.rom_dt) - f32(1e-5)):
                v = self.input(i)
                head = (self.win[i, -1] + (self.rom_dt * v).astype(f32)).astype(f32)      # z + rom_dt * v, no contraction
                self.win[i, :-1] = self.win[i, 1:]
                self.win[i, -1] = head
                self.v_in[i] = v
                self.k[i] = f32(self.k[i] + f32(1))
                stepped[i] = True
            self.t[i] = f32(self.t[i] + self.dt)
        return stepped


def chain(z0, v, rom_dt):
    """The float32 chain z_{j+1} = z_j + rom_dt * v_j from z0 (n, 2) under v (n, N, 2): (n, N + 1, 2)."""
    z = [np.asarray(z0, f32)]
    for j in range(v.shape[1]):
        z.append((z[-1] + (f32(rom_dt) * np.asarray(v[:, j], f32)).astype(f32)).astype(f32))
    return np.stack(z, 1)


class Recorder:
    """lg_traj_rec's three rules for n envs, rows_max rows."""

    def __init__(self, n, rows_max, x_n=0):
        self.rows_max = rows_max
        self.z, self.pz_x = np.zeros((n, rows_max, 2), f32), np.zeros((n, rows_max, 2), f32)
        self.v = np.zeros((n, rows_max - 1, 2), f32)
        self.x = np.zeros((n, rows_max, x_n), f32) if x_n else None
        self.rows, self.dead, self.k_mark = np.zeros(n, np.int32), np.zeros(n, np.uint8), np.zeros(n, f32)

    def begin(self, z, pz_x, k, x=None):
        self.z[:, 0], self.pz_x[:, 0] = z, pz_x
        if self.x is not None:
            self.x[:, 0] = x
        self.rows[:], self.dead[:], self.k_mark[:] = 1, 0, k

    def step(self, reset, z, pz_x, k, v_in, x=None):
        for i in range(len(self.rows)):
            if self.dead[i]:
                continue                                            # rule 1
            if reset[i]:
                self.dead[i] = 1                                    # rule 2: rows kept
                continue
            r = self.rows[i]
            if k[i] != self.k_mark[i] and r < self.rows_max:        # rule 3
                self.z[i, r], self.pz_x[i, r], self.v[i, r - 1] = z[i], pz_x[i], v_in[i]
                if self.x is not None:
                    self.x[i, r] = x[i]
                self.rows[i], self.k_mark[i] = r + 1, k[i]


def align(rec_z, rec_pz, rows, dead, z0, Nw, Np, H_rev=0):
    """Plan node j is recorder row Nw + j.  The plan's frame: (row - z of row 0) + z0 in float64, rounded once."""
    sl = slice(Nw, Nw + Np + 1)
    origin = rec_z[:, :1].astype(np.float64)
    shift = lambda t: ((t[:, sl].astype(np.float64) - origin) + np.asarray(z0, np.float64)[:, None, :]).astype(f32)
    d = rec_z - rec_pz
    w_all = np.sqrt((d.astype(np.float64) ** 2).sum(-1))           # float64 norm: compare with a tolerance of float32 spacing
    return {"pz_x": shift(rec_pz), "z_ref": shift(rec_z), "w_true": w_all[:, sl], "completed": (rows == Nw + Np + 1) & (dead == 0),
            "e_past": w_all[:, Nw - H_rev:Nw], "w0": w_all[:, Nw]}


def audit_env(w, min_clear, w_true, pz_x, completed, dead, obs_c, obs_r):
    """audit_env in NumPy float64: plan.audit over the completed plans + the counts."""
    done = np.asarray(completed, bool)
    B, n = len(done), int(done.sum())
    out = {"plans": B, "completed": n, "terminated": int(np.asarray(dead, bool).sum()), "nodes": int(np.shape(w_true)[1])}
    keys = ("coverage_by_node", "coverage", "covered_plans", "predicted_safe", "actually_safe", "table", "w_true_mean", "w_true_max")
    if n == 0:
        return {**out, **{k: None for k in keys}, "covered_plans_of_all": 0.0}
    w, wt, pz = (np.asarray(a, np.float64)[done] for a in (w, w_true, pz_x))
    cov = w >= wt
    pred = np.asarray(min_clear, np.float64)[done] >= 0
    act = np.ones(n, bool)
    for c, r in zip(obs_c, obs_r):
        act &= ~(np.sqrt(((pz - np.asarray(c, np.float64)) ** 2).sum(-1)) < r).any(1)
    sh = lambda m: float(np.mean(m))
    out.update({"coverage_by_node": [float(x) for x in cov.mean(0)], "coverage": sh(cov), "covered_plans": sh(cov.all(1)),
                "predicted_safe": sh(pred), "actually_safe": sh(act),
                "table": {"safe_safe": sh(pred & act), "safe_unsafe": sh(pred & ~act), "unsafe_safe": sh(~pred & act),
                          "unsafe_unsafe": sh(~pred & ~act)},
                "w_true_mean": float(wt.mean()), "w_true_max": float(wt.max()),
                "covered_plans_of_all": float(cov.all(1).sum()) / B})
    return out
