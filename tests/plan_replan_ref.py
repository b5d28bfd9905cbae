"""NumPy restatement of replanning on the legged env (csrc/lg_traj.h tg_replan, lg_traj_replan; legged_gym_dev_amd/tube/plan_env.py
rom_schedule): tests/plan_env_ref.PlanLaw with a per-env plan base, the replan law one float32 rounding at
a time -- skip, the base, inputs 0 outside the plan -- and the generator's clock schedule.  Nothing here imports the library."""
import numpy as np

from tests.plan_env_ref import PlanLaw, f32


class ReplanLaw(PlanLaw):
    """PlanLaw whose env i reads node k - k0[i] of its plan.  k0 is 0 after a reset and after set_plans; replan moves it."""

    def __init__(self, plans, Nw, rom_dt, dt):
        super().__init__(plans, Nw, rom_dt, dt)
        self.k0 = np.zeros(self.n, np.int64)
        self.traj = np.zeros((self.n, self.Nw, 2), f32)

    def reset(self, ids, z):
        super().reset(ids, z)
        self.k0[np.atleast_1d(ids)] = 0

    def set_plans(self, plans):
        self.plans = np.asarray(plans, f32)
        self.n_nodes = self.plans.shape[1]
        self.k0[:] = 0

    def input(self, i):
        j = int(self.k[i]) - int(self.k0[i])
        return self.plans[i, j] if 0 <= j < self.n_nodes else np.zeros(2, f32)

    def interpolate(self, i):
        """tg_window_interpolate at the env's stored t, k: a + (b - a) * frac / rom_dt, frac = t - (k - 1) rom_dt."""
        frac = f32(self.t[i] - f32(f32(self.k[i] - f32(1)) * self.rom_dt))
        a, b = self.win[i, :-1], self.win[i, 1:]
        self.traj[i] = (a + (((b - a).astype(f32) * frac).astype(f32) / self.rom_dt).astype(f32)).astype(f32)

    def step(self):
        stepped = super().step()
        for i in range(self.n):
            self.interpolate(i)
        return stepped

    def replan(self, v, skip=None):
        """lg_traj_replan: v (n, n_nodes, 2) with n_nodes >= 1.  The node count is shared, so it changes for skipped envs too; their
        window, plan rows, base, v_in and trajectory stay."""
        v = np.asarray(v, f32)
        n_nodes = v.shape[1]
        assert 1 <= n_nodes <= 64
        if self.plans.shape[1] < 64:                               # the context's padded buffer: rows past the node count are kept
            self.plans = np.concatenate([self.plans, np.zeros((self.n, 64 - self.plans.shape[1], 2), f32)], 1)
        self.n_nodes = n_nodes
        for i in range(self.n):
            if skip is not None and skip[i]:
                continue
            self.plans[i, :n_nodes] = v[i]
            u = np.zeros(2, f32)
            for p in range(2, self.Nw + 1):
                u = v[i, p - 2] if p - 2 < n_nodes else np.zeros(2, f32)
                self.win[i, p] = (self.win[i, p - 1] + (self.rom_dt * u).astype(f32)).astype(f32)
            if self.Nw >= 2:
                self.v_in[i] = u
            self.k0[i] = int(self.k[i]) - (self.Nw - 1)
            self.interpolate(i)


def clock_schedule(Nw, rom_dt, dt, n_rom_steps):
    """Env steps up to and including each of the next n_rom_steps ROM steps after a reset: PlanLaw's clock alone."""
    law = PlanLaw(np.zeros((1, 0, 2), f32), Nw, rom_dt, dt)
    law.reset([0], [[0, 0]])
    out, steps = [], 0
    while len(out) < n_rom_steps:
        steps += 1
        if law.step()[0]:
            out.append(steps)
            steps = 0
    return out
