#!/usr/bin/env python3
"""Timing of the ROM-on-ROM simulator on the default configuration (8192 envs, T = 200 records = 400 env steps):

  (a) HipRomSim.collect_epoch: one launch per epoch
  (b) the stepwise path: scripts/collect_trajectory_data.py::collect on HipRomSim (one launch per env step + the policy launch)
  (c) a torch-eager restatement of CustomSim with its generator on the same device (our own code, below): the baseline
  (d) (a) + the device-to-host copy + the pickle: where an epoch's wall time goes

Median of 3 after a warm-up run, every timing closed by a device synchronise.  Prints the figures and the resources of the new
kernels (tools/kernel_resources.py romsim).

    python tools/bench_rom_sim.py [--num_envs 8192 --T 200] > profiles/rom_sim_bench.txt
"""
import argparse
import os
import pickle
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
import torch  # noqa: E402

from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg  # noqa: E402


class EagerRomSim:
    """CustomSim + TrajectoryGenerator + DoubleSingleTracking as plain torch ops on the device, batched over envs the way the
    reference batches them (index tensors for the envs that resample / step)."""

    def __init__(self, cfg, device):
        self.c, self.dev = cfg, device
        n, tg = cfg.env.num_envs, cfg.trajectory_generator
        f = dict(device=device, dtype=torch.float32)
        self.n, self.N, self.dt, self.rom_dt = n, tg.N, cfg.env.model.dt, cfg.rom.dt
        self.vmin, self.vmax = torch.tensor(cfg.rom.v_min, **f), torch.tensor(cfg.rom.v_max, **f)
        self.amin, self.amax = torch.tensor(cfg.env.model.v_min, **f), torch.tensor(cfg.env.model.v_max, **f)
        self.zmin, self.zmax = torch.tensor(cfg.env.model.z_min, **f), torch.tensor(cfg.env.model.z_max, **f)
        self.lo, self.hi = torch.tensor(cfg.init_state.default_noise_lower, **f), torch.tensor(cfg.init_state.default_noise_upper, **f)
        self.maxd = torch.tensor(cfg.domain_rand.max_rom_distance, **f)
        z = lambda *s: torch.zeros(s, **f)
        self.w, self.t_final, self.t, self.k = z(n, 4), z(n), z(n), z(n)
        self.const, self.extreme, self.ramp_t0, self.ramp_v0 = z(n, 2), z(n, 2), z(n), z(n, 2)
        self.ramp_v1 = (self.vmax - self.vmin) * torch.rand(n, 2, device=device) + self.vmin
        self.sin_mag, self.sin_freq, self.sin_off, self.sin_mean = z(n, 2), z(n, 2), z(n, 2), z(n, 2)
        self.traj, self.vtraj, self.v = z(n, self.N + 1, 2), z(n, self.N, 2), z(n, 2)
        self.stationary = torch.zeros(n, dtype=torch.bool, device=device)
        self.root, self.trajectory = z(n, 4), z(n, self.N, 2)
        self.all = torch.arange(n, device=device)
        self.A = torch.tensor([[1.0, 0, self.dt, 0], [0, 1.0, 0, self.dt], [0, 0, 1.0, 0], [0, 0, 0, 1.0]], **f)
        self.B = torch.tensor([[0, 0], [0, 0], [self.dt, 0], [0, self.dt]], **f)

    def uni(self, lo, hi, size):
        return (hi - lo) * torch.rand(*size, device=self.dev) + lo

    def resample(self, idx):
        if len(idx) == 0:
            return
        m, tg = len(idx), self.c.trajectory_generator
        self.const[idx] = self.uni(self.vmin, self.vmax, (m, 2))
        self.ramp_v0[idx] = self.ramp_v1[idx]
        self.ramp_v1[idx] = self.uni(self.vmin, self.vmax, (m, 2))
        self.ramp_t0[idx] = self.t_final[idx]
        arr = torch.stack((self.vmin.expand(m, 2), torch.zeros(m, 2, device=self.dev), self.vmax.expand(m, 2)), -1)
        self.extreme[idx] = torch.gather(arr, 2, torch.randint(0, 3, (m, 2, 1), device=self.dev)).squeeze(-1)
        self.sin_mag[idx] = self.uni(torch.zeros_like(self.vmax), (self.vmax - self.vmin) / 2, (m, 2))
        self.sin_mean[idx] = self.uni(self.vmin + self.sin_mag[idx], self.vmax - self.sin_mag[idx], (m, 2))
        self.sin_freq[idx] = self.uni(tg.freq_low, tg.freq_high, (m, 2))
        self.sin_off[idx] = self.uni(-torch.pi, torch.pi, (m, 2))
        self.t_final[idx] += self.uni(tg.t_low, tg.t_high, (m,))
        w = torch.rand(m, 4, device=self.dev)
        if tg.weight_samp_cls == "UniformWeightSamplerNoRamp":
            w[:, 1] = 0
        self.w[idx] = w / w.sum(-1, keepdim=True)
        self.stationary[idx] = torch.rand(m, device=self.dev) < tg.prob_stationary

    def input(self, t):
        self.resample(torch.nonzero(t > self.t_final).reshape(-1))
        ramp = self.ramp_v0 + (self.ramp_v1 - self.ramp_v0) * ((t - self.ramp_t0) / (self.t_final - self.ramp_t0))[:, None]
        sinus = self.sin_mag * torch.sin(self.sin_freq * t[:, None] + self.sin_off) + self.sin_mean
        v = self.w[:, 0:1] * self.const + self.w[:, 1:2] * ramp + self.w[:, 2:3] * self.extreme + self.w[:, 3:4] * sinus
        v[self.stationary] = 0
        return v

    def rom_step(self, idx, inc=False):
        self.v = self.input(self.t)
        znext = self.traj[idx, -1] + self.rom_dt * self.v[idx]
        self.traj[idx, :-1] = self.traj[idx, 1:].clone()
        self.traj[idx, -1] = znext
        self.vtraj[idx, :-1] = self.vtraj[idx, 1:].clone()
        self.vtraj[idx, -1] = self.v[idx]
        self.k[idx] += 1
        if inc:
            self.t[idx] += self.rom_dt

    def get_trajectory(self):
        a, b = self.traj[:, :-1], self.traj[:, 1:]
        return a + (b - a) * (self.t - (self.k - 1) * self.rom_dt)[:, None, None] / self.rom_dt

    def obs(self):
        return torch.cat((self.root.clone(), self.trajectory[:, 0], self.vtraj[:, 1].clone()), 1)

    def step(self, a):
        self.root = (self.A @ self.root.T).T + (self.B @ a.T).T
        self.rom_step(self.all[self.t >= self.k * self.rom_dt - 1e-5])
        self.t += self.dt
        self.trajectory = self.get_trajectory().clone()
        return self.obs()

    def reset(self):
        dr = self.c.domain_rand
        self.root = self.uni(self.lo, self.hi, (self.n, 4))
        p = self.root[:, :2].clone()
        if dr.randomize_rom_distance:
            mask = torch.rand(self.n, device=self.dev) > dr.zero_rom_dist_llh
            p[mask] += self.uni(-self.maxd, self.maxd, (int(mask.sum()), 2))
        self.traj.zero_(); self.vtraj.zero_()
        self.traj[:, -1] = p
        self.k[:] = -self.N
        self.t = self.k * self.rom_dt
        self.t_final = self.k * self.rom_dt
        self.resample(self.all)
        for _ in range(self.N):
            self.rom_step(self.all, inc=True)
        return self.step(torch.zeros(self.n, 2, device=self.dev))

    def policy(self, o):
        x = o[:, :4]
        u = self.c.controller.Kp * (o[:, 4:6] - x[:, :2]) + self.c.controller.Kd * (o[:, 6:] - x[:, 2:])
        hi = torch.min(self.amax, (self.zmax[2:] - x[:, 2:]) / self.dt)
        lo = torch.max(self.amin, (self.zmin[2:] - x[:, 2:]) / self.dt)
        return torch.max(torch.min(u, hi), lo)

    def collect_epoch(self, T):
        n, f = self.n, dict(device=self.dev)
        z, pz, v = torch.zeros(n, T + 1, 2, **f), torch.zeros(n, T + 1, 2, **f), torch.zeros(n, T, 2, **f)
        done = torch.zeros(n, T, dtype=torch.bool, **f)
        o = self.reset()
        z[:, 0], pz[:, 0] = self.traj[:, 0], self.root[:, :2]
        for t in range(T):
            k = self.k.clone()
            while bool(torch.any(self.k == k)):
                o = self.step(self.policy(o))
            v[:, t], z[:, t + 1], pz[:, t + 1] = self.v, self.trajectory[:, 0], self.root[:, :2]
        return {"z": z, "v": v, "pz_x": pz, "done": done}


def timed(fn, reps=3):
    fn()                                               # warm-up
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num_envs", type=int, default=8192)
    ap.add_argument("--T", type=int, default=200)
    a = ap.parse_args()
    import collect_trajectory_data as ctd
    dev = "cuda:0"
    cfg = RomSimCfg()
    cfg.env.num_envs = a.num_envs
    cfg.env.episode_length_s = a.T * cfg.rom.dt + 1e-6
    print(f"ROM-on-ROM simulator, {a.num_envs} envs, T = {a.T} records ({int(round(cfg.rom.dt / cfg.env.model.dt)) * a.T} env steps), "
          f"{torch.cuda.get_device_name(0)}; median of 3 after a warm-up run, each timing closed by a device synchronise")
    sim = HipRomSim(cfg, seed=0, device=dev)
    tmp = tempfile.mkdtemp()

    def leg_d():
        rec = sim.collect_epoch(a.T)
        host = {k: v.cpu().numpy() for k, v in rec.items()}
        with open(os.path.join(tmp, "epoch.pickle"), "wb") as f:
            pickle.dump(host, f)
    ta, ra = timed(lambda: sim.collect_epoch(a.T))
    tb, rb = timed(lambda: ctd.collect(sim, sim.policy, 1))
    td, rd = timed(leg_d)
    sim.close()
    eager = EagerRomSim(cfg, dev)
    tc, rc = timed(lambda: eager.collect_epoch(a.T))
    ms = lambda r: " ".join(f"{x * 1e3:.2f}" for x in r)
    print(f"(a) collect_epoch, one launch            {ta * 1e3:10.3f} ms   [{ms(ra)}]")
    print(f"(b) stepwise through collect()           {tb * 1e3:10.3f} ms   [{ms(rb)}]   (includes its device-to-host copies)")
    print(f"(c) torch-eager restatement              {tc * 1e3:10.3f} ms   [{ms(rc)}]")
    print(f"(d) (a) + device-to-host copy + pickle   {td * 1e3:10.3f} ms   [{ms(rd)}]")
    print(f"(c) / (a) = {tc / ta:.1f}   (b) / (a) = {tb / ta:.1f}   (d) - (a) = {(td - ta) * 1e3:.3f} ms of copy and pickle")
    if ta >= tc:
        print("(a) does NOT beat (c)")
    sys.stdout.flush()
    subprocess.call([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "romsim"])


if __name__ == "__main__":
    main()
