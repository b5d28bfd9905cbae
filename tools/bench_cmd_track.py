#!/usr/bin/env python3
"""Time of the command tracker (legged_gym_dev_amd/tube/cmd_track.py, lg_cmdtrack_*): one MI355X,
4096 envs of anymal_c_flat, a freshly initialised policy (the timing does not depend on the weights), T = 1000 env steps.
    step      lg_cmdtrack_step alone: 10 T calls per timing
    collect   an epoch of collect(): policy + env.step + one tracker launch per env step, per env step.  The loop runs under
              torch.cuda.set_sync_debug_mode("error"): a device-to-host copy or any other synchronising call inside it raises
    bare      the same env steps with no tracker; collect - bare is what the tracker adds to an env step
    eager     the only route before the tracker: the torch-eager transcription of data_collection_velocity.py:112-156 on the
              device (the generator's get_input_t with its nonzero(), SingleInt2D.f and des_pose_vel, quat2yaw as the atan2 it
              is, yaw2rot, wrap_angles, the 3 x 3 gain, the clip, the observation write, the record lines), per env step with the
              same policy and env
Every timing ends in a device synchronise; the median of --repeats runs after a warm-up run of the same shape.

    python tools/bench_cmd_track.py [--repeats 3] [--envs 4096] [--T 1000] [--out profiles/cmd_track_bench.txt]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TASK, DEV = "anymal_c_flat", "cuda:0"


def median_of(fn, repeats):
    fn()                                                            # warm-up: the same shape
    ts = sorted(fn() for _ in range(repeats))
    return ts[len(ts) // 2], [round(t, 3) for t in ts]


class EagerGen:
    """TrajectoryGenerator (trajopt/rom_dynamics.py:441-566, torch backend) as far as get_input_t reaches, op for op."""

    def __init__(self, n, v_min, v_max, t_low, t_high, freq_low, freq_high, prob_stationary, dev):
        import torch
        z = lambda *s: torch.zeros(s, device=dev)
        self.n, self.dev = n, dev
        self.v_min, self.v_max = torch.tensor(v_min, device=dev), torch.tensor(v_max, device=dev)
        self.t_low, self.t_high, self.freq_low, self.freq_high, self.prob_stationary = t_low, t_high, freq_low, freq_high, prob_stationary
        self.weights, self.t_final = z(n, 4), z(n)
        self.sample_hold_input, self.extreme_input, self.ramp_v_start = z(n, 2), z(n, 2), z(n, 2)
        self.ramp_t_start = z(n)
        self.ramp_v_end = self.uniform(self.v_min, self.v_max, (n, 2))
        self.sin_mag, self.sin_freq, self.sin_off, self.sin_mean = z(n, 2), z(n, 2), z(n, 2), z(n, 2)
        self.stationary_inds = z(n).bool()

    def uniform(self, low, high, size):
        import torch
        return (high - low) * torch.rand(*size, device=self.dev) + low

    def resample(self, idx):
        import torch
        if len(idx) > 0:
            m = len(idx)
            v_min, v_max = self.v_min.expand(m, 2), self.v_max.expand(m, 2)
            self.sample_hold_input[idx, :] = self.uniform(v_min, v_max, (m, 2))
            self.ramp_v_start[idx, :] = self.ramp_v_end[idx, :]
            self.ramp_v_end[idx, :] = self.uniform(v_min, v_max, (m, 2))
            self.ramp_t_start[idx] = self.t_final[idx]
            arr = torch.concatenate((v_min[:, :, None], torch.zeros_like(v_min)[:, :, None], v_max[:, :, None]), dim=-1)
            mask = torch.arange(3, device=self.dev)[None, None, :] == torch.randint(0, 3, (m, 2, 1), device=self.dev)
            self.extreme_input[idx, :] = arr[mask].reshape(v_min.shape)
            self.sin_mag[idx, :] = self.uniform(torch.zeros_like(v_max), (v_max - v_min) / 2, (m, 2))
            self.sin_mean[idx, :] = self.uniform(v_min + self.sin_mag[idx, :], v_max - self.sin_mag[idx, :], (m, 2))
            self.sin_freq[idx, :] = self.uniform(torch.tensor([self.freq_low], device=self.dev), torch.tensor([self.freq_high], device=self.dev), (m, 2))
            self.sin_off[idx, :] = self.uniform(torch.tensor([-torch.pi], device=self.dev), torch.tensor([torch.pi], device=self.dev), (m, 2))
            self.t_final[idx] += (self.t_high - self.t_low) * torch.rand(m, device=self.dev) + self.t_low
            w = torch.rand(m, 4, device=self.dev)
            self.weights[idx, :] = w / torch.sum(w, dim=-1, keepdim=True)
            self.stationary_inds[idx] = self.uniform(torch.tensor([0.0], device=self.dev), torch.tensor([1.0], device=self.dev),
                                                     (m, 1)).squeeze(-1) < self.prob_stationary

    def get_input_t(self, t):
        import torch
        idx = torch.nonzero(t > self.t_final).reshape((-1,))
        self.resample(idx)
        ramp = self.ramp_v_start + (self.ramp_v_end - self.ramp_v_start) * ((t - self.ramp_t_start) / (self.t_final - self.ramp_t_start))[:, None]
        sinus = self.sin_mag * torch.sin(self.sin_freq * t[:, None] + self.sin_off) + self.sin_mean
        return self.weights[:, 0][:, None] * self.sample_hold_input + self.weights[:, 1][:, None] * ramp + \
            self.weights[:, 2][:, None] * self.extreme_input + self.weights[:, 3][:, None] * sinus


def eager_epoch(env, policy, gen, Kp, u_min, u_max, T, track_yaw):
    """data_collection_velocity.py:101-156 in torch on the device, env-major records.  Returns milliseconds of the step loop."""
    import torch
    n, dev, dt = env.num_envs, env.device, float(env.dt)
    A, B = torch.eye(2, device=dev), torch.eye(2, device=dev) * dt
    z, pz_x = torch.zeros(n, T + 1, 2, device=dev), torch.zeros(n, T + 1, 2, device=dev)
    v, u, done = torch.zeros(n, T, 2, device=dev), torch.zeros(n, T, 3, device=dev), torch.zeros(n, T, dtype=torch.bool, device=dev)
    with torch.no_grad():
        env.reset()
        obs = env.get_observations()
        base = env.root_states
        z[:, 0], pz_x[:, 0] = base[:, :2], base[:, :2]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for t in range(T):
            vt = gen.get_input_t(t * torch.ones(n, device=dev) * dt)
            zt = z[:, t]
            zt_p1 = (A @ zt.T).T + (B @ vt.T).T
            des_pose = torch.hstack((zt, torch.arctan2(vt[:, 1], vt[:, 0])[:, None]))
            des_vel = torch.hstack((vt, torch.zeros(n, 1, device=dev)))
            q = base[:, 3:7]
            yaw = torch.atan2(2 * (q[:, 0] * q[:, 1] + q[:, 3] * q[:, 2]), q[:, 3] ** 2 + q[:, 0] ** 2 - q[:, 1] ** 2 - q[:, 2] ** 2)
            robot_pose = torch.hstack((base[:, :2], yaw[:, None]))
            cy, sy = torch.cos(yaw), torch.sin(yaw)
            y2r = torch.zeros(n, 2, 2, device=dev)
            y2r[:, 0, 0], y2r[:, 0, 1], y2r[:, 1, 0], y2r[:, 1, 1] = cy, sy, -sy, cy
            err_global = des_pose - robot_pose
            err_global[:, 2] = ((err_global[:, 2] + math.pi) % (2 * math.pi)) - math.pi if track_yaw else 0
            err_local = err_global.clone()
            err_local[:, :2] = torch.squeeze(y2r @ err_global[:, :2][:, :, None], -1)
            des_vel_local = des_vel.clone()
            des_vel_local[:, :2] = torch.squeeze(y2r @ des_vel[:, :2, None], -1)
            ut = des_vel_local + (Kp @ err_local.T).T
            ut = torch.clip(ut, u_min, u_max)
            obs[:, 9:12] = ut
            actions = policy(obs.detach())
            obs, _, _, dones, _ = env.step(actions.detach())
            base = env.root_states
            done[:, t] = dones
            u[:, t], v[:, t] = ut, vt
            z[:, t + 1] = zt_p1
            z[dones, t + 1] = base[dones, :2]
            pz_x[:, t + 1] = base[:, :2]
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cmd_track_bench.txt"))
    a = ap.parse_args()
    import copy
    import torch
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.tube import cmd_track as ct
    from legged_gym_dev_amd.utils import get_args
    args = get_args(["--task", TASK, "--num_envs", str(a.envs), "--headless"])
    args.sim_device = args.rl_device = DEV
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(TASK))
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = False
    runner, _ = task_registry.make_alg_runner(env=env, name=TASK, args=args, train_cfg=train_cfg, log_root=None)
    policy = runner.get_inference_policy(device=env.device)
    T, n = a.T, env.num_envs
    cfg = ct.CmdTrackCfg.from_env(env, kind=ct.RANDOM, track_yaw=True)
    tracker = ct.HipCommandTracker(env, cfg)

    def steps_alone():
        tracker.begin(T)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            for t in range(T):
                tracker.step(t)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e2                     # milliseconds per T calls

    def epoch(track):
        with torch.no_grad():
            env.reset()
            tracker.begin(T)
            obs = env.get_observations()
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")                 # no device-to-host copy inside an epoch: it would raise
            try:
                t0 = time.perf_counter()
                for t in range(T):
                    obs = env.step(policy(obs.detach()).detach())[0]
                    if track:
                        tracker.step(t)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
    gen = EagerGen(n, cfg.rom_v_min, cfg.rom_v_max, cfg.t_low, cfg.t_high, cfg.freq_low, cfg.freq_high, cfg.prob_stationary, env.device)
    Kp = torch.tensor(cfg.Kp, device=env.device).reshape(3, 3)
    u_min, u_max = torch.tensor(cfg.u_min, device=env.device), torch.tensor(cfg.u_max, device=env.device)
    out = {"envs": n, "T": T, "repeats": a.repeats}
    for name, fn in (("step", steps_alone), ("collect", lambda: epoch(True)), ("bare", lambda: epoch(False)),
                     ("eager", lambda: eager_epoch(env, policy, gen, Kp, u_min, u_max, T, True)),
                     ("collect2", lambda: epoch(True)), ("bare2", lambda: epoch(False))):            # the loops once more, alternating
        ms, every = median_of(fn, a.repeats)
        out[name + "_us_per_step"], out[name + "_all_ms"] = round(ms * 1e3 / T, 3), every
    out["tracker_adds_us_per_env_step"] = round(out["collect2_us_per_step"] - out["bare2_us_per_step"], 3)
    out["eager_adds_us_per_env_step"] = round(out["eager_us_per_step"] - out["bare2_us_per_step"], 3)
    out["sync_debug_mode_error"] = "no synchronising call inside the collect epochs"
    rec = tracker.records()
    out["done_rate"] = round(float(rec["done"].float().mean()), 5)
    tracker.close()
    runner.ppo.close()
    env.close()
    text = json.dumps(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/bench_cmd_track.py --repeats {a.repeats} --envs {a.envs} --T {a.T}\n" + text)


if __name__ == "__main__":
    main()
