#!/usr/bin/env python3
"""Time of tracking a batch of plans on the legged env (legged_gym_dev_amd/tube/plan_env.py): one MI355X,
4096 envs of anymal_c_flat_trajectory, Nw = 10, Np = 50, a freshly initialised policy (the timing does not depend on the weights).
    record    (a) track_env's loop: env.step(policy(obs)) + one k_traj_record launch per env step, no host read
    bare      (b) the same env steps with no recording; (a) - (b) is the recorder's cost per env step
    collect   (c) the only route to such a record before the recorder: the loop body of scripts/collect_trajectory_data.py::collect()
              -- one device-to-host read per env step and indexed torch copies per ROM step -- on a Square env for the same number
              of ROM steps with the same policy; with --parent_lib on that library (LG_HIP_LIB), else on this one
    post      lg_post_physics_step alone, kind PLAN (this library) against kind Square (--parent_lib, else this library), in
              alternating child processes; the spread over the children is reported
Every timing ends in a device synchronise; median of --repeats runs after a warm-up of the same shape.  Each measurement runs in
a fresh child process (LG_HIP_LIB is read when the library loads).

    python tools/bench_plan_env.py [--repeats 3] [--parent_lib PATH] [--out profiles/plan_env_bench.txt]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "legged_gym_dev_amd", "scripts"))
TASK, DEV = "anymal_c_flat_trajectory", "cuda:0"


def timed(fn, repeats):
    import torch
    fn()                                # warm-up: the same shape
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3, [round(t * 1e3, 3) for t in ts]


def make(a, cls):
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.tube.plan_env import plan_env_cfg
    from legged_gym_dev_amd.utils import get_args
    env_cfg, train_cfg = plan_env_cfg(TASK, a.envs)
    env_cfg.trajectory_generator.cls = cls
    env_cfg.trajectory_generator.N = a.Nw
    env_cfg.env.num_observations = 9 + 2 * a.Nw + 36
    args = get_args(["--task", TASK, "--num_envs", str(a.envs), "--headless"])
    args.sim_device = args.rl_device = DEV
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = False
    runner, _ = task_registry.make_alg_runner(env=env, name=TASK, args=args, train_cfg=train_cfg, log_root=None)
    return env, runner, runner.get_inference_policy(device=env.device)


def child_track(a):
    """(a) and (b) on one env: the loop of track_env with and without the recorder."""
    import torch
    from legged_gym_dev_amd.tube import plan_env as pe
    env, runner, policy = make(a, "PlanTrajectoryGenerator")
    g = torch.Generator().manual_seed(0)
    v = (torch.rand(a.envs, a.Np, 2, generator=g) * 0.4 - 0.2).to(DEV)
    _, _, Nw, S, steps = pe.check_track(env, v, torch.zeros(a.envs, 2, device=DEV))
    rec = pe.TrajRecorder(env, Nw + a.Np + 1)

    def loop(record):
        with torch.no_grad():
            env.reset()
            env.traj_gen.set_plans(v)
            env.traj_gen.reset(env.rom.proj_z(env.root_states).clone())
            rec.begin()
            obs = env.get_observations()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(steps):
                obs = env.step(policy(obs.detach()).detach())[0]
                if record:
                    rec.step()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3
    out = {"mode": "track", "envs": a.envs, "Nw": Nw, "Np": a.Np, "env_steps": steps}
    for name, record in (("record", True), ("bare", False), ("record", True), ("bare", False)):     # alternating; the first pair warms up
        ts = sorted(loop(record) for _ in range(a.repeats))
        out[name + "_ms"], out[name + "_all_ms"] = round(ts[len(ts) // 2], 3), [round(t, 3) for t in ts]
    out["completed"] = int(((rec.rows == rec.rows_max) & (rec.dead == 0)).sum())
    runner.ppo.close()
    env.close()
    return out


def child_collect(a):
    """(c): collect()'s loop body on a Square env for Nw + Np ROM steps (the rows track_env records)."""
    import torch
    env, runner, policy = make(a, "SquareTrajectoryGenerator")
    rom, tg, N, T = env.rom, env.traj_gen, env.num_envs, a.Nw + a.Np
    x_n = env.get_state().shape[1]

    def loop():
        with torch.no_grad():
            x = torch.zeros((N, T + 1, x_n), device=env.device)
            z, pz_x = torch.zeros((N, T + 1, rom.n), device=env.device), torch.zeros((N, T + 1, rom.n), device=env.device)
            v, done = torch.zeros((N, T, rom.m), device=env.device), torch.zeros((N, T), dtype=torch.bool, device=env.device)
            obs, _ = env.reset()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x[:, 0], pz_x[:, 0], z[:, 0] = env.get_state(), rom.proj_z(env.root_states), tg.trajectory[:, 0, :]
            n = 0
            for t in range(T):
                k = tg.k.clone()
                dones = None
                while bool(torch.any(tg.k == k)):                 # the host read per env step
                    obs, _, _, dones, _ = env.step(policy(obs.detach()).detach())
                    n += 1
                d = dones.clone()
                proj = rom.proj_z(env.root_states)
                done[:, t], v[:, t], x[:, t + 1] = d, tg.v, env.get_state()
                z[:, t + 1] = tg.get_trajectory()[:, 0, :]
                z[d, t + 1] = proj[d]
                pz_x[:, t + 1] = proj
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, n
    loop()
    runs = sorted(loop() for _ in range(a.repeats))
    out = {"mode": "collect", "lib": os.environ.get("LG_HIP_LIB", "this"), "rom_steps": T, "env_steps": runs[len(runs) // 2][1],
           "collect_ms": round(runs[len(runs) // 2][0], 3), "collect_all_ms": [round(r[0], 3) for r in runs]}
    runner.ppo.close()
    env.close()
    return out


def child_post(a):
    """lg_post_physics_step alone, 200 calls per timing, on an env of --kind."""
    import torch
    env, runner, _ = make(a, a.kind)
    env.reset()
    if a.kind == "PlanTrajectoryGenerator":
        g = torch.Generator().manual_seed(0)
        env.traj_gen.set_plans((torch.rand(a.envs, a.Np, 2, generator=g) * 0.4 - 0.2).to(DEV))
        env.traj_gen.reset(env.rom.proj_z(env.root_states).clone())

    def run():
        for _ in range(200):
            env.episode_length_buf.zero_()
            env.core.call("post_physics_step")
    ms, every = timed(run, a.repeats)
    runner.ppo.close()
    env.close()
    return {"mode": "post", "kind": a.kind, "lib": os.environ.get("LG_HIP_LIB", "this"), "post_step_us": round(ms * 1e3 / 200, 3),
            "all_us": [round(t * 1e3 / 200, 3) for t in every]}


def spawn(a, mode, lib=None, kind=None):
    env = dict(os.environ)
    if lib:
        env["LG_HIP_LIB"] = lib
    cmd = [sys.executable, os.path.abspath(__file__), "--child", mode, "--repeats", str(a.repeats), "--envs", str(a.envs), "--Nw", str(a.Nw),
           "--Np", str(a.Np)] + (["--kind", kind] if kind else [])
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"{mode} child failed ({r.returncode}):\n{r.stdout[-2000:]}\n{r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--Nw", type=int, default=10)
    ap.add_argument("--Np", type=int, default=50)
    ap.add_argument("--parent_lib", default=None, help="a liblegged_hip.so built from the parent commit, for (c) and the Square post-step")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_env_bench.txt"))
    ap.add_argument("--child", choices=["track", "collect", "post"], default=None)
    ap.add_argument("--kind", default="PlanTrajectoryGenerator")
    a = ap.parse_args()
    if a.child:
        print(json.dumps({"track": child_track, "collect": child_collect, "post": child_post}[a.child](a)), flush=True)
        return
    lines = []
    trk = spawn(a, "track")
    col = spawn(a, "collect", lib=a.parent_lib)
    lines += [json.dumps(trk), json.dumps(col)]
    per_step = (trk["record_ms"] - trk["bare_ms"]) * 1e3 / trk["env_steps"]
    lines.append(json.dumps({"recorder_us_per_env_step": round(per_step, 3), "collect_over_record": round(col["collect_ms"] / trk["record_ms"], 3),
                             "record_us_per_env_step": round(trk["record_ms"] * 1e3 / trk["env_steps"], 3),
                             "collect_us_per_env_step": round(col["collect_ms"] * 1e3 / col["env_steps"], 3)}))
    posts = []
    for _ in range(3):                                             # alternating children
        posts.append(spawn(a, "post", kind="PlanTrajectoryGenerator"))
        posts.append(spawn(a, "post", lib=a.parent_lib, kind="SquareTrajectoryGenerator"))
    lines += [json.dumps(p) for p in posts]
    for kind in ("PlanTrajectoryGenerator", "SquareTrajectoryGenerator"):
        us = sorted(p["post_step_us"] for p in posts if p["kind"] == kind)
        lines.append(json.dumps({"kind": kind, "post_step_us_median": us[1], "min": us[0], "max": us[-1]}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/bench_plan_env.py --repeats {a.repeats} --envs {a.envs} --Nw {a.Nw} --Np {a.Np}"
                f"{' --parent_lib <parent build>' if a.parent_lib else ''}\n" + text)


if __name__ == "__main__":
    main()
