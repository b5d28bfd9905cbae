#!/usr/bin/env python3
"""Time of replanning on the legged env (legged_gym_dev_amd/tube/plan_env.py closed_loop_env): one MI355X,
4096 envs of anymal_c_flat_trajectory (Nw = 10), the `gap` problem with the `l1` tube, MPPI at K = 512 and 30 iterations, a freshly
initialised policy (the timing does not depend on the weights).  Per ROM step:
    env       the env steps of one ROM interval, each env.step(policy(obs)) + one recorder launch
    planner   one planner.plan from the window's point 1 with the previous plan shifted as the warm start
    replan    the lg_traj_replan launch alone (--launches of them per timing)
    set_plans lg_traj_set_plans, the nearest launch that existed before, the same way
    loop      closed_loop_env itself over --H ROM steps, per ROM step
Every timing ends in a device synchronise; median of --repeats runs after a warm-up of the same shape.

    python tools/bench_plan_replan.py [--repeats 3] [--out profiles/plan_replan_bench.txt]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--K", type=int, default=512)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--N", type=int, default=50)
    ap.add_argument("--H", type=int, default=10)
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_replan_bench.txt"))
    a = ap.parse_args()
    import torch
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube import plan_env as pe
    from legged_gym_dev_amd.utils import get_args
    env_cfg, train_cfg = pe.plan_env_cfg(TASK, a.envs)
    args = get_args(["--task", TASK, "--num_envs", str(a.envs), "--headless"])
    args.sim_device = args.rl_device = DEV
    env, _ = task_registry.make_env(name=TASK, args=args, env_cfg=env_cfg)
    train_cfg.runner.resume = False
    runner, _ = task_registry.make_alg_runner(env=env, name=TASK, args=args, train_cfg=train_cfg, log_root=None)
    policy = runner.get_inference_policy(device=env.device)
    p = pl.PlanProblem.named("gap", tube_kind="l1", N=a.N)
    planner = pl.HipMppiPlanner(None, p, pl.MppiCfg(K=a.K, iters=a.iters), device=DEV)
    B, Nw, sched = pe.check_closed_loop(env, p, a.H)
    S = pe.rom_substeps(env)
    rec = pe.TrajRecorder(env, a.H + 2)
    lines = []
    with torch.no_grad():
        env.reset()
        env.traj_gen.set_plans(torch.zeros(B, 0, 2, device=DEV))
        env.traj_gen.reset(env.rom.proj_z(env.root_states).clone())
        rec.begin()
        z0 = torch.tensor(p.start, dtype=torch.float32, device=DEV).repeat(B, 1)
        e, v_prev = torch.zeros(B, p.H_rev, device=DEV), torch.zeros(B, p.H_rev, 2, device=DEV)
        sol = planner.plan(z0, None, e, v_prev, None)
        warm = pl.shift_plan(sol["v"])
        state = {"obs": env.get_observations()}

        def env_steps():
            for _ in range(S):
                state["obs"] = env.step(policy(state["obs"].detach()).detach())[0]
                rec.step()

        def launches(fn):
            def run():
                for _ in range(a.launches):
                    fn()
            return run
        ms, every = timed(env_steps, a.repeats)
        lines.append({"what": "env", "env_steps": S, "ms_per_rom_step": round(ms, 3), "all_ms": every})
        ms, every = timed(lambda: planner.plan(z0, warm, e, v_prev, None), a.repeats)
        lines.append({"what": "planner", "K": a.K, "iters": a.iters, "N": a.N, "ms_per_rom_step": round(ms, 3), "all_ms": every})
        v = sol["v"].contiguous()
        ms, every = timed(launches(lambda: env.traj_gen.replan(v, skip=rec.dead)), a.repeats)
        lines.append({"what": "replan", "launches": a.launches, "us_per_launch": round(ms * 1e3 / a.launches, 3),
                      "all_us": [round(t * 1e3 / a.launches, 3) for t in every]})
        ms, every = timed(launches(lambda: env.traj_gen.set_plans(v)), a.repeats)
        lines.append({"what": "set_plans", "launches": a.launches, "us_per_launch": round(ms * 1e3 / a.launches, 3),
                      "all_us": [round(t * 1e3 / a.launches, 3) for t in every]})
    res = {}

    def loop():
        res["out"] = pe.closed_loop_env(env, policy, planner, a.H)
    ms, every = timed(loop, a.repeats)
    out = res["out"]
    lines.append({"what": "loop", "H": a.H, "schedule": sched, "ms_per_rom_step": round(ms / (a.H + 1), 3), "all_ms": every,
                  "completed": int(out["completed"].sum()), "reset": int(out["dead"].sum())})
    lines.insert(0, {"envs": B, "Nw": Nw, "problem": "gap", "tube": "l1"})
    runner.ppo.close()
    env.close()
    text = "\n".join(json.dumps(ln) for ln in lines) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/bench_plan_replan.py --repeats {a.repeats} --envs {a.envs} --K {a.K} --iters {a.iters} --N {a.N} --H {a.H}\n" + text)


if __name__ == "__main__":
    main()
