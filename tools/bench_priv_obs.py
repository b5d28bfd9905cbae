#!/usr/bin/env python3
"""Cost of the privileged observations (envs/base/privileged_obs.py, lg_priv_obs_*) on one MI355X:
4096 envs of anymal_c_flat and of anymal_c_rough, terms obs,friction,base_mass,feet_contact,feet_air_time.
    step_off / step_on   HIP-event time per env.step over --steps steps, the median of --repeats, without and with the terms
    priv_alone           lg_priv_obs_compute alone, back to back
    post_step            lg_post_physics_step alone, back to back: k_post_step plus its single-workgroup epilogue, the yardstick
                         (the new launch reads a subset of what k_post_step reads and does no Philox or reward work)
    learn_off / learn_on one runner.learn iteration (24-step rollout + update), ms, anymal_c_flat with the bench line's policy
Every timing is between two HIP events on the env's stream, after a warm-up of the same shape.

    python tools/bench_priv_obs.py [--repeats 3] [--envs 4096] [--steps 200] [--out profiles/priv_obs_bench.txt]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
DEV = "cuda:0"
TERMS = ["obs", "friction", "base_mass", "feet_contact", "feet_air_time"]


def event_us(fn, reps, repeats):
    """Median over `repeats` of the HIP-event time of `reps` calls of fn, in microseconds per call."""
    import torch
    out = []
    for k in range(repeats + 1):                                    # the first round is the warm-up
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(reps):
            fn()
        e.record()
        e.synchronize()
        if k:
            out.append(s.elapsed_time(e) * 1e3 / reps)
    out.sort()
    return round(out[len(out) // 2], 3), [round(v, 3) for v in out]


def make(task, n, terms):
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.utils import get_args
    args = get_args(["--task", task, "--num_envs", str(n), "--headless"])
    args.sim_device = args.rl_device = DEV
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(task))
    env_cfg.env.num_envs = n
    env_cfg.privileged_obs.terms = list(terms)
    env, _ = task_registry.make_env(name=task, args=args, env_cfg=env_cfg)
    return env, train_cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "priv_obs_bench.txt"))
    a = ap.parse_args()
    import torch
    from legged_gym_dev_amd.rl.runner import OnPolicyRunner
    from legged_gym_dev_amd.utils.helpers import class_to_dict
    out = {"envs": a.envs, "steps": a.steps, "repeats": a.repeats, "terms": TERMS}
    for task in ("anymal_c_flat", "anymal_c_rough"):
        res = {}
        for on in (False, True):
            env, _ = make(task, a.envs, TERMS if on else [])
            env.reset()
            g = torch.Generator().manual_seed(1)
            act = (torch.rand(a.envs, env.num_actions, generator=g) - 0.5).to(env.device)
            key = "on" if on else "off"
            res["step_" + key + "_us"], res["step_" + key + "_all"] = event_us(lambda: env.step(act), a.steps, a.repeats)
            if on:
                res["width"] = int(env.num_privileged_obs)
                res["row_bytes_written"] = int(env.num_privileged_obs) * a.envs * 4
                res["priv_alone_us"], res["priv_alone_all"] = event_us(env._priv.compute, a.steps, a.repeats)
                res["post_step_us"], res["post_step_all"] = event_us(lambda: env.core.call("post_physics_step"), a.steps, a.repeats)
            env.close()
        res["step_adds_us"] = round(res["step_on_us"] - res["step_off_us"], 3)
        out[task] = res
    # one PPO iteration with and without the asymmetric critic
    learn = {}
    for on in (False, True):
        env, train_cfg = make("anymal_c_flat", a.envs, TERMS if on else [])
        torch.manual_seed(1)
        runner = OnPolicyRunner(env, class_to_dict(train_cfg), None, device=DEV)
        ms, every = event_us(lambda: (runner.rollout(), runner.ppo.update(runner._grad_reduce)), 1, max(a.repeats, 5))
        learn["learn_on_ms" if on else "learn_off_ms"], learn["learn_on_all" if on else "learn_off_all"] = round(ms / 1e3, 3), [round(v / 1e3, 3) for v in every]
        env.close()
        runner.ppo.close()
    learn["learn_adds_ms"] = round(learn["learn_on_ms"] - learn["learn_off_ms"], 3)
    out["learn_anymal_c_flat"] = learn
    text = json.dumps(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/bench_priv_obs.py --repeats {a.repeats} --envs {a.envs} --steps {a.steps}\n" + text)


if __name__ == "__main__":
    main()
