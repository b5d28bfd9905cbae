#!/usr/bin/env python3
"""Cost of the actor's observation history (envs/base/obs_history.py, lg_obs_hist_*) on one MI355X:
4096 envs of anymal_c_flat with H = 5 (W = 240) and of anymal_c_rough with H = 5, columns 0:48 (W = 427).
    step_off / step_on   HIP-event time per env.step over --steps steps, the median of --repeats, without and with the history
    hist_alone           lg_obs_hist_compute alone, back to back
    priv_alone           lg_priv_obs_compute alone, back to back (terms obs,friction,base_mass,feet_contact,feet_air_time), and
    post_step            lg_post_physics_step alone, back to back: the yardsticks of section 10.17, measured in the same run
    learn_off / learn_on one PPO iteration (rollout() + update() between two events), ms, [512, 256, 128], per case: the
                         history's launches plus the wider first layer of the actor
Every timing is between two HIP events on the env's stream, after a warm-up of the same shape.

    python tools/bench_obs_history.py [--repeats 3] [--envs 4096] [--steps 200] [--out profiles/obs_history_bench.txt]
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
CASES = {"anymal_c_flat": (5, None), "anymal_c_rough": (5, [[0, 48]])}


NOTES = """\
# learn_*_ms: rollout() + ppo.update() of OnPolicyRunner between two HIP events, [512, 256, 128], median of max(repeats, 5);
#   fused_act: lg_ppo_debug_get_fused_act with the history on (1: the one-launch act took the shape)
# post_step_us: lg_post_physics_step back to back = k_post_step + its single-workgroup epilogue; priv_alone_us: lg_priv_obs_compute
#   back to back, terms obs,friction,base_mass,feet_contact,feet_air_time (the yardsticks of DESIGN.md 10.17, same run)
# the bench.py comparison against the parent commit is kept in profiles/obs_history_bench_vs_parent.txt
"""


def resource_note():
    """The k_obs_history line of tools/kernel_resources.py as a comment (empty when the LLVM tools are not there)."""
    import subprocess
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_obs_history"], capture_output=True,
                             text=True, timeout=120).stdout.split("\n")
        row = [l for l in out if l.startswith("k_obs_history")][0].split()
        return "# k_obs_history resources (tools/kernel_resources.py k_obs_history): vgpr {}, agpr {}, sgpr {}, scratch {}, lds {}\n".format(*row[-5:])
    except Exception:
        return ""


def write_profile(path, header, text):
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        f.write(header + text + NOTES + resource_note())


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


def make(task, n, length=1, columns=None, terms=()):
    from legged_gym_dev_amd.envs import task_registry
    from legged_gym_dev_amd.utils import get_args
    args = get_args(["--task", task, "--num_envs", str(n), "--headless"])
    args.sim_device = args.rl_device = DEV
    env_cfg, train_cfg = (copy.deepcopy(c) for c in task_registry.get_cfgs(task))
    env_cfg.env.num_envs = n
    env_cfg.obs_history.length, env_cfg.obs_history.columns = length, columns
    env_cfg.privileged_obs.terms = list(terms)
    env, _ = task_registry.make_env(name=task, args=args, env_cfg=env_cfg)
    return env, train_cfg


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_history_bench.txt"))
    a = ap.parse_args()
    import torch
    from legged_gym_dev_amd.rl.runner import OnPolicyRunner
    from legged_gym_dev_amd.utils.helpers import class_to_dict
    out = {"envs": a.envs, "steps": a.steps, "repeats": a.repeats}
    for task, (H, columns) in CASES.items():
        res = {"length": H, "columns": columns}
        for on in (False, True):
            env, _ = make(task, a.envs, H if on else 1, columns)
            env.reset()
            g = torch.Generator().manual_seed(1)
            act = (torch.rand(a.envs, env.num_actions, generator=g) - 0.5).to(env.device)
            key = "on" if on else "off"
            res["step_" + key + "_us"], res["step_" + key + "_all"] = event_us(lambda: env.step(act), a.steps, a.repeats)
            if on:
                res["width"] = int(env.num_actor_obs)
                res["row_bytes"] = int(env.num_actor_obs) * a.envs * 4
                res["hist_alone_us"], res["hist_alone_all"] = event_us(env._hist.compute, a.steps, a.repeats)
                res["post_step_us"], res["post_step_all"] = event_us(lambda: env.core.call("post_physics_step"), a.steps, a.repeats)
            env.close()
        env, _ = make(task, a.envs, terms=TERMS)                     # the privileged row's launch, the other yardstick
        env.reset()
        res["priv_alone_us"], res["priv_alone_all"] = event_us(env._priv.compute, a.steps, a.repeats)
        env.close()
        res["step_adds_us"] = round(res["step_on_us"] - res["step_off_us"], 3)
        # one PPO iteration with and without the history, the bench line's policy
        for on in (False, True):
            env, train_cfg = make(task, a.envs, H if on else 1, columns)
            train_cfg.policy.actor_hidden_dims = train_cfg.policy.critic_hidden_dims = [512, 256, 128]
            torch.manual_seed(1)
            runner = OnPolicyRunner(env, class_to_dict(train_cfg), None, device=DEV)
            if on:
                res["fused_act"] = int(runner.ppo.lib.lg_ppo_debug_get_fused_act(runner.ppo.ctx))
            ms, every = event_us(lambda: (runner.rollout(), runner.ppo.update(runner._grad_reduce)), 1, max(a.repeats, 5))
            key = "learn_on" if on else "learn_off"
            res[key + "_ms"], res[key + "_all"] = round(ms / 1e3, 3), [round(v / 1e3, 3) for v in every]
            env.close()
            runner.ppo.close()
        res["learn_adds_ms"] = round(res["learn_on_ms"] - res["learn_off_ms"], 3)
        out[task] = res
    text = json.dumps(out) + "\n"
    print(text, end="")
    write_profile(a.out, f"# tools/bench_obs_history.py --repeats {a.repeats} --envs {a.envs} --steps {a.steps}\n", text)


if __name__ == "__main__":
    main()
