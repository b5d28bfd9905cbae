#!/usr/bin/env python3
"""Cost of the empirical observation normalisation (rl/obs_norm.py, lg_obs_norm_*) on one MI355X, 4096
envs, by the protocol of tools/bench_obs_history.py.
    step_off / step_on    HIP-event time per env.step of anymal_c_flat over --steps steps, the median of --repeats, alone and
                          followed by one training compute of obs_buf (W = 48)
    train_us / frozen_us  the training (two launches) and the frozen (one launch) compute alone, back to back, on random rows:
                          W = 48, the pair 240 / 48 (flat history beside the single frame) and the pair 427 / 245 (rough history
                          beside a privileged row)
    priv_alone            lg_priv_obs_compute alone, back to back: the yardstick of section 10.17, measured in the same run
    learn_off / learn_on  one PPO iteration (rollout() + update() between two events), ms, [512, 256, 128], without and with
                          runner.empirical_normalization
Every timing is between two HIP events on the current stream, after a warm-up of the same shape.

    python tools/bench_obs_norm.py [--repeats 3] [--envs 4096] [--steps 200] [--out profiles/obs_norm_bench.txt]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
DEV = "cuda:0"
SHAPES = [(48,), (240, 48), (427, 245)]

NOTES = """\
# train_us: k_obs_norm_stats + k_obs_norm_apply (update, then normalise), frozen_us: k_obs_norm_apply alone; a pair shares the launches
# learn_*_ms: rollout() + ppo.update() of OnPolicyRunner between two HIP events, [512, 256, 128], median of max(repeats, 5)
# priv_alone_us: lg_priv_obs_compute back to back, terms obs,friction,base_mass,feet_contact,feet_air_time (DESIGN.md 10.17)
# the bench.py comparison against the parent commit is kept in profiles/obs_norm_bench_vs_parent.txt
"""


def resource_note():
    """The k_obs_norm_* lines of tools/kernel_resources.py as comments (empty when the LLVM tools are not there)."""
    import subprocess
    try:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "kernel_resources.py"), "k_obs_norm"], capture_output=True,
                             text=True, timeout=120).stdout.split("\n")
        rows = [l.split() for l in out if l.startswith("k_obs_norm")]
        return "".join("# {} resources (tools/kernel_resources.py k_obs_norm): vgpr {}, agpr {}, sgpr {}, scratch {}, lds {}\n".format(
            r[0].split("(")[0], *r[-5:]) for r in rows)
    except Exception:
        return ""


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obs_norm_bench.txt"))
    a = ap.parse_args()
    import torch
    from bench_obs_history import TERMS, event_us, make
    from legged_gym_dev_amd.rl.obs_norm import HipObsNormalizer, ObsNormSpec, compute_pair
    from legged_gym_dev_amd.rl.runner import OnPolicyRunner
    from legged_gym_dev_amd.utils.helpers import class_to_dict
    out = {"envs": a.envs, "steps": a.steps, "repeats": a.repeats}
    # env.step alone and followed by the training compute
    env, _ = make("anymal_c_flat", a.envs)
    env.reset()
    g = torch.Generator().manual_seed(1)
    act = (torch.rand(a.envs, env.num_actions, generator=g) - 0.5).to(env.device)
    norm = HipObsNormalizer(ObsNormSpec(int(env.num_obs)), a.envs, DEV)
    out["step_off_us"], out["step_off_all"] = event_us(lambda: env.step(act), a.steps, a.repeats)
    out["step_on_us"], out["step_on_all"] = event_us(lambda: (env.step(act), norm.compute(env.obs_buf, True)), a.steps, a.repeats)
    out["step_adds_us"] = round(out["step_on_us"] - out["step_off_us"], 3)
    norm.close()
    env.close()
    env, _ = make("anymal_c_flat", a.envs, terms=TERMS)
    env.reset()
    out["priv_alone_us"], out["priv_alone_all"] = event_us(env._priv.compute, a.steps, a.repeats)
    env.close()
    # the computes alone
    for widths in SHAPES:
        hs = [HipObsNormalizer(ObsNormSpec(w), a.envs, DEV) for w in widths]
        xs = [torch.randn(a.envs, w, generator=g).to(DEV) * 3.0 + 1.0 for w in widths]
        res = {"bytes_read_and_written": sum(2 * a.envs * w * 4 for w in widths)}
        for key, update in (("train", True), ("frozen", False)):
            fn = (lambda: hs[0].compute(xs[0], update)) if len(hs) == 1 else (lambda: compute_pair(hs[0], xs[0], hs[1], xs[1], update))
            res[key + "_us"], res[key + "_all"] = event_us(fn, a.steps, a.repeats)
        out["compute_" + "_".join(str(w) for w in widths)] = res
        for h in hs:
            h.close()
    # one PPO iteration without and with the switch
    for on in (False, True):
        env, train_cfg = make("anymal_c_flat", a.envs)
        train_cfg.policy.actor_hidden_dims = train_cfg.policy.critic_hidden_dims = [512, 256, 128]
        train_cfg.runner.empirical_normalization = on
        torch.manual_seed(1)
        runner = OnPolicyRunner(env, class_to_dict(train_cfg), None, device=DEV)
        ms, every = event_us(lambda: (runner.rollout(), runner.ppo.update(runner._grad_reduce)), 1, max(a.repeats, 5))
        key = "learn_on" if on else "learn_off"
        out[key + "_ms"], out[key + "_all"] = round(ms / 1e3, 3), [round(v / 1e3, 3) for v in every]
        env.close()
        runner.ppo.close()
    out["learn_adds_ms"] = round(out["learn_on_ms"] - out["learn_off_ms"], 3)
    text = json.dumps(out) + "\n"
    print(text, end="")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(f"# tools/bench_obs_norm.py --repeats {a.repeats} --envs {a.envs} --steps {a.steps}\n" + text + NOTES + resource_note())


if __name__ == "__main__":
    main()
