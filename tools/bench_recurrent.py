"""Training throughput of the recurrent policy (runner.policy_class_name = 'ActorCriticRecurrent'): env-steps/s of full PPO
iterations (rollout + update) on a registered task, and the mean episode return of each iteration.  bench.py measures the
feed-forward headline and stays as it is; this is its recurrent counterpart.

  python tools/bench_recurrent.py --envs 4096 --rnn 256 --hidden 512,256,128 --iters 5 --warmup 2
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

import bench  # noqa: E402
from legged_gym_dev_amd.rl.runner import OnPolicyRunner  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--task", default="anymal_c_flat")
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--rnn", type=int, default=256)
    ap.add_argument("--hidden", default="512,256,128")
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--policy", default="ActorCriticRecurrent", help="ActorCritic: the same run on the feed-forward learner (A/B)")
    a = ap.parse_args()
    hidden = [int(v) for v in a.hidden.split(",")]
    env, runner = bench.make_runner(a.envs, hidden, "cuda:0", 0, 1, task=a.task)
    cfg = {"runner": dict(runner.cfg, policy_class_name=a.policy), "algorithm": runner.alg_cfg,
           "policy": dict(runner.policy_cfg, rnn_type="lstm", rnn_hidden_size=a.rnn, rnn_num_layers=1), "seed": 1}
    runner.ppo.close()
    torch.manual_seed(1)
    runner = OnPolicyRunner(env, cfg, log_dir=None, device="cuda:0")
    os.environ["LG_LOG_SYNC"] = "1"
    runner.learn(a.warmup, init_at_random_ep_len=True)
    rets = []
    torch.cuda.synchronize()
    t0 = time.time()
    for _ in range(a.iters):
        runner.learn(1)
        rets.append(sum(runner.rewbuffer) / max(len(runner.rewbuffer), 1))
    torch.cuda.synchronize()
    dt = time.time() - t0
    steps = a.iters * runner.num_steps_per_env * env.num_envs
    print(json.dumps({"task": a.task, "policy": a.policy, "envs": a.envs, "rnn_hidden": a.rnn, "hidden": hidden, "iters": a.iters,
                      "env_steps_per_s": steps / dt, "iter_ms": 1e3 * dt / a.iters, "mean_return": rets}))


if __name__ == "__main__":
    main()
