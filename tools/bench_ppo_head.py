"""lg_ppo_minibatch_backward on every head path, parent library against this tree's, side by side on one device.

    python tools/bench_ppo_head.py --parent_lib <liblegged_hip.so of the parent commit> [--rounds 5] [--out FILE]

The quantity is the one bench.py's gemm_roofline brackets: HIP events around each lg_ppo_minibatch_backward inside a real update
(begin_update, then epochs x minibatches of {backward, optimiser step}; the update's first minibatch, which gathers for itself, left
out), mean over the update, ms.  4096 envs x 24 steps / 4 minibatches = 24 576 rows, 48 observations; one configuration per head
kernel: [512,256,128] elu with 12 and with 16 actions (k_head_net<128, 12|16> + k_head_finish), [128,64,64] and [128,64,32] elu
(k_head_fused<64|32>), [512,256,128] tanh (k_loss).  Rounds alternate parent, this, parent, ...: a fresh process each (LG_HIP_LIB is read
when the library loads), which runs one warm-up update and one measured update per configuration.  The rule per configuration: this
tree's slowest round must not exceed the parent's slowest round plus the parent's own spread (max - min) over the same rounds."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, T, MB, EPOCHS, O = 4096, 24, 4, 5, 48
CONFIGS = (("net128_12", [512, 256, 128], "elu", 12), ("net128_16", [512, 256, 128], "elu", 16), ("fused64", [128, 64, 64], "elu", 12),
           ("fused32", [128, 64, 32], "elu", 12), ("generic", [512, 256, 128], "tanh", 12))
ALG = dict(num_learning_epochs=EPOCHS, num_mini_batches=MB, value_loss_coef=1.0, clip_param=0.2, entropy_coef=0.01, learning_rate=1e-3,
           gamma=0.99, lam=0.95, desired_kl=0.01, max_grad_norm=1.0, schedule="adaptive", use_clipped_value_loss=True)


def timed_update(ppo):
    import torch
    ppo._call("begin_update")
    pairs = []
    for epoch in range(EPOCHS):
        for mb in range(MB):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ppo._call("minibatch_backward", epoch, mb)
            e1.record()
            ppo._call("minibatch_step")
            pairs.append((e0, e1))
    ppo._call("end_update")
    torch.cuda.synchronize()
    return sum(a.elapsed_time(b) for a, b in pairs[1:]) / (len(pairs) - 1)


def worker():
    import torch
    from legged_gym_dev_amd.rl.ppo import HipPPO
    for label, hidden, act, A in CONFIGS:
        torch.manual_seed(7)
        policy = dict(actor_hidden_dims=hidden, critic_hidden_dims=hidden, activation=act, init_noise_std=1.0)
        ppo = HipPPO(N, O, O, A, policy, ALG, T, device="cuda:0", seed=3)
        g = torch.Generator(device="cuda:0").manual_seed(11)
        ms = []
        for _ in range(2):                                  # a warm-up update, then the measured one
            for t in range(T):
                obs = torch.randn(N, O, generator=g, device="cuda:0")
                ppo.act(obs, obs)
                rew = torch.randn(N, generator=g, device="cuda:0")
                dones = (torch.rand(N, generator=g, device="cuda:0") < 0.02).to(torch.uint8)
                ppo.process_env_step(rew, dones, {"time_outs": torch.zeros_like(dones)})
            ppo.compute_returns(torch.randn(N, O, generator=g, device="cuda:0"))
            ms.append(timed_update(ppo))
        print(json.dumps({"config": label, "ms": ms[-1]}), flush=True)
        del ppo


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib", required=True, help="liblegged_hip.so of the parent commit")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report here (profiles/ppo_loss_once_bench.txt holds one, with bench.py's rounds appended)")
    ap.add_argument("--worker", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker()
    ms = {}
    for rnd in range(a.rounds):
        for lib in ("parent", "this"):
            env = dict(os.environ)
            env.pop("LG_HIP_LIB", None)
            if lib == "parent":
                env["LG_HIP_LIB"] = os.path.abspath(a.parent_lib)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", "--parent_lib", a.parent_lib], env=env, check=True,
                                 capture_output=True, text=True, timeout=300).stdout
            for ln in out.splitlines():
                if ln.startswith("{"):
                    r = json.loads(ln)
                    ms.setdefault(r["config"], {}).setdefault(lib, []).append(r["ms"])
            print("round", rnd, lib, "done", flush=True)
    lines = [f"tools/bench_ppo_head.py: lg_ppo_minibatch_backward by HIP events inside a real update, ms per minibatch; {N} envs x {T} steps / {MB} "
             f"minibatches, O = {O}; {a.rounds} rounds alternating parent / this, a fresh process each"]
    ok = True
    for label, hidden, act, A in CONFIGS:
        p, t = ms[label]["parent"], ms[label]["this"]
        limit = max(p) + (max(p) - min(p))
        ok &= max(t) <= limit
        lines.append(json.dumps({"config": label, "hidden": hidden, "activation": act, "A": A, "parent_ms": [round(x, 4) for x in p],
                                 "this_ms": [round(x, 4) for x in t], "parent_min_max": [round(min(p), 4), round(max(p), 4)],
                                 "this_min_max": [round(min(t), 4), round(max(t), 4)], "limit_ms": round(limit, 4), "pass": max(t) <= limit}))
    lines.append("every configuration inside the limit: " + ("yes" if ok else "NO"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    raise SystemExit(main())
