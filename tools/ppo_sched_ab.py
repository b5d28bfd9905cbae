"""A/B worker for the learner's host side: everything the scheduling of the PPO update decides, dumped so that two builds of the
library can be compared array for array on the paths bench.py --dump-outputs does not take (it runs the flat MLP only).

    LG_HIP_LIB=<library> python tools/ppo_sched_ab.py --out DIR      one fresh process per library
    python tools/ppo_sched_ab.py --compare DIR_A DIR_B [--report FILE]

Every path runs with lg_ppo_set_deterministic and fixed seeds, two updates, and dumps parameters, Adam moments, the rollout
storage and `stats`.  Shapes: the smallest at which the scheduling can still go wrong -- 100 envs (off the 32-row act tile) x 4
steps x 2 minibatches, 48 observations with a privileged critic row of 53 (both off the 32-column pad), hidden [64, 32]:
  ff/<act>/<widths>/act<0|1>/ov<0|1>   feed-forward: fused head (elu, equal last widths) against k_loss (tanh; unequal last widths),
                                       fused act on / off, overlap on / off
  head/<label>/cv<0|1>                 every head path of tests/ppo_loss_ref.PATHS (generic, fused32, fused64, net128_12, net128_16 at
                                       16 actions), `use_clipped_value_loss` on / off: 200 rows = three 64-row tiles and one of 8
  rnn/ov<0|1>                          the same sizes with an LSTM of 32
  runner                               one runner iteration at 64 envs with the env attached (fused rollout epilogue)
--compare counts the arrays that differ in shape, dtype or bytes (a non-finite value equals itself).  One array is order-dependent by
construction: a finished episode takes the ring slot `atomicAdd(ep_ring_count, 1) % 100`, so which (return, length) pair lands in
which slot is the arrival order of the step's lanes and differs between two runs of one library.  The dump therefore holds the
ring twice: `ep_ring` with its (return, length) columns sorted, which is compared like every other array, and `ep_ring_slots` as
it lies in memory, whose differences are counted apart and do not fail the comparison."""
import argparse
import glob
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N, T, MB, O, OC, A = 100, 4, 2, 48, 53, 12
ALG = dict(num_learning_epochs=2, num_mini_batches=MB, value_loss_coef=1.0, clip_param=0.2, entropy_coef=0.01, learning_rate=1e-3,
           gamma=0.99, lam=0.95, desired_kl=0.01, max_grad_norm=1.0, schedule="adaptive", use_clipped_value_loss=True)


ORDER_DEPENDENT = ("ep_ring_slots",)


def learner_state(ppo):
    import torch
    torch.cuda.synchronize()
    out = {k: v.detach().cpu().numpy().copy() for k, v in ppo.t.items()}
    ring = out["ep_ring"]
    out["ep_ring_slots"] = ring
    out["ep_ring"] = ring[:, np.lexsort((ring[1], ring[0]))]
    return out


def run_learner(activation, actor_hidden, critic_hidden, fused_act, overlap, recurrent, A=A, clipped_value=True):
    import torch
    from legged_gym_dev_amd.rl.ppo import HipPPO
    torch.manual_seed(7)
    policy = dict(actor_hidden_dims=actor_hidden, critic_hidden_dims=critic_hidden, activation=activation, init_noise_std=1.0,
                  rnn_type="lstm", rnn_hidden_size=32, rnn_num_layers=1)
    ppo = HipPPO(N, O, OC, A, policy, dict(ALG, use_clipped_value_loss=clipped_value), T, device="cuda:0", seed=3,
                 policy_class_name="ActorCriticRecurrent" if recurrent else "ActorCritic")
    ppo.set_deterministic(True)
    ppo.lib.lg_ppo_debug_set_overlap(ppo.ctx, overlap)
    ppo.lib.lg_ppo_debug_set_fused_act(ppo.ctx, fused_act)
    took_fused_act = int(ppo.lib.lg_ppo_debug_get_fused_act(ppo.ctx))
    g = torch.Generator().manual_seed(11)
    for _ in range(2):
        for t in range(T):
            obs = torch.randn(N, O, generator=g).cuda()
            cobs = torch.randn(N, OC, generator=g).cuda()
            ppo.act(obs, cobs)
            rew = torch.randn(N, generator=g).cuda()
            dones = (torch.rand(N, generator=g) < 0.1).to(torch.uint8).cuda()
            tos = (torch.rand(N, generator=g) < 0.05).to(torch.uint8).cuda()
            ppo.process_env_step(rew, dones, {"time_outs": tos})
        ppo.compute_returns(torch.randn(N, OC, generator=g).cuda())
        ppo.update()
    out = learner_state(ppo)
    out["took_fused_act"] = np.array([took_fused_act], np.int32)
    return out


def run_runner():
    import torch
    import bench
    env, runner = bench.make_runner(64, [128, 64, 32], "cuda:0", 0, 1)
    runner.ppo.set_deterministic(True)
    runner.rollout()
    runner.ppo.update(runner._grad_reduce)
    out = learner_state(runner.ppo)
    out["env_obs"] = env.obs_buf.detach().cpu().numpy().copy()
    return out


def paths():
    for act, ah, ch in (("elu", [64, 32], [64, 32]), ("tanh", [64, 32], [64, 32]), ("elu", [64, 32], [64, 16])):
        for fa in (1, 0):
            for ov in (1, 0):
                yield (f"ff_{act}_{ah[-1]}-{ch[-1]}_act{fa}_ov{ov}", lambda act=act, ah=ah, ch=ch, fa=fa, ov=ov: run_learner(act, ah, ch, fa, ov, False))
    from tests.ppo_loss_ref import PATHS
    for label, (hidden, critic, act) in PATHS.items():
        for cv in (1, 0):
            yield (f"head_{label}_cv{cv}", lambda hidden=hidden, critic=critic, act=act, label=label, cv=cv: run_learner(
                act, hidden, critic or hidden, 1, 1, False, A=16 if label == "net128_16" else 12, clipped_value=bool(cv)))
    for ov in (1, 0):
        yield f"rnn_ov{ov}", lambda ov=ov: run_learner("elu", [64, 32], [64, 32], 0, ov, True)
    yield "runner", run_runner


def compare(a, b, report):
    lines, total = [], 0
    names = sorted(os.path.basename(f) for f in glob.glob(os.path.join(a, "*.npz")))
    assert names and names == sorted(os.path.basename(f) for f in glob.glob(os.path.join(b, "*.npz"))), "the two dumps hold different paths"
    for n in names:
        za, zb = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert sorted(za.files) == sorted(zb.files), n
        diff = [k for k in za.files if za[k].shape != zb[k].shape or za[k].dtype != zb[k].dtype or za[k].tobytes() != zb[k].tobytes()]
        bad = [k for k in diff if k not in ORDER_DEPENDENT]
        total += len(bad)
        extra = f"  fused act taken: {int(za['took_fused_act'][0])}" if "took_fused_act" in za.files else ""
        extra += "  (ring slots in another order)" if len(diff) > len(bad) else ""
        lines.append(f"{n[:-4]:34s} arrays {len(za.files) - len(ORDER_DEPENDENT):3d}  differ {len(bad):3d}{extra}" + (f"  {bad}" if bad else ""))
    lines.append(f"arrays that differ in all: {total}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if report:
        open(report, "w").write(text)
    return 1 if total else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="DIR")
    ap.add_argument("--report")
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(compare(args.compare[0], args.compare[1], args.report))
    os.makedirs(args.out, exist_ok=True)
    for name, fn in paths():
        np.savez(os.path.join(args.out, name + ".npz"), **fn())
        print("dumped", name, flush=True)


if __name__ == "__main__":
    main()
