#!/usr/bin/env python3
"""What per-plan scenes cost: three launches on the gap problem, N = 50, for the l1 kind and the reference
one-shot shape (H_rev 10, 130 -> 128 x 2 Softplus(5) -> 50),
    score      lg_plan_score at B = 65536, no optional output
    mppi       one MPPI iteration (score + update) at P x K = 64 x 512
    descend    the evaluate-and-step launch lg_plan_descend_step (what = 3) at B = 4096
each in four variants that alternate on one device, a fresh process per variant and round:
    parent     the parent commit's library (--parent_lib, a liblegged_hip.so built from that commit)
    this       this tree's library, no scenes: the instantiations the entries without scenes launch
    uniform    this tree's library with Scenes.repeat(problem): the problem's own goal and two obstacles through the scene rows --
               what the shared-problem launches would cost if the scene row were the only code path
    scenes     this tree's library with heterogeneous scenes (random_scenes, 0..8 obstacles, a goal per scene)
Every timing ends in a device synchronise; median of --repeats runs after a warm-up of the same shape.  Per launch and variant the
tool prints every round's median, and the verdict for `this` against `parent`: the spread is the largest (max - min) / min over the
rounds of one variant of that launch, and `this` lies inside it where |median(this) - median(parent)| / median(parent) <= spread.

    python tools/bench_plan_scenes.py --parent_lib PATH [--rounds 3] [--repeats 3] [--out profiles/plan_scenes_bench.txt]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, HF, HR, U, NL, BETA = 50, 50, 10, 128, 2, 5.0
LAUNCHES = ("score", "mppi", "descend")


def worker(a):
    """One variant in this process: a JSON line per (launch, kind)."""
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_plan import DEV, timed
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.trainer import initial_params
    model = HipTubeModel(initial_params(HR + 2 * (HR + HF), HF, U, NL, 1), activation="softplus", softplus_beta=BETA, horizon=(HF, HR), device=DEV)
    with_scenes = a.worker in ("uniform", "scenes")

    def scenes(p, S):
        if not with_scenes:
            return None
        if a.worker == "uniform":
            sc = pl.Scenes.repeat(p, S)
            sc.to(DEV)
            return sc
        lo, hi = [min(s, g) - 0.25 for s, g in zip(p.start, p.goal)], [max(s, g) + 0.25 for s, g in zip(p.start, p.goal)]
        one = pl.random_scenes(min(S, 4096), 0, p.start, n_obs=(0, 8), centre_box=(lo, hi), radius=(0.05, 0.3),
                               goal_box=([g - 0.5 for g in p.goal], [g + 0.5 for g in p.goal]), margin=0.05)
        sc = one.take(torch.arange(S).numpy() % one.S)                 # 4096 distinct scenes, repeated on the host
        sc.to(DEV)                                                      # the upload is not part of a timing
        return sc
    try:
        for kind, mdl, Hr in (("l1", None, 0), ("nn", model, HR)):
            p = pl.PlanProblem.named("gap", N=N, H_rev=Hr, tube_kind=kind)
            _, v0 = pl.warm_start("interpolate", p.start, p.goal, N, p.dt)
            res = {"variant": a.worker, "kind": kind}
            B = a.plans
            v = pl.perturb(v0, 0.05, B, 0, [-0.3, -0.3], [0.3, 0.3]).to(DEV)
            z0 = torch.tensor(p.start, device=DEV).repeat(B, 1)
            scorer, sc = pl.HipPlanScorer(mdl, p, device=DEV), scenes(p, B)
            kw = {} if sc is None else {"scenes": sc}
            res["score"] = timed(lambda: scorer.score(z0, v, want=(), **kw), a.repeats)[0]
            kw = {} if not with_scenes else {"scenes": scenes(p, a.P)}
            mp = pl.HipMppiPlanner(mdl, p, pl.MppiCfg(K=a.K, iters=1, sigma=0.1, seed=1), device=DEV, **kw)
            zP = torch.tensor(p.start, device=DEV).repeat(a.P, 1)
            st = mp.state(zP, mp.warm_start(zP.cpu().numpy()))
            res["mppi"] = timed(lambda: mp.step(st, 1, what=3, reset=True), a.repeats)[0]
            Bg = a.grad_plans
            kw = {} if not with_scenes else {"scenes": scenes(p, Bg)}
            gp = pl.HipGradPlanner(mdl, p, pl.GradCfg(iters=1), device=DEV, **kw)
            sg = gp.state(z0[:Bg], v[:Bg])
            res["descend"] = timed(lambda: gp.step(sg, 0, what=3, reset=True), a.repeats)[0]
            print(json.dumps(res), flush=True)
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib", default=None, help="liblegged_hip.so of the parent commit; without it the parent column is left out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plans", type=int, default=65536)
    ap.add_argument("--grad_plans", type=int, default=4096)
    ap.add_argument("--P", type=int, default=64)
    ap.add_argument("--K", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_scenes_bench.txt"))
    ap.add_argument("--worker", choices=["parent", "this", "uniform", "scenes"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    variants = (["parent"] if a.parent_lib else []) + ["this", "uniform", "scenes"]
    rows = {}
    for rnd in range(a.rounds):
        for var in variants:                                            # alternating: one fresh process after the other
            env = dict(os.environ)
            env.pop("LG_HIP_LIB", None)
            if var == "parent":
                env["LG_HIP_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", var, "--repeats", str(a.repeats), "--plans", str(a.plans),
                   "--grad_plans", str(a.grad_plans), "--P", str(a.P), "--K", str(a.K)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout
            for ln in out.splitlines():
                if ln.startswith("{"):
                    r = json.loads(ln)
                    for launch in LAUNCHES:
                        rows.setdefault((r["kind"], launch), {}).setdefault(var, []).append(r[launch])
    lines = [f"tools/bench_plan_scenes.py: gap problem, N = {N}; score B = {a.plans}, mppi {a.P} x {a.K}, descend B = {a.grad_plans}; "
             f"{a.rounds} rounds alternating, a fresh process each; ms, median of {a.repeats} after a warm-up, closed by a device synchronise"]
    for (kind, launch), by in sorted(rows.items()):
        spread = max((max(t) - min(t)) / min(t) for t in by.values())
        med = {k: statistics.median(t) for k, t in by.items()}
        rec = {"kind": kind, "launch": launch, **{k + "_ms": [round(x, 4) for x in t] for k, t in by.items()},
               **{k + "_median_ms": round(m, 4) for k, m in med.items()}, "spread": round(spread, 4)}
        if "parent" in med:
            rec["this_over_parent"] = round(med["this"] / med["parent"], 4)
            rec["this_inside_spread"] = abs(med["this"] - med["parent"]) / med["parent"] <= spread
            rec["scenes_over_parent"] = round(med["scenes"] / med["parent"], 4)
        rec["uniform_over_this"] = round(med["uniform"] / med["this"], 4)
        rec["scenes_over_this"] = round(med["scenes"] / med["this"], 4)
        lines.append(json.dumps(rec))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
