#!/usr/bin/env python3
"""What moving obstacles and a fleet's scenes cost, by the protocol of tools/bench_plan_scenes.py: the
same three launches on the gap problem, N = 50, for the l1 kind and the reference one-shot shape,
    score      lg_plan_score at B = 65536, no optional output
    mppi       one MPPI iteration (score + update) at P x K = 64 x 512
    descend    the evaluate-and-step launch lg_plan_descend_step (what = 3) at B = 4096
with two libraries that alternate on one device, a fresh process per library and round:
    parent     the parent commit's library (--parent_lib, a liblegged_hip.so built from that commit): no scenes, static scenes
    this       this tree's library: no scenes, static scenes (the same heterogeneous random scenes of 0..8 obstacles), and the same
               scenes with a velocity of 0.02 .. 0.08 m/s per obstacle -- the moving rows beside their static twins
and, on this tree's library alone, lg_plan_fleet_scenes at P = 64, 1024, 4096 (robots uniform in a square of 4 sqrt(P) x 0.25 m,
sense radius 1.0, 8 neighbours, no static part) beside one MPPI iteration (l1, K = 512) at the same P, the launch it sits next to.
Every timing ends in a device synchronise; median of --repeats runs after a warm-up of the same shape.  Per row the tool prints
every round's median; for the no-scenes and static-scenes rows the verdict of `this` against `parent`: the spread is the largest
(max - min) / min over the rounds of one library on that row, and `this` lies inside it where |median(this) - median(parent)| /
median(parent) <= spread.  The moving and fleet rows are reported, not bounded.

    python tools/bench_plan_fleet.py --parent_lib PATH [--rounds 3] [--repeats 3] [--out profiles/plan_fleet_bench.txt]
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
FLEET_P = (64, 1024, 4096)


def worker(a):
    """One library in this process: a JSON line per (kind, scenes variant), then the fleet lines."""
    import numpy as np
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from bench_plan import DEV, timed
    from legged_gym_dev_amd.tube import plan as pl
    from legged_gym_dev_amd.tube.model import HipTubeModel
    from legged_gym_dev_amd.tube.trainer import initial_params
    model = HipTubeModel(initial_params(HR + 2 * (HR + HF), HF, U, NL, 1), activation="softplus", softplus_beta=BETA, horizon=(HF, HR), device=DEV)

    def scenes(p, S, variant):
        if variant == "none":
            return None
        lo, hi = [min(s, g) - 0.25 for s, g in zip(p.start, p.goal)], [max(s, g) + 0.25 for s, g in zip(p.start, p.goal)]
        one = pl.random_scenes(min(S, 4096), 0, p.start, n_obs=(0, 8), centre_box=(lo, hi), radius=(0.05, 0.3),
                               goal_box=([g - 0.5 for g in p.goal], [g + 0.5 for g in p.goal]), margin=0.05,
                               speed=(0.02, 0.08))                      # the speeds are drawn after each scene: the static twin is
        if variant == "static":                                         # not the draw without speeds, but these scenes without them
            one = pl.Scenes(one.goal, one.obs_c, one.obs_r, one.n_obs)
        sc = one.take(np.arange(S) % one.S)
        sc.to(DEV)                                                      # the upload is not part of a timing
        return sc
    try:
        for kind, mdl, Hr in (("l1", None, 0), ("nn", model, HR)):
            p = pl.PlanProblem.named("gap", N=N, H_rev=Hr, tube_kind=kind)
            _, v0 = pl.warm_start("interpolate", p.start, p.goal, N, p.dt)
            B, Bg = a.plans, a.grad_plans
            v = pl.perturb(v0, 0.05, B, 0, [-0.3, -0.3], [0.3, 0.3]).to(DEV)
            z0 = torch.tensor(p.start, device=DEV).repeat(B, 1)
            zP = torch.tensor(p.start, device=DEV).repeat(a.P, 1)
            for variant in ("none", "static") + (("moving",) if a.worker == "this" else ()):
                res = {"lib": a.worker, "kind": kind, "scenes": variant}
                kw = lambda S: {} if variant == "none" else {"scenes": scenes(p, S, variant)}
                scorer, skw = pl.HipPlanScorer(mdl, p, device=DEV), kw(B)
                res["score"] = timed(lambda: scorer.score(z0, v, want=(), **skw), a.repeats)[0]
                mp = pl.HipMppiPlanner(mdl, p, pl.MppiCfg(K=a.K, iters=1, sigma=0.1, seed=1), device=DEV, **kw(a.P))
                st = mp.state(zP, mp.warm_start(zP.cpu().numpy()))
                res["mppi"] = timed(lambda: mp.step(st, 1, what=3, reset=True), a.repeats)[0]
                gp = pl.HipGradPlanner(mdl, p, pl.GradCfg(iters=1), device=DEV, **kw(Bg))
                sg = gp.state(z0[:Bg], v[:Bg])
                res["descend"] = timed(lambda: gp.step(sg, 0, what=3, reset=True), a.repeats)[0]
                print(json.dumps(res), flush=True)
        if a.worker == "this":
            p = pl.PlanProblem.named("gap", N=N, H_rev=0, tube_kind="l1")
            for P in FLEET_P:
                g = torch.Generator().manual_seed(P)
                pos = (torch.rand(P, 2, generator=g) * float(np.sqrt(P))).to(DEV)          # about 3 robots within the sense radius of 1.0
                vel = (torch.rand(P, 2, generator=g) - 0.5).to(DEV)
                fleet = pl.FleetScenes(P, pl.FleetCfg(separation=0.2, sense_radius=1.0, max_neighbours=8))
                fleet.to(DEV)
                res = {"lib": "this", "fleet_P": P, "fleet": timed(lambda: fleet.update(pos, vel, 0.1), a.repeats)[0],
                       "neighbours_mean": float(fleet.to(DEV)[1][2].float().mean())}
                mp = pl.HipMppiPlanner(None, p, pl.MppiCfg(K=a.K, iters=1, sigma=0.1, seed=1), device=DEV, scenes=fleet)
                st = mp.state(pos, mp.warm_start(pos.cpu().numpy()))
                res["mppi"] = timed(lambda: mp.step(st, 1, what=3, reset=True), a.repeats)[0]
                print(json.dumps(res), flush=True)
    finally:
        model.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent_lib", default=None, help="liblegged_hip.so of the parent commit; without it the parent rows are left out")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--plans", type=int, default=65536)
    ap.add_argument("--grad_plans", type=int, default=4096)
    ap.add_argument("--P", type=int, default=64)
    ap.add_argument("--K", type=int, default=512)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plan_fleet_bench.txt"))
    ap.add_argument("--worker", choices=["parent", "this"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a)
    rows, fleet = {}, {}
    for rnd in range(a.rounds):
        for lib in (["parent"] if a.parent_lib else []) + ["this"]:     # alternating: one fresh process after the other
            env = dict(os.environ)
            env.pop("LG_HIP_LIB", None)
            if lib == "parent":
                env["LG_HIP_LIB"] = os.path.abspath(a.parent_lib)
            cmd = [sys.executable, os.path.abspath(__file__), "--worker", lib, "--repeats", str(a.repeats), "--plans", str(a.plans),
                   "--grad_plans", str(a.grad_plans), "--P", str(a.P), "--K", str(a.K)]
            out = subprocess.run(cmd, env=env, check=True, capture_output=True, text=True, timeout=300).stdout
            for ln in out.splitlines():
                if not ln.startswith("{"):
                    continue
                r = json.loads(ln)
                if "fleet_P" in r:
                    for k in ("fleet", "mppi", "neighbours_mean"):
                        fleet.setdefault(r["fleet_P"], {}).setdefault(k, []).append(r[k])
                    continue
                for launch in LAUNCHES:
                    rows.setdefault((r["kind"], launch, r["scenes"]), {}).setdefault(lib, []).append(r[launch])
    lines = [f"tools/bench_plan_fleet.py: gap problem, N = {N}; score B = {a.plans}, mppi {a.P} x {a.K}, descend B = {a.grad_plans}; "
             f"{a.rounds} rounds alternating, a fresh process each; ms, median of {a.repeats} after a warm-up, closed by a device synchronise"]
    med = lambda t: statistics.median(t)
    for (kind, launch, variant), by in sorted(rows.items()):
        spread = max((max(t) - min(t)) / min(t) for t in by.values())
        rec = {"kind": kind, "launch": launch, "scenes": variant, **{k + "_ms": [round(x, 4) for x in t] for k, t in by.items()},
               **{k + "_median_ms": round(med(t), 4) for k, t in by.items()}, "spread": round(spread, 4)}
        if "parent" in by:
            rec["this_over_parent"] = round(med(by["this"]) / med(by["parent"]), 4)
            rec["this_inside_spread"] = abs(med(by["this"]) - med(by["parent"])) / med(by["parent"]) <= spread
        if variant == "moving":
            rec["moving_over_static"] = round(med(by["this"]) / med(rows[(kind, launch, "static")]["this"]), 4)
        lines.append(json.dumps(rec))
    for P, by in sorted(fleet.items()):
        lines.append(json.dumps({"fleet_P": P, "fleet_ms": [round(x, 4) for x in by["fleet"]], "fleet_median_ms": round(med(by["fleet"]), 4),
                                 "mppi_iteration_ms": [round(x, 4) for x in by["mppi"]], "mppi_iteration_median_ms": round(med(by["mppi"]), 4),
                                 "fleet_over_mppi_iteration": round(med(by["fleet"]) / med(by["mppi"]), 4),
                                 "neighbours_mean": round(by["neighbours_mean"][0], 2)}))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
