#!/usr/bin/env python3
"""Time of one MPPI iteration on a learned tube (lg_plan_mppi_step) on the reference one-shot shape -- H_rev 10,
N 50, 130 inputs, 128 units x 2 layers Softplus(beta 5) -- and the gap problem, at P * K = 65536 candidates split as P = 16 x K = 4096
and as P = 2048 x K = 32, and at P = 1 x K = 4096, where the update has the least parallelism.  Per split:
    fused          one lg_plan_mppi_step with both kernels (k_plan_sample_score, k_plan_mppi_update)
    score, update  each kernel alone
    materialised   what the library had before the planner: the candidates by torch (randn, clamp) into a (P, K, N, 2) array,
                   lg_plan_score on them without its optional outputs, J = cost + rho_g max(0, -min_clear), and the softmin mean in
                   torch eager
    plan_score     lg_plan_score without its optional outputs on the same B = P K stored candidates: k_plan_sample_score does its
                   work plus one Philox block per node, and reads less
and the time of one closed-loop control step (plan with `iters` iterations, score, track, shifts) for 2048 robots at K = 32.
Every timing ends in a device synchronise; median of --repeats runs after a warm-up run of the same shape.

    python tools/bench_mppi.py [--repeats 3] [--iters 4]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from legged_gym_dev_amd.tube import plan as pl  # noqa: E402
from legged_gym_dev_amd.tube.model import HipTubeModel  # noqa: E402
from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg  # noqa: E402
from legged_gym_dev_amd.tube.trainer import initial_params  # noqa: E402

DEV = "cuda:0"
HF, HR, U, NL, BETA = 50, 10, 128, 2, 5.0


def timed(fn, repeats):
    fn()                                # warm-up: the same shape
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2] * 1e3, [t * 1e3 for t in ts]


def line(res):
    return json.dumps({k: (round(x, 4) if isinstance(x, float) else [round(q, 4) for q in x] if isinstance(x, list) else x) for k, x in res.items()})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=4, help="iterations per plan of the closed-loop step")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mppi.py needs the GPU")
    p = pl.PlanProblem.named("gap", N=HF, H_rev=HR)
    I = HR + 2 * (HR + HF)
    model = HipTubeModel(initial_params(I, HF, U, NL, 1), activation="softplus", softplus_beta=BETA, horizon=(HF, HR), device=DEV)
    lo, hi = torch.tensor(p.rom_v_min, device=DEV), torch.tensor(p.rom_v_max, device=DEV)
    for P, K in ((16, 4096), (2048, 32), (1, 4096)):
        cfg = pl.MppiCfg(K=K, iters=a.iters, sigma=0.05, lambda_=1.0, rho_g=1e4)
        pln = pl.HipMppiPlanner(model, p, cfg, device=DEV)
        g = torch.Generator().manual_seed(P)
        z0 = torch.tensor(p.start) + 0.02 * torch.randn(P, 2, generator=g)
        vbar = torch.as_tensor(pln.warm_start(z0.numpy()))
        st = pln.state(z0, vbar)
        keep = st["vbar"].clone()
        pln.step(st, 0, what=3, reset=True)
        zr = st["z0"].repeat_interleave(K, dim=0)
        cand = pln.candidates(keep, 0).reshape(P * K, HF, 2).contiguous()
        res = {"config": "mppi_bench", "P": P, "K": K, "N": HF, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}

        def fused():
            st["vbar"].copy_(keep)
            pln.step(st, 0, what=3)

        def update():
            st["vbar"].copy_(keep)
            pln.step(st, 0, what=2)

        def materialised():
            c = torch.maximum(torch.minimum(keep[:, None] + cfg.sigma * torch.randn(P, K, HF, 2, device=DEV), hi), lo)
            s = pln.scorer.score(zr, c.reshape(P * K, HF, 2), want=())
            J = (s["cost"] + cfg.rho_g * (-s["min_clear"]).clamp(min=0)).reshape(P, K)
            w = torch.exp(-(J - J.min(dim=1, keepdim=True).values) / cfg.lambda_)
            return (w[:, :, None, None] * c).sum(dim=1) / w.sum(dim=1)[:, None, None]
        for name, fn in (("fused", fused), ("score", lambda: pln.step(st, 0, what=1)), ("update", update), ("materialised", materialised),
                         ("plan_score", lambda: pln.scorer.score(zr, cand, want=())), ("copy_vbar", lambda: st["vbar"].copy_(keep))):
            res[name + "_ms"], res[name + "_ms_all"] = timed(fn, a.repeats)
        res["materialised_over_fused"] = res["materialised_ms"] / res["fused_ms"]
        res["score_over_plan_score"] = res["score_ms"] / res["plan_score_ms"]
        res["plan_score_spread_ms"] = res["plan_score_ms_all"][-1] - res["plan_score_ms_all"][0]
        res["update_share_of_iteration"] = (res["update_ms"] - res["copy_vbar_ms"]) / max(res["fused_ms"] - res["copy_vbar_ms"], 1e-9)
        print(line(res), flush=True)

    # one closed-loop control step for 2048 robots: the default simulator configuration (model 0.05 s, ROM 0.1 s: S = 2)
    P, K, H = 2048, 32, 4
    rc = RomSimCfg()
    rc.env.num_envs = 1
    sim = HipRomSim(rc, device=DEV)
    pln = pl.HipMppiPlanner(model, p, pl.MppiCfg(K=K, iters=a.iters, sigma=0.05, lambda_=1.0, rho_g=1e4), device=DEV)
    start = torch.tensor(p.start) + 0.02 * torch.randn(P, 2, generator=torch.Generator().manual_seed(0))
    cres = {"config": "mppi_closed_loop_bench", "robots": P, "K": K, "iters": a.iters, "N": HF, "steps": H, "repeats": a.repeats}
    ms, ms_all = timed(lambda: pl.closed_loop(pln, sim, H, start), a.repeats)
    cres["control_step_ms"], cres["control_step_ms_all"] = ms / H, [t / H for t in ms_all]
    print(line(cres), flush=True)
    sim.close()
    model.close()


if __name__ == "__main__":
    main()
