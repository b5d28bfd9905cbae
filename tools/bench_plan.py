#!/usr/bin/env python3
"""Time of scoring and tracking a batch of plans (lg_plan_score, lg_plan_track) on the reference one-shot
shape: H_rev 10, N 50, 130 inputs, 128 units x 2 layers Softplus(beta 5), the gap problem's 2 obstacles, B = 65536 plans.
Scoring, three ways to the same cost / min_clear / n_viol / fw / z / w:
    a  plan_score        one lg_plan_score launch
    b  windows_eager     lg_tube_predict_windows on host-built (device-resident) window arrays, then the nodes, clearance, cost and
                         counts in torch eager on the device
    c  torch_eager       the MLP in torch eager too (three GEMMs), then the same tail
and `predict_only`, the lg_tube_predict_windows launch alone: what the scoring tail adds to k_tube_predict is a - predict_only.
Tracking, two ways: `plan_track`, one lg_plan_track launch, and `stepwise`, lg_romsim_policy per model step with the model in
torch eager (the path the tests compare the launch with).  Every timing ends in a device synchronise; median of --repeats runs
after a warm-up run of the same shape.

    python tools/bench_plan.py [--plans 65536] [--repeats 3]
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from legged_gym_dev_amd.tube import plan as pl  # noqa: E402
from legged_gym_dev_amd.tube.model import HipTubeModel  # noqa: E402
from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg  # noqa: E402
from legged_gym_dev_amd.tube.trainer import initial_params  # noqa: E402
from tests import tube_ref  # noqa: E402

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
    return json.dumps({k: (float(f"{x:.3g}") if k.startswith("max_abs") else round(x, 4) if isinstance(x, float)
                           else [round(q, 4) for q in x] if isinstance(x, list) else x) for k, x in res.items()})


def eager_tail(p, z0, v, fw):
    """Nodes, clearance, cost and counts of lg_plan_score in torch eager (batched over the plans, the node loop on the host)."""
    B, N = v.shape[:2]
    f = lambda x: torch.tensor(x, device=DEV, dtype=torch.float32)
    z = torch.cat([z0[:, None], z0[:, None] + torch.cumsum(p.dt * v, dim=1)], dim=1)
    w = torch.cat([torch.zeros(B, 1, device=DEV), fw], dim=1)
    oc, orad, goal = f(p.obs_c), f(p.obs_r), f(p.goal)
    d = z[:, :, None, :] - oc[None, None]
    g = (d * d).sum(-1) - (orad[None, None] + w[:, :, None]) ** 2
    gmin, node = g.min(dim=2).values.min(dim=1)
    Q, Qf, R = f(p.Q).view(2, 2), f(p.Qf or p.Q).view(2, 2), f(p.R).view(2, 2)
    dz = z - goal
    cost = ((dz[:, :-1] @ Q) * dz[:, :-1]).sum((1, 2)) + ((dz[:, -1] @ Qf) * dz[:, -1]).sum(1) + ((v @ R) * v).sum((1, 2)) + p.Qw * (w * w).sum(1)
    nv = torch.stack([(g < 0).any(dim=2).sum(1), ((v < f(p.rom_v_min)) | (v > f(p.rom_v_max))).any(dim=2).sum(1),
                      ((z < f(p.rom_z_min)) | (z > f(p.rom_z_max))).any(dim=2).sum(1), (w > p.w_max).sum(1)], dim=1)
    return cost, gmin, node, nv, z, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--plans", type=int, default=65536)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan.py needs the GPU")
    B = a.plans
    p = pl.PlanProblem.named("gap", N=HF, H_rev=HR)
    I = HR + 2 * (HR + HF)
    sd = initial_params(I, HF, U, NL, 1)
    model = HipTubeModel(sd, activation="softplus", softplus_beta=BETA, horizon=(HF, HR), device=DEV)
    ref = tube_ref.MLP(I, HF, U, NL, "softplus", BETA)
    ref.load_state_dict(sd)
    ref = ref.to(DEV)
    _, v0 = pl.warm_start("interpolate", p.start, p.goal, HF, p.dt)
    v = pl.perturb(v0, 0.05, B, 0, [-0.3, -0.3], [0.3, 0.3]).to(DEV)
    z0 = torch.tensor(p.start, device=DEV).repeat(B, 1)
    ds = types.SimpleNamespace(H_fwd=HF, H_rev=HR, w=torch.zeros(B, HR + HF, device=DEV), z=torch.zeros(B, HR + HF, 0, device=DEV),
                               v=torch.cat([torch.zeros(B, HR, 2, device=DEV), v], dim=1).contiguous())
    env, start = torch.arange(B, dtype=torch.int32, device=DEV), torch.full((B,), HR, dtype=torch.int32, device=DEV)
    item = torch.cat([torch.zeros(B, 3 * HR, device=DEV), v.reshape(B, -1)], dim=1).contiguous()
    scorer = pl.HipPlanScorer(model, p)
    res = {"config": "plan_bench", "plans": B, "N": HF, "obstacles": p.n_obs, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}

    def eager():
        with torch.no_grad():
            return eager_tail(p, z0, v, ref(item))
    for name, fn in (("plan_score", lambda: scorer.score(z0, v)), ("plan_score_no_optional", lambda: scorer.score(z0, v, want=())),
                     ("predict_only", lambda: model.predict_windows(ds, env, start)),
                     ("windows_eager", lambda: eager_tail(p, z0, v, model.predict_windows(ds, env, start))), ("torch_eager", eager)):
        res[name + "_ms"], res[name + "_ms_all"] = timed(fn, a.repeats)
    s, e = scorer.score(z0, v), eager()
    res["max_abs_diff_cost_rel"] = float(((s["cost"] - e[0]).abs() / e[0].abs()).max())
    res["max_abs_diff_min_clear"] = float((s["min_clear"] - e[1]).abs().max())
    res["tail_share_of_launch"] = (res["plan_score_ms"] - res["predict_only_ms"]) / res["plan_score_ms"]
    res["windows_eager_over_plan_score"] = res["windows_eager_ms"] / res["plan_score_ms"]
    res["torch_eager_over_plan_score"] = res["torch_eager_ms"] / res["plan_score_ms"]
    print(line(res), flush=True)

    # tracking: the default simulator configuration (model 0.05 s, ROM 0.1 s: S = 2)
    rc = RomSimCfg()
    rc.env.num_envs = 1
    sim = HipRomSim(rc, device=DEV)
    z = s["z"]
    dt = torch.tensor(rc.env.model.dt, device=DEV)

    def stepwise():
        x = torch.cat([z[:, 0], torch.zeros(B, 2, device=DEV)], dim=1)
        for t in range(HF):
            ff = v[:, min(t + 1, HF - 1)]
            for sub in range(2):
                refp = z[:, t] + (z[:, t + 1] - z[:, t]) * (sub * 0.5)
                act = sim.policy(torch.cat([x, refp, ff], dim=1))
                x = torch.cat([x[:, :2] + dt * x[:, 2:], x[:, 2:] + dt * act], dim=1)
        return x
    tres = {"config": "plan_track_bench", "plans": B, "N": HF, "S": 2, "repeats": a.repeats}
    tres["plan_track_ms"], tres["plan_track_ms_all"] = timed(lambda: pl.track(sim, z, v), a.repeats)
    tres["stepwise_ms"], tres["stepwise_ms_all"] = timed(stepwise, a.repeats)
    tres["stepwise_over_plan_track"] = tres["stepwise_ms"] / tres["plan_track_ms"]
    tres["max_abs_diff_final_state"] = float((pl.track(sim, z, v)["x"][:, -1] - stepwise()).abs().max())
    print(line(tres), flush=True)
    sim.close()
    model.close()


if __name__ == "__main__":
    main()
