#!/usr/bin/env python3
"""Time of the gradient planner on a learned tube (lg_plan_descend_step) on the reference one-shot shape --
H_rev 10, N 50, 130 inputs, 128 units x 2 layers Softplus(beta 5) -- and the gap problem, at B = 4096 and B = 64 plans:
    fused        one lg_plan_descend_step that evaluates and steps (k_plan_grad with the optimiser tail); v is restored first (copy_v)
    eval         the same launch without the step
    torch_eager  the only route to the same gradient before k_plan_grad: J restated in torch on the device, vectorised over the
                 plans and the nodes (cumsum for the ROM, one batched expression per term), torch autograd, then Adam, the clip and
                 the elite as torch-eager operations.  Its gradient is compared with the kernel's once, and the difference printed.
    plan_score   lg_plan_score without its optional outputs on the same B: the forward pass alone
and the wall time of a whole plan() that reaches the acceptance of the tests -- SMALL: min_clear >= 0, no node inside the obstacle,
J <= 66.12; gap with the l1 tube, N 50: min_clear >= 0, no node inside; each judged on the elite -- by mppi, grad and mppi+grad (5
MPPI iterations at K = 64, then the gradient), each at the fewest iterations of a short ladder that reach it.  Every timing ends in
a device synchronise; median of --repeats runs after a warm-up of the same shape.

    python tools/bench_plan_grad.py [--repeats 3]
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


class TorchJ:
    """J of section 10.10 on device tensors, vectorised; the tube is the MLP of a state dict."""

    def __init__(self, p, sd, cfg):
        t = lambda x: torch.tensor(x, dtype=torch.float32, device=DEV)
        self.W = [(sd[k].to(DEV), sd[k.replace("weight", "bias")].to(DEV)) for k in sd if k.endswith("weight")]
        self.dt, self.goal, self.oc, self.orad = p.dt, t(p.goal), t(p.obs_c), t(p.obs_r)
        self.Q, self.Qf, self.R = (t(m).reshape(2, 2) for m in (p.Q, p.Q if p.Qf is None else p.Qf, p.R))
        self.Qw, self.w_max, self.zmin, self.zmax = p.Qw, p.w_max, t(p.rom_z_min), t(p.rom_z_max)
        self.lo, self.hi, self.cfg = t(p.rom_v_min), t(p.rom_v_max), cfg

    def __call__(self, z0, v, e, v_prev, w0):
        B, N = v.shape[:2]
        h = torch.cat([e, v_prev.reshape(B, -1), v.reshape(B, -1)], dim=1)
        for i, (W, b) in enumerate(self.W):
            h = torch.nn.functional.linear(h, W, b)
            if i + 1 < len(self.W):
                h = torch.nn.functional.softplus(h, beta=BETA, threshold=20.0)
        w = torch.cat([w0[:, None], h], dim=1)
        z = z0[:, None] + self.dt * torch.cat([torch.zeros(B, 1, 2, device=DEV), torch.cumsum(v, dim=1)], dim=1)
        d = z[:, :, None, :] - self.oc
        g = (d * d).sum(dim=-1) - (self.orad + w[:, :, None]) ** 2
        quad = lambda M, x: ((x @ M) * x).sum(dim=-1)
        cost = quad(self.Q, z[:, :N] - self.goal).sum(dim=1) + quad(self.Qf, z[:, N] - self.goal) + quad(self.R, v).sum(dim=1) + self.Qw * (w * w).sum(dim=1)
        pen_g, pen_w = (-g).clamp(min=0).sum(dim=(1, 2)), (w - self.w_max).clamp(min=0).sum(dim=1)
        pen_z = ((z - self.zmax).clamp(min=0) + (self.zmin - z).clamp(min=0)).sum(dim=(1, 2))
        c = self.cfg
        return cost + c.rho_g * pen_g + c.rho_w * pen_w + c.rho_z * pen_z

    def step(self, st, t):
        """Evaluate, take the elite, step: what one fused launch does."""
        c = self.cfg
        v = st["v"].detach().requires_grad_(True)
        J = self(st["z0"], v, st["e"], st["v_prev"], st["w0"])
        (g,) = torch.autograd.grad(J.sum(), v)
        J = J.detach()
        win = J < st["best_J"]
        st["best_J"] = torch.where(win, J, st["best_J"])
        st["best_v"] = torch.where(win[:, None, None], st["v"], st["best_v"])
        st["m"].mul_(c.beta1).add_(g, alpha=1 - c.beta1)
        st["s"].mul_(c.beta2).addcmul_(g, g, value=1 - c.beta2)
        x = st["v"] - c.lr * (st["m"] / (1 - c.beta1 ** t)) / ((st["s"] / (1 - c.beta2 ** t)).sqrt() + c.eps)
        st["v"] = torch.maximum(torch.minimum(x, self.hi), self.lo)
        return g


def accepted(sol, J_max=None):
    """The tests' acceptance, on the elite of a plan()."""
    score = sol["best_score"]
    ok = bool((score["min_clear"] >= 0).all()) and not bool(score["n_viol"][:, 0].any())
    return ok and (J_max is None or bool((sol["best_J"] <= J_max).all()))


def first_accepting(make, ladder, z0, J_max):
    """The first rung of `ladder` whose plan() is accepted: (rung, the planner) or (None, None)."""
    for n in ladder:
        pln = make(n)
        if accepted(pln.plan(z0), J_max):
            return n, pln
    return None, None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_plan_grad.py needs the GPU")
    p = pl.PlanProblem.named("gap", N=HF, H_rev=HR)
    I = HR + 2 * (HR + HF)
    sd = initial_params(I, HF, U, NL, 1)
    model = HipTubeModel(sd, activation="softplus", softplus_beta=BETA, horizon=(HF, HR), device=DEV)
    cfg = pl.GradCfg(iters=100, lr=0.01, rho_g=1e4, rho_w=30.0, rho_z=7.0)
    gp = pl.HipGradPlanner(model, p, cfg, device=DEV)
    tj = TorchJ(p, sd, cfg)
    for B in (4096, 64):
        g = torch.Generator().manual_seed(B)
        z0 = torch.tensor(p.start) + 0.02 * torch.randn(B, 2, generator=g)
        v = torch.as_tensor(gp.warm_start(z0.numpy())) + 0.02 * torch.randn(B, HF, 2, generator=g)
        e, vp = 0.05 * torch.rand(B, HR, generator=g), 0.1 * (2 * torch.rand(B, HR, 2, generator=g) - 1)
        st = gp.state(z0, v, e, vp, None, want=("grad",))
        keep = st["v"].clone()
        gp.step(st, 0, what=3, reset=True)
        ts = {"z0": st["z0"], "e": st["e"], "v_prev": st["v_prev"], "w0": torch.zeros(B, device=DEV), "v": keep.clone(), "m": torch.zeros_like(keep),
              "s": torch.zeros_like(keep), "best_J": torch.full((B,), float("inf"), device=DEV), "best_v": keep.clone()}
        gt = tj.step(ts, 1)
        res = {"config": "plan_grad_bench", "B": B, "N": HF, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               "grad_abs_max": float(st["grad"].abs().max()), "torch_minus_kernel_abs_max": float((gt - st["grad"]).abs().max()),
               "stepped_v_torch_minus_kernel_abs_max": float((ts["v"] - st["v"]).abs().max())}

        def fused():
            st["v"].copy_(keep)
            gp.step(st, 1, what=3)

        def eager():
            ts["v"] = keep.clone()
            tj.step(ts, 2)
        for name, fn in (("fused", fused), ("eval", lambda: gp.step(st, 1, what=1)), ("torch_eager", eager),
                         ("plan_score", lambda: gp.scorer.score(st["z0"], keep, st["e"], st["v_prev"], None, want=())),
                         ("copy_v", lambda: st["v"].copy_(keep))):
            res[name + "_ms"], res[name + "_ms_all"] = timed(fn, a.repeats)
        res["torch_eager_over_fused"] = res["torch_eager_ms"] / res["fused_ms"]
        res["fused_over_plan_score"] = (res["fused_ms"] - res["copy_v_ms"]) / res["plan_score_ms"]
        res["eval_over_plan_score"] = res["eval_ms"] / res["plan_score_ms"]
        res["plan_score_spread_ms"] = res["plan_score_ms_all"][-1] - res["plan_score_ms_all"][0]
        print(line(res), flush=True)
    model.close()

    # wall time of a plan() that reaches the acceptance, one start
    small = pl.PlanProblem(N=8, dt=0.1, start=[0.0, 0.0], goal=[1.0, 0.0], obs_c=[[0.5, 0.15]], obs_r=[0.2], tube_kind="l2", scaling=0.02,
                           Q=[10.0, 0, 0, 10.0], R=[1.0, 0, 0, 1.0], rom_v_min=[-2.0, -2.0], rom_v_max=[2.0, 2.0])
    gap = pl.PlanProblem.named("gap", tube_kind="l1", N=50)
    for name, q, J_max, K, sigma, lr in (("SMALL", small, 0.1 * 661.2, 256, 0.3, 0.05), ("gap-l1", gap, None, 512, 0.05, 0.01)):
        z0 = torch.tensor([q.start])
        mk_m = lambda n, K=K: pl.HipMppiPlanner(None, q, pl.MppiCfg(K=K, iters=n, sigma=sigma, lambda_=1.0, rho_g=1e4), device=DEV)
        mk_g = lambda n: pl.HipGradPlanner(None, q, pl.GradCfg(iters=n, lr=lr, rho_g=1e4), device=DEV)
        mk_c = lambda n: pl.ChainedPlanner(mk_m(5, 64), mk_g(n))
        for planner, make, ladder in (("mppi", mk_m, (5, 10, 15, 20, 30, 40)), ("grad", mk_g, (10, 20, 30, 50, 75, 100, 150)),
                                      ("mppi+grad", mk_c, (5, 10, 20, 30, 50, 75, 100))):
            n, pln = first_accepting(make, ladder, z0, J_max)
            res = {"config": "plan_accept_bench", "problem": name, "planner": planner, "iters": n, "K": K if planner == "mppi" else 64 if "+" in planner else None}
            if pln is not None:
                sol = pln.plan(z0)
                res["best_J"], res["min_clear"] = float(sol["best_J"][0]), float(sol["best_score"]["min_clear"][0])
                res["evaluations"] = n * K if planner == "mppi" else n + 1 + (5 * 64 if "+" in planner else 0)
                res["plan_ms"], res["plan_ms_all"] = timed(lambda: pln.plan(z0), a.repeats)
            print(line(res), flush=True)


if __name__ == "__main__":
    main()
