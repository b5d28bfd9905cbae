#!/usr/bin/env python3
"""Steps/s and rows/s of the HIP tube trainer against torch eager with the tensors already on the device, on the same
synthetic data.  Two configs:
    default   ScalarTubeDataset rows (w, v: 3 columns), 32 units x 2 layers ReLU, ScalarTubeLoss, batch 2048, 8192 x 200 rows
    oneshot   ScalarHorizonTubeDataset 50 / 10 (130 inputs, 50 outputs), 128 units x 2 layers Softplus(beta 5), VectorTubeLoss,
              batch 2048 over 8192 envs x 200 steps
Torch eager: the reference's step (train_tube.py:99-127) minus the DataLoader -- gather by a device permutation, forward,
loss, backward, Adam, StepLR, gradient norm -- with no .item() in the loop.

    python tools/bench_tube.py [--steps 400] [--repeats 3]

--sweep 1,4,16 adds the sweep leg: for every K, the time per step of one HipTubeSweep of K members
against K HipTubeTrainer runs with the same member configurations executed one after the other (their timed stretches summed),
same warm-up, same steps, each timing closed by a device synchronise.
    python tools/bench_tube.py --steps 300 --sweep 1,4,16

--level adds the level-conditioned leg: the time per step of a level-conditioned trainer (loss
scalar_level: data of 3 columns, the level drawn on the device as the 4th input) against the unconditioned trainer of the same
shape whose data holds one more column (4 inputs), default model and batch.  Median of --repeats after a warm-up, every timing
closed by a device synchronise.
    python tools/bench_tube.py --steps 400 --level
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from legged_gym_dev_amd.tube.sweep import HipTubeSweep  # noqa: E402
from legged_gym_dev_amd.tube.trainer import HipTubeTrainer  # noqa: E402
from tests import tube_ref  # noqa: E402

DEV = "cuda:0"


class _Flat:
    def __init__(self, x, y):
        self.data, self.target = x, y


class _Horizon:
    def __init__(self, w, z, v, H_fwd, H_rev):
        self.w, self.z, self.v, self.H_fwd, self.H_rev = w, z, v, H_fwd, H_rev


def make(cfg, g):
    E, T = 8192, 200
    if cfg == "default":
        n = E * T
        x = torch.rand(n, 3, generator=g)
        y = (x[:, :1] + 0.1 * torch.rand(n, 1, generator=g))
        return dict(kw=dict(input_dim=3, output_dim=1, num_units=32, num_layers=2, activation="relu", loss="scalar",
                            alpha=0.8, step_size=2000), data=_Flat(x.to(DEV), y.to(DEV)), rows=n, horizon=None)
    Hf, Hr = 50, 10
    w = torch.rand(E, T + Hr, generator=g)
    v = torch.rand(E, T + Hr, 2, generator=g)
    z = torch.zeros(E, T + Hr, 0)
    return dict(kw=dict(input_dim=Hr + 2 * (Hr + Hf), output_dim=Hf, num_units=128, num_layers=2, activation="softplus",
                        softplus_beta=5.0, loss="vector", alpha=0.9, step_size=1000, gamma=0.75, horizon=(Hf, Hr)),
                data=_Horizon(w.to(DEV), z.to(DEV), v.to(DEV), Hf, Hr), rows=E, horizon=(Hf, Hr))


def make_level(g):
    """The default config's rows; `plain` carries a 4th data column where `level` draws its level column on the device."""
    n = 8192 * 200
    x = torch.rand(n, 4, generator=g)
    y = (x[:, :1] + 0.1 * torch.rand(n, 1, generator=g)).to(DEV)
    kw = dict(input_dim=4, output_dim=1, num_units=32, num_layers=2, activation="relu", step_size=2000)
    return {"level": dict(kw=dict(loss="scalar_level", **kw), data=_Flat(x[:, :3].contiguous().to(DEV), y), rows=n, horizon=None),
            "plain": dict(kw=dict(loss="scalar", alpha=0.8, **kw), data=_Flat(x.to(DEV), y), rows=n, horizon=None)}


def sweep_members(K):
    return [dict(alpha=0.5 + 0.45 * (k + 1) / K, seed=1 + k) for k in range(K)]


def time_hip(c, steps, B, member=None, K=None):
    """One HipTubeTrainer (with `member` on top of the config), or with K one HipTubeSweep of sweep_members(K)."""
    if K is not None:
        tr = HipTubeSweep(c["kw"]["input_dim"], c["kw"]["output_dim"], members=sweep_members(K), batch_size=B, device=DEV,
                          **{k: v for k, v in c["kw"].items() if k not in ("input_dim", "output_dim", "alpha")})
    else:
        tr = HipTubeTrainer(batch_size=B, device=DEV, **{"seed": 1, **c["kw"], **(member or {})})
    tr.set_data(c["data"])
    n, per_epoch = c["rows"], (c["rows"] + B - 1) // B

    def run(k, epoch0):
        s = 0
        while s < k:
            tr.begin_epoch(epoch0 + s // per_epoch)
            for b in range(min(per_epoch, k - s)):
                tr.step(min(B, n - b * B))
            s += min(per_epoch, k - s)
    run(20, 0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps, 1000)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    tr.close()
    return dt


def time_torch(c, steps, B, g):
    kw = c["kw"]
    torch.manual_seed(1)
    m = tube_ref.MLP(kw["input_dim"], kw["output_dim"], kw["num_units"], kw["num_layers"], kw["activation"],
                     kw.get("softplus_beta", 1.0)).to(DEV)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    sched = torch.optim.lr_scheduler.StepLR(opt, step_size=kw["step_size"], gamma=kw.get("gamma", 0.1))
    n, d = c["rows"], c["data"]
    name = {"scalar": "scalar", "vector": "vector"}[kw["loss"]]

    def batch(idx):
        if c["horizon"] is None:
            return d.data[idx], d.target[idx]
        Hf, Hr = c["horizon"]
        T = d.w.shape[1]
        ind = torch.randint(Hr, T - Hf - 1, (idx.numel(),), device=DEV)
        tr_ = torch.arange(-Hr, 0, device=DEV)
        tv = torch.arange(-Hr, Hf, device=DEV)
        tf = torch.arange(1, Hf + 1, device=DEV)
        e = idx[:, None]
        x = torch.cat((d.w[e, ind[:, None] + tr_], d.v[e, ind[:, None] + tv].reshape(idx.numel(), -1)), dim=1)
        return x, d.w[e, ind[:, None] + tf]

    def run(k):
        perm = torch.randperm(n, device=DEV)
        pos = 0
        for _ in range(k):
            if pos >= n:
                perm, pos = torch.randperm(n, device=DEV), 0
            idx = perm[pos:pos + B]
            pos += B
            x, y = batch(idx)
            opt.zero_grad()
            lv = tube_ref.loss(name, m(x), y, kw["alpha"], 1.0)
            lv.backward()
            opt.step()
            sched.step()
            torch.cat([p.grad.detach().flatten() for p in m.parameters()]).norm()
    run(20)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    run(steps)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--configs", default="default,oneshot")
    ap.add_argument("--sweep", default=None, help="member counts of the sweep leg, e.g. 1,4,16 (replaces the torch comparison)")
    ap.add_argument("--level", action="store_true", help="the level-conditioned step against the unconditioned step (replaces the torch comparison)")
    a = ap.parse_args()
    B = 2048
    if a.level:
        cs = make_level(torch.Generator().manual_seed(0))
        res = {"config": "level_step", "steps": a.steps, "batch": B, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
        for who in ("plain", "level", "plain_again"):            # the unconditioned leg twice: the run-to-run spread
            ts = sorted(time_hip(cs[who.split("_")[0]], a.steps, B) for _ in range(a.repeats))
            res[who] = {"us_per_step_median": round(1e6 * ts[len(ts) // 2] / a.steps, 1),
                        "us_per_step_all": [round(1e6 * t / a.steps, 1) for t in ts]}
        res["level_over_plain"] = round(res["level"]["us_per_step_median"] / res["plain"]["us_per_step_median"], 3)
        print(json.dumps(res), flush=True)
        return
    if a.sweep:
        for cfg in a.configs.split(","):
            c = make(cfg, torch.Generator().manual_seed(0))
            for K in (int(k) for k in a.sweep.split(",")):
                legs = {"sweep": lambda: time_hip(c, a.steps, B, K=K),
                        "sequential": lambda: sum(time_hip(c, a.steps, B, member=m) for m in sweep_members(K))}
                res = {"config": cfg, "K": K, "steps": a.steps, "batch": B, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
                for who, fn in legs.items():
                    ts = sorted(fn() for _ in range(a.repeats))
                    res[who] = {"us_per_step_median": round(1e6 * ts[len(ts) // 2] / a.steps, 1),
                                "us_per_step_all": [round(1e6 * t / a.steps, 1) for t in ts]}
                res["sequential_over_sweep"] = round(res["sequential"]["us_per_step_median"] / res["sweep"]["us_per_step_median"], 2)
                print(json.dumps(res), flush=True)
        return
    for cfg in a.configs.split(","):
        c = make(cfg, torch.Generator().manual_seed(0))
        res = {"config": cfg, "steps": a.steps, "batch": B, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
        for who, fn in (("hip", lambda: time_hip(c, a.steps, B)), ("torch_eager", lambda: time_torch(c, a.steps, B, None))):
            ts = sorted(fn() for _ in range(a.repeats))
            med = ts[len(ts) // 2]
            res[who] = {"steps_per_s": round(a.steps / med, 1), "rows_per_s": round(a.steps * B / med),
                        "us_per_step_median": round(1e6 * med / a.steps, 1),
                        "us_per_step_all": [round(1e6 * t / a.steps, 1) for t in ts]}
        res["speedup"] = round(res["hip"]["steps_per_s"] / res["torch_eager"]["steps_per_s"], 2)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
