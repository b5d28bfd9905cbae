"""A/B worker for the tube trainer: every array a HipTubeTrainer and a 3-member HipTubeSweep produce, dumped so that two trees
(library and Python) can be compared array for array.  It reads the public surface of tube/trainer.py and tube/sweep.py only, so
the same file runs in either tree.

    python tools/tube_trainer_ab.py --out FILE.npz                   one fresh process per tree
    python tools/tube_trainer_ab.py --compare A.npz B.npz [--report FILE]

Cases (the shapes of tests/test_hip_tube_sweep.py: the smallest with a two-tile step and a tail):
  vector-tanh, mse-elu, mixed-activations, scalar-relu   70 training / 33 test rows at batch 64, two epochs (4 steps), evaluate()
  horizon               H_fwd 4, H_rev 2, nz 2, m 2, T 12, 40 / 20 envs at batch 32, two epochs, evaluate()
  scalar_level          the flat sizes with a level column; evaluate() and eval_level(0.9)
  horizon_vector_level  the horizon sizes with a level column; evaluate() and eval_level(0.9)
  explicit-rows         two steps on a row list (two tiles, one row twice), then on its first 7 rows
Per case and per model (`single<k>`: the trainer of member k's configuration; `sweep<k>`: member k of the sweep): params, grads,
adam_m, adam_v, perm, starts, levels, the log rows and the eval vectors.  --compare counts the arrays that differ in shape, dtype
or bytes (a nan equals itself)."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEV = "cuda:0"
MEMBERS3 = [dict(alpha=0.8, lr=1e-3, delta=1.0, seed=3), dict(alpha=0.9, lr=3e-3, delta=0.5, seed=4),
            dict(alpha=0.95, lr=1e-2, delta=0.25, seed=5)]
MIXED = [dict(activation="relu", alpha=0.8, seed=1), dict(activation="softplus", softplus_beta=5.0, alpha=0.9, seed=2),
         dict(activation="tanh", alpha=0.7, seed=3)]
LEVELS3 = [dict(lr=1e-3, delta=1.0, seed=3, level_lo=0.5, level_hi=1.0), dict(lr=3e-3, delta=0.5, seed=4),
           dict(lr=1e-2, delta=0.25, seed=5, level_lo=0.1, level_hi=0.9)]
HF, HR, T = 4, 2, 12


class Flat:
    def __init__(self, x, y):
        self.data, self.target = x, y


class Horizon:
    def __init__(self, w, z, v):
        self.w, self.z, self.v, self.H_fwd, self.H_rev = w, z, v, HF, HR


def flat_data(I, O, seed):
    import torch
    g = torch.Generator().manual_seed(seed)
    x, y = torch.randn(103, I, generator=g), torch.rand(103, O, generator=g) * 2
    return Flat(x[:70], y[:70]), Flat(x[70:], y[70:])


def horizon_data():
    import torch
    g = torch.Generator().manual_seed(7)
    w, z, v = torch.rand(60, T, generator=g), torch.randn(60, T, 2, generator=g), torch.randn(60, T, 2, generator=g)
    return Horizon(w[:40], z[:40], v[:40]), Horizon(w[40:], z[40:], v[40:])


def cases():
    flat = dict(num_units=32, num_layers=2, batch_size=64)
    yield "vector-tanh", 6, 2, dict(num_units=48, num_layers=4, activation="tanh", loss="vector", batch_size=64), MEMBERS3, flat_data(6, 2, 11)
    yield "mse-elu", 6, 2, dict(num_units=16, num_layers=1, activation="elu", loss="error", batch_size=64), MEMBERS3, flat_data(6, 2, 7)
    yield "mixed-activations", 6, 2, dict(loss="scalar", **flat), MIXED, flat_data(6, 2, 17)
    yield "scalar-relu", 3, 1, dict(activation="relu", loss="scalar", gamma=0.5, step_size=3, **flat), MEMBERS3, flat_data(3, 1, 0)
    hz = dict(num_units=128, num_layers=2, activation="softplus", softplus_beta=5.0, batch_size=32, horizon=(HF, HR))
    yield "horizon", HR + 2 + (HR + HF) * 2, HF, dict(loss="scalar_horizon", **hz), MEMBERS3, horizon_data()
    yield "scalar_level", 4, 1, dict(loss="scalar_level", **flat), LEVELS3, flat_data(3, 1, 5)
    yield "horizon_vector_level", HR + 2 + (HR + HF) * 2 + 1, HF, dict(loss="vector_level", **hz), LEVELS3, horizon_data()


def state(obj, k, steps, evals):
    """Member k's arrays (k None: the single trainer)."""
    pick = (lambda a: a) if k is None else (lambda a: a[k])
    out = {n: pick(getattr(obj, n)) for n in ("params", "grads", "adam_m", "adam_v", "perm", "starts", "levels")}
    out = {n: a.detach().cpu().numpy().copy() for n, a in out.items() if a is not None}
    out["log"] = (obj.read_log(1, steps) if k is None else obj.read_log(k, 1, steps)).numpy().copy()
    for n, e in evals.items():
        out[n] = pick(e).detach().cpu().numpy().copy()
    return out


def run(obj, train, test, batch, level):
    """Two epochs, full batches and the tail; the eval vectors by name."""
    obj.set_data(train, test)
    n, steps = obj.n_train(), 0
    for epoch in range(2):
        obj.begin_epoch(epoch)
        for b in range(0, n, batch):
            obj.step(min(batch, n - b))
            steps += 1
    evals = {"eval": obj.evaluate()}
    if level:
        evals["eval_level"] = obj.eval_level(0.9)
    return steps, evals


def dump():
    import torch
    from legged_gym_dev_amd.tube.sweep import HipTubeSweep
    from legged_gym_dev_amd.tube.trainer import HipTubeTrainer
    out = {}

    def both(name, I, O, shared, members, body):
        objs = [(None, HipTubeTrainer(I, O, device=DEV, **{**shared, **m})) for m in members]
        objs.append(("sweep", HipTubeSweep(I, O, members=members, device=DEV, **shared)))
        try:
            for j, (kind, obj) in enumerate(objs):
                steps, evals = body(obj)
                torch.cuda.synchronize()
                for k in ([None] if kind is None else range(len(members))):
                    who = f"single{j}" if kind is None else f"sweep{k}"
                    for n, a in state(obj, k, steps, evals).items():
                        out[f"{name}/{who}/{n}"] = a
        finally:
            for _, obj in objs:
                obj.close()
        print("ran", name, flush=True)

    for name, I, O, shared, members, (train, test) in cases():
        both(name, I, O, shared, members, lambda obj: run(obj, train, test, shared["batch_size"], "level" in name))
    train, _ = flat_data(3, 1, 0)
    rows = torch.tensor([5, 5, 0, 69, 17] + list(range(20, 55)), dtype=torch.int32).to(DEV)

    def explicit(obj):
        obj.set_data(train)
        obj.step(rows=rows)
        obj.step(rows=rows[:7])
        return 2, {}
    both("explicit-rows", 3, 1, dict(num_units=32, num_layers=2, loss="scalar", batch_size=64), MEMBERS3, explicit)
    return out


def compare(a, b, report):
    za, zb = np.load(a), np.load(b)
    assert sorted(za.files) == sorted(zb.files), "the two dumps hold different arrays"
    lines, total = [], 0
    for k in sorted(za.files):
        same = za[k].shape == zb[k].shape and za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes()
        total += not same
        lines.append(f"{k:48s} {str(za[k].dtype):8s} {str(za[k].shape):14s} {'equal' if same else 'DIFFERS'}")
    lines.append(f"arrays: {len(za.files)}  differ: {total}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if report:
        open(report, "w").write(text)
    return 1 if total else 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar="NPZ")
    ap.add_argument("--report")
    args = ap.parse_args()
    if args.compare:
        raise SystemExit(compare(args.compare[0], args.compare[1], args.report))
    arrays = dump()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    np.savez(args.out, **arrays)
    print("dumped", len(arrays), "arrays", flush=True)


if __name__ == "__main__":
    main()
