"""Train a tube model on ROM tracking data recorded by collect_trajectory_data.py: the loop of the reference's
deep_tube_learning/train_tube.py:53-141 on the HIP trainer, without hydra or wandb.  Flags carry the names of the
configs/tube_learning YAML keys; defaults are default.yaml's, and torch's where that file leaves a value undefined.

    python legged_gym_dev_amd/scripts/train_tube.py --data rom_tracking_data/run0 --out tube_runs/run0 \\
        [--dataset scalar --loss scalar --alpha 0.8 --num_units 32 --num_layers 2 --activation relu ...]

Writes to --out: model.pth (the latest checkpoint) and model_best.pth (the checkpoint with the lowest step loss; wandb's
"latest" and "best" aliases), and metrics.jsonl: one line per step with loss_step, lr_step, grad_norm (plus the test metrics
on evaluation steps), one line per epoch with loss_epoch and lr_epoch.  loss_epoch is the true mean step loss of the epoch:
the reference adds every step's loss twice (epoch_loss += loss.item() and epoch_loss += loss), so its value is twice this.
config.json holds the dataset, window, horizon, loss and model flags: what evaluate_tube.py needs to rebuild the model and its inputs.

The host waits for the device only at checkpoints and once per epoch (to write the log); steps and evaluations are queued.
"""
import argparse
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from legged_gym_dev_amd.tube.data import DATASETS, construct_dataset  # noqa: E402
from legged_gym_dev_amd.tube.trainer import HipTubeTrainer  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--data", required=True, help="folder of epoch_<k>.pickle files")
    ap.add_argument("--dataset", choices=sorted(DATASETS), default="scalar")
    ap.add_argument("--N", type=int, default=1)
    ap.add_argument("--dN", type=int, default=1)
    ap.add_argument("--recursive", action="store_true")
    ap.add_argument("--H_fwd", type=int, default=50)
    ap.add_argument("--H_rev", type=int, default=10)
    ap.add_argument("--loss", choices=["scalar", "vector", "scalar_horizon", "error"], default="scalar")
    ap.add_argument("--alpha", type=float, default=0.8, help="tube quantile (default.yaml leaves it unset; tube_learning.yaml's)")
    ap.add_argument("--delta", type=float, default=1.0)
    ap.add_argument("--num_units", type=int, default=32)
    ap.add_argument("--num_layers", type=int, default=2)
    ap.add_argument("--activation", choices=["relu", "softplus", "tanh", "elu"], default="relu")
    ap.add_argument("--softplus_beta", type=float, default=1.0)
    ap.add_argument("--batch_size", type=int, default=2048)
    ap.add_argument("--num_epochs", type=int, default=10)
    ap.add_argument("--validation_split", type=float, default=0.8, help="fraction of the rows that trains")
    ap.add_argument("--lr", type=float, default=1e-3)
    ap.add_argument("--gamma", type=float, default=0.1, help="StepLR gamma (torch's default)")
    ap.add_argument("--step_size", type=int, default=10000)
    ap.add_argument("--seed", type=int, default=42)
    ap.add_argument("--steps_per_model_checkpoint", type=int, default=1000)
    ap.add_argument("--steps_per_model_evaluation", type=int, default=100)
    ap.add_argument("--out", default="tube_runs/run")
    ap.add_argument("--device", default="cuda:0")
    return ap.parse_args(argv)


CONFIG_KEYS = ("dataset", "N", "dN", "recursive", "H_fwd", "H_rev", "loss", "alpha", "delta", "num_units", "num_layers", "activation",
               "softplus_beta", "seed", "validation_split")


def run_config(a):
    """The flags a later evaluation needs, as the dict written to config.json."""
    return {k: getattr(a, k) for k in CONFIG_KEYS}


def make_dataset(a):
    ds = construct_dataset(a.data)
    if a.dataset == "scalar":
        return DATASETS[a.dataset].from_folder(ds, N=a.N, dN=a.dN, recursive=a.recursive)
    if a.dataset == "scalar_horizon":
        return DATASETS[a.dataset].from_folder(ds, H_fwd=a.H_fwd, H_rev=a.H_rev)
    return DATASETS[a.dataset].from_folder(ds, N=a.N, dN=a.dN)


def eval_metrics(a, ev):
    if a.loss == "error":
        return {"Test Loss": float(ev[0])}
    t = f"(alpha={a.alpha:.1f})"
    return {f"Test Loss {t}": float(ev[0]), f"Proportion Correct, fw > w {t}": float(ev[1]),
            f"Mean Error when Correct, fw > w {t}": float(ev[2])}


def main(argv=None):
    a = parse_args(argv)
    torch.manual_seed(a.seed)
    np.random.seed(a.seed)
    dataset = make_dataset(a)
    train, test = dataset.random_split(a.validation_split)
    horizon = (a.H_fwd, a.H_rev) if a.dataset == "scalar_horizon" else None
    tr = HipTubeTrainer(dataset.input_dim, dataset.output_dim, num_units=a.num_units, num_layers=a.num_layers,
                        activation=a.activation, softplus_beta=a.softplus_beta, loss=a.loss, alpha=a.alpha, delta=a.delta,
                        lr=a.lr, gamma=a.gamma, step_size=a.step_size, batch_size=a.batch_size, seed=a.seed, horizon=horizon,
                        device=a.device)
    tr.set_data(train, test)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "config.json"), "w") as f:
        json.dump(run_config(a), f, indent=1)
    n = tr.n_train()
    steps_per_epoch = math.ceil(n / a.batch_size)          # DataLoader(shuffle=True), drop_last=False
    best = float("inf")
    step = 0
    with open(os.path.join(a.out, "metrics.jsonl"), "w") as mf:
        for epoch in range(a.num_epochs):
            tr.begin_epoch(epoch)
            first, pending, total = step + 1, {}, 0.0

            def flush(last):
                nonlocal first, total
                log = tr.read_log(first, last)                   # waits for the stream
                for s in range(first, last + 1):
                    row = log[s - first]
                    rec = {"step": s, "epoch": epoch, "loss_step": float(row[0]), "lr_step": float(row[1]),
                           "grad_norm": float(row[2])}
                    if s in pending:
                        rec.update(eval_metrics(a, pending.pop(s).cpu()))
                    total += float(row[0])
                    mf.write(json.dumps(rec) + "\n")
                first = last + 1

            for b in range(steps_per_epoch):
                tr.step(min(a.batch_size, n - b * a.batch_size))
                step += 1
                if step % a.steps_per_model_checkpoint == 0:
                    loss = float(tr.read_log(step, step)[0, 0])
                    sd = tr.state_dict()
                    torch.save(sd, os.path.join(a.out, "model.pth"))
                    if loss < best:
                        best = loss
                        torch.save(sd, os.path.join(a.out, "model_best.pth"))
                if step % a.steps_per_model_evaluation == 0:
                    pending[step] = tr.evaluate()
                if step - first + 1 == tr.log_cap:
                    flush(step)
            flush(step)
            lr_epoch = float(tr.read_log(step, step)[0, 1])
            mf.write(json.dumps({"step": step, "epoch": epoch, "loss_epoch": total / steps_per_epoch, "lr_epoch": lr_epoch}) + "\n")
            mf.flush()
            print(f"epoch {epoch}: loss {total / steps_per_epoch:.6f} lr {lr_epoch:.3g} ({steps_per_epoch} steps)", flush=True)
            dataset.update()
    sd = tr.state_dict()
    torch.save(sd, os.path.join(a.out, "model.pth"))
    if not os.path.isfile(os.path.join(a.out, "model_best.pth")):
        torch.save(sd, os.path.join(a.out, "model_best.pth"))
    tr.close()
    return a.out


if __name__ == "__main__":
    main()
