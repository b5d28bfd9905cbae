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

--sweep NAME=v1,v2,... (repeatable; NAME one of alpha, delta, activation, softplus_beta, lr, gamma, step_size, seed) trains the
cartesian product of the flags' values as one HipTubeSweep: every member in the same two launches per step, on one dataset split.
--out then holds one folder per member, <name>=<value>[,<name>=<value>...], with exactly what a single run writes (usable by
evaluate_tube.py --run as it is and bit-identical to the single run with those flags on the same split), and sweep.json: per
member its hyperparameters, final train loss and test metrics.

--dataset scalar_level | vector_level trains a level-conditioned tube: the coverage level is the model's
last input column, drawn per row and step from [--level_lo, --level_hi) on the device; --alpha is not read and the loss follows
the dataset.  On evaluation steps metrics.jsonl also holds the test coverage at the levels 0.5, 0.8, 0.9 and 0.95.  --sweep works
on top of it (over seed or lr, say).  The split is drawn once, seeded by --seed, or by the first
value of a swept seed: the member with that seed matches its single run, the other seeds train on that split too.

--dataset scalar_horizon_level --H_fwd F --H_rev R [--level_lo --level_hi] trains the level-conditioned one-shot tube (DESIGN.md
section 10.8): the scalar_horizon window item with the level appended, one level drawn per window and shared by its H_fwd outputs;
the loss is scalar_level (Huber per element), or vector_level with --loss vector_level (summed over the H_fwd outputs, then Huber).
H_rev must be at least 1.  It logs the same coverages and composes with --sweep and --sim like the flat level datasets.

--sim in place of --data trains straight from the ROM-on-ROM simulator (tube/rom_sim.py HipRomSim): the epochs
are collected, and the rows built, on the device; nothing is written to disk or copied to the host.  --sim_envs, --sim_T and --sim_seed
set the simulator (defaults: its own 8192 envs and 200 steps, seed 0); the data set holds the last --sim_resident epochs and after
every training epoch --sim_refresh new ones replace the oldest (the loop's dataset.update()), --sim_refresh 0 keeps it static: then
the run equals, bit for bit, collect_rom_sim_data.py with those flags followed by --data.  It composes with --sweep and the level
datasets; config.json records the sim flags.
"""
import argparse
import itertools
import json
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from legged_gym_dev_amd.tube.data import DATASETS, HORIZON_KINDS, HORIZON_LEVEL_KIND, LEVEL_KINDS, construct_dataset  # noqa: E402
from legged_gym_dev_amd.tube.trainer import HipTubeTrainer  # noqa: E402


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data", help="folder of epoch_<k>.pickle files")
    src.add_argument("--sim", action="store_true", default=argparse.SUPPRESS, help="train on epochs simulated on the device (HipRomSim)")
    for name, (tp, _, hlp) in SIM_FLAGS.items():
        ap.add_argument("--" + name, type=tp, default=argparse.SUPPRESS, help="--sim: " + hlp)
    ap.add_argument("--dataset", choices=sorted(DATASETS), default="scalar")
    ap.add_argument("--N", type=int, default=1)
    ap.add_argument("--dN", type=int, default=1)
    ap.add_argument("--recursive", action="store_true")
    ap.add_argument("--H_fwd", type=int, default=50)
    ap.add_argument("--H_rev", type=int, default=10)
    ap.add_argument("--loss", choices=["scalar", "vector", "scalar_horizon", "error", "scalar_level", "vector_level"], default="scalar",
                    help="a level dataset (scalar_level, vector_level) sets the loss of its own name")
    ap.add_argument("--level_lo", type=float, default=argparse.SUPPRESS,
                    help="level datasets: levels are drawn from [level_lo, level_hi) (default 0, 1)")
    ap.add_argument("--level_hi", type=float, default=argparse.SUPPRESS)
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
    ap.add_argument("--sweep", action="append", default=None, metavar="NAME=v1,v2,...",
                    help="train every combination of the listed values in one sweep (repeatable); NAME: " + ", ".join(SWEEP_FIELDS))
    a = ap.parse_args(argv)
    if a.dataset in LEVEL_KINDS:        # the level fields exist on a level-conditioned run only: every other run is as it was
        a.level_input, a.loss = True, a.dataset
        a.level_lo, a.level_hi = getattr(a, "level_lo", 0.0), getattr(a, "level_hi", 1.0)
    elif a.dataset == HORIZON_LEVEL_KIND:   # one level per window for its H_fwd outputs: Huber per element, or per window (vector_level)
        if a.loss not in ("scalar", "scalar_level", "vector_level"):
            ap.error("--dataset scalar_horizon_level takes --loss scalar_level (the default) or vector_level")
        a.level_input, a.loss = True, "vector_level" if a.loss == "vector_level" else "scalar_level"
        a.level_lo, a.level_hi = getattr(a, "level_lo", 0.0), getattr(a, "level_hi", 1.0)
    elif a.loss in LEVEL_KINDS or hasattr(a, "level_lo") or hasattr(a, "level_hi"):
        ap.error("--loss scalar_level / vector_level, --level_lo and --level_hi need --dataset scalar_level, vector_level or scalar_horizon_level")
    if getattr(a, "sim", False):        # the sim fields exist on a --sim run only: a --data run is as it was
        for name, (_, default, _) in SIM_FLAGS.items():
            setattr(a, name, getattr(a, name, default))
        if a.sim_envs < 2 or a.sim_resident < 1 or a.sim_refresh < 0 or (a.sim_T is not None and a.sim_T < 1):
            ap.error("--sim_envs must be at least 2 (every epoch's last env is dropped), --sim_resident and --sim_T at least 1, --sim_refresh at least 0")
    elif any(hasattr(a, name) for name in SIM_FLAGS):
        ap.error("--" + ", --".join(SIM_FLAGS) + " need --sim")
    try:
        a.sweep = parse_sweep(a.sweep)
    except ValueError as e:
        ap.error(str(e))
    return a


# --sim's sub-flags: name -> (type, default, help)
SIM_FLAGS = {"sim_envs": (int, 8192, "envs per epoch"), "sim_T": (int, None, "records per env and epoch (default: the simulator's 200)"),
             "sim_seed": (int, 0, "the simulator's seed"), "sim_resident": (int, 1, "epochs the data set holds"),
             "sim_refresh": (int, 1, "new epochs after every training epoch; 0: a static data set")}

# the per-member fields of a sweep (tube/sweep.py MEMBER_FIELDS) and how their values parse; every other flag is shared
SWEEP_FIELDS = {"alpha": float, "delta": float, "activation": str, "softplus_beta": float, "lr": float, "gamma": float,
                "step_size": int, "seed": int}
SHARED_ONLY = ("num_units", "num_layers", "loss", "batch_size", "H_fwd", "H_rev", "dataset", "N", "dN")


def parse_sweep(flags):
    """["alpha=0.8,0.95", "seed=1,2"] -> [("alpha", [0.8, 0.95]), ("seed", [1, 2])]; None without the flag."""
    if not flags:
        return None
    axes = []
    for f in flags:
        name, eq, vals = f.partition("=")
        if name in SHARED_ONLY:
            raise ValueError(f"--sweep {name}: the members of a sweep share {name}; sweep one of {', '.join(SWEEP_FIELDS)}")
        if name not in SWEEP_FIELDS:
            raise ValueError(f"--sweep {name}: unknown field; one of {', '.join(SWEEP_FIELDS)}")
        if not eq or not vals or any(v == "" for v in vals.split(",")):
            raise ValueError(f"--sweep {f}: expected {name}=v1,v2,...")
        if name in [n for n, _ in axes]:
            raise ValueError(f"--sweep {name}: given twice")
        try:
            parsed = [SWEEP_FIELDS[name](v) for v in vals.split(",")]
        except ValueError:
            raise ValueError(f"--sweep {f}: values must parse as {SWEEP_FIELDS[name].__name__}") from None
        if name == "activation" and any(v not in ("relu", "softplus", "tanh", "elu") for v in parsed):
            raise ValueError(f"--sweep {f}: activation is one of relu, softplus, tanh, elu")
        if len(set(parsed)) != len(parsed):
            raise ValueError(f"--sweep {f}: a value is repeated")
        axes.append((name, parsed))
    return axes


def sweep_members(axes):
    """The cartesian product of the axes, first flag slowest: [(folder name, {field: value})]."""
    out = []
    for combo in itertools.product(*(vals for _, vals in axes)):
        m = {name: v for (name, _), v in zip(axes, combo)}
        out.append((",".join(f"{k}={v}" for k, v in m.items()), m))
    return out


CONFIG_KEYS = ("dataset", "N", "dN", "recursive", "H_fwd", "H_rev", "loss", "alpha", "delta", "num_units", "num_layers", "activation",
               "softplus_beta", "seed", "validation_split")
LEVEL_CONFIG_KEYS = ("level_input", "level_lo", "level_hi")     # a level-conditioned run records these too
SIM_CONFIG_KEYS = ("sim",) + tuple(SIM_FLAGS)                  # a --sim run records these too
EVAL_LEVELS = (0.5, 0.8, 0.9, 0.95)     # a level-conditioned run logs its test coverage at these on every evaluation step


def run_config(a):
    """The flags a later evaluation needs, as the dict written to config.json."""
    return {k: getattr(a, k) for k in CONFIG_KEYS + (LEVEL_CONFIG_KEYS if _level(a) else ()) + (SIM_CONFIG_KEYS if _sim(a) else ())}


def _level(a):
    return getattr(a, "level_input", False)


def _sim(a):
    return getattr(a, "sim", False)


def make_sim_dataset(a):
    """--sim: a HipRomSim of the reference's double_single_int configuration and the data set that lives on the device with it."""
    from legged_gym_dev_amd.tube.device_data import SimTubeDataset
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg
    cfg = RomSimCfg()
    cfg.env.num_envs = a.sim_envs
    sim = HipRomSim(cfg, seed=a.sim_seed, device=a.device)
    return SimTubeDataset(sim, a.dataset, N=a.N, dN=a.dN, recursive=a.recursive, H_fwd=a.H_fwd, H_rev=a.H_rev, T=a.sim_T,
                          resident_epochs=a.sim_resident, refresh=a.sim_refresh)


def make_dataset(a):
    if _sim(a):
        return make_sim_dataset(a)
    ds = construct_dataset(a.data)
    if a.dataset in ("scalar", "scalar_level"):
        return DATASETS[a.dataset].from_folder(ds, N=a.N, dN=a.dN, recursive=a.recursive)
    if a.dataset in HORIZON_KINDS:
        return DATASETS[a.dataset].from_folder(ds, H_fwd=a.H_fwd, H_rev=a.H_rev)
    return DATASETS[a.dataset].from_folder(ds, N=a.N, dN=a.dN)


def eval_metrics(a, ev):
    if a.loss == "error":
        return {"Test Loss": float(ev[0])}
    if _level(a):                       # ev: the drawn-level evaluation, then one fixed-level evaluation per EVAL_LEVELS entry
        out = {"Test Loss (level drawn)": float(ev[0])}
        for i, lv in enumerate(EVAL_LEVELS):
            out[f"Proportion Correct, fw > w (level={lv:.2f})"] = float(ev[4 * (i + 1) + 1])
        return out
    t = f"(alpha={a.alpha:.1f})"
    return {f"Test Loss {t}": float(ev[0]), f"Proportion Correct, fw > w {t}": float(ev[1]),
            f"Mean Error when Correct, fw > w {t}": float(ev[2])}


def main(argv=None):
    a = parse_args(argv)
    members = sweep_members(a.sweep) if a.sweep else None
    # one split for the whole run: a swept seed's first value stands in for --seed here
    split_seed = dict(a.sweep)["seed"][0] if a.sweep and "seed" in dict(a.sweep) else a.seed
    torch.manual_seed(split_seed)
    np.random.seed(split_seed)
    dataset = make_dataset(a)
    train, test = dataset.random_split(a.validation_split)
    horizon = (a.H_fwd, a.H_rev) if a.dataset in HORIZON_KINDS else None
    shared = dict(num_units=a.num_units, num_layers=a.num_layers, activation=a.activation, softplus_beta=a.softplus_beta, loss=a.loss,
                  alpha=a.alpha, delta=a.delta, lr=a.lr, gamma=a.gamma, step_size=a.step_size, batch_size=a.batch_size, seed=a.seed,
                  horizon=horizon, device=a.device)
    if _level(a):
        shared.update(level_lo=a.level_lo, level_hi=a.level_hi)
    if members is None:
        tr = HipTubeTrainer(dataset.input_dim, dataset.output_dim, **shared)
        runs = [(a, tr, a.out)]                                    # (flags, what answers read_log / state_dict, folder)
    else:
        from legged_gym_dev_amd.tube.sweep import HipTubeSweep
        tr = HipTubeSweep(dataset.input_dim, dataset.output_dim, members=[m for _, m in members], **shared)
        runs = [(argparse.Namespace(**{**vars(a), **m}), tr.member(k), os.path.join(a.out, name)) for k, (name, m) in enumerate(members)]
    tr.set_data(train, test)
    K = len(runs)
    for ma, _, out in runs:
        os.makedirs(out, exist_ok=True)
        with open(os.path.join(out, "config.json"), "w") as f:
            json.dump(run_config(ma), f, indent=1)
    if members is not None:
        print(f"sweep of {K} members; the dataset split is drawn with seed {split_seed}", flush=True)
    n = tr.n_train()
    steps_per_epoch = math.ceil(n / a.batch_size)          # DataLoader(shuffle=True), drop_last=False
    best = [float("inf")] * K
    step = 0
    mfs = [open(os.path.join(out, "metrics.jsonl"), "w") for _, _, out in runs]
    try:
        for epoch in range(a.num_epochs):
            tr.begin_epoch(epoch)
            first, pending, total = step + 1, {}, [0.0] * K

            def flush(last):
                nonlocal first
                for k, (ma, mem, _) in enumerate(runs):
                    log = mem.read_log(first, last)                  # waits for the stream
                    for s in range(first, last + 1):
                        row = log[s - first]
                        rec = {"step": s, "epoch": epoch, "loss_step": float(row[0]), "lr_step": float(row[1]),
                               "grad_norm": float(row[2])}
                        if s in pending:
                            rec.update(eval_metrics(ma, pending[s][k]))
                        total[k] += float(row[0])
                        mfs[k].write(json.dumps(rec) + "\n")
                for s in [s for s in pending if s <= last]:
                    del pending[s]
                first = last + 1

            for b in range(steps_per_epoch):
                tr.step(min(a.batch_size, n - b * a.batch_size))
                step += 1
                if step % a.steps_per_model_checkpoint == 0:
                    for k, (_, mem, out) in enumerate(runs):
                        loss = float(mem.read_log(step, step)[0, 0])
                        sd = mem.state_dict()
                        torch.save(sd, os.path.join(out, "model.pth"))
                        if loss < best[k]:
                            best[k] = loss
                            torch.save(sd, os.path.join(out, "model_best.pth"))
                if step % a.steps_per_model_evaluation == 0:
                    ev = tr.evaluate().reshape(K, 4)
                    if _level(a):
                        ev = torch.cat([ev] + [tr.eval_level(lv).reshape(K, 4) for lv in EVAL_LEVELS], dim=1)
                    pending[step] = _LazyRows(ev, K)
                if step - first + 1 == tr.log_cap:
                    flush(step)
            flush(step)
            for k, (_, mem, _) in enumerate(runs):
                lr_epoch = float(mem.read_log(step, step)[0, 1])
                mfs[k].write(json.dumps({"step": step, "epoch": epoch, "loss_epoch": total[k] / steps_per_epoch, "lr_epoch": lr_epoch}) + "\n")
                mfs[k].flush()
                tag = "" if members is None else f" [{members[k][0]}]"
                print(f"epoch {epoch}{tag}: loss {total[k] / steps_per_epoch:.6f} lr {lr_epoch:.3g} ({steps_per_epoch} steps)", flush=True)
            dataset.update()
            if getattr(dataset, "changed", False) and epoch + 1 < a.num_epochs:      # fresh rows, the same split: n_train is as it was
                tr.set_data(*dataset.split())
                dataset.changed = False
    finally:
        for mf in mfs:
            mf.close()
    for _, mem, out in runs:
        sd = mem.state_dict()
        torch.save(sd, os.path.join(out, "model.pth"))
        if not os.path.isfile(os.path.join(out, "model_best.pth")):
            torch.save(sd, os.path.join(out, "model_best.pth"))
    if members is not None:
        ev = tr.evaluate().cpu()
        summary = {"split_seed": split_seed, "steps": step, "members": []}
        for k, ((name, m), (ma, mem, _)) in enumerate(zip(members, runs)):
            summary["members"].append({"name": name, "hyperparameters": {f: getattr(ma, f) for f in SWEEP_FIELDS},
                                       "final_train_loss": float(mem.read_log(step, step)[0, 0]) if step else None,
                                       "test": {"loss": float(ev[k, 0]), "proportion_fw_gt_w": float(ev[k, 1]),
                                                "mean_error_fw_gt_w": float(ev[k, 2]), "rows": int(ev[k, 3])}})
        with open(os.path.join(a.out, "sweep.json"), "w") as f:
            json.dump(_nan_to_none(summary), f, indent=1, allow_nan=False)
    tr.close()
    if _sim(a):
        dataset.sim.close()
    return a.out


class _LazyRows:
    """An evaluation's device result, (K, 4) -- (K, 4 + 4 levels) on a level-conditioned run --, read back once when the log is written."""

    def __init__(self, ev, K):
        self.ev, self.K, self.host = ev, K, None

    def __getitem__(self, k):
        if self.host is None:
            self.host = self.ev.cpu().reshape(self.K, -1)
        return self.host[k]


def _nan_to_none(o):
    if isinstance(o, dict):
        return {k: _nan_to_none(v) for k, v in o.items()}
    if isinstance(o, list):
        return [_nan_to_none(v) for v in o]
    return None if isinstance(o, float) and o != o else o


if __name__ == "__main__":
    main()
