"""Evaluate a trained tube model on recorded ROM tracking data: the numerical content of the reference's
deep_tube_learning/evaluation/evaluate_tube.py, evaluate_error_dyn.py, evaluate_tube_oneshot.py, evaluate_tube_simple.py and
evaluate_error_dyn_simple.py on the HIP kernels, without
wandb or hydra, on recorded data (--data) or on a fresh simulation (--sim).

    python legged_gym_dev_amd/scripts/evaluate_tube.py --run tube_runs/run0 (--data rom_tracking_data/run1 | --sim) \\
        [--checkpoint best|latest] [--horizon K] [--window_stride S] [--plot] [--out DIR] [--calibration [PATH]] \\
        [--age_calibration [PATH]]

The run's config.json (train_tube.py writes it) says how the model and its inputs are built; for a run without one, give
--dataset, --activation and the other train_tube.py flags here (a flag given here replaces the file's value).

Flat datasets (scalar, vector, error_dynamics): the one-step prediction fw_single = model(data) on every row, and the closed-loop
roll-out fw[t+1] = model([fw[t], rest of row t]) -- one launch for all envs and steps -- reseeded from the data at t = 0, after
every done and, with --horizon K, every K steps.  Windowed rows (N > 1 with recursive scalar, vector or error_dynamics) hold the
fed-back quantity in every delayed tap too: tap i takes the roll-out's own output of i rows earlier once that row lies after the
last reseed (HipTubeModel.rollout_window; evaluate_tube_simple.py:62-72, evaluate_error_dyn_simple.py:44-50).  eval.json's
feedback_dN is that distance in rows, 1 for every dataset (tube/data.py feedback_layout).  scalar_horizon: the one-shot
prediction at the window starts H_rev, H_rev + S, ... of every env, scored overall and per step ahead.  Writes eval.json to --out (default: the run folder) and prints the
reference's "Total Success Rate" (and, for error_dynamics, "Mean Error" / "Mean One Step Error") lines.

A level-conditioned run (config.json level_input; datasets scalar_level, vector_level) is scored per coverage level (--levels,
default 0.5,0.8,0.9,0.95): eval.json's "levels" has one entry per level with the one-step metrics -- every level of every row from one
predict_levels launch -- and the closed-loop roll-out with the level column filled.  The success rate rises with the level but need
not equal it.  A level-conditioned one-shot run (dataset scalar_horizon_level; section 10.8) is scored per level
on the windows scalar_horizon scores: "levels" has one entry per level with the one-shot metrics -- every level of every window from
one predict_windows_levels launch -- and "level_crossings" is the share of (window, step ahead, pair of adjacent levels) where the
prediction falls as the level rises.

--sim in place of --data scores the model on fresh robots, as the reference's evaluation scripts do: --sim_resident epochs (default 1)
of --sim_envs envs x --sim_T steps are simulated then and there by the ROM-on-ROM simulator (tube/rom_sim.py HipRomSim) with
--sim_seed, whose default differs from the run's training seeds, and the rows are built on the device (tube/device_data.py); every
env is scored (the simulator never sets done).  --sim_envs and --sim_T default to the run's own sim flags, if it has them, then to the
simulator's 8192 x 200.  eval.json then holds "source": "sim" and the sim flags instead of "data".

--calibration [PATH] (default PATH: the run's calibration.json, which calibrate_tube.py writes) scores the conformally calibrated
tube as well: beside every metrics dict eval.json gains a "calibrated" dict with the same metrics on Calibration.apply'd
predictions (prediction + offset), the offsets used and "covered", the count of scored elements with w - fw <= offset (the exact
form of the comparison).  Evaluating on the calibration's own --sim_seed or --data folder is refused: coverage measured on the rows
the offsets were fitted on says nothing.  Without the flag eval.json and the printed lines are what they were.

--age_calibration [PATH] (flat datasets; default PATH: the run's calibration_age.json, which calibrate_tube.py --by_age writes) scores
the roll-out with one offset per age of the fed-back state: eval.json gains "calibrated_by_age" with, per
coverage, the roll-out metrics on prediction + offset[age], the exact count "covered" and its curve over ages, and "trajectory": the
fraction of envs whose every kept step is covered (tube/evaluate.py trajectory_metrics), per column, for the raw roll-out, for the
per-age tube and, when the calibration holds a trajectory margin, for the per-age + margin tube.  The calibration's own --sim_seed or
--data folder is refused as for --calibration.  Without the flag eval.json and the printed lines are what they were.

Deliberate deviations from the reference scripts:
  * evaluate_tube.py:53 feeds the full z[t] to a model that ScalarTubeDataset trained on z[:, 2:] (the input widths differ).  The
    rows here are the dataset's own (tube/data.py sequences()): what the model was trained on.
  * evaluate_tube_oneshot.py:111 divides a sum over 100 windows by n_robots = 2.  The success rate here is a mean over the windows.
  * The scripts score one robot and prepend the initial value to the prediction; here every env is scored, prediction t against
    the dataset's target t (the quantity at t + 1), and done rows are left out.
  * evaluate_error_dyn_simple.py:48 indexes fe[t - n*dN] with a negative index while t < n*dN, which Python wraps to the end of
    the array.  Here such a tap keeps the dataset's own front padding: what the model was trained on.
  * The same line delays tap n by n*dN raw samples, while datasets.py get_slice, which built the training rows, keeps every
    dN-th sample in every tap, so that tap n trails tap 0 by n rows of a subsampled series.  The two agree for dN = 1 (every
    reference configuration); for dN > 1 the rows and the tap distance here are the dataset's: what the model was trained on.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import torch  # noqa: E402

from legged_gym_dev_amd.tube import evaluate as ev  # noqa: E402
from legged_gym_dev_amd.tube.data import (DATASETS, HORIZON_KINDS, HORIZON_LEVEL_KIND, LEVEL_KINDS, construct_dataset,  # noqa: E402
                                          feedback_layout, sequences)
from legged_gym_dev_amd.tube.model import CONFIG_NAME, HipTubeModel, read_config  # noqa: E402

DEFAULTS = {"N": 1, "dN": 1, "recursive": False, "H_fwd": 50, "H_rev": 10, "softplus_beta": 1.0}


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--run", required=True, help="folder train_tube.py wrote (model.pth, model_best.pth, config.json)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data", help="folder of epoch_<k>.pickle files")
    src.add_argument("--sim", action="store_true", help="score fresh robots simulated on the device (HipRomSim)")
    ap.add_argument("--sim_envs", type=int, default=None)
    ap.add_argument("--sim_T", type=int, default=None)
    ap.add_argument("--sim_seed", type=int, default=None, help="default: the smallest seed >= 1 the run did not train with")
    ap.add_argument("--sim_resident", type=int, default=None, help="epochs to simulate (default 1)")
    ap.add_argument("--sim_refresh", type=int, default=None, help="accepted for symmetry with train_tube.py; not read")
    ap.add_argument("--checkpoint", choices=["best", "latest"], default="best")
    ap.add_argument("--horizon", type=int, default=None, help="flat datasets: reseed the roll-out every K steps")
    ap.add_argument("--window_stride", type=int, default=1, help="scalar_horizon: distance between window starts")
    ap.add_argument("--levels", default=None, help="level-conditioned runs: comma-separated coverage levels (default 0.5,0.8,0.9,0.95)")
    ap.add_argument("--calibration", nargs="?", const="", default=None, metavar="PATH",
                    help="also score the calibrated tube; PATH defaults to the run's calibration.json")
    ap.add_argument("--age_calibration", nargs="?", const="", default=None, metavar="PATH",
                    help="flat datasets: also score the per-age calibrated roll-out; PATH defaults to the run's calibration_age.json")
    ap.add_argument("--plot", action="store_true", help="save w / fw / fw_single PNGs per env to --out")
    ap.add_argument("--plot_envs", type=int, default=4)
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    # what config.json holds; for runs older than it
    ap.add_argument("--dataset", choices=sorted(DATASETS), default=None)
    ap.add_argument("--N", type=int, default=None)
    ap.add_argument("--dN", type=int, default=None)
    ap.add_argument("--recursive", action="store_true", default=None)
    ap.add_argument("--H_fwd", type=int, default=None)
    ap.add_argument("--H_rev", type=int, default=None)
    ap.add_argument("--activation", choices=["relu", "softplus", "tanh", "elu"], default=None)
    ap.add_argument("--softplus_beta", type=float, default=None)
    return ap.parse_args(argv)


def resolve_config(a):
    """config.json of the run, with the flags given here on top; without the file, --dataset and --activation are required."""
    path = os.path.join(a.run, CONFIG_NAME)
    if os.path.isfile(path):
        cfg = read_config(a.run)
    elif a.dataset is None or a.activation is None:
        raise FileNotFoundError(f"{path} is missing: give --dataset and --activation (and the window / horizon flags the run used)")
    else:
        cfg = {}
    for k in ("dataset", "N", "dN", "recursive", "H_fwd", "H_rev", "activation", "softplus_beta"):
        if getattr(a, k) is not None:
            cfg[k] = getattr(a, k)
    return {**DEFAULTS, **cfg}


def sim_flags(a, cfg):
    """The sim flags of an evaluation: what is given here, else the run's own (config.json of a --sim run), else the defaults."""
    used = {cfg.get("seed"), cfg.get("sim_seed")}
    f = {"sim_envs": a.sim_envs or cfg.get("sim_envs") or 8192, "sim_T": a.sim_T or cfg.get("sim_T"), "sim_resident": a.sim_resident or 1,
         "sim_seed": a.sim_seed if a.sim_seed is not None else min(s for s in range(1, 4) if s not in used)}
    if f["sim_envs"] < 1 or f["sim_resident"] < 1 or (f["sim_T"] is not None and f["sim_T"] < 1):
        raise ValueError(f"--sim_envs, --sim_T and --sim_resident must be at least 1; got {f}")
    return f


def sim_records(f, device):
    """Fresh robots: f["sim_resident"] epochs of the ROM-on-ROM simulator as one record dict of device tensors."""
    from legged_gym_dev_amd.tube.rom_sim import HipRomSim, RomSimCfg
    rc = RomSimCfg()
    rc.env.num_envs = f["sim_envs"]
    sim = HipRomSim(rc, seed=f["sim_seed"], device=device)
    try:
        recs = [sim.collect_epoch(f["sim_T"]) for _ in range(f["sim_resident"])]
        torch.cuda.synchronize(sim.device)
    finally:
        sim.close()
    return recs[0] if len(recs) == 1 else {k: torch.cat([r[k] for r in recs], dim=0) for k in ("z", "pz_x", "v", "done")}


def rows(kind, raw, win, dev):
    """sequences(kind, raw, **win) on `dev`: built there when the records already live on a device, on the host otherwise."""
    if isinstance(raw["z"], torch.Tensor) and raw["z"].is_cuda:
        from legged_gym_dev_amd.tube.device_data import build_rows
        data, target = build_rows(raw, kind, compact=False, **win)
        return data, target, raw["done"].ne(0)
    return tuple(t.to(dev) for t in sequences(kind, raw, **win))


def load_calibration(a, cfg, sim):
    """The Calibration --calibration names, or None without the flag.  Refuses, with the reason, a calibration of another kind of
    model and an evaluation on the calibration's own robots."""
    if a.calibration is None:
        return None
    from legged_gym_dev_amd.tube.calibrate import Calibration, default_path
    path = a.calibration or default_path(a.run)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} is missing: calibrate_tube.py --run {a.run} writes it")
    c = Calibration.load(path)
    kind = "levels" if cfg["dataset"] in LEVEL_KINDS else "horizon_levels" if cfg["dataset"] == HORIZON_LEVEL_KIND \
        else "horizon" if cfg["dataset"] == "scalar_horizon" else "flat"
    if c.kind != kind or c.provenance.get("dataset", cfg["dataset"]) != cfg["dataset"]:
        raise ValueError(f"{path} calibrates a {c.provenance.get('dataset', c.kind)} model; the run is {cfg['dataset']}")
    refuse_own_rows(c, path, a, sim)
    return c


def refuse_own_rows(c, path, a, sim):
    """An evaluation on the robots or rows the calibration c (read from path) was fitted on is refused."""
    if sim is not None and c.provenance.get("source") == "sim" and c.provenance.get("sim_seed") == sim["sim_seed"]:
        raise ValueError(f"--sim_seed {sim['sim_seed']} is the seed {path} was calibrated on: coverage on the calibration's own robots "
                         "says nothing about fresh ones; give another --sim_seed")
    if a.data is not None and c.provenance.get("data") == os.path.abspath(a.data):
        raise ValueError(f"--data {a.data} is the folder {path} was calibrated on: coverage on the calibration's own rows says nothing "
                         "about fresh ones; give another folder")


def load_age_calibration(a, cfg, sim):
    """The AgeCalibration --age_calibration names, or None without the flag; load_calibration's refusals."""
    if a.age_calibration is None:
        return None
    from legged_gym_dev_amd.tube.calibrate import FLAT_KINDS, AgeCalibration, default_age_path
    if cfg["dataset"] not in FLAT_KINDS:
        raise ValueError(f"--age_calibration: per-age offsets exist for the roll-out of the flat kinds ({', '.join(FLAT_KINDS)}); the run is {cfg['dataset']}")
    path = a.age_calibration or default_age_path(a.run)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"{path} is missing: calibrate_tube.py --run {a.run} --by_age writes it")
    c = AgeCalibration.load(path)
    if c.provenance.get("dataset", cfg["dataset"]) != cfg["dataset"]:
        raise ValueError(f"{path} calibrates a {c.provenance['dataset']} model; the run is {cfg['dataset']}")
    refuse_own_rows(c, path, a, sim)
    return c


def calibrated_by_age(c, fw, target, done, reseed):
    """eval.json's "calibrated_by_age": per coverage the roll-out metrics on the per-age tube, and the trajectory rates of the raw
    roll-out, the per-age tube and (with a stored margin) the per-age + margin tube."""
    age = ev.steps_since(reseed)
    keep = ~done.bool()[:, :, None]
    n_age = int(age[keep[:, :, 0]].max()) + 1 if bool(keep.any()) else 1
    res = {"max_age": c.max_age, "coverages": c.coverages, "counts": c.counts, "ranks": c.ranks, "rollout": [],
           "trajectory": {"raw": ev.trajectory_metrics(fw >= target, done), "by_age": []}}
    if c.margin is not None:
        res.update({"margin": c.margin.tolist(), "margin_n": c.margin_n, "margin_ranks": c.margin_ranks})
        res["trajectory"]["by_age_margin"] = []
    for cv in c.coverages:
        cov = c.covers(fw, target, age, cv)
        m = ev.tube_metrics(c.apply(fw, age, cv), target, done, reseed)
        m["offset_by_age"] = c.offsets[c.index(cv)].tolist()
        m["covered"] = int((cov & keep).sum())
        by_age = torch.zeros(n_age, dtype=torch.int64, device=fw.device).index_add_(0, age.reshape(-1).clamp(max=n_age - 1),
                                                                                   (cov & keep).sum(dim=2).reshape(-1))
        m["covered_by_age"] = by_age.tolist()
        res["rollout"].append(m)
        res["trajectory"]["by_age"].append(ev.trajectory_metrics(cov, done))
        if c.margin is not None:
            res["trajectory"]["by_age_margin"].append(ev.trajectory_metrics(c.covers(fw, target, age, cv, trajectory=True), done))
    return _cal_safe(res)


def _cal_safe(o):
    """inf (the offset of a set with too few calibration rows, and what it does to a mean) becomes the string "inf"."""
    if isinstance(o, dict):
        return {k: _cal_safe(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_cal_safe(v) for v in o]
    return ("inf" if o > 0 else "-inf") if isinstance(o, float) and o in (float("inf"), float("-inf")) else o


def calibrated_tube(c, fw, target, done, reseed, coverage, part, level=None):
    """tube_metrics of the calibrated prediction, the offsets, and the exact count of covered scored elements."""
    m = ev.tube_metrics(c.apply(fw, coverage, level, part), target, done, reseed)
    m["offset"] = c.offset(coverage, level, part).tolist()
    m["covered"] = int((c.covers(fw, target, coverage, level, part) & ~done.bool()[:, :, None]).sum())
    return _cal_safe(m)


def evaluate_flat(model, cfg, raw, horizon, dev, calib=None, age_calib=None):
    kind = cfg["dataset"]
    win = {"N": cfg["N"], "dN": cfg["dN"]}
    if kind == "scalar":
        win["recursive"] = cfg["recursive"]
    data, target, done = rows(kind, raw, win, dev)
    fb, taps, lag, stride = feedback_layout(kind, cfg["N"], cfg["dN"], cfg["recursive"], n=raw["z"].shape[-1], m=raw["v"].shape[-1])
    E, T, I = data.shape
    fw_single = model.predict(data.reshape(E * T, I)).reshape(E, T, -1)
    reseed = ev.reseed_mask(done, horizon)
    fw = model.rollout_window(data, fb, taps, lag, stride, reseed)
    ed = kind == "error_dynamics"
    res = {"one_step": ev.tube_metrics(fw_single, target, done, None, ed), "rollout": ev.tube_metrics(fw, target, done, reseed, ed),
           "feedback_width": fb, "feedback_taps": taps, "feedback_dN": lag, "feedback_stride": stride, "envs": E, "steps_per_env": T, "reseed_every": horizon}
    if calib is not None:
        res["calibrated"] = {"n": calib.n, "coverages": calib.coverages, "ranks": calib.ranks,
                             "one_step": [calibrated_tube(calib, fw_single, target, done, None, cv, "one_step") for cv in calib.coverages],
                             "rollout": [calibrated_tube(calib, fw, target, done, reseed, cv, "rollout") for cv in calib.coverages]}
    if age_calib is not None:
        res["calibrated_by_age"] = calibrated_by_age(age_calib, fw, target, done, reseed)
    return res, {"w": target, "fw": fw, "fw_single": fw_single, "done": done}


DEFAULT_LEVELS = (0.5, 0.8, 0.9, 0.95)


def evaluate_levels(model, cfg, raw, horizon, dev, levels, calib=None):
    """evaluate_flat per level of a level-conditioned model: the one-step predictions of all levels from one predict_levels
    launch, the roll-out per level on the rows with the column filled."""
    kind = cfg["dataset"]
    win = {"N": cfg["N"], "dN": cfg["dN"]}
    if LEVEL_KINDS[kind] == "scalar":
        win["recursive"] = cfg["recursive"]
    data, target, done = rows(kind, raw, win, dev)
    fb, taps, lag, stride = feedback_layout(kind, cfg["N"], cfg["dN"], cfg["recursive"], n=raw["z"].shape[-1], m=raw["v"].shape[-1])
    E, T, I = data.shape
    single = model.predict_levels(data.reshape(E * T, I), torch.tensor(levels, dtype=torch.float32))      # (E T, levels, out)
    reseed = ev.reseed_mask(done, horizon)
    per_level, series = [], None
    for i, lv in enumerate(levels):
        fw_single = single[:, i, :].reshape(E, T, -1)
        fw = model.rollout_window(model.with_level(data, lv), fb, taps, lag, stride, reseed)
        per_level.append({"level": lv, "one_step": ev.tube_metrics(fw_single, target, done), "rollout": ev.tube_metrics(fw, target, done, reseed)})
        if calib is not None:
            per_level[-1]["calibrated"] = {"n": calib.n, "rank": calib.ranks[calib.index(lv)],
                                           "one_step": calibrated_tube(calib, fw_single, target, done, None, lv, "one_step"),
                                           "rollout": calibrated_tube(calib, fw, target, done, reseed, lv, "rollout")}
        if i == len(levels) - 1:
            series = {"w": target, "fw": fw, "fw_single": fw_single, "done": done}
    res = {"levels": per_level, "feedback_width": fb, "feedback_taps": taps, "feedback_dN": lag, "feedback_stride": stride, "envs": E,
           "steps_per_env": T, "reseed_every": horizon}
    return res, series


def horizon_windows(cfg, raw, stride, dev, kind="scalar_horizon"):
    """The windows a one-shot evaluation scores: (ds, env, start, target (windows, H_fwd), starts) with the starts H_rev,
    H_rev + stride, ... of every env, env-major."""
    if isinstance(raw["z"], torch.Tensor) and raw["z"].is_cuda:
        from legged_gym_dev_amd.tube.device_data import from_records
        ds = from_records(DATASETS[kind], raw, H_fwd=cfg["H_fwd"], H_rev=cfg["H_rev"])
    else:
        ds = DATASETS[kind].from_folder(raw, H_fwd=cfg["H_fwd"], H_rev=cfg["H_rev"])
    Hf, Hr = ds.H_fwd, ds.H_rev
    E, T = ds.w.shape
    starts = torch.arange(Hr, T - Hf, max(1, stride), dtype=torch.int32)        # targets reach w[start + H_fwd] <= w[T - 1]
    if starts.numel() == 0:
        raise ValueError(f"episodes of {T - Hr} steps are shorter than H_fwd + 1 = {Hf + 1}")
    env = torch.arange(E, dtype=torch.int32).repeat_interleave(starts.numel())
    start = starts.repeat(E)
    w = ds.w.to(dev)
    idx = start.to(dev).long()[:, None] + torch.arange(1, Hf + 1, device=dev)[None, :]
    return ds, env, start, w[env.to(dev).long()[:, None], idx], starts


def evaluate_horizon_levels(model, cfg, raw, stride, dev, levels, calib=None):
    """evaluate_horizon per level of a level-conditioned one-shot model: every level of every window from
    one predict_windows_levels launch, one window_metrics entry per level, and level_crossings over the adjacent levels."""
    ds, env, start, target, starts = horizon_windows(cfg, raw, stride, dev, HORIZON_LEVEL_KIND)
    E, Hf = ds.w.shape[0], ds.H_fwd
    fw = model.predict_windows_levels(ds, env, start, torch.tensor(levels, dtype=torch.float32))          # (windows, levels, H_fwd)
    per_level = []
    for i, lv in enumerate(levels):
        per_level.append({"level": lv, "one_shot": ev.window_metrics(fw[:, i, :], target)})
        if calib is not None:
            per_level[-1]["calibrated"] = {"n": calib.n, "rank": calib.ranks[calib.index(level=lv)], "one_shot": _cal_safe(
                {**ev.window_metrics(calib.apply(fw[:, i, :], level=lv), target), "offset": calib.offset(level=lv).tolist(),
                 "covered_by_step": calib.covers(fw[:, i, :], target, level=lv).sum(dim=0).tolist()})}
    res = {"levels": per_level, "level_crossings": ev.level_crossings(fw, levels), "envs": E, "windows_per_env": int(starts.numel()),
           "window_stride": stride}
    return res, {"w": target.reshape(E, -1, Hf), "fw": fw[:, -1, :].reshape(E, -1, Hf), "fw_levels": fw, "target": target, "starts": starts}


def evaluate_horizon(model, cfg, raw, stride, dev, calib=None):
    ds, env, start, target, starts = horizon_windows(cfg, raw, stride, dev)
    E, Hf = ds.w.shape[0], ds.H_fwd
    fw = model.predict_windows(ds, env, start)
    res = {"one_shot": ev.window_metrics(fw, target), "envs": E, "windows_per_env": int(starts.numel()), "window_stride": stride}
    if calib is not None:
        res["calibrated"] = {"n": calib.n, "coverages": calib.coverages, "ranks": calib.ranks, "one_shot": [_cal_safe(
            {**ev.window_metrics(calib.apply(fw, cv), target), "offset": calib.offset(cv).tolist(),
             "covered_by_step": calib.covers(fw, target, cv).sum(dim=0).tolist()}) for cv in calib.coverages]}
    return res, {"w": target.reshape(E, -1, Hf), "fw": fw.reshape(E, -1, Hf), "starts": starts}


def plot(kind, series, out, n_envs):
    import matplotlib
    matplotlib.use("Agg")
    import matplotlib.pyplot as plt
    files = []
    for e in range(min(n_envs, series["w"].shape[0])):
        fig, ax = plt.subplots(figsize=(9, 4))
        if kind in HORIZON_KINDS:
            for k in range(0, series["w"].shape[1], max(1, series["w"].shape[1] // 8)):
                t = int(series["starts"][k]) + 1 + torch.arange(series["w"].shape[2])
                ax.plot(t, series["w"][e, k].cpu(), "b", label="w" if k == 0 else None)
                ax.plot(t, series["fw"][e, k].cpu(), "k", label="fw (one shot)" if k == 0 else None)
        else:
            for name, style in (("w", "-"), ("fw", "-"), ("fw_single", "--")):
                ax.plot(series[name][e].cpu().norm(dim=-1) if series[name].shape[-1] > 1 else series[name][e, :, 0].cpu(), style, label=name)
        ax.set_xlabel("Time")
        ax.set_ylabel("Tube Size")
        ax.legend()
        files.append(os.path.join(out, f"tube_env{e}.png"))
        fig.savefig(files[-1], dpi=100)
        plt.close(fig)
    return files


def _json_safe(o):
    """nan (an age or a selection with nothing in it) becomes null: eval.json stays strict JSON."""
    if isinstance(o, dict):
        return {k: _json_safe(v) for k, v in o.items()}
    if isinstance(o, (list, tuple)):
        return [_json_safe(v) for v in o]
    return None if isinstance(o, float) and o != o else o


def main(argv=None):
    a = parse_args(argv)
    cfg = resolve_config(a)
    dev = torch.device(a.device)
    out = a.out or a.run
    os.makedirs(out, exist_ok=True)
    horizon = (cfg["H_fwd"], cfg["H_rev"]) if cfg["dataset"] in HORIZON_KINDS else None
    sim = sim_flags(a, cfg) if a.sim else None
    calib = load_calibration(a, cfg, sim)
    extra = {} if calib is None else {"calib": calib}
    age_calib = load_age_calibration(a, cfg, sim)
    if age_calib is not None:
        extra["age_calib"] = age_calib
    model = HipTubeModel.load(a.run, checkpoint=a.checkpoint, activation=cfg["activation"], softplus_beta=cfg["softplus_beta"],
                              horizon=horizon, device=a.device, level_input=DATASETS[cfg["dataset"]].conditioned)
    raw = sim_records(sim, a.device) if a.sim else construct_dataset(a.data)
    levels = None
    if model.level_input:
        levels = [float(v) for v in a.levels.split(",")] if a.levels else list(DEFAULT_LEVELS)
    try:
        if levels is not None and horizon is not None:
            res, series = evaluate_horizon_levels(model, cfg, raw, a.window_stride, dev, levels, **extra)
        elif levels is not None:
            res, series = evaluate_levels(model, cfg, raw, a.horizon, dev, levels, **extra)
        elif horizon is None:
            res, series = evaluate_flat(model, cfg, raw, a.horizon, dev, **extra)
        else:
            res, series = evaluate_horizon(model, cfg, raw, a.window_stride, dev, **extra)
        torch.cuda.synchronize(dev)
    finally:
        model.close()
    if calib is not None:
        res["calibration"] = os.path.abspath(a.calibration or os.path.join(a.run, "calibration.json"))
    if age_calib is not None:
        res["age_calibration"] = os.path.abspath(a.age_calibration or os.path.join(a.run, "calibration_age.json"))
    res.update({"run": os.path.abspath(a.run), **({"source": "sim", **sim} if a.sim else {"data": os.path.abspath(a.data)}),
                "checkpoint": a.checkpoint, "dataset": cfg["dataset"]})
    if a.plot:
        res["plots"] = plot(cfg["dataset"], series, out, a.plot_envs)
    with open(os.path.join(out, "eval.json"), "w") as f:
        json.dump(_json_safe(res), f, indent=1, allow_nan=False)
    if levels is not None and horizon is not None:
        for r in res["levels"]:
            print(f"level {r['level']}: Total Success Rate: {r['one_shot']['success_rate']}")
        print(f"Level crossings: {res['level_crossings']}")
    elif levels is not None:
        for r in res["levels"]:
            print(f"level {r['level']}: Single Success Rate: {r['one_step']['success_rate']}  Total Success Rate: {r['rollout']['success_rate']}")
    elif horizon is None:
        print(f"Single Success Rate: {res['one_step']['success_rate']}")
        print(f"Total Success Rate: {res['rollout']['success_rate']}")
        if cfg["dataset"] == "error_dynamics":
            print(f"Mean Error: {res['rollout']['mse']}")
            print(f"Mean One Step Error: {res['one_step']['mse']}")
    else:
        print(f"Total Success Rate: {res['one_shot']['success_rate']}")
    if calib is not None:
        if levels is not None and horizon is not None:
            for r in res["levels"]:
                print(f"calibrated level {r['level']} one_shot: Success Rate: {r['calibrated']['one_shot']['success_rate']}")
        elif levels is not None:
            for r in res["levels"]:
                print(f"calibrated level {r['level']}: Single Success Rate: {r['calibrated']['one_step']['success_rate']}  "
                      f"Total Success Rate: {r['calibrated']['rollout']['success_rate']}")
        else:
            for part in ("one_step", "rollout", "one_shot"):
                for cv, m in zip(calib.coverages, res["calibrated"].get(part, [])):
                    print(f"calibrated coverage {cv} {part}: Success Rate: {m['success_rate']}")
    if age_calib is not None:
        ba = res["calibrated_by_age"]
        print(f"Trajectory Success Rate: {ba['trajectory']['raw']['trajectory_success_rate']}")
        for i, cv in enumerate(age_calib.coverages):
            print(f"calibrated by age, coverage {cv} rollout: Success Rate: {ba['rollout'][i]['success_rate']}  Trajectory Success Rate: "
                  f"{ba['trajectory']['by_age'][i]['trajectory_success_rate']}" + (
                      f"  with the margin: {ba['trajectory']['by_age_margin'][i]['trajectory_success_rate']}" if age_calib.margin is not None else ""))
    return res


if __name__ == "__main__":
    main()
