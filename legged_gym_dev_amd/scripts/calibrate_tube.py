"""Calibrate a trained tube model: split conformal offsets on a held-out calibration set.

    python legged_gym_dev_amd/scripts/calibrate_tube.py --run tube_runs/run0 (--data rom_tracking_data/cal | --sim) \\
        [--coverage 0.9,0.95 | --levels 0.5,0.8,0.9,0.95] [--checkpoint best|latest] [--horizon K] [--window_stride S] [--out DIR] \\
        [--by_age [--max_age A] [--trajectory]]

Every calibration row is scored with s = w - fw on the predictions evaluate_tube.py scores -- the one-step prediction and the
closed-loop roll-out (same reseed mask, pooled over ages) for the flat datasets scalar and vector, per level for a
level-conditioned run (level l is calibrated to coverage l, which makes "the level is the coverage" true), per step ahead for
scalar_horizon, per level and step ahead for scalar_horizon_level (--levels; every level of every window from one launch) -- and
the ceil((n + 1) c)-th smallest score of every set, taken exactly on the device (lg_select_kth), is the
offset that evaluate_tube.py --calibration adds to the prediction.  error_dynamics is refused: it predicts a signed error, not a
bound.  Rows after a done are left out, as in the evaluation.

Writes calibration.json to --out (default: the run folder) and prints one line per set: rank, n, offset.  An offset of inf says
the set has fewer rows than the coverage needs (rank > n): the calibrated tube is then the trivial one.

--sim calibrates on fresh robots of the ROM-on-ROM simulator.  The default --sim_seed is the smallest seed >= 1 the run did not
train with, plus 100, so that evaluate_tube.py --sim (default seeds 1..3) never scores the robots the offsets were fitted on;
evaluate_tube.py refuses a --sim_seed or a --data folder equal to the calibration's.

The guarantee is the split conformal one: on calibration and test rows that are exchangeable, P(w <= fw + q) >= c.  Envs are
exchangeable; the steps of one env are correlated, so the effective sample is smaller than n and the margin over c on fresh
robots is not promised (section 10.6).

--by_age (flat datasets scalar and vector) also writes calibration_age.json next to calibration.json, which
is written exactly as without the flag: one roll-out offset per age of the fed-back state (steps since the last reseed; with
--horizon K that is K ages) instead of one pooled over ages, every age's ceil((count + 1) c)-th smallest score from one grouped
selection on the device (lg_select_kth_grouped).  --max_age A pools the ages >= A - 1 into the last group; the default is one
group per age that occurs, at most 1024.  Prints one line per (coverage, age, column): rank, count, offset.  Level-conditioned
runs, scalar_horizon (which already has one offset per step ahead) and error_dynamics are refused.

--trajectory (with --by_age) fits the per-age offsets on the envs of even index only and, on the envs of odd index, a margin
delta per coverage and column: the conformal_rank(E_margin, c)-th smallest, over those envs, of the env's largest score
w - fw - q[age] over its kept steps.  What that buys, per output column: P(every kept step of a fresh env lies inside
fw + q[age] + delta) >= c.  That is exact split conformal over envs, which are exchangeable (independent draws of the simulator's
seed stream), unlike the steps of one env.  It is per column, not joint over the columns of a vector tube, and it covers the env's
whole recorded length: for the statement over one planning horizon of K steps, simulate with --sim_T K.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import torch  # noqa: E402

import evaluate_tube as et  # noqa: E402
from legged_gym_dev_amd.tube import calibrate as cal  # noqa: E402
from legged_gym_dev_amd.tube import evaluate as ev  # noqa: E402
from legged_gym_dev_amd.tube.data import HORIZON_KINDS, HORIZON_LEVEL_KIND, LEVEL_KINDS, construct_dataset, feedback_layout  # noqa: E402
from legged_gym_dev_amd.tube.model import HipTubeModel  # noqa: E402

DEFAULT_COVERAGE = (0.9, 0.95)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--run", required=True, help="folder train_tube.py wrote (model.pth, model_best.pth, config.json)")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--data", help="folder of epoch_<k>.pickle files: the calibration set")
    src.add_argument("--sim", action="store_true", help="calibrate on fresh robots simulated on the device (HipRomSim)")
    ap.add_argument("--sim_envs", type=int, default=None)
    ap.add_argument("--sim_T", type=int, default=None)
    ap.add_argument("--sim_seed", type=int, default=None, help="default: the smallest seed >= 1 the run did not train with, plus 100")
    ap.add_argument("--sim_resident", type=int, default=None, help="epochs to simulate (default 1)")
    what = ap.add_mutually_exclusive_group()
    what.add_argument("--coverage", default=None, help="comma-separated coverages (default 0.9,0.95)")
    what.add_argument("--levels", default=None, help="level-conditioned runs: comma-separated levels, each calibrated to itself "
                                                     "(default 0.5,0.8,0.9,0.95)")
    ap.add_argument("--checkpoint", choices=["best", "latest"], default="best")
    ap.add_argument("--horizon", type=int, default=None, help="flat datasets: reseed the roll-out every K steps")
    ap.add_argument("--window_stride", type=int, default=1, help="scalar_horizon: distance between window starts")
    ap.add_argument("--by_age", action="store_true", help="flat datasets: also write calibration_age.json, one roll-out offset per age")
    ap.add_argument("--max_age", type=int, default=None, help="--by_age: number of age groups; ages >= A - 1 share the last (default: every age, at most 1024)")
    ap.add_argument("--trajectory", action="store_true", help="--by_age: offsets from the even envs, a per-env margin from the odd envs")
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", default="cuda:0")
    for name, kw in (("dataset", dict(choices=sorted(et.DATASETS))), ("N", dict(type=int)), ("dN", dict(type=int)),
                     ("recursive", dict(action="store_true")), ("H_fwd", dict(type=int)), ("H_rev", dict(type=int)),
                     ("activation", dict(choices=["relu", "softplus", "tanh", "elu"])), ("softplus_beta", dict(type=float))):
        ap.add_argument("--" + name, default=None, **kw)
    return ap.parse_args(argv)


def sim_flags(a, cfg):
    """evaluate_tube.sim_flags with the calibration's own default seed."""
    if a.sim_seed is None:
        used = {cfg.get("seed"), cfg.get("sim_seed")}
        a.sim_seed = min(s for s in range(1, 4) if s not in used) + 100
    return et.sim_flags(a, cfg)


def check_kind(cfg, a):
    """The dataset kinds that are bounds; the coverages or levels asked for, as the decimals written."""
    kind = cfg["dataset"]
    if LEVEL_KINDS.get(kind, kind) not in cal.FLAT_KINDS + HORIZON_KINDS:
        raise ValueError(f"--run was trained on {kind}: it predicts a signed error, not a bound, and is not calibrated "
                         f"(bounds: {', '.join(cal.FLAT_KINDS)}, their level kinds, scalar_horizon and scalar_horizon_level)")
    if et.DATASETS[kind].conditioned:
        if a.coverage is not None:
            raise ValueError("a level-conditioned run is calibrated per level: give --levels, not --coverage")
        wanted = a.levels.split(",") if a.levels else [str(v) for v in et.DEFAULT_LEVELS]
    else:
        if a.levels is not None:
            raise ValueError(f"--levels is for level-conditioned runs; {kind} takes --coverage")
        wanted = a.coverage.split(",") if a.coverage else [str(v) for v in DEFAULT_COVERAGE]
    for c in wanted:
        cal.conformal_rank(0, c.strip())                   # refuses anything outside (0, 1)
    return [float(c) for c in wanted]


def check_by_age(cfg, a):
    """--by_age, --max_age and --trajectory: flat kinds only."""
    if not a.by_age:
        if a.trajectory:
            raise ValueError("--trajectory needs --by_age: the margin is fitted on top of the per-age offsets")
        if a.max_age is not None:
            raise ValueError("--max_age needs --by_age: it is the number of age groups")
        return
    kind = cfg["dataset"]
    if kind in LEVEL_KINDS:
        raise ValueError(f"--by_age: {kind} is level-conditioned; per-age and trajectory calibration of conditioned tubes is not built "
                         f"(flat kinds only: {', '.join(cal.FLAT_KINDS)})")
    if kind in HORIZON_KINDS:
        raise ValueError(f"--by_age: {kind} predicts all steps ahead in one shot and already has one offset per step ahead")
    if kind not in cal.FLAT_KINDS:
        raise ValueError(f"--by_age: {kind} predicts a signed error, not a bound, and is not calibrated")
    if a.max_age is not None and not 1 <= a.max_age <= cal.MAX_GROUPS:
        raise ValueError(f"--max_age must be 1..{cal.MAX_GROUPS}; got {a.max_age}")


def calibrate_age(model, cfg, raw, a, wanted, dev):
    """The AgeCalibration of --by_age [--trajectory] on the rows calibrate() scores."""
    kind = cfg["dataset"]
    win = {"N": cfg["N"], "dN": cfg["dN"]}
    if kind == "scalar":
        win["recursive"] = cfg["recursive"]
    data, target, done = et.rows(kind, raw, win, dev)
    layout = feedback_layout(kind, cfg["N"], cfg["dN"], cfg["recursive"], n=raw["z"].shape[-1], m=raw["v"].shape[-1])
    reseed = ev.reseed_mask(done, a.horizon)
    if a.trajectory:
        return cal.calibrate_trajectory(model, data, target, done, layout, reseed, wanted, kind, a.max_age)
    return cal.AgeCalibration(wanted, *cal.calibrate_by_age(model, data, target, done, layout, reseed, wanted, kind, a.max_age))


def calibrate(model, cfg, raw, a, wanted, dev):
    kind = cfg["dataset"]
    if kind == HORIZON_LEVEL_KIND:                          # one launch scores every level of every window
        _, series = et.evaluate_horizon_levels(model, cfg, raw, a.window_stride, dev, wanted)
        return cal.calibrate_horizon_levels(series["fw_levels"], series["target"], wanted)
    if kind == "scalar_horizon":
        _, series = et.evaluate_horizon(model, cfg, raw, a.window_stride, dev)
        Hf = series["fw"].shape[-1]
        return cal.calibrate_horizon(series["fw"].reshape(-1, Hf), series["w"].reshape(-1, Hf), wanted)
    base = LEVEL_KINDS.get(kind, kind)
    win = {"N": cfg["N"], "dN": cfg["dN"]}
    if base == "scalar":
        win["recursive"] = cfg["recursive"]
    data, target, done = et.rows(kind, raw, win, dev)
    layout = feedback_layout(kind, cfg["N"], cfg["dN"], cfg["recursive"], n=raw["z"].shape[-1], m=raw["v"].shape[-1])
    reseed = ev.reseed_mask(done, a.horizon)
    if kind in LEVEL_KINDS:
        return cal.calibrate_levels(model, data, target, done, layout, reseed, wanted)[0]
    return cal.calibrate_flat(model, data, target, done, layout, reseed, wanted, kind)[0]


def main(argv=None):
    a = parse_args(argv)
    cfg = et.resolve_config(a)
    check_by_age(cfg, a)
    wanted = check_kind(cfg, a)
    dev = torch.device(a.device)
    out = a.out or a.run
    os.makedirs(out, exist_ok=True)
    horizon = (cfg["H_fwd"], cfg["H_rev"]) if cfg["dataset"] in HORIZON_KINDS else None
    sim = sim_flags(a, cfg) if a.sim else None
    model = HipTubeModel.load(a.run, checkpoint=a.checkpoint, activation=cfg["activation"], softplus_beta=cfg["softplus_beta"],
                              horizon=horizon, device=a.device, level_input=et.DATASETS[cfg["dataset"]].conditioned)
    try:
        raw = et.sim_records(sim, a.device) if a.sim else construct_dataset(a.data)
        c = calibrate(model, cfg, raw, a, wanted, dev)
        by_age = calibrate_age(model, cfg, raw, a, wanted, dev) if a.by_age else None
        torch.cuda.synchronize(dev)
    finally:
        model.close()
    c.provenance = {"run": os.path.abspath(a.run), "checkpoint": a.checkpoint, "dataset": cfg["dataset"], "reseed_every": a.horizon,
                    "window_stride": a.window_stride, **({"source": "sim", **sim} if a.sim else {"data": os.path.abspath(a.data)})}
    c.save(os.path.join(out, cal.CALIBRATION_NAME))
    for line in c.lines():
        print(line)
    if by_age is not None:
        by_age.provenance = dict(c.provenance)
        by_age.save(os.path.join(out, cal.AGE_CALIBRATION_NAME))
        for line in by_age.lines():
            print(line)
    return c


if __name__ == "__main__":
    main()
