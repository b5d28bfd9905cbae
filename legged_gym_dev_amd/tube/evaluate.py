"""Tube evaluation metrics (the numerical content of the reference's evaluation/evaluate_tube.py, evaluate_error_dyn.py and
evaluate_tube_oneshot.py), in torch on whatever device the tensors live on.

Everything takes (pred, target, done): pred and target (E, T, out), done (E, T) bool.  Row (e, t) is scored unless done[e, t]
(its target belongs to the next episode).  Every metric also comes as a curve over "steps since the last reseed": the age of a
roll-out's fed-back state, 0 where the row was taken from the data.
"""
import torch


def reseed_mask(done, horizon=None):
    """(E, T) bool: where a closed-loop roll-out takes its input from the data -- t = 0, the step after every done, and, with
    horizon = K, every K steps after the last of those."""
    E, T = done.shape
    forced = torch.zeros_like(done, dtype=torch.bool)
    forced[:, 0] = True
    forced[:, 1:] = done[:, :-1].bool()
    if horizon is None:
        return forced
    if horizon < 1:
        raise ValueError("horizon must be positive")
    return (steps_since(forced) % int(horizon)) == 0


def steps_since(reseed):
    """(E, T) int64: steps since the last set entry of `reseed` along time (0 at a set entry; reseed[:, 0] counts as set)."""
    T = reseed.shape[1]
    t = torch.arange(T, device=reseed.device).expand_as(reseed)
    last = torch.cummax(torch.where(reseed.bool(), t, torch.zeros_like(t)), dim=1).values
    return t - last


def _curve(value, weight, age, n):
    """sum(value * weight) / sum(weight) per age 0..n-1 (nan where nothing has that age)."""
    num = torch.zeros(n, dtype=torch.float64, device=value.device).index_add_(0, age.reshape(-1), (value * weight).reshape(-1).double())
    den = torch.zeros(n, dtype=torch.float64, device=value.device).index_add_(0, age.reshape(-1), weight.reshape(-1).double())
    return num / den                    # entries past the oldest scored step are cut by the caller


def tube_metrics(pred, target, done, reseed=None, error_dynamics=False):
    """dict of python floats / lists:
        success_rate   mean(pred >= target) over the scored elements (the scripts' mean(err >= 0))
        mean_excess    mean(pred - target) over the scored elements that cover (nan if none does)
        steps          scored steps;  elements = steps * out
        mse, mean_error_norm   (error_dynamics) MSE over scored elements and mean over scored steps of |pred - target|_2
        *_by_age       the same per steps since the last reseed (reseed (E, T) bool; all-true when None, so one entry)
    """
    if pred.shape != target.shape or pred.dim() != 3 or done.shape != pred.shape[:2]:
        raise ValueError(f"shapes: pred {tuple(pred.shape)}, target {tuple(target.shape)}, done {tuple(done.shape)}")
    keep = ~done.bool()
    if reseed is None:
        reseed = torch.ones_like(keep)
    age = steps_since(reseed.to(keep.device))
    n_age, n_all = (int(age[keep].max()) + 1 if bool(keep.any()) else 1), int(age.max()) + 1
    O = pred.shape[2]
    w_el = keep[:, :, None].expand_as(pred).double()
    age_el = age[:, :, None].expand_as(pred)
    diff = pred.double() - target.double()
    cover = (pred >= target).double()
    out = {"steps": int(keep.sum()), "elements": int(keep.sum()) * O,
           "success_rate": float((cover * w_el).sum() / w_el.sum()),
           "mean_excess": float((diff * cover * w_el).sum() / (cover * w_el).sum()),
           "success_rate_by_age": _curve(cover, w_el, age_el, n_all)[:n_age].tolist(),
           "mean_excess_by_age": _curve(diff, cover * w_el, age_el, n_all)[:n_age].tolist()}
    if error_dynamics:
        w_st = keep.double()
        norm = diff.norm(dim=-1)
        out.update({"mse": float((diff * diff * w_el).sum() / w_el.sum()),
                    "mean_error_norm": float((norm * w_st).sum() / w_st.sum()),
                    "mse_by_age": _curve(diff * diff, w_el, age_el, n_all)[:n_age].tolist(),
                    "mean_error_norm_by_age": _curve(norm, w_st, age, n_all)[:n_age].tolist()})
    return out


def window_metrics(pred, target):
    """One-shot windows: pred, target (count, H_fwd).  success_rate over every element and per step ahead (mean over the windows,
    not the reference's sum over 100 windows divided by n_robots), mean_excess as in tube_metrics."""
    cover = (pred >= target).double()
    diff = pred.double() - target.double()
    return {"windows": int(pred.shape[0]), "success_rate": float(cover.mean()),
            "mean_excess": float((diff * cover).sum() / cover.sum()),
            "success_rate_by_step": cover.mean(dim=0).tolist()}


def level_crossings(pred, levels):
    """pred (count, n_levels, H_fwd) of a level-conditioned one-shot model, levels in any order: the share of (window, step ahead,
    pair of adjacent levels in ascending order) where the prediction FALLS as the level rises -- 0 for a model whose bounds are
    nested.  nan with fewer than two levels."""
    order = torch.argsort(torch.as_tensor(levels, dtype=torch.float64))
    p = pred[:, order.to(pred.device), :]
    if p.shape[1] < 2:
        return float("nan")
    return float((p[:, 1:, :] < p[:, :-1, :]).double().mean())


def trajectory_metrics(covered, done):
    """covered (E, T, out) bool, done (E, T): the fraction of envs whose every kept step is covered, per output column --
    the quantity a trajectory margin (tube/calibrate.py calibrate_trajectory) bounds.  An env without a kept step counts as covered."""
    if covered.dim() != 3 or done.shape != covered.shape[:2]:
        raise ValueError(f"shapes: covered {tuple(covered.shape)}, done {tuple(done.shape)}")
    whole = (covered.bool() | done.bool()[:, :, None]).all(dim=1)                            # (E, out)
    return {"envs": int(covered.shape[0]), "trajectory_success_rate": whole.double().mean(dim=0).tolist()}
