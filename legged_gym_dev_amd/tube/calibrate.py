"""Split conformal calibration of tubes: a one-sided bound that covers with a stated probability.

Score every row of a held-out calibration set with s = w - fw, take the ceil((n + 1) c)-th smallest score as an offset q, and use
fw + q as the tube: on exchangeable data it covers with probability >= c, whatever the model learned.  The scores come from the
entries that exist (predict, predict_levels, predict_windows, rollout_window); the order statistic is lg_select_kth, exact, per
output column, per level and per step ahead.

    select_kth(values, ranks, keep=None)      the k-th smallest per batch row, on the device
    conformal_rank(n, coverage)               ceil((n + 1) c) in exact rational arithmetic
    Calibration                               offsets, ranks, provenance; save / load (calibration.json); apply / covers
    calibrate_flat / calibrate_levels / calibrate_horizon      the three score layouts

There is no CPU fallback for the selection: without the library or a GPU it raises.
"""
import ctypes as C
import json
import math
import os
from fractions import Fraction

import torch

CALIBRATION_NAME = "calibration.json"
FLAT_KINDS = ("scalar", "vector")
PARTS = ("one_step", "rollout")


def select_kth(values, ranks, keep=None):
    """values (B, n) float32 on the device, rows n apart or further (a row stride becomes ld; anything else is copied); ranks (B, R)
    or (R,) for every row, 1-based; keep None or (n) bool / uint8 shared by the rows.  Returns (out (B, R) float32, n_kept a device
    int64 tensor of one element): lg_select_kth's semantics (include/legged_hip.h).  Queues on the current stream, waits for nothing."""
    from ..lib import LeggedHipError, load
    lib = load()
    if not (torch.is_tensor(values) and values.is_cuda and values.dtype == torch.float32 and values.dim() == 2):
        raise LeggedHipError(f"select_kth needs a (B, n) float32 tensor on a GPU device (no CPU fallback); got {type(values).__name__} "
                             f"{tuple(getattr(values, 'shape', ()))} on {getattr(values, 'device', None)}")
    B, n = values.shape
    if n >= 1 and not (values.stride(1) == 1 and (B == 1 or values.stride(0) >= n)):
        values = values.contiguous()
    ld = n if B == 1 else values.stride(0)
    dev = values.device
    ranks = torch.as_tensor(ranks, dtype=torch.int64)
    if ranks.dim() == 1:
        ranks = ranks[None, :].expand(B, -1)
    if ranks.dim() != 2 or ranks.shape[0] != B:
        raise ValueError(f"ranks must be (R,) or (B = {B}, R); got {tuple(ranks.shape)}")
    ranks = ranks.to(dev).contiguous()
    R = ranks.shape[1]
    if keep is not None:
        keep = torch.as_tensor(keep).to(dev).reshape(-1)
        keep = (keep.view(torch.uint8) if keep.dtype == torch.bool else keep.ne(0).to(torch.uint8)).contiguous()
        if keep.numel() != n:
            raise ValueError(f"keep must have n = {n} elements; got {keep.numel()}")
    nbytes = lib.lg_select_workspace(B, R)
    if nbytes < 0:
        raise ValueError(lib.lg_last_error().decode())
    ws = torch.empty(nbytes // 8, dtype=torch.int64, device=dev)
    out = torch.empty((B, R), dtype=torch.float32, device=dev)
    n_kept = torch.empty(1, dtype=torch.int64, device=dev)
    p = lambda t: C.c_void_p(t.data_ptr())
    with torch.cuda.device(dev):
        rc = lib.lg_select_kth(p(values), ld, B, n, p(keep) if keep is not None else None, p(ranks), R, p(out), p(n_kept), p(ws),
                               C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise (ValueError if rc == -1 else LeggedHipError)(f"lg_select_kth failed ({rc}): {lib.lg_last_error().decode()}")
    return out, n_kept


def conformal_rank(n, coverage):
    """ceil((n + 1) c), exact on the decimal the caller wrote: Fraction(str(c)).  In float64 100 * 0.07 is 7.000000000000001 and
    would round up to 8.  A rank above n means too few calibration rows for this coverage: the offset is +inf."""
    c = Fraction(str(coverage))
    if not 0 < c < 1:
        raise ValueError(f"coverage must lie inside (0, 1); got {coverage}")
    if n < 0:
        raise ValueError(f"n must not be negative; got {n}")
    return math.ceil((int(n) + 1) * c)


def _enc(o):
    if isinstance(o, list):
        return [_enc(v) for v in o]
    if isinstance(o, float) and math.isinf(o):
        return "inf" if o > 0 else "-inf"
    return o


def _dec(o):
    if isinstance(o, list):
        return [_dec(v) for v in o]
    return float(o) if isinstance(o, str) else o


class Calibration:
    """Offsets of one calibration run.

    kind "flat":    parts one_step and rollout; offsets (2, n_coverages, out)
    kind "levels":  a level-conditioned model, level l calibrated to coverage l; offsets (2, n_levels, out); coverages are the levels
    kind "horizon": one offset per coverage and step ahead; offsets (n_coverages, H_fwd)
    n: kept calibration rows; ranks[i] = conformal_rank(n, coverages[i]); provenance: run, checkpoint, dataset, data or the sim flags."""
    KINDS = ("flat", "levels", "horizon")

    def __init__(self, kind, coverages, offsets, n, ranks, provenance=None):
        if kind not in self.KINDS:
            raise ValueError(f"kind {kind!r}: one of {self.KINDS}")
        self.kind = kind
        self.coverages = [float(c) for c in coverages]
        self.offsets = torch.as_tensor(offsets, dtype=torch.float32).cpu()
        self.n, self.ranks = int(n), [int(r) for r in ranks]
        self.provenance = dict(provenance or {})
        want = 2 if kind == "horizon" else 3
        if self.offsets.dim() != want or self.offsets.shape[want - 2] != len(self.coverages) or len(self.ranks) != len(self.coverages) \
                or (kind != "horizon" and self.offsets.shape[0] != len(PARTS)):
            raise ValueError(f"{kind}: offsets {tuple(self.offsets.shape)} do not fit {len(self.coverages)} coverages")
        if bool(torch.isnan(self.offsets).any()):
            bad = torch.isnan(self.offsets).nonzero()[0].tolist()
            raise ValueError(f"NaN offset in set {self.set_name(bad)}: a NaN score reached the rank")

    def set_name(self, idx):
        """The name of offsets[idx] for messages and printed lines."""
        if self.kind == "horizon":
            return f"coverage {self.coverages[idx[0]]}, step ahead {idx[1] + 1}"
        return f"{PARTS[idx[0]]}, {'level' if self.kind == 'levels' else 'coverage'} {self.coverages[idx[1]]}, column {idx[2]}"

    def index(self, coverage, level=None):
        if self.kind == "levels":
            if level is not None and abs(float(level) - float(coverage)) > 1e-9:
                raise ValueError(f"level {level} is calibrated to coverage {level}, not {coverage}: a level-conditioned model's level is its coverage")
        elif level is not None:
            raise ValueError(f"a {self.kind} calibration has no levels")
        for i, c in enumerate(self.coverages):
            if abs(c - float(coverage)) <= 1e-9:
                return i
        raise KeyError(f"coverage {coverage} was not calibrated; have {self.coverages}")

    def offset(self, coverage, level=None, part="one_step"):
        """The offsets of one set: (out) for flat and levels, (H_fwd) for horizon."""
        i = self.index(coverage, level)
        if self.kind == "horizon":
            return self.offsets[i]
        if part not in PARTS:
            raise ValueError(f"part {part!r}: one of {PARTS}")
        return self.offsets[PARTS.index(part), i]

    def apply(self, fw, coverage, level=None, part="one_step"):
        """fw + offset, the offset broadcast over the rows (fw (..., out), or (..., H_fwd) for horizon)."""
        return fw + self.offset(coverage, level, part).to(fw.device)

    def covers(self, fw, w, coverage, level=None, part="one_step"):
        """(w - fw) <= offset: the exact form of apply(fw) >= w, which can differ from it by an ulp of the sum."""
        return (w - fw) <= self.offset(coverage, level, part).to(fw.device)

    def to_json(self):
        return {"kind": self.kind, "coverages": self.coverages, "n": self.n, "ranks": self.ranks,
                "offsets": _enc(self.offsets.tolist()), "parts": list(PARTS) if self.kind != "horizon" else None, **self.provenance}

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_json(), f, indent=1, allow_nan=False)

    @classmethod
    def load(cls, path):
        with open(path) as f:
            d = json.load(f)
        core = ("kind", "coverages", "n", "ranks", "offsets", "parts")
        return cls(d["kind"], d["coverages"], _dec(d["offsets"]), d["n"], d["ranks"], {k: v for k, v in d.items() if k not in core})

    def lines(self):
        """One printed line per set: rank, n, offset."""
        out = []
        for idx in torch.cartesian_prod(*[torch.arange(s) for s in self.offsets.shape]).reshape(-1, self.offsets.dim()).tolist():
            ci = idx[0] if self.kind == "horizon" else idx[1]
            out.append(f"{self.set_name(idx)}: rank {self.ranks[ci]} of n {self.n}, offset {float(self.offsets[tuple(idx)])}")
        return out


def _ranks(n, coverages):
    return [conformal_rank(n, c) for c in coverages]


def calibrate_flat(model, data, target, done, layout, reseed, coverages, kind="scalar"):
    """Flat kinds.  data (E, T, I), target (E, T, out), done (E, T) bool; layout = feedback_layout(...) = (fb, taps, lag, stride).
    Scores of predict and of rollout_window (pooled over ages; the value fed back stays the raw model output), keep = ~done.
    Returns (Calibration, {fw_single, fw})."""
    if kind not in FLAT_KINDS:
        raise ValueError(f"{kind}: only bounds are calibrated ({', '.join(FLAT_KINDS)}, their level kinds and scalar_horizon); "
                         "error_dynamics predicts a signed error, not a bound")
    E, T, I = data.shape
    fw_single = model.predict(data.reshape(E * T, I)).reshape(E, T, -1)
    fw = model.rollout_window(data, *layout, reseed)
    O = target.shape[2]
    scores = torch.stack((target - fw_single, target - fw)).reshape(2, E * T, O).permute(0, 2, 1).reshape(2 * O, E * T)
    keep = ~done.bool().reshape(-1)
    n = int(keep.sum())
    ranks = _ranks(n, coverages)
    q, _ = select_kth(scores, torch.tensor(ranks), keep)                       # (2 O, n_coverages)
    offsets = q.reshape(2, O, len(ranks)).permute(0, 2, 1)
    return Calibration("flat", coverages, offsets, n, ranks), {"fw_single": fw_single, "fw": fw}


def calibrate_levels(model, data, target, done, layout, reseed, levels):
    """Level-conditioned kinds: data without the level column.  One predict_levels launch for all levels, the roll-out per level
    with the column filled; level l is calibrated to coverage l.  Returns (Calibration, {fw_single, fw}), both (levels, E, T, out)."""
    E, T, I = data.shape
    L, O = len(levels), target.shape[2]
    single = model.predict_levels(data.reshape(E * T, I), torch.tensor(levels, dtype=torch.float32))      # (E T, L, out)
    fw_single = single.permute(1, 0, 2).reshape(L, E, T, O)
    fw = torch.stack([model.rollout_window(model.with_level(data, lv), *layout, reseed) for lv in levels])
    scores = torch.stack((target[None] - fw_single, target[None] - fw)).reshape(2 * L, E * T, O).permute(0, 2, 1).reshape(2 * L * O, E * T)
    keep = ~done.bool().reshape(-1)
    n = int(keep.sum())
    ranks = _ranks(n, levels)
    per_row = torch.tensor(ranks).repeat_interleave(O).repeat(2)[:, None]      # row (part, level, column) takes its level's rank
    q, _ = select_kth(scores, per_row, keep)
    return Calibration("levels", levels, q.reshape(2, L, O), n, ranks), {"fw_single": fw_single, "fw": fw}


def calibrate_horizon(fw, target, coverages):
    """scalar_horizon: fw, target (windows, H_fwd) from predict_windows on the window starts.  One offset per coverage and step."""
    W, H = fw.shape
    ranks = _ranks(W, coverages)
    q, _ = select_kth((target - fw).t(), torch.tensor(ranks))                  # (H_fwd, n_coverages)
    return Calibration("horizon", coverages, q.t(), W, ranks)


def default_path(run):
    return os.path.join(run, CALIBRATION_NAME)
