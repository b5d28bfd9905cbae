"""Split conformal calibration of tubes: a one-sided bound that covers with a stated probability.

Score every row of a held-out calibration set with s = w - fw, take the ceil((n + 1) c)-th smallest score as an offset q, and use
fw + q as the tube: on exchangeable data it covers with probability >= c, whatever the model learned.  The scores come from the
entries that exist (predict, predict_levels, predict_windows, predict_windows_levels, rollout_window); the order statistic is lg_select_kth, exact, per
output column, per level and per step ahead.

    select_kth(values, ranks, keep=None)      the k-th smallest per batch row, on the device
    conformal_rank(n, coverage)               ceil((n + 1) c) in exact rational arithmetic
    Calibration                               offsets, ranks, provenance; save / load (calibration.json); apply / covers
    calibrate_flat / calibrate_levels / calibrate_horizon / calibrate_horizon_levels      the four score layouts

Per age and per trajectory, for the closed-loop roll-out of the flat kinds:

    select_kth_grouped(values, group, G, coverages)      the conformal order statistic of every group, ranks computed on the device
    calibrate_by_age / calibrate_trajectory              one offset per age of the fed-back state; a margin from a score per env
    AgeCalibration                                       per-age offsets and the margin; save / load (calibration_age.json)

There is no CPU fallback for the selection: without the library or a GPU it raises.
"""
import ctypes as C
import json
import math
import os
from fractions import Fraction

import torch

CALIBRATION_NAME = "calibration.json"
AGE_CALIBRATION_NAME = "calibration_age.json"
MAX_GROUPS = 1024                                       # LG_SELECT_MAX_GROUPS
FLAT_KINDS = ("scalar", "vector")
PARTS = ("one_step", "rollout")


def _device_rows(values, who):
    """(values, B, n, ld, dev) of a (B, n) float32 device tensor for lg_select_*: a row stride becomes ld, anything else is copied."""
    from ..lib import LeggedHipError
    if not (torch.is_tensor(values) and values.is_cuda and values.dtype == torch.float32 and values.dim() == 2):
        raise LeggedHipError(f"{who} needs a (B, n) float32 tensor on a GPU device (no CPU fallback); got {type(values).__name__} "
                             f"{tuple(getattr(values, 'shape', ()))} on {getattr(values, 'device', None)}")
    B, n = values.shape
    if n >= 1 and not (values.stride(1) == 1 and (B == 1 or values.stride(0) >= n)):
        values = values.contiguous()
    return values, B, n, (n if B == 1 else values.stride(0)), values.device


def _workspace(lib, nbytes, dev):
    """The workspace a size query asked for; a refused query (-1) raises with the library's reason."""
    if nbytes < 0:
        raise ValueError(lib.lg_last_error().decode())
    return torch.empty(nbytes // 8, dtype=torch.int64, device=dev)


def _call(lib, entry, dev, *args):
    """lib.<entry>(*args, dev's current stream), tensors as their pointers; -1 raises ValueError, another failure LeggedHipError."""
    from ..lib import LeggedHipError
    args = [C.c_void_p(a.data_ptr()) if torch.is_tensor(a) else a for a in args]
    with torch.cuda.device(dev):
        rc = getattr(lib, entry)(*args, C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
    if rc != 0:
        raise (ValueError if rc == -1 else LeggedHipError)(f"{entry} failed ({rc}): {lib.lg_last_error().decode()}")


def select_kth(values, ranks, keep=None):
    """values (B, n) float32 on the device, rows n apart or further (a row stride becomes ld; anything else is copied); ranks (B, R)
    or (R,) for every row, 1-based; keep None or (n) bool / uint8 shared by the rows.  Returns (out (B, R) float32, n_kept a device
    int64 tensor of one element): lg_select_kth's semantics (include/legged_hip.h).  Queues on the current stream, waits for nothing."""
    from ..lib import load
    lib = load()
    values, B, n, ld, dev = _device_rows(values, "select_kth")
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
    ws = _workspace(lib, lib.lg_select_workspace(B, R), dev)
    out = torch.empty((B, R), dtype=torch.float32, device=dev)
    n_kept = torch.empty(1, dtype=torch.int64, device=dev)
    _call(lib, "lg_select_kth", dev, values, ld, B, n, keep, ranks, R, out, n_kept, ws)
    return out, n_kept


def coverage_fractions(coverages):
    """[(num, den)] of the decimals the caller wrote, Fraction(str(c)) as in conformal_rank: what lg_select_kth_grouped takes."""
    out = []
    for c in coverages:
        f = Fraction(str(c).strip())
        if not 0 < f < 1:
            raise ValueError(f"coverage must lie inside (0, 1); got {c}")
        if f.denominator > 2 ** 31 - 1:
            raise ValueError(f"coverage {c} has the denominator {f.denominator}, above 2^31 - 1: write it with fewer digits")
        out.append((f.numerator, f.denominator))
    return out


def select_kth_grouped(values, group, G, coverages):
    """values (B, n) float32 on the device, handled as in select_kth; group (n) integers shared by the rows, element i belongs to
    group[i] when 0 <= group[i] < G and takes no part otherwise; coverages: decimals inside (0, 1).  Returns (out (B, G, R) float32,
    counts (G) int64, ranks (G, R) int64), all on the device: out[b, g, r] is the ceil((counts[g] + 1) c_r)-th smallest member of
    group g in row b, +inf where the group has fewer members (lg_select_kth_grouped, include/legged_hip.h).  Queues on the current
    stream, waits for nothing."""
    from ..lib import load
    lib = load()
    values, B, n, ld, dev = _device_rows(values, "select_kth_grouped")
    fr = coverage_fractions(coverages)
    R, G = len(fr), int(G)
    group = torch.as_tensor(group).to(dev).reshape(-1)
    if group.dtype != torch.int32 or group.stride(0) != 1:
        group = group.to(torch.int32).contiguous()
    if group.numel() != n:
        raise ValueError(f"group must have n = {n} elements; got {group.numel()}")
    ws = _workspace(lib, lib.lg_select_grouped_workspace(B, G, R), dev)
    out = torch.empty((B, G, R), dtype=torch.float32, device=dev)
    counts = torch.empty(G, dtype=torch.int64, device=dev)
    ranks = torch.empty((G, R), dtype=torch.int64, device=dev)
    num, den = (C.c_int64 * R)(*[f[0] for f in fr]), (C.c_int64 * R)(*[f[1] for f in fr])
    _call(lib, "lg_select_kth_grouped", dev, values, ld, B, n, group, G, num, den, R, out, counts, ranks, ws)
    return out, counts, ranks


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


def _coverage_index(coverages, coverage):
    for i, c in enumerate(coverages):
        if abs(c - float(coverage)) <= 1e-9:
            return i
    raise KeyError(f"coverage {coverage} was not calibrated; have {coverages}")


class Calibration:
    """Offsets of one calibration run.

    kind "flat":    parts one_step and rollout; offsets (2, n_coverages, out)
    kind "levels":  a level-conditioned model, level l calibrated to coverage l; offsets (2, n_levels, out); coverages are the levels
    kind "horizon": one offset per coverage and step ahead; offsets (n_coverages, H_fwd)
    kind "horizon_levels": a level-conditioned one-shot model, level l calibrated to coverage l, one offset
                    per level and step ahead; offsets (n_levels, H_fwd); coverages are the levels
    n: kept calibration rows; ranks[i] = conformal_rank(n, coverages[i]); provenance: run, checkpoint, dataset, data or the sim flags."""
    KINDS = ("flat", "levels", "horizon", "horizon_levels")
    WINDOW_KINDS = ("horizon", "horizon_levels")            # offsets (sets, H_fwd), no parts
    LEVEL_KINDS = ("levels", "horizon_levels")              # the sets are levels, each calibrated to itself

    def __init__(self, kind, coverages, offsets, n, ranks, provenance=None):
        if kind not in self.KINDS:
            raise ValueError(f"kind {kind!r}: one of {self.KINDS}")
        self.kind = kind
        self.coverages = [float(c) for c in coverages]
        self.offsets = torch.as_tensor(offsets, dtype=torch.float32).cpu()
        self.n, self.ranks = int(n), [int(r) for r in ranks]
        self.provenance = dict(provenance or {})
        self.windowed = kind in self.WINDOW_KINDS
        want = 2 if self.windowed else 3
        if self.offsets.dim() != want or self.offsets.shape[want - 2] != len(self.coverages) or len(self.ranks) != len(self.coverages) \
                or (not self.windowed and self.offsets.shape[0] != len(PARTS)):
            raise ValueError(f"{kind}: offsets {tuple(self.offsets.shape)} do not fit {len(self.coverages)} coverages")
        if bool(torch.isnan(self.offsets).any()):
            bad = torch.isnan(self.offsets).nonzero()[0].tolist()
            raise ValueError(f"NaN offset in set {self.set_name(bad)}: a NaN score reached the rank")

    def set_name(self, idx):
        """The name of offsets[idx] for messages and printed lines."""
        word = "level" if self.kind in self.LEVEL_KINDS else "coverage"
        if self.windowed:
            return f"{word} {self.coverages[idx[0]]}, step ahead {idx[1] + 1}"
        return f"{PARTS[idx[0]]}, {word} {self.coverages[idx[1]]}, column {idx[2]}"

    def index(self, coverage=None, level=None):
        """The set of `coverage`; on the level kinds `level` alone names it too (a level is its own coverage).  KeyError for a set
        that was not calibrated."""
        if self.kind in self.LEVEL_KINDS:
            if coverage is None:
                coverage = level
            if coverage is None:
                raise ValueError(f"a {self.kind} calibration needs the level (or its coverage)")
            if level is not None and abs(float(level) - float(coverage)) > 1e-9:
                raise ValueError(f"level {level} is calibrated to coverage {level}, not {coverage}: a level-conditioned model's level is its coverage")
        elif level is not None:
            raise ValueError(f"a {self.kind} calibration has no levels")
        elif coverage is None:
            raise ValueError(f"a {self.kind} calibration needs the coverage")
        return _coverage_index(self.coverages, coverage)

    def offset(self, coverage=None, level=None, part="one_step"):
        """The offsets of one set: (out) for flat and levels, (H_fwd) for horizon and horizon_levels."""
        i = self.index(coverage, level)
        if self.windowed:
            return self.offsets[i]
        if part not in PARTS:
            raise ValueError(f"part {part!r}: one of {PARTS}")
        return self.offsets[PARTS.index(part), i]

    def apply(self, fw, coverage=None, level=None, part="one_step"):
        """fw + offset, the offset broadcast over the rows (fw (..., out), or (..., H_fwd) for horizon)."""
        return fw + self.offset(coverage, level, part).to(fw.device)

    def covers(self, fw, w, coverage=None, level=None, part="one_step"):
        """(w - fw) <= offset: the exact form of apply(fw) >= w, which can differ from it by an ulp of the sum."""
        return (w - fw) <= self.offset(coverage, level, part).to(fw.device)

    def to_json(self):
        return {"kind": self.kind, "coverages": self.coverages, "n": self.n, "ranks": self.ranks,
                "offsets": _enc(self.offsets.tolist()), "parts": None if self.windowed else list(PARTS), **self.provenance}

    def save(self, path):
        with open(path, "w") as f:
            json.dump(self.to_json(), f, indent=1, allow_nan=False)       # strict JSON: to_json's _enc has named the infinities

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
            ci = idx[0] if self.windowed else idx[1]
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


def calibrate_horizon_levels(fw, target, levels):
    """scalar_horizon_level: fw (windows, n_levels, H_fwd) from ONE predict_windows_levels launch on the window starts, target
    (windows, H_fwd).  The scores target - fw are laid out (n_levels * H_fwd, windows), row (level, step) taking its level's rank:
    one offset per level and step ahead, level l calibrated to coverage l."""
    W, L, H = fw.shape
    if len(levels) != L or tuple(target.shape) != (W, H):
        raise ValueError(f"fw {tuple(fw.shape)} does not fit {len(levels)} levels and target {tuple(target.shape)}")
    if L * H > 4096:
        raise ValueError(f"{L} levels x {H} steps ahead = {L * H} score rows exceed the selection's 4096 batch rows: calibrate fewer levels at once")
    ranks = _ranks(W, levels)
    scores = (target[:, None, :] - fw).permute(1, 2, 0).reshape(L * H, W)
    q, _ = select_kth(scores, torch.tensor(ranks).repeat_interleave(H)[:, None])
    return Calibration("horizon_levels", levels, q.reshape(L, H), W, ranks)


def default_path(run):
    return os.path.join(run, CALIBRATION_NAME)


class AgeCalibration:
    """Roll-out offsets per age of the fed-back state (steps since the last reseed), and optionally a trajectory margin.

    offsets (n_coverages, max_age, out): offsets[c, a] is the conformal offset of the steps of age a; ages >= max_age - 1 share
    the last group.  counts (max_age): calibration steps per group; ranks (max_age, n_coverages).  margin (n_coverages, out), with
    margin_n envs and margin_ranks (n_coverages): delta of calibrate_trajectory, or None.  provenance as for Calibration."""

    def __init__(self, coverages, offsets, counts, ranks, margin=None, margin_n=None, margin_ranks=None, provenance=None):
        self.coverages = [float(c) for c in coverages]
        self.offsets = torch.as_tensor(offsets, dtype=torch.float32).cpu()
        self.counts = [int(v) for v in torch.as_tensor(counts).reshape(-1).tolist()]
        self.ranks = [[int(v) for v in row] for row in torch.as_tensor(ranks).tolist()]
        self.provenance = dict(provenance or {})
        C_ = len(self.coverages)
        if self.offsets.dim() != 3 or self.offsets.shape[0] != C_ or self.offsets.shape[1] != len(self.counts) \
                or len(self.ranks) != len(self.counts) or any(len(r) != C_ for r in self.ranks):
            raise ValueError(f"offsets {tuple(self.offsets.shape)} do not fit {C_} coverages and {len(self.counts)} ages")
        self.max_age = self.offsets.shape[1]
        self.margin = None if margin is None else torch.as_tensor(margin, dtype=torch.float32).cpu()
        self.margin_n = None if margin is None else int(margin_n)
        self.margin_ranks = None if margin is None else [int(r) for r in margin_ranks]
        if self.margin is not None and (tuple(self.margin.shape) != (C_, self.offsets.shape[2]) or len(self.margin_ranks) != C_):
            raise ValueError(f"margin {tuple(self.margin.shape)} does not fit offsets {tuple(self.offsets.shape)}")
        if bool(torch.isnan(self.offsets).any()):
            c, a, o = torch.isnan(self.offsets).nonzero()[0].tolist()
            raise ValueError(f"NaN offset at coverage {self.coverages[c]}, age {a}, column {o}: a NaN score reached the rank")
        if self.margin is not None and bool(torch.isnan(self.margin).any()):
            c, o = torch.isnan(self.margin).nonzero()[0].tolist()
            raise ValueError(f"NaN margin at coverage {self.coverages[c]}, column {o}: a NaN score reached the rank")

    def index(self, coverage):
        return _coverage_index(self.coverages, coverage)

    def _gather(self, age, coverage, dev):
        age = torch.as_tensor(age).long().clamp(0, self.max_age - 1)
        return self.offsets[self.index(coverage)].to(dev)[age.to(dev)]

    def _margin(self, coverage, dev):
        if self.margin is None:
            raise ValueError("this calibration holds no trajectory margin: calibrate_tube.py --by_age --trajectory writes one")
        return self.margin[self.index(coverage)].to(dev)

    def offset_at(self, age, coverage, trajectory=False):
        """(..., out) for ages (...): the offset of each age, clamped to max_age - 1; with trajectory the margin added."""
        dev = age.device if torch.is_tensor(age) else "cpu"
        q = self._gather(age, coverage, dev)
        return q + self._margin(coverage, dev) if trajectory else q

    def apply(self, fw, age, coverage, trajectory=False):
        """fw + offset_at(age): fw (..., out), age (...)."""
        return fw + self.offset_at(torch.as_tensor(age).to(fw.device), coverage, trajectory)

    def covers(self, fw, w, age, coverage, trajectory=False):
        """(w - fw) <= offset, the exact form of apply(fw) >= w.  With trajectory: ((w - fw) - offset) <= margin, the arithmetic of
        the score the margin was selected from, so that the count on the margin envs is exact."""
        q = self._gather(age, coverage, fw.device)
        if trajectory:
            return ((w - fw) - q) <= self._margin(coverage, fw.device)
        return (w - fw) <= q

    def to_json(self):
        return {"kind": "age", "coverages": self.coverages, "max_age": self.max_age, "counts": self.counts, "ranks": self.ranks,
                "offsets": _enc(self.offsets.tolist()), "margin": None if self.margin is None else _enc(self.margin.tolist()),
                "margin_n": self.margin_n, "margin_ranks": self.margin_ranks, **self.provenance}

    save = Calibration.save                                # the same strict-JSON writer, on this class's to_json

    @classmethod
    def load(cls, path):
        with open(path) as f:
            d = json.load(f)
        if d.get("kind") != "age":
            raise ValueError(f"{path} holds a {d.get('kind')!r} calibration, not a per-age one ({AGE_CALIBRATION_NAME})")
        core = ("kind", "coverages", "max_age", "counts", "ranks", "offsets", "margin", "margin_n", "margin_ranks")
        return cls(d["coverages"], _dec(d["offsets"]), d["counts"], d["ranks"], None if d["margin"] is None else _dec(d["margin"]),
                   d["margin_n"], d["margin_ranks"], {k: v for k, v in d.items() if k not in core})

    def lines(self):
        """One printed line per (coverage, age, column): rank, count, offset; then the margin lines."""
        out = []
        for c, cv in enumerate(self.coverages):
            for a in range(self.max_age):
                for o in range(self.offsets.shape[2]):
                    out.append(f"rollout, coverage {cv}, age {a}{'+' if a == self.max_age - 1 else ''}, column {o}: rank {self.ranks[a][c]} of "
                               f"count {self.counts[a]}, offset {float(self.offsets[c, a, o])}")
        if self.margin is not None:
            for c, cv in enumerate(self.coverages):
                for o in range(self.margin.shape[1]):
                    out.append(f"trajectory margin, coverage {cv}, column {o}: rank {self.margin_ranks[c]} of {self.margin_n} envs, "
                               f"margin {float(self.margin[c, o])}")
        return out


def age_groups(done, reseed, max_age=None):
    """(group (E, T) int32, G): group = min(steps since the last reseed, G - 1) where the step is kept (~done), else -1.  G = max_age
    if given, otherwise min(oldest kept age + 1, MAX_GROUPS); ages past the last group share it."""
    from .evaluate import steps_since
    keep = ~done.bool()
    age = steps_since(reseed.to(keep.device))
    if max_age is None:
        G = min(int(age[keep].max()) + 1, MAX_GROUPS) if bool(keep.any()) else 1
    else:
        G = int(max_age)
        if not 1 <= G <= MAX_GROUPS:
            raise ValueError(f"max_age must be 1..{MAX_GROUPS}; got {max_age}")
    return torch.where(keep, age.clamp(max=G - 1), torch.full_like(age, -1)).to(torch.int32), G


def _take_envs(envs, *tensors):
    if envs is None:
        return tensors
    envs = torch.as_tensor(envs).long()
    return tuple(t[envs.to(t.device)] for t in tensors)


def calibrate_by_age(model, data, target, done, layout, reseed, coverages, kind="scalar", max_age=None, envs=None):
    """Flat kinds: the roll-out scores target - rollout_window(...) of calibrate_flat, one conformal offset per age of the fed-back
    state instead of one for all -- one lg_select_kth_grouped call, the batch rows the output columns, the groups the ages
    (age_groups).  envs: an index tensor, the envs to calibrate on (default all).
    Returns (offsets (n_coverages, G, out), counts (G), ranks (G, n_coverages)), on the device."""
    if kind not in FLAT_KINDS:
        raise ValueError(f"{kind}: per-age offsets are for the roll-out of the flat kinds ({', '.join(FLAT_KINDS)})")
    data, target, done, reseed = _take_envs(envs, data, target, done, reseed)
    E, T, _ = data.shape
    O = target.shape[2]
    fw = model.rollout_window(data, *layout, reseed)
    group, G = age_groups(done, reseed, max_age)
    scores = (target - fw).reshape(E * T, O).t()
    q, counts, ranks = select_kth_grouped(scores, group.reshape(-1), G, coverages)          # (out, G, n_coverages)
    return q.permute(2, 1, 0).contiguous(), counts, ranks


def calibrate_trajectory(model, data, target, done, layout, reseed, coverages, kind="scalar", max_age=None, envs=None, split=None):
    """calibrate_by_age on one half of the envs, and on the other half a margin from one score per env, so that
    P(every kept step of a fresh env is covered) >= c per output column: exact split conformal over envs, which are exchangeable
    (DESIGN.md section 10.7).  split: (shape envs, margin envs) index tensors; default the even and the odd entries of envs (of
    all envs).  The score of margin env e is s[c, o, e] = max over its kept steps t of (target - fw - q[c, group(e, t), o]), an
    infinite q contributing -inf; delta[c, o] is the conformal_rank(E_margin, c)-th smallest of s[c, o, :] (select_kth).
    Returns an AgeCalibration with offsets q and margin delta."""
    if split is None:
        idx = torch.arange(data.shape[0]) if envs is None else torch.as_tensor(envs).long().cpu()
        split = (idx[0::2], idx[1::2])
    shape_envs, margin_envs = split
    if len(margin_envs) < 1 or len(shape_envs) < 1:
        raise ValueError("a trajectory margin needs at least two envs: one for the offsets and one for the margin")
    q, counts, ranks = calibrate_by_age(model, data, target, done, layout, reseed, coverages, kind, max_age, shape_envs)
    data, target, done, reseed = _take_envs(margin_envs, data, target, done, reseed)
    Em, T, _ = data.shape
    O, G, nc = target.shape[2], q.shape[1], q.shape[0]
    fw = model.rollout_window(data, *layout, reseed)
    group, _ = age_groups(done, reseed, G)
    keep = group.ge(0)
    qs = q[:, group.clamp(min=0).long()]                                                   # (n_coverages, E_margin, T, out)
    s = (target - fw)[None] - qs
    s = torch.where(keep[None, :, :, None], s, torch.full_like(s, -math.inf)).amax(dim=2)   # (n_coverages, E_margin, out)
    m_ranks = _ranks(Em, coverages)
    per_row = torch.tensor(m_ranks).repeat_interleave(O)[:, None]                           # row (coverage, column)
    delta, _ = select_kth(s.permute(0, 2, 1).reshape(nc * O, Em), per_row)
    return AgeCalibration(coverages, q, counts, ranks, delta.reshape(nc, O), Em, m_ranks)


def default_age_path(run):
    return os.path.join(run, AGE_CALIBRATION_NAME)
