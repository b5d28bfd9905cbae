"""Tube-learning datasets (the semantics of deep_tube_learning/datasets.py, built from a local folder instead of wandb).

The input is the folder ``scripts/collect_trajectory_data.py`` writes: ``epoch_<k>.pickle`` files, each a dict of numpy arrays
z (N, T+1, n), pz_x (N, T+1, n), v (N, T, m) and done (N, T).  Datasets hold host float32 torch tensors; the trainer copies them
to the device once.
"""
import glob
import os
import pickle
import re

import numpy as np
import torch


def _epoch_files(folder):
    files = glob.glob(os.path.join(folder, "epoch_*.pickle"))
    key = lambda f: int(re.match(r"epoch_(\d+)\.pickle$", os.path.basename(f)).group(1))
    return sorted((f for f in files if re.match(r"epoch_\d+\.pickle$", os.path.basename(f))), key=key)


def construct_dataset(folder):
    """Concatenate the epochs of `folder` on axis 0 (in numeric epoch order) and add the one-step-ahead arrays.

    Returns a dict with z, pz_x (E*N, T+1, n), v (E*N, T, m), z_p1 = z[:, 1:], pz_x_p1 = pz_x[:, 1:] and done (E*N, T).

    Every epoch's ``done[-1, :]`` is set before concatenating, as the reference does.  On this (env, time) layout that marks
    every step of the *last env* of each epoch as done (so its rows are all dropped by the row datasets), not the last step of
    every env.  Nothing is cached on disk.
    """
    files = _epoch_files(folder)
    if not files:
        raise FileNotFoundError(f"no epoch_<k>.pickle files in {folder}")
    parts = {k: [] for k in ("z", "pz_x", "v", "done")}
    for f in files:
        with open(f, "rb") as fh:
            rec = pickle.load(fh)
        done = np.array(rec["done"], copy=True)
        done[-1, :] = True
        parts["done"].append(done)
        for k in ("z", "pz_x", "v"):
            parts[k].append(rec[k])
    out = {k: np.concatenate(v, axis=0) for k, v in parts.items()}
    out["z_p1"] = out["z"][:, 1:, :].copy()
    out["pz_x_p1"] = out["pz_x"][:, 1:, :].copy()
    return out


def get_slice(data, i, dN, m):
    """data (E, T, c) delayed by i * dN steps with stride dN: entry t holds data[:, t - i*dN - k*dN] for the k that keeps the
    steps aligned to the end of the window; the front that has no such step is filled with the first sample, whose last m
    (input) columns are zeroed."""
    T = data.shape[-2]
    steps = np.arange(T - 1 - i * dN, -1, -dN)[::-1]
    first = data[:, :1, :].copy()
    first[:, :, -m:] = 0
    return np.concatenate((np.repeat(first, T - steps.size, axis=-2), data[:, steps, :]), axis=-2)


def sliding_window(data, N, dN, m):
    """The N delayed copies of get_slice side by side on the last axis (delay 0 first)."""
    return np.concatenate([get_slice(data, i, dN, m) for i in range(N)], axis=-1)


def _load(src):
    return construct_dataset(src) if isinstance(src, (str, os.PathLike)) else src


class TubeDataset:
    """Rows of (data, target): float32 torch tensors (rows, input_dim), (rows, output_dim)."""
    conditioned = False                 # True: the model takes one more, last, input column that the data does not hold (the level)

    def __init__(self, data, target, input_dim, output_dim):
        self.data, self.target = data, target
        self.input_dim, self.output_dim = input_dim, output_dim

    def __len__(self):
        return self.data.shape[0]

    def __getitem__(self, idx):
        return self.data[idx, :], self.target[idx, :]

    def update(self):
        pass

    def random_split(self, p):
        """Train part: one contiguous piece of int(len * p) rows starting at np.random.randint(len - that); test: the rest."""
        n = int(len(self) * p)
        s = np.random.randint(len(self) - n)
        cut = lambda t: (t[s:s + n], torch.vstack((t[:s], t[s + n:])))
        (d1, d2), (t1, t2) = cut(self.data), cut(self.target)
        return (type(self)(d1, t1, self.input_dim, self.output_dim), type(self)(d2, t2, self.input_dim, self.output_dim))

    @staticmethod
    def _rows(data, target, done):
        flat = data.reshape((-1, data.shape[-1]))
        tgt = target.reshape((flat.shape[0], -1))
        keep = np.logical_not(done.reshape(-1))
        return torch.from_numpy(flat[keep]).float(), torch.from_numpy(tgt[keep]).float()


class ScalarTubeDataset(TubeDataset):
    """Input: the tracking error norm w_t = |pz_x - z| and the non-position ROM state and input, over a window of N samples
    dN apart (recursive: the window covers w too); target w_{t+1}."""

    @staticmethod
    def _sequences(ds, N=1, dN=1, recursive=False):
        z, pz_x, v = ds["z"][:, :-1, :], ds["pz_x"][:, :-1, :], ds["v"]
        w = np.linalg.norm(pz_x - z, axis=-1)
        w_p1 = np.linalg.norm(ds["pz_x_p1"] - ds["z_p1"], axis=-1)
        m = v.shape[-1]
        if recursive:
            data = sliding_window(np.concatenate((w[:, :, None], z[:, :, 2:], v), axis=-1), N, dN, m)
        else:
            data = np.concatenate((w[:, :, None], sliding_window(np.concatenate((z[:, :, 2:], v), axis=-1), N, dN, m)), axis=-1)
        return data, w_p1[:, :, None]

    @classmethod
    def from_folder(cls, src, N=1, dN=1, recursive=False):
        ds = _load(src)
        x, y = cls._rows(*cls._sequences(ds, N, dN, recursive), ds["done"])
        return cls(x, y, x.shape[1], 1)


class VectorTubeDataset(TubeDataset):
    """Input: |pz_x - z| per axis, z and v over the window; target |pz_x - z| per axis one step ahead."""

    @staticmethod
    def _sequences(ds, N=1, dN=1):
        z, pz_x, v = ds["z"][:, :-1, :], ds["pz_x"][:, :-1, :], ds["v"]
        data = sliding_window(np.concatenate((np.abs(pz_x - z), z, v), axis=-1), N, dN, v.shape[-1])
        return data, np.abs(ds["pz_x_p1"] - ds["z_p1"])

    @classmethod
    def from_folder(cls, src, N=1, dN=1):
        ds = _load(src)
        x, y = cls._rows(*cls._sequences(ds, N, dN), ds["done"])
        return cls(x, y, x.shape[1], y.shape[1])


class ErrorDynamicsDataset(TubeDataset):
    """Input: the signed error pz_x - z, z and v over the window; target the signed error one step ahead."""

    @staticmethod
    def _sequences(ds, N=1, dN=1):
        z, pz_x, v = ds["z"][:, :-1, :], ds["pz_x"][:, :-1, :], ds["v"]
        data = sliding_window(np.concatenate((pz_x - z, z, v), axis=-1), N, dN, v.shape[-1])
        return data, ds["pz_x_p1"] - ds["z_p1"]

    @classmethod
    def from_folder(cls, src, N=1, dN=1):
        ds = _load(src)
        x, y = cls._rows(*cls._sequences(ds, N, dN), ds["done"])
        return cls(x, y, x.shape[1], y.shape[1])


class ScalarHorizonTubeDataset:
    """Per env: the error norm w, the non-position ROM state z and the input v over time, padded in front by H_rev steps
    (w and z with their first sample, v with zeros).  Item (env, ind) -- ind drawn uniformly from [H_rev, T' - H_fwd - 1) -- is
    input [w[ind-H_rev:ind], z[ind], v[ind-H_rev:ind+H_fwd].flatten()] and target w[ind+1:ind+H_fwd+1].  As in the reference,
    the input does not hold the current error w[ind]."""
    conditioned = False

    def __init__(self, w, z, v, H_fwd, H_rev, input_dim, output_dim):
        self.w, self.z, self.v = w, z, v
        self.H_fwd, self.H_rev = H_fwd, H_rev
        self.input_dim, self.output_dim = input_dim, output_dim

    @classmethod
    def from_folder(cls, src, H_fwd=50, H_rev=10):
        ds = _load(src)
        z, pz_x, v = ds["z"][:, :-1, :], ds["pz_x"][:, :-1, :], ds["v"]
        v = np.concatenate((np.zeros((v.shape[0], H_rev, v.shape[2])), v), axis=1)
        z = np.concatenate((np.repeat(z[:, None, 0, :], H_rev, axis=1), z), axis=1)
        pz_x = np.concatenate((np.repeat(pz_x[:, None, 0, :], H_rev, axis=1), pz_x), axis=1)
        w = np.linalg.norm(pz_x - z, axis=-1)
        z_no_pos = z[:, :, 2:]
        input_dim = H_rev + z_no_pos.shape[-1] + (H_rev + H_fwd) * v.shape[-1]
        return cls(torch.from_numpy(w).float(), torch.from_numpy(z_no_pos).float(), torch.from_numpy(v).float(),
                   H_fwd, H_rev, input_dim, H_fwd)

    def __len__(self):
        return self.w.shape[0]

    def __getitem__(self, idx):
        ind = int(torch.randint(self.H_rev, self.w.shape[1] - self.H_fwd - 1, (1,)))
        return self._get_item_helper(idx, ind)

    def _get_item_helper(self, idx, ind):
        Hr, Hf = self.H_rev, self.H_fwd
        x = torch.cat((self.w[idx, ind - Hr:ind], self.z[idx, ind, :], self.v[idx, ind - Hr:ind + Hf].reshape((-1,))))
        return x, self.w[idx, ind + 1:ind + Hf + 1]

    def update(self):
        pass

    def random_split(self, p):
        """As TubeDataset.random_split, over envs."""
        n = int(len(self) * p)
        s = np.random.randint(len(self) - n)
        cut = lambda t: (t[s:s + n], torch.vstack((t[:s], t[s + n:])))
        (w1, w2), (z1, z2), (v1, v2) = cut(self.w), cut(self.z), cut(self.v)
        mk = lambda w, z, v: type(self)(w, z, v, self.H_fwd, self.H_rev, self.input_dim, self.output_dim)
        return mk(w1, z1, v1), mk(w2, z2, v2)


_ALPHA_REASON = ("is not supported: in the reference, alpha = data[:, -1] has shape (B,) while the residual has shape (B, 1), so "
                 "torch.where broadcasts the loss to B x B; no configuration uses it")


class AlphaScalarTubeDataset(TubeDataset):
    def __init__(self, *a, **k):
        raise NotImplementedError("AlphaScalarTubeDataset " + _ALPHA_REASON)

    @classmethod
    def from_folder(cls, *a, **k):
        raise NotImplementedError("AlphaScalarTubeDataset " + _ALPHA_REASON)


class AlphaVectorTubeDataset(TubeDataset):
    def __init__(self, *a, **k):
        raise NotImplementedError("AlphaVectorTubeDataset " + _ALPHA_REASON)

    @classmethod
    def from_folder(cls, *a, **k):
        raise NotImplementedError("AlphaVectorTubeDataset " + _ALPHA_REASON)


class LevelScalarTubeDataset(ScalarTubeDataset):
    """ScalarTubeDataset's rows and targets for a level-conditioned tube: the model's input is the row
    plus one last column, the coverage level, so input_dim is the data width + 1.  The data holds no level: the trainer draws one
    per row at every step on the device, and the row's pinball loss takes it in place of alpha -- one level per row, where the
    reference's AlphaScalarTubeLoss broadcasts (B,) against (B, 1) to B x B."""
    conditioned = True

    @classmethod
    def from_folder(cls, src, N=1, dN=1, recursive=False):
        ds = _load(src)
        x, y = cls._rows(*cls._sequences(ds, N, dN, recursive), ds["done"])
        return cls(x, y, x.shape[1] + 1, 1)


class LevelVectorTubeDataset(VectorTubeDataset):
    """VectorTubeDataset's rows and targets for a level-conditioned tube; see LevelScalarTubeDataset."""
    conditioned = True

    @classmethod
    def from_folder(cls, src, N=1, dN=1):
        ds = _load(src)
        x, y = cls._rows(*cls._sequences(ds, N, dN), ds["done"])
        return cls(x, y, x.shape[1] + 1, y.shape[1])


class LevelScalarHorizonTubeDataset(ScalarHorizonTubeDataset):
    """ScalarHorizonTubeDataset's arrays for a level-conditioned one-shot tube: the model's item is the
    window item plus one last column, the coverage level, so input_dim is the item width + 1.  The arrays hold no level: the trainer
    draws one per row at every step, and the row's H_fwd outputs share it in the pinball loss."""
    conditioned = True

    @classmethod
    def from_folder(cls, src, H_fwd=50, H_rev=10):
        ds = ScalarHorizonTubeDataset.from_folder(src, H_fwd, H_rev)
        return cls(ds.w, ds.z, ds.v, H_fwd, H_rev, ds.input_dim + 1, H_fwd)


DATASETS = {"scalar": ScalarTubeDataset, "vector": VectorTubeDataset, "error_dynamics": ErrorDynamicsDataset,
            "scalar_horizon": ScalarHorizonTubeDataset, "scalar_level": LevelScalarTubeDataset,
            "vector_level": LevelVectorTubeDataset, "scalar_horizon_level": LevelScalarHorizonTubeDataset}
LEVEL_KINDS = {"scalar_level": "scalar", "vector_level": "vector"}     # conditioned flat kind -> the kind whose rows it has
HORIZON_KINDS = ("scalar_horizon", "scalar_horizon_level")             # window kinds: no per-step rows, no closed loop
HORIZON_LEVEL_KIND = "scalar_horizon_level"                            # the conditioned window kind (section 10.8)


def sequences(kind, src, **window_args):
    """The per-env, time-ordered rows that ``DATASETS[kind].from_folder(src, **window_args)`` builds before it drops the done
    rows: float32 tensors data (E, T, input_dim) and target (E, T, output_dim), and done (E, T) bool.  Row (e, t) holds the
    model's input at step t and its target, the quantity one step ahead; a done row's target belongs to the next episode.
    Flat kinds only: the horizon dataset has no rows.  A level kind returns its base kind's rows (input_dim - 1 columns: the
    level column is the caller's to append, HipTubeModel.with_level)."""
    if kind not in DATASETS or kind in HORIZON_KINDS:
        raise ValueError(f"sequences: kind {kind!r} has no per-step rows; one of {[k for k in DATASETS if k not in HORIZON_KINDS]}")
    ds = _load(src)
    data, target = DATASETS[kind]._sequences(ds, **window_args)
    return (torch.from_numpy(np.ascontiguousarray(data)).float(), torch.from_numpy(np.ascontiguousarray(target)).float(),
            torch.from_numpy(np.array(ds["done"], dtype=bool)))


def feedback_width(kind, N=1, dN=1, recursive=False, n=None):
    """How many leading input columns of a `kind` row are the model's own previous output, i.e. what a closed-loop roll-out
    feeds back: 1 (the error norm w) for scalar, n (the ROM state width) for vector and error_dynamics.  Raises
    NotImplementedError where the fed-back quantity also sits in delayed window taps (N > 1 with vector, error_dynamics or
    recursive=True): those taps would have to come from the roll-out's own past, and the reference rolls out N = 1 only.
    A level kind has its base kind's width: the level column is the last one."""
    kind = LEVEL_KINDS.get(kind, kind)
    if kind == "scalar":
        if N > 1 and recursive:
            raise NotImplementedError("roll-out of a recursive scalar window (N > 1): the delayed taps hold w too")
        return 1
    if kind in ("vector", "error_dynamics"):
        if N > 1:
            raise NotImplementedError(f"roll-out of a {kind} window with N > 1: the delayed taps hold the error too")
        if n is None or n < 1:
            raise ValueError(f"feedback_width({kind!r}) needs n, the ROM state width")
        return int(n)
    raise ValueError(f"feedback_width: kind {kind!r} has no closed loop")


def feedback_layout(kind, N=1, dN=1, recursive=False, n=None, m=None):
    """(fb, taps, lag, stride) of a `kind` row of sequences() for the windowed closed-loop roll-out
    (HipTubeModel.rollout_window(x, fb, taps, lag, stride)): the row is `taps` blocks of `stride` columns, block i is block 0 of
    the row i * lag steps earlier, and the leading fb columns of every block hold the model's own output.  n: the width of z,
    m: the width of v.
        scalar, not recursive   (1, 1, 1, input width): only the leading w is fed back, the window holds z and v alone
        scalar, recursive       (1, N, 1, 1 + (n - 2) + m): every block is (w, z without its position, v)
        vector, error_dynamics  (n, N, 1, 2 n + m): every block is (error, z, v)
    The lag is 1 row whatever dN is: get_slice keeps every dN-th sample counted back from the end of the episode in EVERY
    block, block 0 included, so the rows of a dN > 1 dataset are a subsampled series (padded in front) in which block i still
    trails block 0 by i rows.  That is the window the model was trained on, so it is the one a roll-out over these rows feeds.
    Unlike feedback_width it refuses no window: the delayed taps come from the roll-out's own past.
    A level kind (scalar_level, vector_level) has its base kind's layout; its row carries the level as one more, last, column, which
    no block reaches ((taps - 1) * stride + fb <= input_dim holds as before), so only the non-recursive scalar stride, which
    counts the whole row, grows by one: 1 + N (n - 2 + m) + 1."""
    level = kind in LEVEL_KINDS
    kind = LEVEL_KINDS.get(kind, kind)
    if N < 1 or dN < 1:
        raise ValueError(f"feedback_layout: N={N} and dN={dN} must be at least 1")
    if kind not in ("scalar", "vector", "error_dynamics"):
        raise ValueError(f"feedback_layout: kind {kind!r} has no closed loop")
    if n is None or m is None or n < 1 or m < 1:
        raise ValueError(f"feedback_layout({kind!r}) needs n and m, the widths of z and v")
    n, m = int(n), int(m)
    if kind == "scalar":
        if not recursive:
            return 1, 1, 1, 1 + N * (n - 2 + m) + int(level)
        return 1, int(N), 1, 1 + (n - 2) + m
    return n, int(N), 1, 2 * n + m
