"""The actor's observation history (include/legged_hip.h lg_obs_hist_*) restated in numpy from a recorded sequence of
(obs_t, reset_t, marks_t).  Pure copying in float32: every comparison against it is bit for bit (``bits``), no tolerance.

Row of env i after step t, newest first:  [ obs_t | sel(obs_t-1) | ... | sel(obs_t-H+1) ].  An env whose reset_t or marks_t is
set is reinitialised at step t: every past frame becomes sel(obs_t) ("repeat") or zeros ("zero").  A fresh history has a row of
zeros and every env marked."""
import numpy as np


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def columns(num_obs, ranges):
    """The selected obs columns in a past frame's order; ranges None or () = all."""
    if not ranges:
        return np.arange(num_obs)
    return np.concatenate([np.arange(lo, hi) for lo, hi in ranges])


class HistoryRef:
    def __init__(self, n, num_obs, length, ranges=None, reset="repeat"):
        assert length >= 2 and reset in ("repeat", "zero")
        self.n, self.O, self.H, self.reset = int(n), int(num_obs), int(length), reset
        self.cols = columns(num_obs, ranges)
        self.S = len(self.cols)
        self.W = self.O + (self.H - 1) * self.S
        self.row = np.zeros((self.n, self.W), np.float32)
        self.fresh = np.ones(self.n, bool)                    # every env starts marked

    def step(self, obs, reset, marks=None):
        """One compute after an env step: obs (n, O) float32, reset (n) the step's dones, marks (n) the envs a reset_idx outside
        the step marked since the previous compute (None: none).  Returns the new (n, W) row (a copy)."""
        obs = np.ascontiguousarray(obs, np.float32)
        assert obs.shape == (self.n, self.O)
        re = np.asarray(reset).astype(bool).reshape(self.n) | self.fresh
        if marks is not None:
            re = re | np.asarray(marks).astype(bool).reshape(self.n)
        self.fresh[:] = False
        old = self.row
        new = np.empty_like(old)
        new[:, :self.O] = obs
        past_old = old[:, self.O:].reshape(self.n, self.H - 1, self.S)
        past_new = new[:, self.O:].reshape(self.n, self.H - 1, self.S)       # a view: writes land in new
        past_new[:, 0] = old[:, :self.O][:, self.cols]
        past_new[:, 1:] = past_old[:, :-1]
        fill = obs[:, self.cols][:, None, :] if self.reset == "repeat" else np.zeros((self.n, 1, self.S), np.float32)
        past_new[re] = np.broadcast_to(fill, past_new.shape)[re]
        self.row = new
        return new.copy()

    def frames(self):
        """The past frames as (n, H - 1, S), and the selected columns of the current block (n, S)."""
        return self.row[:, self.O:].reshape(self.n, self.H - 1, self.S), self.row[:, :self.O][:, self.cols]


def restate(seq, num_obs, length, ranges=None, reset="repeat"):
    """Rows after every step of seq = [(obs_t, reset_t, marks_t or None), ...] from a fresh history: a list of (n, W) arrays."""
    ref = HistoryRef(len(seq[0][0]), num_obs, length, ranges, reset)
    return [ref.step(*item) for item in seq]
