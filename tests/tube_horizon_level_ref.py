"""Test-only NumPy / float64 restatement of the level-conditioned one-shot item: the
ScalarHorizonTubeDataset item at (env, start) with the coverage level appended as the last column, and its target.  The loss is
tests/tube_level_ref.py's, one level per row shared by the row's H_fwd outputs."""
import numpy as np
import torch


def item(w, z, v, env, start, H_fwd, H_rev, level=None):
    """w (n, T), z (n, T, nz), v (n, T, m) as arrays; returns (x float64 (H_rev + nz + (H_rev + H_fwd) m [+ 1]), y float64 (H_fwd))."""
    w, z, v = (np.asarray(a, dtype=np.float64) for a in (w, z, v))
    parts = [w[env, start - H_rev:start], z[env, start, :], v[env, start - H_rev:start + H_fwd, :].reshape(-1)]
    if level is not None:
        parts.append(np.array([level], dtype=np.float64))
    return np.concatenate(parts), w[env, start + 1:start + H_fwd + 1]


def items(ds, env, start, level=None, dtype=torch.float64, targets=True):
    """Stacked items of a dataset (w, z, v, H_fwd, H_rev): x (count, I), y (count, H_fwd).  level: None, a number, or one per item.
    targets=False returns y = None: a query window may start as late as T - H_fwd, where the target w[start + 1 : start + H_fwd + 1]
    no longer exists."""
    w, z, v = (t.detach().cpu().numpy() for t in (ds.w, ds.z, ds.v))
    env, start = np.asarray(env).reshape(-1), np.asarray(start).reshape(-1)
    lv = [None] * env.size if level is None else np.broadcast_to(np.asarray(level, dtype=np.float64).reshape(-1), (env.size,))
    pairs = [item(w, z, v, int(e), int(s), ds.H_fwd, ds.H_rev, l) for e, s, l in zip(env, start, lv)]
    return (torch.from_numpy(np.stack([p[0] for p in pairs])).to(dtype),
            torch.from_numpy(np.stack([p[1] for p in pairs])).to(dtype) if targets else None)


def dataset(n, T, nz, m, H_fwd, H_rev, seed, conditioned=True):
    """A random window dataset of the kind under test: w >= 0 (n, T), z (n, T, nz), v (n, T, m)."""
    from legged_gym_dev_amd.tube import data as td
    g = torch.Generator().manual_seed(seed)
    w, z, v = torch.rand(n, T, generator=g), torch.randn(n, T, nz, generator=g), torch.randn(n, T, m, generator=g)
    cls = td.LevelScalarHorizonTubeDataset if conditioned else td.ScalarHorizonTubeDataset
    return cls(w, z, v, H_fwd, H_rev, H_rev + nz + (H_rev + H_fwd) * m + int(conditioned), H_fwd)
