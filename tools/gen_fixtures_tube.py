#!/usr/bin/env python3
"""Golden fixtures for the tube-learning datasets and losses (deep_tube_learning/datasets.py, losses.py):
    tests/golden/tube_{dataset,rows,horizon,losses}.npz

TEST INFRASTRUCTURE -- needs the reference tree (REF below); the .npz files it writes are committed.  It imports the reference's
datasets and losses modules at run time (wandb, which they import but never touch on these paths, is stubbed) and runs them on a
small seeded synthetic data folder: two epochs of N = 6 envs x T = 40 ROM steps, n = m = 2, some done flags set.  The reference
reads epoch files in glob order; the glob is pinned to numeric epoch order here, the one intended difference.

Files:
    tube_dataset.npz   the synthetic epochs (e<k>_<key>) and construct_dataset's output (cd_<key>)
    tube_rows.npz      data / target of ScalarTubeDataset (N=1; N=3 recursive and not), VectorTubeDataset (N=2, dN=2),
                       ErrorDynamicsDataset (N=2)
    tube_horizon.npz   ScalarHorizonTubeDataset(H_fwd=8, H_rev=3): w, z, v and _get_item_helper at fixed (idx, ind)
    tube_losses.npz    value and d/dfw (autograd) of ScalarTubeLoss, ScalarHorizonTubeLoss, VectorTubeLoss, ErrorLoss, with
                       ties at r = 0 and |l| = delta

    python tools/gen_fixtures_tube.py
"""
import glob as _glob
import os
import pickle
import re
import sys
import tempfile
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("LG_REFERENCE", "/root/reference")
OUT = os.path.join(ROOT, "tests", "golden")

HORIZON_ITEMS = [(0, 3), (5, 20), (11, 9), (7, 33)]    # (env, window start in [H_rev, T + H_rev - H_fwd - 1)) for _get_item_helper


def synthetic_epochs(seed=7, E=2, N=6, T=40, n=2, m=2):
    rng = np.random.default_rng(seed)
    eps = []
    for _ in range(E):
        z = rng.normal(size=(N, T + 1, n)).cumsum(axis=1).astype(np.float32) * 0.1
        pz_x = (z + rng.normal(scale=0.05, size=z.shape)).astype(np.float32)
        v = rng.uniform(-0.35, 0.35, size=(N, T, m)).astype(np.float32)
        done = rng.uniform(size=(N, T)) < 0.05
        eps.append({"z": z, "pz_x": pz_x, "v": v, "done": done})
    return eps


def reference_modules():
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    sys.path.insert(0, REF)
    import deep_tube_learning.datasets as ds
    import deep_tube_learning.losses as ls
    numeric = lambda pat: sorted(_glob.glob(pat), key=lambda f: int(re.search(r"epoch_(\d+)\.pickle$", f).group(1)))
    ds.glob = types.SimpleNamespace(glob=numeric)
    return ds, ls


def main():
    ds, ls = reference_modules()
    eps = synthetic_epochs()
    fx = {}
    with tempfile.TemporaryDirectory() as d:
        cwd = os.getcwd()
        os.chdir(d)
        try:
            folder = os.path.join("rom_tracking_data", "synth")
            os.makedirs(folder)
            for k, e in enumerate(eps):
                with open(os.path.join(folder, f"epoch_{k}.pickle"), "wb") as f:
                    pickle.dump({kk: vv.copy() for kk, vv in e.items()}, f)
                for kk, vv in e.items():
                    fx[f"e{k}_{kk}"] = vv
            cd = ds.construct_dataset(folder)
            ds_fx = dict(fx)
            ds_fx.update({f"cd_{k}": v for k, v in cd.items()})
            np.savez_compressed(os.path.join(OUT, "tube_dataset.npz"), **ds_fx)

            rows = {}
            for name, obj in [("scalar_n1", ds.ScalarTubeDataset.from_wandb("synth", N=1, dN=1)),
                              ("scalar_n3", ds.ScalarTubeDataset.from_wandb("synth", N=3, dN=1, recursive=False)),
                              ("scalar_n3_rec", ds.ScalarTubeDataset.from_wandb("synth", N=3, dN=1, recursive=True)),
                              ("vector_n2", ds.VectorTubeDataset.from_wandb("synth", N=2, dN=2)),
                              ("error_n2", ds.ErrorDynamicsDataset.from_wandb("synth", N=2, dN=1))]:
                rows[f"{name}_data"] = obj.data.numpy()
                rows[f"{name}_target"] = obj.target.numpy()
                rows[f"{name}_dims"] = np.array([obj.input_dim, obj.output_dim])
            np.savez_compressed(os.path.join(OUT, "tube_rows.npz"), **rows)

            hz = ds.ScalarHorizonTubeDataset.from_wandb("synth", H_fwd=8, H_rev=3)
            h = {"w": hz.w.numpy(), "z": hz.z.numpy(), "v": hz.v.numpy(), "dims": np.array([hz.input_dim, hz.output_dim]),
                 "items": np.array(HORIZON_ITEMS)}
            for i, (idx, ind) in enumerate(HORIZON_ITEMS):
                x, y = hz._get_item_helper(idx, ind)
                h[f"x{i}"], h[f"y{i}"] = x.numpy(), y.numpy()
            np.savez_compressed(os.path.join(OUT, "tube_horizon.npz"), **h)
        finally:
            os.chdir(cwd)

    # losses: fw, w (B=16, out=5) with exact ties r = 0 and |l| = delta planted
    g = torch.Generator().manual_seed(3)
    B, O, alpha, delta = 16, 5, 0.8, 0.5
    w = torch.rand(B, O, generator=g, dtype=torch.float32) * 2.0
    fw = w + torch.randn(B, O, generator=g, dtype=torch.float32)
    fw[0, :] = w[0, :]                                   # r = 0
    fw[1, 0] = w[1, 0] - delta / alpha                   # r > 0, l = alpha r = delta
    fw[1, 1] = w[1, 1] + delta / (1 - alpha)             # r < 0, l = (1 - alpha)|r| = delta (up to rounding)
    lo = {"w": w.numpy(), "fw": fw.numpy(), "alpha": np.float64(alpha), "delta": np.float64(delta)}
    for name, fn in [("scalar", ls.ScalarTubeLoss(alpha, delta)), ("scalar_horizon", ls.ScalarHorizonTubeLoss(alpha, delta)),
                     ("vector", ls.VectorTubeLoss(alpha, delta)), ("error", ls.ErrorLoss())]:
        f = fw.clone().requires_grad_(True)
        val = fn(f, w, None)
        val.backward()
        lo[f"{name}_value"] = val.detach().numpy()
        lo[f"{name}_grad"] = f.grad.numpy()
    np.savez_compressed(os.path.join(OUT, "tube_losses.npz"), **lo)
    for n in ("tube_dataset", "tube_rows", "tube_horizon", "tube_losses"):
        print(n, os.path.getsize(os.path.join(OUT, n + ".npz")), "bytes")


if __name__ == "__main__":
    main()
