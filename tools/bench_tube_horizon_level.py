#!/usr/bin/env python3
"""Time of the level-conditioned one-shot window query (predict_windows_levels) on the reference one-shot
shape: ScalarHorizonTubeDataset 50 / 10 with nz = 0 and m = 2 (130 shared columns + the level), 128 units x 2 layers
Softplus(beta 5) -> 50, 4096 envs x every 10th window of 1000 steps, for L = 1 / 4 / 16 levels.  Three ways to the same
(windows, L, 50) predictions:
    a  new_launch        one predict_windows_levels launch: the first layer's chain over the 130 shared columns once per window
    b  per_level         L predict_windows launches of an UNCONDITIONED model of the same hidden shape (130 inputs): the closest
                         thing the library could do before the conditioned kind existed.  --only b runs on a library without the
                         new entry too (LG_HIP_LIB, or a checkout of an older commit)
    c  torch_eager       torch eager on the (windows L, 131) rows, rows and model resident on the device (the rows are built
                         outside the timing): three GEMMs
Each timing ends in a device synchronise; median of --repeats runs after a warm-up run of the same shape.

    python tools/bench_tube_horizon_level.py [--only a,b,c] [--levels 1,4,16] [--repeats 3] [--envs 4096]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

from legged_gym_dev_amd.tube.model import HipTubeModel  # noqa: E402
from legged_gym_dev_amd.tube.trainer import initial_params  # noqa: E402
from tests import tube_ref  # noqa: E402

DEV = "cuda:0"
T, HF, HR, NZ, MV, U, NL, BETA = 1000, 50, 10, 0, 2, 128, 2, 5.0


class _Horizon:
    def __init__(self, w, z, v, H_fwd, H_rev):
        self.w, self.z, self.v, self.H_fwd, self.H_rev = w, z, v, H_fwd, H_rev


def timed(fn, repeats):
    fn()                                # warm-up: the same shape
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2], ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="a,b,c")
    ap.add_argument("--levels", default="1,4,16")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--envs", type=int, default=4096)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tube_horizon_level.py needs the GPU")
    ways = a.only.split(",")
    E = a.envs
    g = torch.Generator().manual_seed(0)
    ds = _Horizon(torch.rand(E, T + HR, generator=g).to(DEV), torch.rand(E, T + HR, NZ, generator=g).to(DEV),
                  torch.rand(E, T + HR, MV, generator=g).to(DEV), HF, HR)
    I = HR + NZ + (HR + HF) * MV
    starts = torch.arange(HR, T + HR - HF, 10, dtype=torch.int32, device=DEV)
    env = torch.arange(E, dtype=torch.int32, device=DEV).repeat_interleave(starts.numel())
    start = starts.repeat(E)
    W = int(env.numel())
    sd = initial_params(I + 1, HF, U, NL, 1)
    cond = plain = ref = x = None
    if "a" in ways or "c" in ways:
        cond = HipTubeModel(sd, activation="softplus", softplus_beta=BETA, horizon=(HF, HR), level_input=True, device=DEV)
    if "b" in ways:
        plain = HipTubeModel(initial_params(I, HF, U, NL, 1), activation="softplus", softplus_beta=BETA, horizon=(HF, HR), device=DEV)
    if "c" in ways:
        ref = tube_ref.MLP(I + 1, HF, U, NL, "softplus", BETA)
        ref.load_state_dict(sd)
        ref = ref.to(DEV)
        el, sl = env.long()[:, None], start.long()[:, None]
        x = torch.cat((ds.w[el, sl + torch.arange(-HR, 0, device=DEV)], ds.z[env.long(), start.long()],
                       ds.v[el, sl + torch.arange(-HR, HF, device=DEV)].reshape(W, -1)), dim=1)            # (W, 130), resident
    for L in [int(v) for v in a.levels.split(",")]:
        levels = torch.linspace(0.5, 0.99, L).to(DEV) if L > 1 else torch.tensor([0.9], device=DEV)
        res = {"config": f"oneshot_levels_{L}", "envs": E, "windows": W, "levels": L, "repeats": a.repeats,
               "device": torch.cuda.get_device_name(0)}
        if "a" in ways:
            t, ts = timed(lambda: cond.predict_windows_levels(ds, env, start, levels), a.repeats)
            res.update(new_launch_ms=t * 1e3, new_launch_ms_all=[v * 1e3 for v in ts])
        if "b" in ways:
            t, ts = timed(lambda: [plain.predict_windows(ds, env, start) for _ in range(L)], a.repeats)
            res.update(per_level_ms=t * 1e3, per_level_ms_all=[v * 1e3 for v in ts])
        if "c" in ways:
            rows = torch.cat((x[:, None, :].expand(W, L, I), levels[None, :, None].expand(W, L, 1)), dim=2).reshape(W * L, I + 1).contiguous()

            def eager():
                with torch.no_grad():
                    return ref(rows)
            t, ts = timed(eager, a.repeats)
            res.update(torch_eager_ms=t * 1e3, torch_eager_ms_all=[v * 1e3 for v in ts])
            if "a" in ways:
                res["max_abs_diff"] = float((cond.predict_windows_levels(ds, env, start, levels).reshape(W * L, HF) - eager()).abs().max())
            del rows
        if "a" in ways and "b" in ways:
            res["per_level_over_new_launch"] = res["per_level_ms"] / res["new_launch_ms"]
        if "a" in ways and "c" in ways:
            res["torch_eager_over_new_launch"] = res["torch_eager_ms"] / res["new_launch_ms"]
        print(json.dumps({k: (float(f"{v:.3g}") if k == "max_abs_diff" else round(v, 4) if isinstance(v, float)
                              else [round(q, 4) for q in v] if isinstance(v, list) else v) for k, v in res.items()}), flush=True)
    for m in (cond, plain):
        if m is not None:
            m.close()


if __name__ == "__main__":
    main()
