#!/usr/bin/env python3
"""Time of the HIP tube inference against torch eager with model and data already on the device, on the same synthetic data
(DESIGN.md section 10).  Configs:
    rollout_default_64 / _4096   closed loop of 64 / 4096 sequences x 1000 steps, 32 units x 2 layers ReLU, scalar rows
                                 (w, v: 3 inputs, 1 output, 1 column fed back)
    rollout_vector_64 / _4096    the same with 128 units x 2 layers Softplus(beta 5), vector rows (|e|, z, v: 6 inputs, 2 outputs,
                                 2 columns fed back)
    oneshot                      ScalarHorizonTubeDataset 50 / 10, 128 units x 2 layers Softplus: 4096 envs x every 10th window
    window_scalar_64 / _4096     the windowed closed loop (rollout_window), recursive scalar rows with N = 10 taps of (w, v):
                                 30 inputs, 1 output, 1 column fed back per tap, 32 units x 2 layers ReLU
    window_error_64 / _4096      the same for error-dynamics rows, N = 10 taps of (e, z, v): 60 inputs, 2 outputs, 2 columns fed
                                 back per tap, 128 units x 2 layers Softplus(beta 5)
                                 Both also time rollout() -- one tap fed back -- on the same model and rows: the ring's cost.
    levels_4096 / _389120        predict_levels with 8 levels on that many rows of the 128 units x 2 layers Softplus model (5 data
                                 columns + the level), against the way without it: 8 predict() calls on the rows with the level
                                 column appended by torch (torch.cat per level; the appended rows are built inside the timing).  Times are per call,
                                 from windows of several calls
Torch eager is the literal loop: T times (write the fed-back columns -- for the windowed configs those of every tap, from the
loop's own past outputs, as the reference's evaluate_error_dyn_simple.py gathers them -- and run the nn.Sequential on the batch);
for the one-shot config the gather of every window by advanced indexing, then one forward.  Each timing ends in a device synchronise; median of
--repeats runs after a warm-up run of the same shape.

    python tools/bench_tube_eval.py [--configs a,b] [--repeats 3] [--steps 1000]
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
MODELS = {"default": dict(I=3, O=1, U=32, L=2, act="relu", beta=1.0, fb=1),
          "vector": dict(I=6, O=2, U=128, L=2, act="softplus", beta=5.0, fb=2)}
WINDOWS = {"scalar": dict(I=30, O=1, U=32, L=2, act="relu", beta=1.0, fb=1, taps=10, dN=1, stride=3),
           "error": dict(I=60, O=2, U=128, L=2, act="softplus", beta=5.0, fb=2, taps=10, dN=1, stride=6)}
CONFIGS = ["rollout_default_64", "rollout_default_4096", "rollout_vector_64", "rollout_vector_4096", "oneshot",
           "window_scalar_64", "window_scalar_4096", "window_error_64", "window_error_4096", "levels_4096", "levels_389120"]


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


def torch_model(m):
    r = tube_ref.MLP(m.input_dim, m.output_dim, m.num_units, m.num_layers, m.activation, m.softplus_beta)
    r.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    return r.to(DEV)


def bench_rollout(name, n_seq, T, repeats):
    k = MODELS[name]
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(n_seq, T, k["I"], generator=g) * 0.8).to(DEV)
    m = HipTubeModel(initial_params(k["I"], k["O"], k["U"], k["L"], 1), activation=k["act"], softplus_beta=k["beta"], device=DEV)
    ref, fb = torch_model(m), k["fb"]
    xt = x.transpose(0, 1).contiguous()             # (T, n_seq, I): the loop reads a contiguous batch per step

    def eager():
        out = torch.empty(T, n_seq, k["O"], device=DEV)
        with torch.no_grad():
            for t in range(T):
                row = xt[t]
                if t:
                    row = row.clone()
                    row[:, :fb] = out[t - 1, :, :fb]
                out[t] = ref(row)
        return out
    hip_t, hip_all = timed(lambda: m.rollout(x, fb), repeats)
    ref_t, ref_all = timed(eager, repeats)
    diff = float((m.rollout(x, fb).transpose(0, 1) - eager()).abs().max())
    m.close()
    return {"n_seq": n_seq, "T": T, "hip_ms": hip_t * 1e3, "torch_eager_ms": ref_t * 1e3, "speedup": ref_t / hip_t,
            "hip_ms_all": [t * 1e3 for t in hip_all], "torch_eager_ms_all": [t * 1e3 for t in ref_all],
            "hip_us_per_step": hip_t * 1e6 / T, "max_abs_diff": diff, "torch_launches": T * (2 * k["L"] + 1)}


def bench_window(name, n_seq, T, repeats):
    k = WINDOWS[name]
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(n_seq, T, k["I"], generator=g) * 0.8).to(DEV)
    m = HipTubeModel(initial_params(k["I"], k["O"], k["U"], k["L"], 1), activation=k["act"], softplus_beta=k["beta"], device=DEV)
    ref, fb, taps, dN, stride = torch_model(m), k["fb"], k["taps"], k["dN"], k["stride"]
    xt = x.transpose(0, 1).contiguous()

    def eager():
        out = torch.empty(T, n_seq, k["O"], device=DEV)
        with torch.no_grad():
            for t in range(T):
                row = xt[t]
                if t:
                    row = row.clone()
                    for i in range(min(taps, (t - 1) // dN + 1)):
                        row[:, i * stride:i * stride + fb] = out[t - 1 - i * dN, :, :fb]
                out[t] = ref(row)
        return out
    hip_t, hip_all = timed(lambda: m.rollout_window(x, fb, taps, dN, stride), repeats)
    one_t, one_all = timed(lambda: m.rollout(x, fb), repeats)
    ref_t, ref_all = timed(eager, repeats)
    diff = float((m.rollout_window(x, fb, taps, dN, stride).transpose(0, 1) - eager()).abs().max())
    m.close()
    return {"n_seq": n_seq, "T": T, "taps": taps, "dN": dN, "hip_ms": hip_t * 1e3, "hip_single_tap_ms": one_t * 1e3,
            "torch_eager_ms": ref_t * 1e3, "speedup": ref_t / hip_t, "window_over_single_tap": hip_t / one_t,
            "hip_ms_all": [t * 1e3 for t in hip_all], "hip_single_tap_ms_all": [t * 1e3 for t in one_all],
            "torch_eager_ms_all": [t * 1e3 for t in ref_all], "hip_us_per_step": hip_t * 1e6 / T,
            "hip_single_tap_us_per_step": one_t * 1e6 / T, "max_abs_diff": diff}


def bench_levels(n, repeats):
    Ix, O, U, L, n_levels = 5, 2, 128, 2, 8
    g = torch.Generator().manual_seed(0)
    x = (torch.rand(n, Ix, generator=g) * 0.8).to(DEV)
    levels = torch.linspace(0.5, 0.99, n_levels).to(DEV)
    m = HipTubeModel(initial_params(Ix + 1, O, U, L, 1), activation="softplus", softplus_beta=5.0, level_input=True, device=DEV)
    lv = [float(v) for v in levels.cpu()]

    iters = max(2, 1600000 // n)        # calls per timed window: a window of one small call would time the clock

    def one_by_one():
        return torch.stack([m.predict(m.with_level(x, v)) for v in lv], dim=1)

    def loop(fn):
        def run():
            for _ in range(iters):
                fn()
        return run
    hip_t, hip_all = (v if i == 0 else [t / iters for t in v] for i, v in enumerate(timed(loop(lambda: m.predict_levels(x, levels)), repeats)))
    ref_t, ref_all = (v if i == 0 else [t / iters for t in v] for i, v in enumerate(timed(loop(one_by_one), repeats)))
    hip_t, ref_t = hip_t / iters, ref_t / iters
    same = bool(torch.equal(m.predict_levels(x, levels), one_by_one()))
    m.close()
    return {"rows": n, "levels": n_levels, "calls_per_timing": iters, "predict_levels_ms": hip_t * 1e3, "predict_per_level_ms": ref_t * 1e3,
            "per_level_over_predict_levels": ref_t / hip_t, "predict_levels_ms_all": [t * 1e3 for t in hip_all],
            "predict_per_level_ms_all": [t * 1e3 for t in ref_all], "bit_identical": same}


def bench_oneshot(repeats):
    E, T, Hf, Hr, nz, mv = 4096, 1000, 50, 10, 2, 2
    g = torch.Generator().manual_seed(0)
    ds = _Horizon(torch.rand(E, T + Hr, generator=g).to(DEV), torch.rand(E, T + Hr, nz, generator=g).to(DEV),
                  torch.rand(E, T + Hr, mv, generator=g).to(DEV), Hf, Hr)
    I = Hr + nz + (Hr + Hf) * mv
    m = HipTubeModel(initial_params(I, Hf, 128, 2, 1), activation="softplus", softplus_beta=5.0, horizon=(Hf, Hr), device=DEV)
    ref = torch_model(m)
    starts = torch.arange(Hr, T + Hr - Hf, 10, dtype=torch.int32, device=DEV)
    env = torch.arange(E, dtype=torch.int32, device=DEV).repeat_interleave(starts.numel())
    start = starts.repeat(E)
    el, sl = env.long()[:, None], start.long()[:, None]
    tr_, tv = torch.arange(-Hr, 0, device=DEV), torch.arange(-Hr, Hf, device=DEV)

    def eager():
        with torch.no_grad():
            x = torch.cat((ds.w[el, sl + tr_], ds.z[env.long(), start.long()], ds.v[el, sl + tv].reshape(env.numel(), -1)), dim=1)
            return ref(x)
    hip_t, hip_all = timed(lambda: m.predict_windows(ds, env, start), repeats)
    ref_t, ref_all = timed(eager, repeats)
    diff = float((m.predict_windows(ds, env, start) - eager()).abs().max())
    m.close()
    return {"envs": E, "windows": int(env.numel()), "hip_ms": hip_t * 1e3, "torch_eager_ms": ref_t * 1e3, "speedup": ref_t / hip_t,
            "hip_ms_all": [t * 1e3 for t in hip_all], "torch_eager_ms_all": [t * 1e3 for t in ref_all], "max_abs_diff": diff}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--configs", default=",".join(CONFIGS))
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--steps", type=int, default=1000)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_tube_eval.py needs the GPU")
    for cfg in a.configs.split(","):
        if cfg == "oneshot":
            res = bench_oneshot(a.repeats)
        elif cfg.startswith("levels_"):
            res = bench_levels(int(cfg.split("_")[1]), a.repeats)
        else:
            kind, name, n = cfg.split("_")
            res = (bench_window if kind == "window" else bench_rollout)(name, int(n), a.steps, a.repeats)
        res = {"config": cfg, "repeats": a.repeats, "device": torch.cuda.get_device_name(0),
               **{k: (round(v, 4) if isinstance(v, float) else v) for k, v in res.items()}}
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
